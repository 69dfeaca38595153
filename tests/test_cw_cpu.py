"""CPU checks of the CW point-perturbation attack (include/ifd_cw.h): the test oracle (tests/cw_oracle.py) against a run of the
reference's own CWPerturb recorded in tests/golden/cw_golden.npz, the C ABI and its binding, refusals that need no GPU, and the host
logic of the perturb_attack CLI and of attack.CWPerturb under a stub classifier."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import cw_oracle as CO
import pointnet_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_cw.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    return I.load_library()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "cw_golden.npz"))


@pytest.fixture(scope="module")
def oracle_runs(sd, golden):
    """The float32 and the float64 oracle on the fixture's inputs and recorded noise, free-running; computed once."""
    g = golden
    kw = dict(binary_step=int(g["binary_step"]), num_iter=int(g["num_iter"]), lr=float(g["attack_lr"]), init_weight=float(g["init_weight"]),
              max_weight=float(g["max_weight"]))
    return tuple(CO.attack(PO.to_torch(sd, dt), g["data"], g["target"], g["noise"], dt, **kw) for dt in (torch.float32, torch.float64))


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_reproduces_the_recorded_reference(golden, oracle_runs):
    """tests/golden/cw_golden.npz: the reference's CWPerturb (L2Dist, LogitsAdvLoss(0)) on its own PointNetCls with the calibrated
    weights, 4 clouds x 32 points, 3 search steps x 20 iterations, with the start noise of every search step captured from the run
    (tests/golden/make_golden_cw.py).  The float32 oracle, fed that noise, must give the reference's success flags and its whole
    weight / lower / upper history EXACTLY (this pins the two strict <, the <=, the -1 guard and the last_input fallback), and
    o_bestdist and o_bestattack to within 4 x the float32 oracle's own distance from the float64 oracle on the same fixture.
    Measured: |f32 - f64| = 5.6e-04 on o_bestdist and 4.2e-02 on o_bestattack - free-running for 60 Adam iterations, whose first steps
    are nearly sign steps (m / sqrt(v)), the two precisions drift apart through the gradient's discontinuities although both take the
    recorded discrete history (asserted below).  The float32 oracle against the recording: 1.2e-07 and 5.4e-03 (the reference
    forwards its 4 clouds as one batch, the oracle one cloud at a time: other rounding in the convolutions, amplified likewise)."""
    g, (a32, a64) = golden, oracle_runs
    roles = list(g["roles"])
    assert "up_down" in roles and sum(r != "never" for r in roles) >= 1
    lower = g["history"][-1, :, 1]
    assert np.array_equal(a32["success"], lower > 0) and a32["success_num"] == int(g["success_num"])
    assert np.array_equal(a32["history"], g["history"])
    assert np.array_equal(a64["history"], g["history"])                # else the bars below would measure a diverged trajectory
    e_dist = np.abs(a32["o_bestdist"] - a64["o_bestdist"]).max()
    e_att = np.abs(a32["o_bestattack"].astype(np.float64) - a64["o_bestattack"]).max()
    d_dist = np.abs(a32["o_bestdist"] - g["o_bestdist"]).max()
    d_att = np.abs(a32["o_bestattack"].astype(np.float64) - g["o_bestattack"]).max()
    print("f32 oracle vs f64 oracle: o_bestdist %.3e, o_bestattack %.3e; f32 oracle vs the recording: %.3e, %.3e" % (e_dist, e_att, d_dist, d_att))
    assert e_dist > 0 and e_att > 0
    assert d_dist <= 4 * e_dist and d_att <= 4 * e_att
    # never-successful clouds carry the last forwarded cloud and the untouched 1e10
    for b in np.nonzero(lower == 0)[0]:
        assert g["o_bestdist"][b] == 1e10 == a32["o_bestdist"][b]


def test_oracle_step_is_torch_adam_and_the_record_is_strict():
    rng = np.random.default_rng(0)
    adv, ori, grad, m = (rng.standard_normal((9, 3)) for _ in range(4))
    v = rng.random((9, 3))
    rec = CO.fresh_record(9)
    p, m1, v1, r1, d, dl = CO.step(grad, 3, 3, adv, ori, 10., m, v, 7, 1e-2, 0.25, rec)
    dist = np.sqrt(((adv - ori) ** 2).sum())
    g = grad + 0.25 * 10. * (adv - ori) / dist
    mm, vv = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
    want = adv - (1e-2 / (1 - 0.9 ** 7)) * mm / (np.sqrt(vv) / np.sqrt(1 - 0.999 ** 7) + 1e-8)
    assert np.allclose(p, want, rtol=0, atol=1e-13) and np.allclose(m1, mm, atol=1e-15) and np.allclose(v1, vv, atol=1e-15)
    assert abs(d - dist) < 1e-14 and abs(dl - 10 * dist) < 1e-13
    assert r1["bestdist"] == d == r1["o_bestdist"] and r1["bestscore"] == 3 and np.array_equal(r1["o_bestattack"], adv)
    # an equal distance does not overwrite (strict <), a wrong prediction never records
    other = adv.copy()
    other[0] = 2 * ori[0] - adv[0]                                      # the same distance, another cloud
    r2 = CO.step(grad, 3, 3, other, ori, 10., m, v, 7, 1e-2, 0.25, r1)[3]
    assert np.array_equal(r2["o_bestattack"], adv)
    r3 = CO.step(grad, 4, 3, ori + 0.5 * (adv - ori), ori, 10., m, v, 7, 1e-2, 0.25, r1)[3]
    assert r3["bestdist"] == d and np.array_equal(r3["o_bestattack"], adv)
    # dist == 0: the distance term is left out, the result is finite
    p0 = CO.step(grad, 3, 3, ori, ori, 10., m, v, 1, 1e-2, 0.25, rec)[0]
    assert np.isfinite(p0).all()
    # the adjustment: <=, the -1 guard
    assert CO.adjust({"bestscore": 3, "bestdist": 1., "o_bestdist": 1.}, 3, 10., 0., 80.)[:3] == (45., 10., 80.)
    assert CO.adjust({"bestscore": 3, "bestdist": 1.5, "o_bestdist": 1.}, 3, 10., 0., 80.)[:3] == (5., 0., 10.)
    assert CO.adjust({"bestscore": -1, "bestdist": 1e10, "o_bestdist": 1e10}, -1, 10., 0., 80.)[:3] == (5., 0., 10.)


# ---------------------------------------------------------------------------------------------- ABI
def declared_symbols(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


def test_cw_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols(HEADER)
    assert names == sorted(_lib.CW_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert lib.ifd_cw_abi_version() == 1 == _lib.CW_ABI_VERSION
    assert ctypes.sizeof(_lib.IfdCwParams) == 36 and ctypes.sizeof(_lib.IfdCwState) == 80
    # the attack header the new one builds on is as it was
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_atk.h"))) == 4 and lib.ifd_atk_abi_version() == 1


def test_cw_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_cw_step(None, None, None, None, None, None, None, None, None, None, 1, 0.01, 1.0, None, 1, 8, None) == -1
    assert lib.ifd_cw_adjust(None, None, None, None, 1, 8, None) == -1
    assert lib.ifd_cw_perturb_attack(None, None, None, None, None, None, 1, 8, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- host logic
class StubClassifier:
    """Stands in for runtime.Classifier on the CPU.  Every cloud reaches its target from the iteration `hit` of a search step on;
    a step moves the cloud by 0.01 in x and reports loss 2 and dist * weight 3."""
    device = "cpu"

    def __init__(self, hit=2):
        self.calls, self.closed, self.hit = [], False, hit

    def cw_perturb_attack(self, pc, target, noise, loss, kappa, scale, lr, init_weight, max_weight, binary_step, num_iter):
        self.calls.append(("attack", tuple(pc.shape), noise.clone(), loss, kappa, scale, lr, init_weight, max_weight, binary_step, num_iter))
        ok = torch.as_tensor(target) == 3
        return pc + 1.0, torch.where(ok, 0.5, 1e10).float(), ok

    def cw_state(self, B, K, init_weight, max_weight):
        self.calls.append(("state", B, K, init_weight, max_weight))
        return {"lower": torch.zeros(B, dtype=torch.float64), "o_bestattack": torch.zeros(B, K, 3), "o_bestdist": torch.full((B,), 1e10)}

    def input_grad(self, pc, target, loss, kappa, scale, want_aux=False):
        self.it = getattr(self, "it", 0)
        pred = target if self.it >= self.hit else target + 1
        return torch.zeros_like(pc), {"pred": pred, "loss": torch.full((len(pc),), 2.0)}

    def cw_step(self, state, grad, pred, target, adv, ori, t, lr, scale, loss=None, last_input=None, want_info=False):
        self.calls.append(("step", t, lr, scale, last_input is not None, want_info))
        assert t == self.it + 1
        if bool((pred == target).all()) and float(state["o_bestdist"][0]) == 1e10:
            state["o_bestattack"].copy_(adv)
            state["o_bestdist"].fill_(0.25)
        if last_input is not None:
            last_input.copy_(adv)
        adv[:, 0, 0] -= 0.01
        self.it += 1
        return torch.tensor([[2.0, 3.0, 0.3]] * len(adv)) if want_info else None

    def cw_adjust(self, state, target):
        self.calls.append(("adjust",))
        if self.it > self.hit:
            state["lower"][:-1] = 10.                                  # the last cloud of a batch never succeeds
        self.it = 0

    def close(self):
        self.closed = True


def _attack_file(path, n=6, k=40):
    rng = np.random.default_rng(3)
    np.savez(path, test_pc=rng.standard_normal((n, k, 3)).astype(np.float32), test_label=np.arange(n).astype(np.uint8),
             target_label=np.array([3, 3, 3, 5, 5, 3][:n], np.uint8))


def test_cli_batches_noise_and_file(tmp_path, capsys):
    from ifdefense_amd import perturb_attack as PA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    stub, made = StubClassifier(), []

    def make(model, ft, path):
        made.append((model, ft, path))
        return stub
    argv = ["--data_root", src, "--num_points", "32", "--binary_step", "3", "--num_iter", "7", "--batch_size", "4", "--kappa", "0.5",
            "--attack_lr", "0.02", "--out_dir", str(tmp_path), "--dataset", "opt_mn40", "--seed", "5"]
    assert PA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("pointnet", False, "pretrain/opt_mn40/pointnet.pth")] and stub.closed
    assert out.count("Successfully attack 3/4") == 1 and out.count("Successfully attack 1/2") == 1 and "Step 0" not in out
    # two reference batches (4 + 2 clouds): one library call each, scale = 1 / batch, the reference's weights 10 / 80
    a, b = stub.calls
    assert a[1] == (4, 32, 3) and b[1] == (2, 32, 3)
    assert a[3:] == ("logits", 0.5, 0.25, 0.02, 10., 80., 3, 7) and b[5] == 0.5
    # the noise: one draw per search step and batch, of the reference's size, from the seeded generator
    na, nb = a[2], b[2]
    assert tuple(na.shape) == (3, 4, 32, 3) and tuple(nb.shape) == (3, 2, 32, 3) and na.dtype == torch.float32
    assert 0 < float(na.abs().max()) < 1e-6 and 1e-8 < float(na.std()) < 2e-7
    assert not torch.equal(na[0], na[1]) and not torch.equal(na[1], na[2]) and not torch.equal(na[0, :2], nb[0])
    gen = torch.Generator().manual_seed(5)
    assert torch.equal(na, torch.stack([torch.randn(4, 32, 3, generator=gen) * 1e-7 for _ in range(3)]))
    d = tmp_path / "attack" / "results" / "opt_mn40_32" / "Perturb"
    name = "Perturb-pointnet-logits_kappa=0.5-success_%.4f-rank_0.npz" % (4 / 6)
    assert os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 32, 3)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8
    assert list(z["test_label"]) == list(range(6)) and list(z["target_label"]) == [3, 3, 3, 5, 5, 3]
    # the same seed gives the same noise, another seed another; cross_entropy names the file without kappa; -1: one batch
    stub.calls.clear()
    assert PA.main(argv[:-1] + ["5", "--batch_size", "-1", "--adv_func", "cross_entropy", "--local_rank", "2"], make_classifier=make) == 0
    assert len(stub.calls) == 1 and stub.calls[0][1] == (6, 32, 3) and stub.calls[0][3] == "cross_entropy"
    assert "Perturb-pointnet-cross_entropy-success_%.4f-rank_2.npz" % (4 / 6) in os.listdir(d)
    first = stub.calls[0][2]
    stub.calls.clear()
    assert PA.main(argv[:-1] + ["5", "--batch_size", "-1"], make_classifier=make) == 0
    assert torch.equal(stub.calls[0][2], first)
    stub.calls.clear()
    assert PA.main(argv[:-1] + ["6", "--batch_size", "-1"], make_classifier=make) == 0
    assert not torch.equal(stub.calls[0][2], first)


def test_cli_refuses_what_is_not_built(capsys):
    from ifdefense_amd import perturb_attack as PA

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--model", "dgcnn"], ["--model", "pointnet2"], ["--model", "pointconv"], ["--feature_transform", "true"]):
        assert PA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "not built" in capsys.readouterr().err
    for argv in (["--binary_step", "0"], ["--num_iter", "0"]):
        assert PA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "at least 1" in capsys.readouterr().err
    from ifdefense_amd import attack as A
    with pytest.raises(ValueError, match="l2"):
        A.CWPerturb(None, dist_func="chamfer")
    assert sorted(A.ATTACKS) == ["fgm", "ifgm", "mifgm", "pgd"]


@pytest.mark.parametrize("num_iter,printed", [(10, [0, 2, 4, 6, 8]), (3, [0, 1, 2])])
def test_host_driven_loop_prints_the_reference_lines(capsys, num_iter, printed):
    """verbose=True: one input_grad and one cw_step an iteration, the reference's line every num_iter // 5 iterations (every
    iteration when num_iter < 5) with the batch means of the PREVIOUS iteration's losses, zeros at iteration 0 of a search step;
    last_input is asked for in the last iteration of the last search step only; the fallback for clouds whose lower stays 0."""
    from ifdefense_amd import attack as A
    stub = StubClassifier(hit=2)
    x = torch.zeros(3, 8, 3)
    dist, adv, n_ok = A.CWPerturb(stub, binary_step=2, num_iter=num_iter, attack_lr=0.03, seed=4, ref_batch=12).attack(x, [1, 2, 3])
    out = capsys.readouterr().out.splitlines()
    want = []
    for s in range(2):
        for it in printed:
            want += ["Step %d, iteration %d, success %d/3" % (s, it, 3 if it >= 2 else 0),
                     "adv_loss: %.4f, dist_loss: %.4f" % ((2.0, 3.0) if it else (0.0, 0.0))]
    assert out == want + ["Successfully attack 2/3"] and n_ok == 2
    steps = [c for c in stub.calls if c[0] == "step"]
    assert len(steps) == 2 * num_iter and [c[1] for c in steps] == list(range(1, num_iter + 1)) * 2
    assert all(c[2] == 0.03 and c[3] == pytest.approx(1 / 12) for c in steps)
    assert [c[4] for c in steps] == [False] * (2 * num_iter - 1) + [True]
    assert [c[0] for c in stub.calls if c[0] != "step"] == ["state", "adjust", "adjust"]
    assert dist.dtype == np.float64 and adv.shape == (3, 8, 3)
    # clouds 0, 1: the recorded attack (the state forwarded at iteration 2 of search step 0); cloud 2: the last forwarded cloud
    assert np.allclose(adv[:2, 0, 0], -0.02, atol=1e-6) and np.isclose(adv[2, 0, 0], -0.01 * (num_iter - 1), atol=1e-6)
