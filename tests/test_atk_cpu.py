"""CPU checks of the attack primitives (include/ifd_atk.h): the C ABI and its binding, refusals that need no GPU, the host logic
of the fgm_attack CLI under a stub classifier, and the test oracle itself (tests/atk_oracle.py): autograd against finite
differences, the tie and hinge rules the header states, the clip against outputs recorded from the reference's ClipPointsL2
(tests/golden/atk_clip_golden.npz), the exclusion rule on the inputs the GPU tests use, and that the shared comparison helpers
refuse wrong answers."""
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import atk_oracle as AO
import pointnet_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_atk.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")

# the GPU parity cases (tests/test_gpu_atk.py imports them): (points per cloud, clouds).  Every case meets both conditions of
# atk_oracle.case_conditions from the oracle alone (test_exclusion_rule_on_the_gpu_test_inputs).
CLOUD_SEED = 77
CASES = [(1, 33), (5, 33), (64, 33), (255, 16), (256, 16), (257, 16), (1024, 8)]


def case_inputs(sd, n, B):
    import bench
    clouds = [c[:n] for c in bench.synth_clouds(B, seed=CLOUD_SEED)]
    lo = PO.forward(PO.to_torch(sd, torch.float64), np.stack(clouds), dtype=torch.float64)[0].numpy()
    return clouds, (lo.argmax(1) + 1) % 40


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    return I.load_library()


def test_atk_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.ATK_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert lib.ifd_atk_abi_version() == 1 == _lib.ATK_ABI_VERSION
    assert lib.ifd_cls_abi_version() == 1 and lib.ifd_abi_version() == 5
    import ctypes
    assert ctypes.sizeof(_lib.IfdFgmParams) == 36 and ctypes.sizeof(_lib.IfdAtkOut) == 48


def test_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_cls_input_grad(None, None, None, 1, 8, None, 0, 0.0, 1.0, None, None, None) == -1
    assert lib.ifd_fgm_update(None, 0, None, None, None, None, 0.0, 0.0, 0.0, None, 1, 8, None) == -1
    assert lib.ifd_fgm_attack(None, None, None, None, None, 1, 8, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- CLI host logic
class StubClassifier:
    """Stands in for runtime.Classifier on the CPU: the class of a cloud is 7 until its first coordinate has moved by 0.01."""
    device = "cpu"

    def __init__(self):
        self.calls, self.closed = [], False

    def predict(self, pc):
        pc = torch.as_tensor(np.asarray(pc))
        return torch.where(pc[:, 0, 0] < self.x0 - 0.01, 3, 7)

    def input_grad(self, pc, target, loss, kappa, scale, want_aux=False):
        self.calls.append(("grad", loss, kappa, scale))
        if getattr(self, "seen", None) != pc.data_ptr():               # a new loop (the loop updates one tensor in place)
            self.seen, self.x0 = pc.data_ptr(), pc[:, 0, 0].clone()
        g = torch.zeros_like(pc)
        g[:, 0, 0] = 1.0
        return g, {"pred": self.predict(pc)}

    def fgm_update(self, kind, grad, pc, ori, mom, step, budget, mu):
        self.calls.append(("update", kind, step, budget, mu))
        pc -= step * grad

    def fgm_attack(self, kind, pc, target, budget, step, num_iter, mu, loss, kappa, scale):
        self.calls.append(("attack", kind, budget, step, num_iter, mu, loss, kappa, scale))
        self.x0 = pc[:, 0, 0].clone()
        out = pc.clone()
        out[:, 0, 0] -= budget
        return out, self.predict(out) == target

    def close(self):
        self.closed = True


def _attack_file(path, n=6, k=40):
    rng = np.random.default_rng(3)
    np.savez(path, test_pc=rng.standard_normal((n, k, 3)).astype(np.float32), test_label=np.arange(n).astype(np.uint8),
             target_label=np.array([3, 3, 3, 5, 5, 3][:n], np.uint8))


def test_cli_arithmetic_path_and_file(tmp_path, capsys):
    from ifdefense_amd import fgm_attack as FA
    assert FA.attack_settings(0.08, 1024, 50) == (float(0.08 * np.sqrt(3072)), float(0.08 * np.sqrt(3072) / 50.0))
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    stub = StubClassifier()
    made = []

    def make(model, ft, path):
        made.append((model, ft, path))
        return stub
    argv = ["--data_root", src, "--num_points", "32", "--attack_type", "IFGM", "--num_iter", "10", "--budget", "0.08", "--batch_size", "4",
            "--kappa", "0.5", "--local_rank", "2", "--out_dir", str(tmp_path), "--dataset", "opt_mn40"]
    assert FA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("pointnet", False, "pretrain/opt_mn40/pointnet.pth")] and stub.closed
    assert "Loading weight pretrain/opt_mn40/pointnet.pth" in out
    # two reference batches (4 + 2 clouds), the reference's lines at iterations 0, 2, 4, 6, 8 and the final one
    assert [l for l in out.splitlines() if l.startswith("iter ")][:5] == ["iter %d/10, success: %d/4" % (i, 3 if i else 0) for i in (0, 2, 4, 6, 8)]
    assert out.count("Final success: 3/4") == 1 and out.count("Final success: 1/2") == 1
    budget = 0.08 * np.sqrt(32 * 3)
    grads = [c for c in stub.calls if c[0] == "grad"]
    assert len(grads) == 20 and grads[0] == ("grad", "logits", 0.5, 0.25) and grads[-1] == ("grad", "logits", 0.5, 0.5)
    ups = [c for c in stub.calls if c[0] == "update"]
    assert ups[0][1] == "ifgm" and ups[0][2] == pytest.approx(budget / 10) and ups[0][3] == pytest.approx(budget)
    d = tmp_path / "attack" / "results" / "opt_mn40_32" / "FGM" / "pointnet"
    name = "ifgm-budget_0.08-iter_10-success_%.4f-rank_2.npz" % (4 / 6)
    assert os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 32, 3)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8 and list(z["test_label"]) == list(range(6))
    # plain FGM: one library call per batch with step = budget, the reference's one line
    stub.calls.clear()
    assert FA.main(["--data_root", src, "--num_points", "32", "--out_dir", str(tmp_path), "--adv_func", "cross_entropy"],
                   make_classifier=make) == 0
    assert "Successfully attack 4/6" in capsys.readouterr().out
    assert stub.calls == [("attack", "fgm", pytest.approx(budget), pytest.approx(budget), 1, 1.0, "cross_entropy", 0.0, pytest.approx(1 / 6))]


def test_cli_refuses_what_is_not_built(capsys):
    from ifdefense_amd import fgm_attack as FA

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--model", "dgcnn"], ["--model", "pointnet2"], ["--model", "pointconv"], ["--feature_transform", "true"]):
        assert FA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "not built" in capsys.readouterr().err


def test_start_noise_is_seeded_and_shaped_like_the_reference():
    from ifdefense_amd import attack as A
    x = torch.zeros(2, 50, 3)
    a, b = A.IFGM(None, seed=5).start(x), A.IFGM(None, seed=5).start(x)
    assert torch.equal(a, b) and 0 < float(a.abs().max()) < 1e-6
    p = A.PGD(None, budget=1.5, seed=5).start(x)
    assert float(p.abs().max()) <= 1.5 / np.sqrt(150) + 1e-6 and float(p.abs().max()) > 0.5 * 1.5 / np.sqrt(150)
    assert torch.equal(A.FGM(None).start(x), x)


# ---------------------------------------------------------------------------------------------- the oracle itself
def test_autograd_against_central_differences(sd):
    W = PO.to_torch(sd, torch.float64)
    pts = case_inputs(sd, 5, 2)[0][1].astype(np.float64)
    for loss in ("logits", "cross_entropy"):
        r = AO.run_cloud(W, pts, 4, loss, kappa=0.3)
        num = np.zeros_like(pts)
        h = 1e-6
        for i in range(5):
            for a in range(3):
                p, m = pts.copy(), pts.copy()
                p[i, a] += h
                m[i, a] -= h
                num[i, a] = (AO.run_cloud(W, p, 4, loss, 0.3)["loss"] - AO.run_cloud(W, m, 4, loss, 0.3)["loss"]) / (2 * h)
        assert np.abs(r["grad"]).max() > 0
        assert np.abs(num - r["grad"]).max() <= 1e-5 * np.abs(r["grad"]).max()


def test_tie_and_hinge_rules_of_torch_on_the_cpu():
    assert int(torch.max(torch.tensor([[1., 3., 3., 2.]]), 1)[1]) == 1                  # the lowest index among equal values
    x = torch.tensor([-1e-3, 0., 1e-3], requires_grad=True)
    torch.clamp(x, min=0.).sum().backward()
    assert x.grad.tolist() == [0., 1., 1.]                                               # the gradient passes AT the corner
    lo = torch.tensor([[2., 5., 5., 1.]], dtype=torch.float64, requires_grad=True)
    lv, h, oi = AO.adv_loss(lo, torch.tensor([3]))
    lv.sum().backward()
    assert int(oi) == 1 and float(h.detach()) == 4. and lo.grad.tolist() == [[0., 1., 0., -1.]]   # the first of two equal runners-up


def test_all_points_equal_routes_to_row_zero(sd):
    W = PO.to_torch(sd, torch.float64)
    r = AO.run_cloud(W, np.tile(np.array([[0.3, -0.2, 0.5]]), (7, 1)), 1)
    assert not r["win_feat"].any() and np.abs(r["grad"][0]).max() > 0 and not r["grad"][1:].any()


def test_clip_against_the_recorded_reference():
    """tests/golden/atk_clip_golden.npz: inputs and outputs of the reference's ClipPointsL2(1.0).forward (clip_utils.py:17-31) run on the
    CPU in float32 and float64, six clouds of 40 points whose ||pc - ori|| is 0.11, 0.55, 1.09, 2.1, 10.9 and 35.6 - two inside the
    ball, one just outside, three far outside.  The same torch ops in the same order: equal to the last bit."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "atk_clip_golden.npz"))
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        got = AO.clip_l2(torch.from_numpy(g["pc"]).to(dt), torch.from_numpy(g["ori"]).to(dt), float(g["budget"])).numpy()
        assert got.dtype == g["out" + name].dtype and np.array_equal(got, g["out" + name])
    n = np.sqrt(((g["out64"] - g["ori"]) ** 2).sum((1, 2)))
    assert np.all(n[:2] < 0.6) and np.allclose(n[2:], 1.0, rtol=1e-12)
    # update() ends in the same clip: a step far outside the budget lands on the sphere
    p, _ = AO.update("ifgm", g["pc"][0].T, g["ori"][0].T, g["ori"][0].T, None, 5.0, 1.0, 1.0)
    assert abs(np.sqrt(((p - g["ori"][0].T) ** 2).sum()) - 1.0) < 1e-9


@pytest.mark.parametrize("n,B", CASES)
def test_exclusion_rule_on_the_gpu_test_inputs(sd, n, B):
    """The conditions every GPU parity case must meet, from the oracle alone.  By whole clouds (atk_oracle.exclusion: any gate on the
    gradient path within 8 e_act of zero) the oracle leaves out 0 / 33 clouds at 1 and 5 points but 8 / 33 at 64, 16 / 33 at 256 and
    6 / 8 at 1024 (about 4 10^5 gated units a 1024-point cloud against a band of 2.5 10^-6), so the cases are judged row by row
    (atk_oracle.row_exclusion).  Measured: whole clouds out 0, 0, 0, 0, 1, 1, 0 of 33, 33, 33, 16, 16, 16, 8; gradient-receiving rows
    judged 100, 100, 79, 85, 74, 67, 59 %."""
    clouds, tg = case_inputs(sd, n, B)
    r32, r64, e, e32, ex = AO.run_case(sd, clouds, tg)
    whole, judged, live = AO.case_conditions(r64, e)
    print("N=%d B=%d: e_32(grad) %.3e, e_act %s, clouds out by the cloud rule %d, wholly out by the row rule %d, rows judged %d of %d"
          % (n, B, e32, {k: "%.1e" % v for k, v in e.items()}, sum(1 for x in ex if x), whole, judged, live))
    assert 0 < e32 < 1e-5
    assert sum(AO.masks_agree(a, b) for a, b in zip(r32, r64)) >= 0.9 * B    # actual flips between the two oracles are rare


def test_helpers_refuse_wrong_gradients(sd):
    clouds, tg = case_inputs(sd, 5, 4)
    r32, r64, e, e32, ex = AO.run_case(sd, clouds, tg)
    r = r64[0]
    good = np.zeros((8, 3))
    good[:5] = r["grad"]
    assert AO.check_grad(good.astype(np.float32), r["grad"], e32) <= 4
    off = good.copy()
    off[np.abs(good).sum(1).argmax()] += 10 * e32 * np.abs(good).max()
    with pytest.raises(AssertionError):
        AO.check_grad(off, r["grad"], e32)
    zero = good.copy()
    zero[np.abs(good).sum(1).argmax()] = 0
    with pytest.raises(AssertionError):
        AO.check_grad(zero, r["grad"], e32)
    pad = good.copy()
    pad[6, 1] = 1e-30
    with pytest.raises(AssertionError):
        AO.check_grad(pad, r["grad"], e32)
    # a gradient routed to the runner-up point of one channel
    act = r["pre"]["c3"]
    c = int(np.argmax(np.sort(act, 1)[:, -1] - np.sort(act, 1)[:, -2]))
    wrong = r["win_feat"].copy()
    wrong[c] = int(np.argsort(act[c])[-2])
    with pytest.raises(AssertionError):
        AO.winners_valid(wrong, act, e["c3"])
    assert AO.winners_valid(r["win_feat"], act, e["c3"]) == 0
    routed = AO.run_cloud(PO.to_torch(sd, torch.float64), clouds[0], tg[0], force_feat=wrong, force_stn=r["win_stn"])["grad"]
    if np.abs(routed - r["grad"]).max() > 4 * e32 * np.abs(r["grad"]).max():
        with pytest.raises(AssertionError):
            AO.check_grad(routed, r["grad"], e32)
