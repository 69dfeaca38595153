"""CPU checks of the CW point-adding attack (include/ifd_add.h): the test oracle (tests/add_oracle.py) against runs of the
reference's own CWAdd recorded in tests/golden/add_golden.npz, the closed form of the distance term's gradient, the selection's
total order, the conditions of the GPU parity cases, the C ABI and its binding, refusals that need no GPU, and the host logic of
the add_attack CLI and of attack.CWAdd under a stub classifier."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import add_oracle as DO
import pointnet_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_add.h")
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
    return np.load(os.path.join(ROOT, "tests", "golden", "add_golden.npz"))


@pytest.fixture(scope="module")
def oracle_runs(sd, golden):
    """{kind: (float32 run, float64 run)} of the oracle on the fixture's inputs and recorded noise, free-running; computed once."""
    g = golden
    out = {}
    for kind in DO.KINDS:
        kw = dict(binary_step=int(g["binary_step"]), num_iter=int(g["num_iter"]), lr=float(g["attack_lr"]),
                  init_weight=float(g[kind + "_init_weight"]), max_weight=float(g[kind + "_max_weight"]))
        out[kind] = tuple(DO.attack(PO.to_torch(sd, dt), g["data"], g["target"], g[kind + "_noise"], kind, int(g["num_add"]), dt, **kw)
                          for dt in (torch.float32, torch.float64))
    return out


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("kind", DO.KINDS)
def test_oracle_reproduces_the_recorded_reference(golden, oracle_runs, kind):
    """tests/golden/add_golden.npz: the reference's CWAdd (ChamferDist / HausdorffDist 'adv2ori', LogitsAdvLoss(0), the script's
    weights) on its own PointNetCls with the calibrated weights, 4 clouds x 32 points, 8 added, 3 search steps x 20 iterations, with
    the start noise of every search step captured from the run (tests/golden/make_golden_add.py).  The float32 oracle, fed that
    noise, must give the reference's critical points, its success count and its whole weight / lower / upper history EXACTLY, and
    o_bestdist and the final clouds to within 4 x the float32 oracle's own distance from the float64 oracle on the same fixture.
    The fixture's selected scores are pairwise distinct (asserted by the script), so torch.topk's order among equals plays no part.
    Measured (printed below): chamfer |f32 - f64| = 7.8e-05 on o_bestdist and 1.2e-02 on the clouds, the float32 oracle against the
    recording 1.0e-04 and 9.9e-03; hausdorff 2.3e-03 and 1.2e-01, against the recording 7.0e-04 and 1.6e-01.  The distances are wide
    for 60 free-running iterations: the record keeps the first state that reaches the target, and when that happens hangs on the last
    bits of the logits (the reference forwards its 4 clouds as one batch, the oracle one cloud at a time).  For Hausdorff the float64
    oracle does not even take the recorded weight history (printed, asserted for Chamfer only): from the 1e-7 start the reference's
    first arg-max is decided by float32 rounding noise that float64 does not have - the deviation include/ifd_add.h states."""
    g, (a32, a64) = golden, oracle_runs[kind]
    K, A = g["data"].shape[1], int(g["num_add"])
    assert np.array_equal(a32["cri"], g[kind + "_cri_data"])
    roles = list(g[kind + "_roles"])
    assert "up_down" in roles and int(g[kind + "_success_num"]) >= 1
    lower = g[kind + "_history"][-1, :, 1]
    assert np.array_equal(a32["success"], lower > 0) and a32["success_num"] == int(g[kind + "_success_num"])
    assert np.array_equal(a32["history"], g[kind + "_history"])
    same64 = np.array_equal(a64["history"], g[kind + "_history"])
    print("%s: the float64 oracle takes the recorded weight history: %s" % (kind, same64))
    if kind == "chamfer":
        assert same64                                                  # else the bars below would measure a diverged trajectory
    ok = lower > 0
    rec_att = g[kind + "_o_bestattack"]
    assert rec_att.shape == (len(ok), K + A, 3)
    for run in (a32, a64):
        assert np.array_equal(run["o_bestattack"][:, :K].astype(np.float32), g["data"])
    e_dist = np.abs(a32["o_bestdist"] - a64["o_bestdist"])[ok].max()
    e_att = np.abs(a32["o_bestattack"].astype(np.float64) - a64["o_bestattack"]).max()
    d_dist = np.abs(a32["o_bestdist"] - g[kind + "_o_bestdist"])[ok].max()
    d_att = np.abs(a32["o_bestattack"].astype(np.float64) - rec_att).max()
    print("%s: f32 oracle vs f64 oracle: o_bestdist %.3e, clouds %.3e; f32 oracle vs the recording: %.3e, %.3e" % (kind, e_dist, e_att, d_dist, d_att))
    assert e_dist > 0 and e_att > 0
    assert d_dist <= 4 * e_dist and d_att <= 4 * e_att
    for b in np.nonzero(~ok)[0]:                                       # never successful: the untouched 1e10
        assert g[kind + "_o_bestdist"][b] == 1e10 == a32["o_bestdist"][b]


@pytest.mark.parametrize("kind", DO.KINDS)
def test_closed_form_gradient_is_autograd_in_float64(kind):
    """The header's step 4 against autograd through the reference's expanded form, float64, to 1e-12 (of values of order 1e2), from
    cri + 0.02 randn; Adam is the real torch.optim.Adam; the record is strict."""
    rng = np.random.default_rng(1)
    ori = rng.standard_normal((40, 3)) * 0.5
    adv = ori[rng.permutation(40)[:9]] + 0.02 * rng.standard_normal((9, 3))
    grad, m = rng.standard_normal((9, 3)), rng.standard_normal((9, 3))
    v = rng.random((9, 3))
    w, scale = 3000., 0.25
    p, m1, v1, r1, d, dl, diag = DO.step(kind, grad, 3, 3, adv, ori, w, m, v, 7, 1e-2, scale, DO.fresh_record(9))
    P = ((adv[:, None] - ori[None]) ** 2).sum(2)
    assert np.array_equal(diag["nn"], P.argmin(1)) and np.abs(diag["min_p"] - P.min(1)).max() < 1e-13
    want = P.min(1).mean() if kind == "chamfer" else P.min(1).max()
    assert abs(d - want) < 1e-13 and abs(dl - w * want) < 1e-9
    assert diag["far"] == (-1 if kind == "chamfer" else int(P.min(1).argmax()))
    cf = DO.closed_form_grad(adv, ori, kind, w, scale, diag["nn"], diag["far"])
    assert np.abs(cf - diag["dist_grad"]).max() <= 1e-12
    if kind == "hausdorff":
        assert np.count_nonzero(np.abs(diag["dist_grad"]).sum(1)) == 1
    g = grad + cf
    mm, vv = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
    want = adv - (1e-2 / (1 - 0.9 ** 7)) * mm / (np.sqrt(vv) / np.sqrt(1 - 0.999 ** 7) + 1e-8)
    assert np.allclose(p, want, rtol=0, atol=1e-12) and np.allclose(m1, mm, atol=1e-13) and np.allclose(v1, vv, atol=1e-12)
    assert r1["bestdist"] == d == r1["o_bestdist"] and r1["bestscore"] == 3 and np.array_equal(r1["o_bestattack"], adv)
    r2 = DO.step(kind, grad, 4, 3, ori[:9], ori, w, m, v, 7, 1e-2, scale, r1)[3]       # nearer, but the wrong class: no record
    assert r2["bestdist"] == d and np.array_equal(r2["o_bestattack"], adv)


def test_the_reference_start_is_rounding_noise_and_the_difference_form_is_not():
    """Why parity is never judged from the 1e-7 start: with every added point within 1e-7 of an original, where the true min_p is
    of order 1e-14, the reference's float32 expanded form gives values of the size of its own rounding, 1e-7, while the argmin still
    names the source point; the difference form gives the true size."""
    rng = np.random.default_rng(5)
    ori = (rng.standard_normal((256, 3)) * 0.5).astype(np.float32)
    idx = rng.permutation(256)[:64]
    adv = ori[idx] + (rng.standard_normal((64, 3)) * 1e-7).astype(np.float32)
    o, a = torch.from_numpy(ori)[None], torch.from_numpy(adv)[None]
    _, mins, nn, _ = DO.set_distance(a, o, "hausdorff")
    _, mins64, nn64, _ = DO.set_distance(a.double(), o.double(), "hausdorff")
    assert np.array_equal(nn.numpy(), idx) and np.array_equal(nn64.numpy(), idx)
    assert 1e-8 < float(mins.abs().max()) < 2e-6 and float(mins64.abs().max()) < 1e-12
    d = adv - ori[idx]
    assert float((d * d).sum(1).max()) < 1e-12


def test_selection_is_a_total_order_on_crafted_ties():
    """add_oracle.select (numpy's stable descending sort) is the header's rank by counting: rank_i = #{j : s_j > s_i or (s_j == s_i
    and j < i)}."""
    rng = np.random.default_rng(2)
    g = np.zeros((50, 3), np.float32)
    g[rng.permutation(50)[:20], 0] = np.repeat(np.array([3., 2., 2., 1., 0.5], np.float32), 4)[rng.permutation(20)]
    s = DO.scores(g)
    rank = np.array([int(((s > s[i]) | ((s == s[i]) & (np.arange(50) < i))).sum()) for i in range(50)])
    assert sorted(rank) == list(range(50))
    for num_add in (1, 7, 20, 21, 35, 50):                             # inside the ties, at the zero boundary, beyond it
        idx = DO.select(g, num_add)
        assert np.array_equal(rank[idx], np.arange(num_add))
    assert np.array_equal(DO.select(np.zeros((9, 3), np.float32), 4), [0, 1, 2, 3])
    # the score's order of operations: (x*x + y*y) + z*z in float32
    g = np.array([[1e-3, 3e-4, 7.7e-5]], np.float32)
    x, y, z = (np.float32(c) for c in g[0])
    assert DO.scores(g)[0] == np.float32(np.float32(np.float32(x * x) + np.float32(y * y)) + np.float32(z * z))


@pytest.mark.parametrize("name", [c[0] for c in DO.STEP_CASES])
@pytest.mark.parametrize("kind", DO.KINDS)
def test_step_cases_meet_their_conditions(name, kind):
    """The GPU parity cases (tests/test_gpu_add.py) from the oracle alone: at most 5 % of a case's rows are excluded, no Hausdorff
    cloud is, and the two oracles agree on every judged decision - asserted inside judge_step_case."""
    for t in (1, 7):
        case = DO.make_step_case(name, kind, t)
        r32, r64 = DO.run_step_case(case, torch.float32), DO.run_step_case(case, torch.float64)
        e, rows_out, _, e32, share = DO.judge_step_case(case, r32, r64)
        print("%s %s t=%d: e %.2e, excluded %.2f %%, e32 %s" % (name, kind, t, e, 100 * share, {k: "%.1e" % x for k, x in e32.items()}))
        assert 0 < e < 1e-5 and all(x > 0 for x in e32.values())


# ---------------------------------------------------------------------------------------------- ABI
def declared_symbols(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


def defined(path, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read()).group(1))


def test_add_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols(HEADER)
    assert names == sorted(_lib.ADD_SIGNATURES) and len(names) == 5
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert lib.ifd_add_abi_version() == 1 == _lib.ADD_ABI_VERSION == defined(HEADER, "IFD_ADD_ABI_VERSION")
    assert (_lib.ADD_CHAMFER, _lib.ADD_HAUSDORFF) == (defined(HEADER, "IFD_ADD_CHAMFER"), defined(HEADER, "IFD_ADD_HAUSDORFF")) == (0, 1)
    assert (_lib.ADD_MAX_ADD, _lib.ADD_MAX_ORI) == (defined(HEADER, "IFD_ADD_MAX_ADD"), defined(HEADER, "IFD_ADD_MAX_ORI")) == (1024, 2048)
    assert ctypes.sizeof(_lib.IfdAddParams) == 44 and ctypes.sizeof(_lib.IfdAddDiag) == 24 and ctypes.sizeof(_lib.IfdCwState) == 80
    # the headers the new one builds on are as they were
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_cw.h"))) == 4 and lib.ifd_cw_abi_version() == 1
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_atk.h"))) == 4 and lib.ifd_atk_abi_version() == 1


def test_add_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_add_select(None, None, None, None, 1, 8, 2, None, None, None) == -1
    assert lib.ifd_add_critical_points(None, None, None, None, 1, 8, 2, 1.0, None, None, None) == -1
    assert lib.ifd_add_step(None, 0, None, None, None, None, None, None, None, None, None, None, 1, 0.01, 1.0, 1, 8, 2, None) == -1
    assert lib.ifd_add_attack(None, None, None, None, None, None, 1, 8, 10, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- host logic
class StubClassifier:
    """Stands in for runtime.Classifier on the CPU.  Every cloud reaches its target from the iteration `hit` of a search step on;
    a step moves the first added point by 0.01 in x and reports loss 2 and dist * weight 3."""
    device = "cpu"

    def __init__(self, hit=2):
        self.calls, self.closed, self.hit = [], False, hit

    def add_attack(self, kind, pc, target, num_add, noise, loss, kappa, scale, lr, init_weight, max_weight, binary_step, num_iter):
        self.calls.append(("attack", kind, tuple(pc.shape), num_add, noise.clone(), loss, kappa, scale, lr, init_weight, max_weight,
                           binary_step, num_iter))
        ok = torch.as_tensor(target) == 3
        return torch.cat([pc, pc[:, :num_add] + 1.0], 1), torch.where(ok, 0.5, 1e10).float(), ok

    def add_critical_points(self, pc, target, num_add, scale):
        self.calls.append(("critical", tuple(pc.shape), num_add, scale))
        return pc[:, :num_add].clone() + 5.0

    def cw_state(self, B, A, init_weight, max_weight):
        self.calls.append(("state", B, A, init_weight, max_weight))
        return {"lower": torch.zeros(B, dtype=torch.float64), "o_bestattack": torch.zeros(B, A, 3), "o_bestdist": torch.full((B,), 1e10)}

    def input_grad(self, pc, target, loss, kappa, scale, want_aux=False):
        self.it = getattr(self, "it", 0)
        self.calls.append(("grad", tuple(pc.shape)))
        pred = target if self.it >= self.hit else target + 1
        return torch.zeros_like(pc), {"pred": pred, "loss": torch.full((len(pc),), 2.0)}

    def add_step(self, kind, state, grad, pred, target, cat, num_add, t, lr, scale, loss=None, last_input=None, want_info=False):
        self.calls.append(("step", kind, num_add, t, lr, scale, last_input is not None, want_info))
        assert t == self.it + 1
        K = cat.shape[1] - num_add
        if bool((pred == target).all()) and float(state["o_bestdist"][0]) == 1e10:
            state["o_bestattack"].copy_(cat[:, K:])
            state["o_bestdist"].fill_(0.25)
        if last_input is not None:
            last_input.copy_(cat[:, K:])
        cat[:, K, 0] -= 0.01
        self.it += 1
        return {"info": torch.tensor([[2.0, 3.0, 0.3]] * len(cat))} if want_info else {}

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


@pytest.mark.parametrize("dist_func,weights", [("chamfer", (5e3, 4e4)), ("hausdorff", (2e2, 9e2))])
def test_cli_batches_noise_and_file(tmp_path, capsys, dist_func, weights):
    from ifdefense_amd import add_attack as AA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    stub, made = StubClassifier(), []

    def make(model, ft, path):
        made.append((model, ft, path))
        return stub
    argv = ["--data_root", src, "--num_points", "32", "--num_add", "8", "--dist_func", dist_func, "--binary_step", "3", "--num_iter", "7",
            "--batch_size", "4", "--kappa", "0.5", "--attack_lr", "0.02", "--out_dir", str(tmp_path), "--dataset", "opt_mn40", "--seed", "5"]
    assert AA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("pointnet", False, "pretrain/opt_mn40/pointnet.pth")] and stub.closed
    assert out.count("Successfully attack 3/4") == 1 and out.count("Successfully attack 1/2") == 1 and "Step 0" not in out
    # two reference batches (4 + 2 clouds): one library call each, scale = 1 / batch, the reference script's weights
    a, b = stub.calls
    assert a[1] == dist_func and a[2] == (4, 32, 3) and b[2] == (2, 32, 3) and a[3] == 8
    assert a[5:] == ("logits", 0.5, 0.25, 0.02) + weights + (3, 7) and b[7] == 0.5
    na, nb = a[4], b[4]
    assert tuple(na.shape) == (3, 4, 8, 3) and tuple(nb.shape) == (3, 2, 8, 3) and na.dtype == torch.float32
    assert 0 < float(na.abs().max()) < 1e-6 and 1e-8 < float(na.std()) < 2e-7
    gen = torch.Generator().manual_seed(5)
    assert torch.equal(na, torch.stack([torch.randn(4, 8, 3, generator=gen) * 1e-7 for _ in range(3)]))
    d = tmp_path / "attack" / "results" / "opt_mn40_32" / "Add" / dist_func
    name = "Add-pointnet-logits_kappa=0.5-success_%.4f-rank_0.npz" % (4 / 6)
    assert os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 40, 3)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8
    assert list(z["test_label"]) == list(range(6)) and list(z["target_label"]) == [3, 3, 3, 5, 5, 3]
    # cross_entropy names the file without kappa; -1: one batch; the rank names the file
    stub.calls.clear()
    assert AA.main(argv + ["--batch_size", "-1", "--adv_func", "cross_entropy", "--local_rank", "2"], make_classifier=make) == 0
    assert len(stub.calls) == 1 and stub.calls[0][2] == (6, 32, 3) and stub.calls[0][5] == "cross_entropy"
    assert "Add-pointnet-cross_entropy-success_%.4f-rank_2.npz" % (4 / 6) in os.listdir(d)


def test_cli_and_class_refuse_what_is_not_built(capsys):
    from ifdefense_amd import add_attack as AA

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--model", "dgcnn"], ["--model", "pointnet2"], ["--model", "pointconv"], ["--feature_transform", "true"]):
        assert AA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "not built" in capsys.readouterr().err
    for argv in (["--binary_step", "0"], ["--num_iter", "0"]):
        assert AA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "at least 1" in capsys.readouterr().err
    for argv in (["--num_add", "0"], ["--num_add", "1025", "--num_points", "2048"], ["--num_add", "64", "--num_points", "63"],
                 ["--num_points", "2049"]):
        assert AA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "are needed" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        AA.main(["--dist_func", "l2"], make_classifier=never)
    capsys.readouterr()
    from ifdefense_amd import attack as A
    with pytest.raises(ValueError, match="chamfer or hausdorff"):
        A.CWAdd(None, dist_func="l2")
    for kw in ({"num_add": 0}, {"num_add": 1025}, {"binary_step": 0}, {"num_iter": 0}):
        with pytest.raises(ValueError):
            A.CWAdd(None, **kw)
    with pytest.raises(ValueError, match="between num_add and 2048"):
        A.CWAdd(StubClassifier(), num_add=9).attack(torch.zeros(2, 8, 3), [1, 2])
    assert sorted(A.ATTACKS) == ["fgm", "ifgm", "mifgm", "pgd"]


@pytest.mark.parametrize("num_iter,printed", [(10, [0, 2, 4, 6, 8]), (3, [0, 1, 2])])
def test_host_driven_loop_prints_the_reference_lines(capsys, num_iter, printed):
    """verbose=True: the critical points once, then one input_grad on the CONCATENATED clouds and one add_step an iteration; the
    reference's line every num_iter // 5 iterations with the batch means of the PREVIOUS iteration's losses, zeros at iteration 0 of
    a search step, and none of its wall-clock lines; last_input in the last iteration of the last search step only; the fallback
    for clouds whose lower stays 0; the originals come back untouched in front of the added rows."""
    from ifdefense_amd import attack as A
    stub = StubClassifier(hit=2)
    x = torch.arange(3 * 8 * 3, dtype=torch.float32).reshape(3, 8, 3)
    dist, adv, n_ok = A.CWAdd(stub, dist_func="hausdorff", binary_step=2, num_iter=num_iter, attack_lr=0.03, num_add=4, seed=4,
                              ref_batch=12).attack(x, [1, 2, 3])
    out = capsys.readouterr().out.splitlines()
    want = []
    for s in range(2):
        for it in printed:
            want += ["Step %d, iteration %d, success %d/3" % (s, it, 3 if it >= 2 else 0),
                     "adv_loss: %.4f, dist_loss: %.4f" % ((2.0, 3.0) if it else (0.0, 0.0))]
    assert out == want + ["Successfully attack 2/3"] and n_ok == 2 and not any("time" in l for l in out)
    steps = [c for c in stub.calls if c[0] == "step"]
    assert len(steps) == 2 * num_iter and [c[3] for c in steps] == list(range(1, num_iter + 1)) * 2
    assert all(c[1] == "hausdorff" and c[2] == 4 and c[4] == 0.03 and c[5] == pytest.approx(1 / 12) for c in steps)
    assert [c[6] for c in steps] == [False] * (2 * num_iter - 1) + [True]
    assert all(c[1] == (3, 12, 3) for c in stub.calls if c[0] == "grad")
    assert [c[0] for c in stub.calls if c[0] not in ("step", "grad")] == ["critical", "state", "adjust", "adjust"]
    assert stub.calls[0] == ("critical", (3, 8, 3), 4, pytest.approx(1 / 12)) and stub.calls[1] == ("state", 3, 4, 5e3, 4e4)
    assert dist.dtype == np.float64 and adv.shape == (3, 12, 3) and np.array_equal(adv[:, :8], x.numpy())
    # clouds 0, 1: the recorded rows (forwarded at iteration 2 of search step 0); cloud 2: the last forwarded rows
    start = x.numpy()[:, 0, 0] + 5.0
    assert np.allclose(adv[:2, 8, 0] - start[:2], -0.02, atol=1e-5) and np.isclose(adv[2, 8, 0] - start[2], -0.01 * (num_iter - 1), atol=1e-4)
    assert np.allclose(adv[:, 9:], x.numpy()[:, 1:4] + 5.0, atol=1e-5)
