"""CPU checks of the kNN attack (include/ifd_knn.h): the test oracle (tests/knn_oracle.py) against a run of the reference's own CWKNN
recorded in tests/golden/knn_golden.npz, against autograd and against clip_utils restated row by row; the C ABI and its binding,
refusals that need no GPU, and the host logic of the knn_attack CLI and of attack.CWKNN under a stub classifier."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import knn_oracle as KO
import pointnet_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_knn.h")
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
    return np.load(os.path.join(ROOT, "tests", "golden", "knn_golden.npz"))


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_reproduces_the_recorded_reference(sd, golden):
    """tests/golden/knn_golden.npz: the reference's CWKNN (ChamferkNNDist('adv2ori', 5, 1.05, 5., 3.), ProjectInnerClipLinf(0.1),
    LogitsAdvLoss(0)) on its own PointNetCls with the calibrated weights, 4 clouds x 32 points x 6 channels, 25 iterations at
    attack_lr 0.01, with the start noise captured from the run (tests/golden/make_golden_knn.py).  One cloud reaches its target,
    three do not; 23 of the 128 rows end on the 0.1 budget and the float64 oracle projects 1883 of the 3200 row-iterations.  The
    float32 oracle, fed that noise, must give the reference's success_num EXACTLY and the final clouds to within 4 x the float32
    oracle's own distance from the float64 oracle on the same fixture (both printed)."""
    g = golden
    pts, nrm = g["data"][:, :, :3], g["data"][:, :, 3:]
    assert int(g["on_budget"]) > 0 and int(g["projected"]) > 0 and 1 <= int(g["success_num"]) <= 3
    kw = dict(num_iter=int(g["num_iter"]), lr=float(g["attack_lr"]), kappa=float(g["kappa"]))
    a32, a64 = (KO.attack(PO.to_torch(sd, dt), pts, nrm, g["target"], g["noise"], dt, **kw) for dt in (torch.float32, torch.float64))
    assert a32["success_num"] == int(g["success_num"]) and np.array_equal(a32["pred"], g["final_pred"])
    e_32 = np.abs(a32["adv"].astype(np.float64) - a64["adv"]).max()
    d_rec = np.abs(a32["adv"].astype(np.float64) - g["adv"]).max()
    print("final adv: f32 oracle vs f64 oracle %.3e, f32 oracle vs the recording %.3e = %.2f e_32" % (e_32, d_rec, d_rec / e_32))
    assert e_32 > 0 and d_rec <= 4 * e_32
    disp = np.sqrt(((a32["adv"].astype(np.float64) - pts) ** 2).sum(-1))
    assert disp.max() <= 0.1 * (1 + 1e-6) and (disp >= 0.1 * (1 - 1e-5)).sum() > 0


def test_oracle_gradient_is_the_closed_form():
    """autograd through the reference-form loss in float64 against the header's formula (difference form, self excluded by index,
    masks and neighbour sets constant), on a cloud small enough that several points are masked and share neighbours."""
    rng = np.random.default_rng(3)
    ori = rng.standard_normal((40, 3)) * 0.4
    ori[:4] *= 2.5                                                       # a few outliers: they are the masked ones
    adv = ori + 0.03 * rng.standard_normal(ori.shape)
    z = np.zeros_like(adv)
    r = KO.step(z, adv, ori, None, z, z + 1., 1, 1e-3, 0.25)
    assert r["self_ok"] and 2 <= r["mask"].sum() <= 20
    want = KO.g_dist_closed(adv, ori, 0.25)
    assert np.abs(want).max() > 0.01 and np.allclose(r["g_dist"], want, rtol=0, atol=1e-12)
    # the pieces: value is the mean of the five smallest squared distances, the threshold's std is unbiased, the mask is strict
    D = ((adv[:, None] - adv[None]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    value = np.sort(D, 1)[:, :5].mean(1)
    assert np.allclose(r["value"], value, atol=1e-13) and abs(r["thr"] - (value.mean() + 1.05 * value.std(ddof=1))) < 1e-13
    assert np.array_equal(r["mask"], value > r["thr"])
    assert abs(r["cd"] - ((adv[:, None] - ori[None]) ** 2).sum(-1).min(1).mean()) < 1e-13
    assert abs(r["dist_loss"] - 40 * (5 * r["cd"] + 3 * r["knn"])) < 1e-12


def _clip_rows_plain(adv, ori, normal, budget=0.1):
    """clip_utils.py:83-112 and 54-59 one row at a time in plain float64 arithmetic."""
    out = np.zeros_like(adv, dtype=np.float64)
    for i in range(len(adv)):
        d = adv[i].astype(np.float64) - ori[i]
        if normal is not None:
            n = normal[i].astype(np.float64)
            if d @ n < 0:
                vng = np.cross(n, d)
                vref = np.cross(vng, n)
                proj = d * vref / (np.sqrt((vref ** 2).sum()) + 1e-9)
                d = np.zeros(3) if np.sqrt((vng ** 2).sum()) < 1e-6 else proj
        d = d * min(budget / (np.sqrt((d ** 2).sum()) + 1e-9), 1.)
        out[i] = ori[i] + d
    return out


def test_oracle_project_clip_on_crafted_rows():
    adv, ori, nrm = KO.crafted_rows()
    got, dn = KO.project_clip_rows(adv, ori, nrm)
    assert np.allclose(got, _clip_rows_plain(adv, ori, nrm), rtol=0, atol=1e-15)
    d_in, d_out = adv.astype(np.float64) - ori, got - ori
    row = {k: i for i, k in enumerate(KO.CRAFTED)}
    assert (dn[[row["inward"], row["anti-parallel"], row["inward and far over"]]] < 0).all()
    assert (dn[[row["outward"], row["on the budget"], row["far over"]]] > 0).all() and dn[row["zero"]] == 0
    for k in ("outward", "zero", "on the budget"):                      # untouched: not inward, not over the budget
        assert np.allclose(d_out[row[k]], d_in[row[k]], atol=1e-9), k
    assert np.array_equal(got[row["zero"]], ori[row["zero"]])
    assert np.array_equal(got[row["anti-parallel"]], ori[row["anti-parallel"]])      # |vng| < 1e-6: the displacement is dropped
    assert not np.allclose(d_out[row["inward"]], d_in[row["inward"]], atol=1e-3)     # projected (the element-wise product)
    for k in ("far over", "inward and far over"):
        assert abs(np.sqrt((d_out[row[k]] ** 2).sum()) - 0.1) < 1e-8, k
    assert np.allclose(d_out[row["far over"]], d_in[row["far over"]] * 0.1 / np.sqrt((d_in[row["far over"]] ** 2).sum()), atol=1e-8)
    assert (np.sqrt((d_out ** 2).sum(1)) <= 0.1 * (1 + 1e-6)).all()
    # without normals: the clip alone
    got3, dn3 = KO.project_clip_rows(adv, ori, None)
    assert dn3 is None and np.allclose(got3, _clip_rows_plain(adv, ori, None), rtol=0, atol=1e-15)
    assert np.allclose(got3[row["inward"]], adv[row["inward"]], atol=1e-9)


# ---------------------------------------------------------------------------------------------- ABI
def declared_symbols(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


def test_knn_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols(HEADER)
    assert names == sorted(_lib.KNN_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert lib.ifd_knn_abi_version() == 1 == _lib.KNN_ABI_VERSION
    assert ctypes.sizeof(_lib.IfdKnnParams) == 40 and ctypes.sizeof(_lib.IfdKnnDiag) == 40
    hdr = open(HEADER).read()
    assert "#define IFD_KNN_MAX_POINTS %d" % _lib.KNN_MAX_POINTS in hdr and "#define IFD_KNN_MIN_POINTS %d" % _lib.KNN_MIN_POINTS in hdr
    # the headers the new one builds on are as they were
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_cw.h"))) == 4 and lib.ifd_cw_abi_version() == 1
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_atk.h"))) == 4 and lib.ifd_atk_abi_version() == 1


def test_knn_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_knn_step(None, None, None, None, None, None, None, None, None, 1, 0.001, 1.0, None, None, 1, 8, None) == -1
    assert lib.ifd_knn_project_clip(None, None, None, None, 0.1, None, 1, 8, None) == -1
    assert lib.ifd_knn_attack(None, None, None, None, None, None, None, 1, 8, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- host logic
class StubClassifier:
    """Stands in for runtime.Classifier on the CPU.  A cloud is predicted as its target from iteration `hit` on, except the last
    cloud of a batch, which never is; a step moves the cloud by 0.01 in x and reports adversarial loss 2 and distance loss 7."""
    device = "cpu"

    def __init__(self, hit=2):
        self.calls, self.closed, self.hit, self.it = [], False, hit, 0

    def knn_attack(self, pc, target, normal, noise, loss, kappa, scale, lr, num_iter, **hyper):
        self.calls.append(("attack", tuple(pc.shape), None if normal is None else normal.clone(), noise.clone(), loss, kappa, scale, lr, num_iter,
                           hyper, pc.clone()))
        ok = torch.as_tensor(target) == 3
        return pc + 1.0, torch.where(ok, torch.as_tensor(target), torch.as_tensor(target) + 1), ok

    def _pred(self, target):
        pred = target.clone() if self.it >= self.hit else target + 1
        pred[-1] = target[-1] + 1
        return pred

    def input_grad(self, pc, target, loss, kappa, scale, want_aux=False):
        return torch.zeros_like(pc), {"pred": self._pred(target), "loss": torch.full((len(pc),), 2.0)}

    def knn_step(self, grad, adv, ori, m, v, t, lr, scale, normal=None, loss=None, want=(), **hyper):
        self.calls.append(("step", t, lr, scale, normal is not None, tuple(want), hyper))
        assert t == self.it + 1 and float(loss[0]) == 2.0
        adv[:, 0, 0] -= 0.01
        self.it += 1
        return {"info": torch.tensor([[2.0, 0.5, 0.25, 7.0]] * len(adv))} if "info" in want else {}

    def predict(self, pc):
        self.calls.append(("predict",))
        return self._pred(self.target)

    def close(self):
        self.closed = True


def _attack_file(path, n=6, k=40, cols=6):
    rng = np.random.default_rng(3)
    np.savez(path, test_pc=rng.standard_normal((n, k, cols)).astype(np.float32), test_label=np.arange(n).astype(np.uint8),
             target_label=np.array([3, 3, 3, 5, 5, 3][:n], np.uint8))


def test_cli_batches_noise_and_file(tmp_path, capsys):
    from ifdefense_amd import knn_attack as KA
    from ifdefense_amd.inference import normalize_points_np
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    raw = np.load(src)["test_pc"]
    stub, made = StubClassifier(), []

    def make(model, ft, path):
        made.append((model, ft, path))
        return stub
    argv = ["--data_root", src, "--num_points", "32", "--num_iter", "7", "--batch_size", "4", "--kappa", "0.5", "--attack_lr", "0.02",
            "--out_dir", str(tmp_path), "--dataset", "opt_mn40", "--seed", "5"]
    assert KA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("pointnet", False, "pretrain/opt_mn40/pointnet.pth")] and stub.closed
    assert out.count("Successfully attack 3/4") == 1 and out.count("Successfully attack 1/2") == 1 and "Iteration" not in out
    assert "no normals" not in out
    # two reference batches (4 + 2 clouds): one library call each, scale = 1 / batch, the reference's hyper-parameters
    a, b = stub.calls
    assert a[1] == (4, 32, 3) and b[1] == (2, 32, 3)
    assert a[4:9] == ("logits", 0.5, 0.25, 0.02, 7) and b[6] == 0.5
    assert a[9] == dict(chamfer_weight=5., knn_weight=3., alpha=1.05, budget=0.1)
    # every cloud is pc[:32, :6]: the points normalised to the unit sphere, the normals as they are
    assert torch.equal(a[2], torch.from_numpy(raw[:4, :32, 3:])) and torch.equal(b[2], torch.from_numpy(raw[4:, :32, 3:]))
    want = np.stack([normalize_points_np(c[:32, :3]) for c in raw[:4]])
    assert np.array_equal(a[10].numpy(), want) and abs(np.sqrt((want ** 2).sum(-1)).max(1) - 1).max() < 1e-6
    # the noise: one draw per batch, of the reference's size, from the seeded generator
    na, nb = a[3], b[3]
    assert tuple(na.shape) == (4, 32, 3) and tuple(nb.shape) == (2, 32, 3) and na.dtype == torch.float32
    assert 0 < float(na.abs().max()) < 1e-6 and 1e-8 < float(na.std()) < 2e-7 and not torch.equal(na[:2], nb)
    gen = torch.Generator().manual_seed(5)
    assert torch.equal(na, torch.randn(4, 32, 3, generator=gen) * 1e-7) and torch.equal(nb, torch.randn(2, 32, 3, generator=gen) * 1e-7)
    d = tmp_path / "attack" / "results" / "opt_mn40_32" / "kNN"
    name = "kNN-pointnet-logits_kappa=0.5-success_%.4f-rank_0.npz" % (4 / 6)
    assert os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 32, 3)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8
    assert list(z["test_label"]) == list(range(6)) and list(z["target_label"]) == [3, 3, 3, 5, 5, 3]
    # cross_entropy names the file without kappa; -1: one batch; the reference's defaults
    stub.calls.clear()
    assert KA.main(["--data_root", src, "--num_points", "32", "--out_dir", str(tmp_path), "--adv_func", "cross_entropy", "--local_rank", "2"],
                   make_classifier=make) == 0
    (c,) = stub.calls
    assert c[1] == (6, 32, 3) and c[4:9] == ("cross_entropy", 15., pytest.approx(1 / 6), 1e-3, 2500)
    assert "kNN-pointnet-cross_entropy-success_%.4f-rank_2.npz" % (4 / 6) in os.listdir(tmp_path / "attack" / "results" / "mn40_32" / "kNN")
    # the same seed gives the same noise, another seed another
    first = c[3]
    stub.calls.clear()
    assert KA.main(["--data_root", src, "--num_points", "32", "--out_dir", str(tmp_path)], make_classifier=make) == 0
    assert torch.equal(stub.calls[0][3], first)
    stub.calls.clear()
    assert KA.main(["--data_root", src, "--num_points", "32", "--out_dir", str(tmp_path), "--seed", "6"], make_classifier=make) == 0
    assert not torch.equal(stub.calls[0][3], first)
    capsys.readouterr()


def test_cli_three_column_file_runs_without_projection(tmp_path, capsys):
    from ifdefense_amd import knn_attack as KA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src, cols=3)
    stub = StubClassifier()
    assert KA.main(["--data_root", src, "--num_points", "16", "--num_iter", "2", "--out_dir", str(tmp_path)], make_classifier=lambda *a: stub) == 0
    out = capsys.readouterr().out
    assert out.count("no normals") == 1 and "without the projection" in out
    (c,) = stub.calls
    assert c[1] == (6, 16, 3) and c[2] is None
    z = np.load(tmp_path / "attack" / "results" / "mn40_16" / "kNN" / ("kNN-pointnet-logits_kappa=15.0-success_%.4f-rank_0.npz" % (4 / 6)))
    assert z["test_pc"].shape == (6, 16, 3) and z["test_pc"].dtype == np.float32


def test_cli_refuses_what_is_not_built(capsys):
    from ifdefense_amd import knn_attack as KA

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--model", "dgcnn"], ["--model", "pointnet2"], ["--model", "pointconv"], ["--feature_transform", "true"]):
        assert KA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "not built" in capsys.readouterr().err
    assert KA.main(["--data_root", "x.npz", "--num_iter", "0"], make_classifier=never) != 0
    assert "at least 1" in capsys.readouterr().err
    from ifdefense_amd import attack as A
    with pytest.raises(ValueError, match="chamfer_knn"):
        A.CWKNN(None, dist_func="l2")
    with pytest.raises(ValueError, match="project_inner_clip_linf"):
        A.CWKNN(None, clip_func="clip_linf")
    with pytest.raises(ValueError, match="num_iter"):
        A.CWKNN(None, num_iter=0)
    with pytest.raises(ValueError, match=r"\[B,K,6\]"):
        A.CWKNN(StubClassifier(), verbose=False).attack(torch.zeros(2, 8, 4), [1, 2])
    assert sorted(A.ATTACKS) == ["fgm", "ifgm", "mifgm", "pgd"]


@pytest.mark.parametrize("num_iter,printed", [(10, [0, 2, 4, 6, 8]), (3, [0, 1, 2])])
def test_host_driven_loop_prints_the_reference_lines(capsys, num_iter, printed):
    """verbose=True: one input_grad and one knn_step an iteration, the reference's two lines every num_iter // 5 iterations (every
    iteration when num_iter < 5) with the batch means of the PREVIOUS iteration's losses, zeros at iteration 0; the diagnostics are
    asked for only in the iteration before a printing one; then one predict and the last line."""
    from ifdefense_amd import attack as A
    stub = StubClassifier(hit=2)
    stub.target = torch.tensor([1, 2, 3])
    x = torch.zeros(3, 8, 6)
    x[:, :, 5] = 1.0
    adv, n_ok = A.CWKNN(stub, num_iter=num_iter, attack_lr=0.03, seed=4, ref_batch=12).attack(x, [1, 2, 3])
    out = capsys.readouterr().out.splitlines()
    want = []
    for it in printed:
        want += ["Iteration %d/%d, success %d/3" % (it, num_iter, 2 if it >= 2 else 0),
                 "adv_loss: %.4f, dist_loss: %.4f" % ((2.0, 7.0) if it else (0.0, 0.0))]
    assert out == want + ["Successfully attack 2/3"] and n_ok == 2
    steps = [c for c in stub.calls if c[0] == "step"]
    assert len(steps) == num_iter and [c[1] for c in steps] == list(range(1, num_iter + 1))
    assert all(c[2] == 0.03 and c[3] == pytest.approx(1 / 12) and c[4] for c in steps)
    assert all(c[6] == dict(chamfer_weight=5., knn_weight=3., alpha=1.05, budget=0.1) for c in steps)
    every = max(num_iter // 5, 1)
    assert [c[5] for c in steps] == [("info",) if it % every == every - 1 else () for it in range(num_iter)]
    assert [c[0] for c in stub.calls if c[0] != "step"] == ["predict"]
    assert adv.shape == (3, 8, 3) and adv.dtype == np.float32 and np.allclose(adv[:, 0, 0], -0.01 * num_iter, atol=1e-6)
    # [B,K,3] data: the same loop without normals
    stub2 = StubClassifier(hit=0)
    stub2.target = torch.tensor([1, 2])
    A.CWKNN(stub2, num_iter=3, seed=4).attack(torch.zeros(2, 8, 3), [1, 2])
    assert [c[4] for c in stub2.calls if c[0] == "step"] == [False] * 3
    capsys.readouterr()
