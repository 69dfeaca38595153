"""CPU checks of the CW object-adding attack (include/ifd_object.h): the oracle against the recorded reference run, the host
initialisation against the recorded objects and centres, the closed-form gradient against autograd, the float32 remainder, the step
cases' conditions, the ABI and the CLI's host logic with a stub in place of the classifier.  No GPU is needed."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import cluster_oracle as KO
import objects_oracle as OO
import pointnet_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_object.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    return I.load_library()


@pytest.fixture(scope="module", autouse=True)
def object_abi(lib):
    """The oracle and the fixture are the yardsticks of THIS version of include/ifd_object.h: without it nothing here is judged."""
    assert lib.ifd_object_abi_version() == 1


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "objects_golden.npz"))


@pytest.fixture(scope="module")
def oracle_runs(sd, golden):
    """(float32 run, float64 run) of the oracle on the fixture's inputs, recorded objects, centres and draws, free-running."""
    g = golden
    kw = dict(binary_step=int(g["binary_step"]), num_iter=int(g["num_iter"]), lr=float(g["attack_lr"]),
              init_weight=float(g["init_weight"]), max_weight=float(g["max_weight"]))
    return tuple(OO.attack(PO.to_torch(sd, dt), g["data"], g["target"], g["objects"], g["centers"], g["noise_obj"], g["noise_shift"],
                           g["angles0"], dt, **kw) for dt in (torch.float32, torch.float64))


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_reproduces_the_recorded_reference(golden, oracle_runs):
    """tests/golden/objects_golden.npz: the reference's CWAddObjects (L2ChamferDist(3, 'adv2ori', 0.2), LogitsAdvLoss(0), init_weight 5,
    max_weight 40) on its own PointNetCls with the calibrated weights and its own airplane.npy, 4 clouds x 192 points, 3 objects of 64,
    3 search steps x 20 iterations, with the objects, the centres and the three draws of every search step captured from the run
    (tests/golden/make_golden_objects.py).  The float32 oracle, fed those, must give the reference's success count and its whole
    weight / lower / upper history EXACTLY, and o_bestdist and the final clouds to within 4 x the float32 oracle's own distance from
    the float64 oracle on the same fixture (test_add_cpu's and test_cluster_cpu's bars).  Measured: f32 oracle vs f64 oracle o_bestdist
    4.5e-03, clouds 3.3e-01 - the float64 oracle does not take the recorded weight history (printed, not asserted): a hit that
    float32 rounding decides falls the other way in one search step and the trajectories part - while the f32 oracle is within 2.6e-08
    and 2.7e-06 of the recording: it tracks the recording far closer than the bar asks; the rule is kept."""
    g, (a32, a64) = golden, oracle_runs
    K, A = g["data"].shape[1], int(g["num_add"]) * int(g["obj_num_p"])
    roles = list(g["roles"])
    assert "up_down" in roles and "never" in roles and "success" in roles and int(g["success_num"]) >= 1
    lower = g["history"][-1, :, 1]
    assert np.array_equal(a32["success"], lower > 0) and a32["success_num"] == int(g["success_num"])
    assert np.array_equal(a32["history"], g["history"])
    print("the float64 oracle takes the recorded weight history: %s" % np.array_equal(a64["history"], g["history"]))
    ok = lower > 0
    rec_att = g["o_bestattack"]
    assert rec_att.shape == (len(ok), K + A, 3)
    for run in (a32, a64):
        assert np.array_equal(run["o_bestattack"][:, :K].astype(np.float32), g["data"])
    e_dist = np.abs(a32["o_bestdist"] - a64["o_bestdist"])[ok].max()
    e_att = np.abs(a32["o_bestattack"].astype(np.float64) - a64["o_bestattack"]).max()
    d_dist = np.abs(a32["o_bestdist"] - g["o_bestdist"])[ok].max()
    d_att = np.abs(a32["o_bestattack"].astype(np.float64) - rec_att).max()
    print("f32 oracle vs f64 oracle: o_bestdist %.3e, clouds %.3e; f32 oracle vs the recording: %.3e, %.3e" % (e_dist, e_att, d_dist, d_att))
    assert e_dist > 0 and e_att > 0
    assert d_dist <= 4 * e_dist and d_att <= 4 * e_att
    for b in np.nonzero(~ok)[0]:                                       # never successful: the untouched 1e10
        assert g["o_bestdist"][b] == 1e10 == a32["o_bestdist"][b]


def test_closed_form_gradient_is_autograd_in_float64():
    """The header's step 5 against autograd through the reference's form, on objects, shifts and angles, to 1e-12."""
    for name, t in (("ref", 1), ("ragged", 7), ("single", 7), ("pairs", 1)):
        case = OO.make_step_case(name, t)
        r64 = OO.run_step_case(case, torch.float64)
        for b, r in enumerate(r64):
            n, A = int(case["n_ori"][b]), case["A"]
            g = OO.closed_form_grad(case["obj"][b], case["shift"][b], case["angle"][b], case["objects"], case["ori"][b, :n],
                                    case["grad"][b, n:n + A], case["weight"][b], OO.STEP_SCALE, r["nn"])
            for mine, auto in zip(g, (r["obj_grad"], r["g_shift"], r["g_angle"])):
                assert np.abs(mine - auto).max() <= 1e-12, (name, t, b)


def test_remainder_is_torchs():
    x = np.array([-0.5, 7.0, OO.TWO_PI + 0.5, -0.0, np.float32(OO.TWO_PI)], np.float32)
    want = torch.remainder(torch.from_numpy(x), OO.TWO_PI).numpy()
    got = OO.remainder32(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want.view(np.uint32), (torch.from_numpy(x) % OO.TWO_PI).numpy().view(np.uint32))
    assert got[4] == 0 and np.signbit(got[3]) and got[0] > 5 and (got[[0, 1, 2, 4]] >= 0).all() and (got < np.float32(OO.TWO_PI)).all()


@pytest.mark.parametrize("name", [c[0] for c in OO.STEP_CASES])
def test_step_cases_meet_their_conditions(name):
    """The cases of the GPU parity test, judged by the oracles alone: at most 5 % of the rows undecidable, the oracles agree on every
    judged nearest original, no new angle at the wrap-around, every quantity's float32 error is measurable, and the crafted angles
    are there: within 1e-3 of 0 and of 2 pi, crossing the wrap-around in the step."""
    for t in (1, 7):
        case = OO.make_step_case(name, t)
        r32, r64 = OO.run_step_case(case, torch.float32), OO.run_step_case(case, torch.float64)
        J = OO.judge(case, r32, r64)
        print("%s t=%d: e_min %.2e, rows excluded %.2f %%, e32 %s" % (name, t, J["e_min"], 100 * J["share"],
                                                                       {k: "%.1e" % x for k, x in J["e32"].items()}))
        assert 0 < J["e_min"] < 1e-5 and all(J["e32"][k] > 0 for k in OO.QUANTITIES if not (t == 1 and k in OO.MOMENTS))
        near = (case["angle"] < 1e-3) | (case["angle"] > OO.TWO_PI - 1e-3)
        assert near.any() and (case["angle"] >= 0).all() and (case["angle"] < np.float32(OO.TWO_PI)).all()
        new = np.stack([r["angle"] for r in r64])
        assert (np.abs(new - case["angle"])[near] > 3).any() or t == 1 or name == "wide"      # a wrap moves the value by 2 pi


# ---------------------------------------------------------------------------------------------- the host start
def test_host_start_reproduces_the_recorded_objects_and_centres(golden):
    from ifdefense_amd import attack as A
    g = golden
    na, P = int(g["num_add"]), int(g["obj_num_p"])
    raw = g["object_raw"].copy()
    rng = np.random.RandomState(int(g["seed"]))
    objects = A.prepare_objects(raw, float(g["scaling"]), na, P, rng)
    assert objects.dtype == np.float64 and np.array_equal(objects, g["objects"]) and np.array_equal(raw, g["object_raw"])
    centers = np.stack([A.init_centers(g["cri"][b], g["labels"][b], na, rng) for b in range(len(g["data"]))])
    assert np.array_equal(centers, g["centers"]) and centers.dtype == np.float32
    # the last cloud has one cluster only: its first centre is that cluster's, the other two are the fallback's draws
    lab = g["labels"][-1]
    assert len(np.unique(lab[lab >= 0])) < na
    # a float64 object stays float64 arithmetic and gives other numbers in the last place
    assert not np.array_equal(A.prepare_objects(raw.astype(np.float64), 0.3, na, P, np.random.RandomState(int(g["seed"]))), objects)


def test_host_start_where_the_reference_raises_or_leaves_the_order_open():
    from ifdefense_amd import attack as A
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((128, 3)).astype(np.float32)
    # every point an outlier: all of them are fallback candidates, drawn with the reference's call
    out = A.init_centers(pts, np.full(128, -1), 3, np.random.RandomState(4))
    r = np.random.RandomState(4)
    assert np.array_equal(out, np.stack([pts[r.choice(128, 1)[0]] for _ in range(3)]))
    # equal counts: the stable argsort keeps the label order among them, so the LAST num_add labels in (count, label) order are taken
    lab = np.repeat(np.arange(4), 32)
    out = A.init_centers(pts, lab, 2, np.random.RandomState(0))
    for c, one in zip(out, (2, 3)):
        q = pts[lab == one]
        assert np.array_equal(c, q[np.argmin(np.sum((q - q.mean(0)[None]) ** 2, axis=1))])
    for bad in (np.zeros((10, 3), np.float32) + 1, np.zeros((70, 2), np.float32), np.zeros((64,), np.float32), np.ones((70, 3), np.float32)):
        with pytest.raises(ValueError):
            A.prepare_objects(bad, 0.3, 3, 64, np.random.RandomState(0))
    ok = A.prepare_objects(rng.standard_normal((64, 3)).astype(np.float32), 0.3, 3, 64, np.random.RandomState(0))
    assert ok.shape == (3, 64, 3) and abs(np.sqrt((ok ** 2).sum(2)).max() - 0.3) < 1e-6


def test_numpy_dbscan_gives_the_recorded_sklearn_labels(golden):
    for b in range(len(golden["cri"])):
        assert KO.eps_margin(golden["cri"][b]) > KO.BAND
        lab, n = KO.dbscan(golden["cri"][b])
        assert np.array_equal(lab, golden["labels"][b]) and n == len(np.unique(lab[lab >= 0]))


# ---------------------------------------------------------------------------------------------- ABI
def declared_symbols(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


def defined(path, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read()).group(1))


def test_object_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols(HEADER)
    assert names == sorted(_lib.OBJECT_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert lib.ifd_object_abi_version() == 1 == _lib.OBJECT_ABI_VERSION == defined(HEADER, "IFD_OBJECT_ABI_VERSION")
    # ifd_object_state: ifd_cw_state (10 pointers) + 7 pointers; ifd_object_diag: 6 pointers; ifd_object_params: 6 int32 + 5 float
    assert ctypes.sizeof(_lib.IfdObjectState) == ctypes.sizeof(_lib.IfdCwState) + 56 == 136
    assert ctypes.sizeof(_lib.IfdObjectDiag) == 48 and ctypes.sizeof(_lib.IfdObjectParams) == 44
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for struct, cls in (("ifd_object_state", _lib.IfdObjectState), ("ifd_object_diag", _lib.IfdObjectDiag), ("ifd_object_params", _lib.IfdObjectParams)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, flags=re.S).group(1)
        members = [m for line in body.split(";") for m in re.findall(r"\*?\s*([a-z_0-9]+)\s*(?:,|$)", line.strip().split(" ", 1)[-1]) if line.strip()]
        assert members == [f[0] for f in cls._fields_], (struct, members)
    # the headers the new one builds on are as they were
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_add.h"))) == 5 and lib.ifd_add_abi_version() == 1
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_cw.h"))) == 4 and lib.ifd_cw_abi_version() == 1
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_cluster.h"))) == 4 and lib.ifd_cluster_abi_version() == 1
    for k in ("object_state", "object_place", "object_step", "object_attack"):
        assert callable(getattr(I.Classifier, k))
    src = "".join(open(os.path.join(ROOT, "if-defense_amd", f)).read() for f in ("attack.py", "object_attack.py", "attack_cli.py"))
    assert "sklearn" not in src.replace("sklearn's", "")              # named in the docstrings only, never imported


def test_object_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_object_place(None, None, None, None, None, None, 1, 8, 1, 2, None) == -1
    assert lib.ifd_object_step(None, None, None, None, None, None, None, None, None, None, None, None, 1, 0.01, 1.0, 1, 8, 1, 2, None) == -1
    assert lib.ifd_object_attack(None, None, None, None, None, None, None, None, None, None, 1, 8, 10, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- host logic
class StubClassifier:
    """Stands in for runtime.Classifier on the CPU.  The critical points are the cloud's first 128 rows, their labels: rows 0 - 39
    cluster 0, 40 - 59 cluster 1, the rest outliers.  The library call succeeds on the clouds whose target is 3."""
    device = "cpu"

    def __init__(self):
        self.calls, self.closed = [], False

    def add_critical_points(self, pc, target, num_add, scale):
        self.calls.append(("critical", tuple(pc.shape), num_add, scale))
        return pc[:, :num_add].clone()

    def cluster_dbscan(self, pts, eps, min_samples):
        self.calls.append(("dbscan", tuple(pts.shape), eps, min_samples))
        lab = torch.full(pts.shape[:2], -1, dtype=torch.int32)
        lab[:, :40], lab[:, 40:60] = 0, 1
        return lab

    def object_attack(self, pc, target, objects, centers, angles0, noise_obj, noise_shift, loss, kappa, scale, lr, init_weight, max_weight,
                      binary_step, num_iter):
        self.calls.append(("attack", tuple(pc.shape), objects.clone(), centers.clone(), angles0.clone(), noise_obj.clone(), noise_shift.clone(),
                           loss, kappa, scale, lr, init_weight, max_weight, binary_step, num_iter))
        ok = torch.as_tensor(target) == 3
        A = objects.shape[0] * objects.shape[1]
        return torch.cat([pc, objects.reshape(1, A, 3).expand(len(pc), A, 3) + 1.0], 1), torch.where(ok, 0.5, 1e10).float(), ok

    def close(self):
        self.closed = True


def _attack_file(path, n=6, k=140):
    rng = np.random.default_rng(3)
    np.savez(path, test_pc=rng.standard_normal((n, k, 3)).astype(np.float32), test_label=np.arange(n).astype(np.uint8),
             target_label=np.array([3, 3, 3, 5, 5, 3][:n], np.uint8))


def test_cli_batches_randomstate_draws_and_file(tmp_path, capsys, golden):
    from ifdefense_amd import attack as A, attack_cli, object_attack as OA
    src, obj = str(tmp_path / "attack_data.npz"), str(tmp_path / "airplane.npy")
    _attack_file(src)
    np.save(obj, golden["object_raw"])
    stub, made = StubClassifier(), []

    def make(model, ft, path):
        made.append((model, ft, path))
        return stub
    argv = ["--data_root", src, "--obj_root", obj, "--num_points", "130", "--num_add", "3", "--obj_num_p", "24", "--binary_step", "3",
            "--num_iter", "7", "--batch_size", "4", "--kappa", "0.5", "--attack_lr", "0.02", "--out_dir", str(tmp_path), "--dataset", "opt_mn40",
            "--seed", "5"]
    assert OA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("pointnet", False, "pretrain/opt_mn40/pointnet.pth")] and stub.closed
    assert out.count("Successfully attack 3/4") == 1 and out.count("Successfully attack 1/2") == 1 and "Step 0" not in out
    assert [c[0] for c in stub.calls] == ["critical", "dbscan", "attack"] * 2
    assert stub.calls[0] == ("critical", (4, 130, 3), 128, 0.25) and stub.calls[3] == ("critical", (2, 130, 3), 128, 0.5)
    assert stub.calls[1] == ("dbscan", (4, 128, 3), 0.2, 3)
    a, b = stub.calls[2], stub.calls[5]
    assert a[1] == (4, 130, 3) and b[1] == (2, 130, 3)
    assert a[7:] == ("logits", 0.5, 0.25, 0.02, 5., 40., 3, 7) and b[9] == 0.5
    # ONE RandomState(seed): the object's shuffles first, then the fallback draws, carried across the clouds AND the batches
    data = attack_cli.load_points(np.load(src), 130)
    rng = np.random.RandomState(5)
    objects = A.prepare_objects(golden["object_raw"], 0.3, 3, 24, rng)
    assert np.array_equal(a[2].numpy(), objects.astype(np.float32)) and torch.equal(a[2], b[2]) and a[2].dtype == torch.float32
    lab = np.full(128, -1)
    lab[:40], lab[40:60] = 0, 1
    want = np.stack([A.init_centers(c[:128], lab, 3, rng) for c in data])
    assert np.array_equal(a[3].numpy(), want[:4]) and np.array_equal(b[3].numpy(), want[4:]) and a[3].dtype == torch.float32
    # the draws: per search step randn [B,A,3], randn [B,3,3], rand [B,3,3] * pi of which component 0 is kept
    gen = torch.Generator().manual_seed(5)
    for call, B in ((a, 4), (b, 2)):
        no, ns, an = [], [], []
        for _ in range(3):
            no.append(torch.randn(B, 72, 3, generator=gen) * 1e-7)
            ns.append(torch.randn(B, 3, 3, generator=gen) * 1e-7)
            an.append((torch.rand(B, 3, 3, generator=gen) * np.pi)[..., 0])
        assert torch.equal(call[5], torch.stack(no)) and torch.equal(call[6], torch.stack(ns)) and torch.equal(call[4], torch.stack(an))
        assert float(call[4].min()) >= 0 and float(call[4].max()) < np.pi + 1e-6
    d = tmp_path / "attack" / "results" / "opt_mn40_130" / "Object" / "3-24"
    name = "Object-pointnet-logits_kappa=0.5-success_%.4f-rank_0.npz" % (4 / 6)
    assert os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 130 + 72, 3) and np.array_equal(z["test_pc"][:, :130], data)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8
    assert list(z["test_label"]) == list(range(6)) and list(z["target_label"]) == [3, 3, 3, 5, 5, 3]
    # cross_entropy names the file without kappa; -1: one batch; the rank names the file
    stub.calls.clear()
    assert OA.main(argv + ["--batch_size", "-1", "--adv_func", "cross_entropy", "--local_rank", "2"], make_classifier=make) == 0
    assert [c[0] for c in stub.calls] == ["critical", "dbscan", "attack"] and stub.calls[2][1] == (6, 130, 3) and stub.calls[2][7] == "cross_entropy"
    assert "Object-pointnet-cross_entropy-success_%.4f-rank_2.npz" % (4 / 6) in os.listdir(d)
    # the defaults and the file name are the reference script's
    args = OA.build_parser().parse_args([])
    assert (args.num_add, args.obj_num_p, args.binary_step, args.num_iter, args.attack_lr, args.batch_size, args.obj_root) == \
        (3, 64, 5, 500, 1e-2, -1, "data/airplane.npy")
    assert OA.save_path(".", "mn40", 1024, 3, 64, "pointnet", "logits", 0.0, 0.5, 0) == \
        (os.path.join(".", "attack", "results", "mn40_1024", "Object", "3-64"), "Object-pointnet-logits_kappa=0.0-success_0.5000-rank_0.npz")
    assert (OA.INIT_WEIGHT, OA.MAX_WEIGHT, OA.SCALING) == (5., 40., 0.3)


def test_cli_and_class_refuse_what_is_not_built(tmp_path, capsys, golden):
    from ifdefense_amd import object_attack as OA

    def never(*a):
        raise AssertionError("the classifier must not be made")
    obj = str(tmp_path / "airplane.npy")
    np.save(obj, golden["object_raw"])
    base = ["--data_root", "x.npz", "--obj_root", obj]
    for argv in (["--model", "dgcnn"], ["--model", "pointnet2"], ["--model", "pointconv"], ["--feature_transform", "true"]):
        assert OA.main(base + argv, make_classifier=never) == 2
        assert "not built" in capsys.readouterr().err
    for argv in (["--binary_step", "0"], ["--num_iter", "0"]):
        assert OA.main(base + argv, make_classifier=never) == 2
        assert "at least 1" in capsys.readouterr().err
    for argv in (["--num_add", "0"], ["--obj_num_p", "0"], ["--num_add", "17"], ["--num_add", "1025", "--obj_num_p", "1"], ["--num_points", "127"],
                 ["--num_points", "2049"]):
        assert OA.main(base + argv, make_classifier=never) == 2
        assert "needed" in capsys.readouterr().err
    # the object file: missing, not [M,3], too short, not an array of floats
    files = {"flat.npy": np.zeros(30, np.float32), "wide.npy": np.zeros((100, 4), np.float32), "short.npy": golden["object_raw"][:63],
             "ints.npy": np.zeros((100, 3), np.int32)}
    for name, arr in files.items():
        np.save(str(tmp_path / name), arr)
    open(str(tmp_path / "text.npy"), "w").write("not an array")
    for name in ["missing.npy", "text.npy"] + list(files):
        assert OA.main(["--data_root", "x.npz", "--obj_root", str(tmp_path / name)], make_classifier=never) == 2, name
        assert "--obj_root" in capsys.readouterr().err
    from ifdefense_amd import attack as A
    raw = golden["object_raw"]
    with pytest.raises(ValueError, match="l2_chamfer"):
        A.CWAddObjects(None, raw, dist_func="chamfer")
    for kw in ({"num_add": 0}, {"obj_num_p": 0}, {"num_add": 17}, {"binary_step": 0}, {"num_iter": 0}, {"obj_num_p": 1025, "num_add": 1}):
        with pytest.raises(ValueError):
            A.CWAddObjects(None, raw, **kw)
    with pytest.raises(ValueError, match="fewer than obj_num_p"):
        A.CWAddObjects(None, raw[:63])
    with pytest.raises(ValueError, match=r"\[M,3\]"):
        A.CWAddObjects(None, raw[:, :2])
    with pytest.raises(ValueError, match="between 128 and 2048"):
        A.CWAddObjects(StubClassifier(), raw).attack(torch.zeros(2, 127, 3), [1, 2])
    assert sorted(A.ATTACKS) == ["fgm", "ifgm", "mifgm", "pgd"]
