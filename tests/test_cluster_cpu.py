"""CPU checks of the CW cluster-adding attack (include/ifd_cluster.h): the test oracle (tests/cluster_oracle.py) against a run of the
reference's own CWAddClusters recorded in tests/golden/cluster_golden.npz, the numpy DBSCAN against sklearn and against the
recorded labels, the host initialisation against the recorded clusters, the closed form of the distance term's gradient, the
(i, j) / (j, i) near-tie, the conditions of the GPU parity cases, the C ABI and its binding, refusals that need no GPU, and the
host logic of the cluster_attack CLI and of attack.CWAddClusters under a stub classifier."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import cluster_oracle as KO
import pointnet_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_cluster.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    return I.load_library()


@pytest.fixture(scope="module", autouse=True)
def cluster_abi(lib):
    """The oracle and the fixture are the yardsticks of THIS version of include/ifd_cluster.h: without it nothing here is judged."""
    assert lib.ifd_cluster_abi_version() == 1


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "cluster_golden.npz"))


@pytest.fixture(scope="module")
def oracle_runs(sd, golden):
    """(float32 run, float64 run) of the oracle on the fixture's inputs, recorded clusters and recorded noise, free-running."""
    g = golden
    A = int(g["num_add"]) * int(g["cl_num_p"])
    kw = dict(binary_step=int(g["binary_step"]), num_iter=int(g["num_iter"]), lr=float(g["attack_lr"]),
              init_weight=float(g["init_weight"]), max_weight=float(g["max_weight"]))
    return tuple(KO.attack(PO.to_torch(sd, dt), g["data"], g["target"], g["clusters"].reshape(len(g["data"]), A, 3), g["noise"],
                           int(g["num_add"]), int(g["cl_num_p"]), dt, **kw) for dt in (torch.float32, torch.float64))


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_reproduces_the_recorded_reference(golden, oracle_runs):
    """tests/golden/cluster_golden.npz: the reference's CWAddClusters (FarChamferDist(3, 'adv2ori', 0.1), LogitsAdvLoss(0), init_weight
    5, max_weight 30) on its own PointNetCls with the calibrated weights, 4 clouds x 192 points, 3 clusters of 32, 3 search steps x 20
    iterations, with the start clusters and the start noise of every search step captured from the run
    (tests/golden/make_golden_cluster.py).  The float32 oracle, fed those, must give the reference's success count and its whole
    weight / lower / upper history EXACTLY, and o_bestdist and the final clouds to within 4 x the float32 oracle's own distance from
    the float64 oracle on the same fixture (test_add_cpu's bars).  The measured figures are printed.  As for test_add_cpu's Hausdorff
    run, the float64 oracle need not take the recorded weight history (printed, not asserted): from the 1e-7 start every pair of a
    cluster that started on one critical point is 1e-7 apart, and which of them is the farthest is decided by float32 rounding that
    float64 does not have; the trajectories part there, and the bars are then as wide as that."""
    g, (a32, a64) = golden, oracle_runs
    K, A = g["data"].shape[1], int(g["num_add"]) * int(g["cl_num_p"])
    roles = list(g["roles"])
    assert "up_down" in roles and int(g["success_num"]) >= 1
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


# ---------------------------------------------------------------------------------------------- DBSCAN and the initialisation
def test_numpy_dbscan_is_sklearn_outside_the_rounding_band():
    """The header's rule against sklearn.cluster.DBSCAN(0.2, min_samples=3).fit_predict, label for label, on random clouds of 1 to 7
    blobs with sigma 0.05 to 0.25 in which no pair has |d^2 - 0.04| <= 4 * 2^-24 in float64 (inside that band the decision is
    float32's own and is not judged)."""
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(11)
    done = 0
    for _ in range(60):
        p = KO.blob_cloud(rng)
        if KO.eps_margin(p) <= KO.BAND:
            continue
        want = cluster.DBSCAN(KO.EPS, min_samples=KO.MIN_SAMPLES).fit_predict(p)
        got, n_clusters = KO.dbscan(p)
        assert np.array_equal(got, want) and n_clusters == want.max() + 1
        done += 1
    assert done >= 50


def test_numpy_dbscan_gives_the_recorded_sklearn_labels(golden):
    for b in range(len(golden["cri"])):
        assert KO.eps_margin(golden["cri"][b]) > KO.BAND
        got, n_clusters = KO.dbscan(golden["cri"][b])
        assert np.array_equal(got, golden["labels"][b]) and n_clusters == golden["labels"][b].max() + 1


def test_dbscan_definition_on_crafted_clouds():
    """Three mutual neighbours are exactly min_samples; a border point within eps of cores of two clusters takes the lower label;
    a non-core point without a core neighbour is -1 even next to another non-core point."""
    f = lambda *rows: np.array(rows, np.float32)                       # noqa: E731
    assert KO.dbscan(f([0, 0, 0]))[0].tolist() == [-1]
    assert KO.dbscan(f([0, 0, 0], [0.1, 0, 0]))[0].tolist() == [-1, -1]
    assert KO.dbscan(f([0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]))[0].tolist() == [0, 0, 0]
    assert KO.dbscan(f([0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]), min_samples=4)[0].tolist() == [-1, -1, -1]
    pts, want = KO.border_cloud()
    lab, n = KO.dbscan(pts, min_samples=4)
    assert n == 2 and np.array_equal(lab, want)
    lab, n = KO.dbscan(pts[::-1].copy(), min_samples=4)                # reversed: the other group comes first and takes the border point
    assert n == 2 and lab.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0]


def test_host_initialisation_reproduces_the_recorded_clusters(golden):
    """Fed the recorded critical points and labels and ONE RandomState(seed) carried over the clouds, the oracle's init_centers and
    the library's attack.init_clusters give the reference's clusters exactly; the fixture holds a draw with replacement, one
    without and two fallbacks."""
    from ifdefense_amd import attack as A
    g = golden
    num_add, P = int(g["num_add"]), int(g["cl_num_p"])
    for fn in (KO.init_centers, A.init_clusters):
        rng = np.random.RandomState(int(g["seed"]))
        got = np.stack([fn(g["cri"][b], g["labels"][b], num_add, P, rng) for b in range(len(g["cri"]))])
        assert got.dtype == np.float32 and np.array_equal(got, g["clusters"])
    counts = [np.unique(l[l >= 0], return_counts=True)[1] for l in g["labels"]]
    assert any(len(c) >= num_add and c.max() <= P for c in counts) and any(len(c) == 1 and c[0] > P for c in counts)


def test_host_initialisation_where_the_reference_raises():
    from ifdefense_amd import attack as A
    pts = np.random.default_rng(0).standard_normal((128, 3)).astype(np.float32)
    for fn in (KO.init_centers, A.init_clusters):
        out = fn(pts, np.full(128, -1), 3, 32, np.random.RandomState(1))       # all outliers: every point is a candidate
        assert out.shape == (3, 32, 3) and all((o[:, None] == pts[None]).all(2).any(1).all() for o in out)
        lab = np.full(128, -1)
        lab[:5] = 0
        out = fn(pts, lab, 2, 8, np.random.RandomState(1))             # one cluster of 5 < cl_num_p: with replacement, then the
        assert out.shape == (2, 8, 3)                                  # fallback's 5 sorted candidates repeated cyclically
        assert np.array_equal(out[1][:3], out[1][5:8]) and len(np.unique(out[1], axis=0)) == 5


# ---------------------------------------------------------------------------------------------- the step
def test_closed_form_gradient_is_autograd_in_float64():
    """The header's step 4 against autograd through the reference's form, float64, to 1e-12; the arg-max is the ordered pair that
    torch's two max return; Adam is the real torch.optim.Adam; the record is strict."""
    rng = np.random.default_rng(1)
    ori = rng.standard_normal((40, 3)) * 0.5
    adv = np.repeat(ori[rng.permutation(40)[:3]], 4, axis=0) + 0.05 * rng.standard_normal((12, 3))
    grad, m = rng.standard_normal((12, 3)), rng.standard_normal((12, 3))
    v = rng.random((12, 3))
    w, scale = 17., 0.25
    p, m1, v1, r1, d, dl, diag = KO.step(grad, 3, 3, adv, ori, w, m, v, 7, 1e-2, scale, KO.fresh_record(12), 3)
    far = 0.
    for c in range(3):
        X = adv[4 * c:4 * c + 4]
        N = np.sqrt((((X[None, :, :] - X[:, None, :]) + 1e-7) ** 2).sum(2))        # N[i, j]
        j = int(N.max(0).argmax())
        i = int(N[:, j].argmax())
        assert (diag["far_i"][c], diag["far_j"][c]) == (4 * c + i, 4 * c + j) and abs(diag["far_val"][c] - N[i, j]) < 1e-14
        far += N[i, j]
    P = ((adv[:, None] - ori[None]) ** 2).sum(2)
    assert abs(d - (far + 0.1 * P.min(1).mean())) < 1e-13 and abs(dl - w * d) < 1e-11
    cf = KO.closed_form_grad(adv, ori, 3, w, scale, diag["nn"], diag["far_i"], diag["far_j"])
    assert np.abs(cf - diag["dist_grad"]).max() <= 1e-12
    g = grad + cf
    mm, vv = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
    want = adv - (1e-2 / (1 - 0.9 ** 7)) * mm / (np.sqrt(vv) / np.sqrt(1 - 0.999 ** 7) + 1e-8)
    assert np.allclose(p, want, rtol=0, atol=1e-12) and np.allclose(m1, mm, atol=1e-13) and np.allclose(v1, vv, atol=1e-12)
    assert r1["bestdist"] == d == r1["o_bestdist"] and r1["bestscore"] == 3 and np.array_equal(r1["o_bestattack"], adv)
    # a forced pair is taken as given: the other order flips the sign of the far term's gradient (up to the 1e-7)
    forced = np.stack([diag["far_j"], diag["far_i"]], 1)
    d2 = KO.step(grad, 3, 3, adv, ori, w, m, v, 7, 1e-2, scale, KO.fresh_record(12), 3, forced=forced)[6]
    assert np.array_equal(d2["far_i"], diag["far_j"]) and np.all(d2["far_val"] < diag["far_val"])
    cf2 = KO.closed_form_grad(adv, ori, 3, w, scale, diag["nn"], d2["far_i"], d2["far_j"])
    assert np.abs(cf2 - d2["dist_grad"]).max() <= 1e-12 and 0 < np.abs(cf2 - cf).max() < 1e-4
    # tied norms: torch's CPU max returns the lowest j, then the lowest i; cl_num_p == 1: i* == j*, no far gradient
    tie = np.array([[1., 0, 0], [-1., 0, 0], [1., 0, 0], [-1., 0, 0]])
    _, _, fi, fj, _ = KO.far_distance(torch.from_numpy(tie)[None], 1)
    assert (fi[0], fj[0]) == (1, 0)                                    # (p_0 - p_1) + 1e-7 is the longer of the two orders
    same = np.zeros((4, 3))
    _, fc, fi, fj, _ = KO.far_distance(torch.from_numpy(same)[None], 1)
    assert (fi[0], fj[0]) == (0, 0) and abs(float(fc[0]) - np.sqrt(3) * 1e-7) < 1e-20
    one = KO.step(grad[:3], 3, 3, adv[:3], ori, w, m[:3], v[:3], 7, 1e-2, scale, KO.fresh_record(3), 3)[6]
    assert np.array_equal(one["far_i"], [0, 1, 2]) and np.array_equal(one["far_j"], [0, 1, 2])
    assert np.abs(one["dist_grad"] - KO.closed_form_grad(adv[:3], ori, 3, w, scale, one["nn"], one["far_i"], one["far_j"])).max() <= 1e-12


def test_the_order_inside_the_farthest_pair_is_a_real_near_tie():
    """On the "ref" step case: the two orders of a cluster's farthest pair differ by 4e-7 sum_k d_k / (2 |d|) in float64, which is of
    the size of the float32 oracle's error of a norm - in a good share of the clusters it is within 8 e, and in some the float32
    oracle does take the other order; flipping it moves the far gradient by more than the parity bar of 4 e_32 allows."""
    case = KO.make_step_case("ref", 7)
    r32, r64 = KO.run_step_case(case, torch.float32), KO.run_step_case(case, torch.float64)
    J = KO.judge(case, r32, r64)
    gaps = []
    for b in range(case["B"]):
        for c in range(case["num_add"]):
            i, j = r64[b]["far_i"][c] - 32 * c, r64[b]["far_j"][c] - 32 * c
            gaps.append(abs(r64[b]["norm"][c, i, j] - r64[b]["norm"][c, j, i]))
    gaps = np.array(gaps)
    print("e_norm %.2e; gap between the two orders: median %.2e, min %.2e; undecided %.0f %% of the clusters"
          % (J["e_norm"], np.median(gaps), gaps.min(), 100 * J["undecided"]))
    assert J["e_norm"] > 0 and np.median(gaps) < 1e-6 and J["undecided"] > 0.05
    flipped = KO.run_step_case(case, torch.float64, KO.pairs_of(r64)[:, :, ::-1])
    moved = max(float(np.abs(a["dist_grad"] - b["dist_grad"]).max()) for a, b in zip(flipped, r64))
    print("flipping every order moves dist_grad by %.2e = %.1f e_32" % (moved, moved / J["e32"]["dist_grad"]))
    assert moved > 4 * J["e32"]["dist_grad"]                            # more than the parity bar allows


@pytest.mark.parametrize("name", [c[0] for c in KO.STEP_CASES])
def test_step_cases_meet_their_conditions(name):
    """The GPU parity cases (tests/test_gpu_cluster.py) from the oracle alone: no cluster's unordered pair is excluded, at most 5 % of
    a case's rows are, and the two oracles agree on every judged decision - asserted inside judge."""
    for t in (1, 7):
        case = KO.make_step_case(name, t)
        r32, r64 = KO.run_step_case(case, torch.float32), KO.run_step_case(case, torch.float64)
        J = KO.judge(case, r32, r64)
        print("%s t=%d: e_min %.2e, e_norm %.2e, rows excluded %.2f %%, orders undecided %.0f %%, e32 %s"
              % (name, t, J["e_min"], J["e_norm"], 100 * J["share"], 100 * J["undecided"], {k: "%.1e" % x for k, x in J["e32"].items()}))
        assert 0 < J["e_min"] < 1e-5 and all(J["e32"][k] > 0 for k in ("adv", "m", "v", "dist", "dist_grad"))
        if case["cl_num_p"] == 1:                                      # i* == j*: nothing to decide, the far gradient is exactly 0
            assert all(np.array_equal(r["far_i"], r["far_j"]) for r in r32 + r64) and J["undecided"] == 0


# ---------------------------------------------------------------------------------------------- ABI
def declared_symbols(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


def defined(path, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read()).group(1))


def test_cluster_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols(HEADER)
    assert names == sorted(_lib.CLUSTER_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert lib.ifd_cluster_abi_version() == 1 == _lib.CLUSTER_ABI_VERSION == defined(HEADER, "IFD_CLUSTER_ABI_VERSION")
    assert _lib.CLUSTER_DBSCAN_MAX_POINTS == defined(HEADER, "IFD_CLUSTER_DBSCAN_MAX_POINTS") == 256
    assert ctypes.sizeof(_lib.IfdClusterParams) == 44 and ctypes.sizeof(_lib.IfdClusterDiag) == 40
    # the headers the new one builds on are as they were
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_add.h"))) == 5 and lib.ifd_add_abi_version() == 1
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_cw.h"))) == 4 and lib.ifd_cw_abi_version() == 1
    for k in ("cluster_dbscan", "cluster_step", "cluster_attack"):
        assert callable(getattr(I.Classifier, k))
    src = "".join(open(os.path.join(ROOT, "if-defense_amd", f)).read() for f in ("attack.py", "cluster_attack.py", "attack_cli.py"))
    assert "sklearn" not in src.replace("sklearn's", "")              # named in the docstring only, never imported


def test_cluster_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_cluster_dbscan(None, None, None, 1, 8, 0.2, 3, None, None, None) == -1
    assert lib.ifd_cluster_step(None, None, None, None, None, None, None, None, None, None, None, 1, 0.01, 1.0, 1, 8, 1, 2, None) == -1
    assert lib.ifd_cluster_attack(None, None, None, None, None, None, None, 1, 8, 10, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- host logic
class StubClassifier:
    """Stands in for runtime.Classifier on the CPU.  The critical points are the cloud's first 128 rows, their labels: rows 0 - 39
    cluster 0, 40 - 59 cluster 1, the rest outliers.  Every cloud reaches its target from the iteration `hit` of a search step on; a
    step moves the first added point by 0.01 in x and reports loss 2 and dist * weight 3."""
    device = "cpu"

    def __init__(self, hit=2):
        self.calls, self.closed, self.hit = [], False, hit

    def add_critical_points(self, pc, target, num_add, scale):
        self.calls.append(("critical", tuple(pc.shape), num_add, scale))
        return pc[:, :num_add].clone()

    def cluster_dbscan(self, pts, eps, min_samples):
        self.calls.append(("dbscan", tuple(pts.shape), eps, min_samples))
        lab = torch.full(pts.shape[:2], -1, dtype=torch.int32)
        lab[:, :40], lab[:, 40:60] = 0, 1
        return lab

    def cluster_attack(self, pc, target, clusters, num_add, cl_num_p, noise, loss, kappa, scale, lr, init_weight, max_weight, binary_step,
                       num_iter):
        self.calls.append(("attack", tuple(pc.shape), clusters.clone(), num_add, cl_num_p, noise.clone(), loss, kappa, scale, lr, init_weight,
                           max_weight, binary_step, num_iter))
        ok = torch.as_tensor(target) == 3
        return torch.cat([pc, clusters + 1.0], 1), torch.where(ok, 0.5, 1e10).float(), ok

    def cw_state(self, B, A, init_weight, max_weight):
        self.calls.append(("state", B, A, init_weight, max_weight))
        return {"lower": torch.zeros(B, dtype=torch.float64), "o_bestattack": torch.zeros(B, A, 3), "o_bestdist": torch.full((B,), 1e10)}

    def input_grad(self, pc, target, loss, kappa, scale, want_aux=False):
        self.it = getattr(self, "it", 0)
        self.calls.append(("grad", tuple(pc.shape)))
        pred = target if self.it >= self.hit else target + 1
        return torch.zeros_like(pc), {"pred": pred, "loss": torch.full((len(pc),), 2.0)}

    def cluster_step(self, state, grad, pred, target, cat, num_add, cl_num_p, t, lr, scale, loss=None, last_input=None, want_info=False):
        self.calls.append(("step", num_add, cl_num_p, t, lr, scale, last_input is not None, want_info))
        assert t == self.it + 1
        K = cat.shape[1] - num_add * cl_num_p
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


def _attack_file(path, n=6, k=140):
    rng = np.random.default_rng(3)
    np.savez(path, test_pc=rng.standard_normal((n, k, 3)).astype(np.float32), test_label=np.arange(n).astype(np.uint8),
             target_label=np.array([3, 3, 3, 5, 5, 3][:n], np.uint8))


def test_cli_batches_randomstate_noise_and_file(tmp_path, capsys):
    from ifdefense_amd import attack_cli, cluster_attack as CA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    stub, made = StubClassifier(), []

    def make(model, ft, path):
        made.append((model, ft, path))
        return stub
    argv = ["--data_root", src, "--num_points", "130", "--num_add", "3", "--cl_num_p", "24", "--binary_step", "3", "--num_iter", "7",
            "--batch_size", "4", "--kappa", "0.5", "--attack_lr", "0.02", "--out_dir", str(tmp_path), "--dataset", "opt_mn40", "--seed", "5"]
    assert CA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("pointnet", False, "pretrain/opt_mn40/pointnet.pth")] and stub.closed
    assert out.count("Successfully attack 3/4") == 1 and out.count("Successfully attack 1/2") == 1 and "Step 0" not in out
    # two reference batches (4 + 2 clouds): 128 critical points, one DBSCAN and one library call each, scale = 1 / batch
    assert [c[0] for c in stub.calls] == ["critical", "dbscan", "attack"] * 2
    assert stub.calls[0] == ("critical", (4, 130, 3), 128, 0.25) and stub.calls[3] == ("critical", (2, 130, 3), 128, 0.5)
    assert stub.calls[1] == ("dbscan", (4, 128, 3), 0.2, 3)
    a, b = stub.calls[2], stub.calls[5]
    assert a[1] == (4, 130, 3) and b[1] == (2, 130, 3) and a[3:5] == (3, 24)
    assert a[6:] == ("logits", 0.5, 0.25, 0.02, 5., 30., 3, 7) and b[8] == 0.5
    # the clusters: ONE RandomState(seed) carried across the clouds AND the batches, the reference's calls in its order
    data = attack_cli.load_points(np.load(src), 130)
    rng = np.random.RandomState(5)
    lab = np.full(128, -1)
    lab[:40], lab[40:60] = 0, 1
    want = np.stack([KO.init_centers(c[:128], lab, 3, 24, rng).reshape(72, 3) for c in data])
    assert np.array_equal(a[2].numpy(), want[:4]) and np.array_equal(b[2].numpy(), want[4:]) and a[2].dtype == torch.float32
    # cluster 1 (20 rows) with replacement, cluster 0 (40 rows) without, then a fallback: 24 distinct non-outlier rows
    first = want[0].reshape(3, 24, 3)
    assert len(np.unique(first[1], axis=0)) == 24 and len(np.unique(first[0], axis=0)) <= 20 and len(np.unique(first[2], axis=0)) == 24
    na, nb = a[5], b[5]
    assert tuple(na.shape) == (3, 4, 72, 3) and tuple(nb.shape) == (3, 2, 72, 3) and na.dtype == torch.float32
    assert 0 < float(na.abs().max()) < 1e-6 and 1e-8 < float(na.std()) < 2e-7
    gen = torch.Generator().manual_seed(5)
    assert torch.equal(na, torch.stack([torch.randn(4, 72, 3, generator=gen) * 1e-7 for _ in range(3)]))
    assert torch.equal(nb, torch.stack([torch.randn(2, 72, 3, generator=gen) * 1e-7 for _ in range(3)]))
    d = tmp_path / "attack" / "results" / "opt_mn40_130" / "Cluster" / "3-24"
    name = "Cluster-pointnet-logits_kappa=0.5-success_%.4f-rank_0.npz" % (4 / 6)
    assert os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 130 + 72, 3) and np.array_equal(z["test_pc"][:, :130], data)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8
    assert list(z["test_label"]) == list(range(6)) and list(z["target_label"]) == [3, 3, 3, 5, 5, 3]
    # cross_entropy names the file without kappa; -1: one batch; the rank names the file
    stub.calls.clear()
    assert CA.main(argv + ["--batch_size", "-1", "--adv_func", "cross_entropy", "--local_rank", "2"], make_classifier=make) == 0
    assert [c[0] for c in stub.calls] == ["critical", "dbscan", "attack"] and stub.calls[2][1] == (6, 130, 3) and stub.calls[2][6] == "cross_entropy"
    assert "Cluster-pointnet-cross_entropy-success_%.4f-rank_2.npz" % (4 / 6) in os.listdir(d)
    # the defaults are the reference script's
    args = CA.build_parser().parse_args([])
    assert (args.num_add, args.cl_num_p, args.binary_step, args.num_iter, args.attack_lr, args.batch_size) == (3, 32, 5, 500, 1e-2, -1)


def test_cli_and_class_refuse_what_is_not_built(capsys):
    from ifdefense_amd import cluster_attack as CA

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--model", "dgcnn"], ["--model", "pointnet2"], ["--model", "pointconv"], ["--feature_transform", "true"]):
        assert CA.main(["--data_root", "x.npz"] + argv, make_classifier=never) == 2
        assert "not built" in capsys.readouterr().err
    for argv in (["--binary_step", "0"], ["--num_iter", "0"]):
        assert CA.main(["--data_root", "x.npz"] + argv, make_classifier=never) == 2
        assert "at least 1" in capsys.readouterr().err
    for argv in (["--num_add", "0"], ["--cl_num_p", "0"], ["--num_add", "33"], ["--num_add", "1025", "--cl_num_p", "1"], ["--num_points", "127"],
                 ["--num_points", "2049"]):
        assert CA.main(["--data_root", "x.npz"] + argv, make_classifier=never) == 2
        assert "needed" in capsys.readouterr().err
    from ifdefense_amd import attack as A
    with pytest.raises(ValueError, match="far_chamfer"):
        A.CWAddClusters(None, dist_func="chamfer")
    for kw in ({"num_add": 0}, {"cl_num_p": 0}, {"num_add": 33}, {"binary_step": 0}, {"num_iter": 0}):
        with pytest.raises(ValueError):
            A.CWAddClusters(None, **kw)
    with pytest.raises(ValueError, match="between 128 and 2048"):
        A.CWAddClusters(StubClassifier()).attack(torch.zeros(2, 127, 3), [1, 2])
    assert sorted(A.ATTACKS) == ["fgm", "ifgm", "mifgm", "pgd"]


@pytest.mark.parametrize("num_iter,printed", [(10, [0, 2, 4, 6, 8]), (3, [0, 1, 2])])
def test_host_driven_loop_prints_the_reference_lines(capsys, num_iter, printed):
    """verbose=True: the critical points and the DBSCAN once, then one input_grad on the CONCATENATED clouds and one cluster_step an
    iteration; the reference's line every num_iter // 5 iterations with the batch means of the PREVIOUS iteration's losses, zeros at
    iteration 0 of a search step, and none of its wall-clock lines; last_input in the last iteration of the last search step only;
    the fallback for clouds whose lower stays 0; the originals come back untouched in front of the added rows."""
    from ifdefense_amd import attack as A
    stub = StubClassifier(hit=2)
    x = torch.arange(3 * 130 * 3, dtype=torch.float32).reshape(3, 130, 3)
    atk = A.CWAddClusters(stub, binary_step=2, num_iter=num_iter, attack_lr=0.03, num_add=2, cl_num_p=4, seed=4, ref_batch=12)
    dist, adv, n_ok = atk.attack(x, [1, 2, 3])
    out = capsys.readouterr().out.splitlines()
    want = []
    for s in range(2):
        for it in printed:
            want += ["Step %d, iteration %d, success %d/3" % (s, it, 3 if it >= 2 else 0),
                     "adv_loss: %.4f, dist_loss: %.4f" % ((2.0, 3.0) if it else (0.0, 0.0))]
    assert out == want + ["Successfully attack 2/3"] and n_ok == 2 and not any("total" in l or "time" in l for l in out)
    steps = [c for c in stub.calls if c[0] == "step"]
    assert len(steps) == 2 * num_iter and [c[3] for c in steps] == list(range(1, num_iter + 1)) * 2
    assert all(c[1:3] == (2, 4) and c[4] == 0.03 and c[5] == pytest.approx(1 / 12) for c in steps)
    assert [c[6] for c in steps] == [False] * (2 * num_iter - 1) + [True]
    assert all(c[1] == (3, 138, 3) for c in stub.calls if c[0] == "grad")
    assert [c[0] for c in stub.calls if c[0] not in ("step", "grad")] == ["critical", "dbscan", "state", "adjust", "adjust"]
    assert stub.calls[0] == ("critical", (3, 130, 3), 128, pytest.approx(1 / 12)) and stub.calls[2] == ("state", 3, 8, 5., 30.)
    assert dist.dtype == np.float64 and adv.shape == (3, 138, 3) and np.array_equal(adv[:, :130], x.numpy())
    rng = np.random.RandomState(4)
    lab = np.full(128, -1)
    lab[:40], lab[40:60] = 0, 1
    start = np.stack([KO.init_centers(c[:128], lab, 2, 4, rng).reshape(8, 3) for c in x.numpy()])
    # clouds 0, 1: the recorded rows (forwarded at iteration 2 of search step 0); cloud 2: the last forwarded rows
    assert np.allclose(adv[:2, 130, 0] - start[:2, 0, 0], -0.02, atol=1e-4) and np.isclose(adv[2, 130, 0] - start[2, 0, 0], -0.01 * (num_iter - 1), atol=1e-3)
    assert np.allclose(adv[:, 131:], start[:, 1:], atol=1e-4)
