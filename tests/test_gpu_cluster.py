"""GPU checks of the CW cluster-adding attack (include/ifd_cluster.h) against tests/cluster_oracle.py.

DBSCAN is exact: the header's definition leaves no bit open, and the numpy restatement of it is the reference.  The step is judged
teacher-forced: one iteration from a given state against the float64 oracle's one iteration from the same state, at 4 x the float32
oracle's own error per quantity (maximum over the case), outside the rows the oracle alone calls undecidable at float32.  The
farthest pair of every cluster is read from ifd_cluster_step's optional diagnostics: the UNORDERED pair must be the float64
oracle's, the order inside it only where the oracle calls it decidable (cluster_oracle.judge); where it is not, the float64
yardstick is the oracle's step with the GPU's order forced.  Parity always starts from a cluster centre + 0.05 randn, never from
the reference's 1e-7 start.  Everything discrete - ties, the records, the weight's binary search, batching, fused against
host-driven - is exact."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import atk_oracle as AO
import cluster_oracle as KO
import pointnet_oracle as PO

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def W64(sd):
    return PO.to_torch(sd, torch.float64)


@pytest.fixture(scope="module")
def net(sd):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as c:
        assert all(hasattr(c, k) for k in ("cluster_dbscan", "cluster_step", "cluster_attack"))
        yield c


@pytest.fixture(scope="module")
def clouds():
    import bench
    return bench.synth_clouds(64, seed=91)


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def make_state(net, B, A, **over):
    st = net.cw_state(B, A, 5., 30.)
    for k, v in over.items():
        st[k] = dev(np.asarray(v), st[k].dtype).reshape(st[k].shape).contiguous()
    return st


# ---------------------------------------------------------------------------------------------- 1. DBSCAN
def serpentine(n=256, step=0.15, row=15):
    """A chain: `row` moves along +-x, then two moves along +y, and so on; neighbours are 0.15 apart, everything else >= 0.21."""
    p, pos, out = np.zeros(3), 0, []
    for k in range(n):
        out.append(p.copy())
        r, q = divmod(pos, row + 2)
        p = p + (np.array([step if r % 2 == 0 else -step, 0, 0]) if q < row else np.array([0, step, 0]))
        pos += 1
    return np.array(out, np.float32)


def _dbscan_case(name):
    """-> (pts [B,stride,3], n_pts or None, min_samples)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "blobs":
        return np.stack([KO.blob_cloud(rng) for _ in range(12)]), None, 3
    if name == "tiny":                                                 # n = 1, 2 and 3: three mutual neighbours are exactly min_samples
        x = np.full((4, 3, 3), np.nan, np.float32)
        tri = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0]], np.float32)
        x[0, :1], x[1, :2], x[2], x[3] = tri[:1], tri[:2], tri, tri * 2.5   # the last: three points, nobody's neighbours
        return x, np.array([1, 2, 3, 3], np.int32), 3
    if name == "tiny4":
        return _dbscan_case("tiny")[0], np.array([1, 2, 3, 3], np.int32), 4
    if name == "outliers":
        g = np.stack(np.meshgrid(np.arange(8), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(128, 3) * 0.5
        return g[None].astype(np.float32), None, 3
    if name == "one":
        return (0.03 * rng.standard_normal((2, 128, 3))).astype(np.float32), None, 3
    if name == "duplicates":
        base = KO.blob_cloud(rng, 40)
        return np.concatenate([base, base, base[:20]])[None][:, rng.permutation(100)].copy(), None, 3
    if name == "chain":
        c = serpentine()
        return np.stack([c, c[rng.permutation(256)], c[::-1]]), None, 3
    if name == "border":
        p = KO.border_cloud()[0]
        return np.stack([p, p[::-1]]), None, 4
    assert name == "ragged"
    x = np.full((4, 140, 3), np.nan, np.float32)
    n = np.array([128, 77, 140, 5], np.int32)
    for b in range(4):
        x[b, :n[b]] = KO.blob_cloud(rng, int(n[b]))
    return x, n, 3


@pytest.mark.parametrize("name", ["blobs", "tiny", "tiny4", "outliers", "one", "duplicates", "chain", "border", "ragged"])
def test_dbscan_is_the_numpy_definition_bit_for_bit(net, name):
    pts, n_pts, min_samples = _dbscan_case(name)
    lab, cnt = net.cluster_dbscan(dev(pts), KO.EPS, min_samples, n_pts=n_pts, want_count=True)
    lab, cnt = lab.cpu().numpy(), cnt.cpu().numpy()
    for b in range(len(pts)):
        n = pts.shape[1] if n_pts is None else int(n_pts[b])
        want, k = KO.dbscan(pts[b, :n], KO.EPS, min_samples)
        assert np.array_equal(lab[b, :n], want) and cnt[b] == k and np.all(lab[b, n:] == -1), (name, b)
    if name == "tiny":
        assert lab[:3].tolist() == [[-1, -1, -1], [-1, -1, -1], [0, 0, 0]] and cnt.tolist() == [0, 0, 1, 0]
    if name == "tiny4":
        assert np.all(lab == -1) and not cnt.any()
    if name == "outliers":
        assert np.all(lab == -1) and cnt[0] == 0
    if name == "one":
        assert not lab.any() and cnt.tolist() == [1, 1]
    if name == "chain":                                                # one cluster, ends included (border points of a core neighbour)
        assert not lab.any() and cnt.tolist() == [1, 1, 1]
    if name == "border":
        assert np.array_equal(lab[0], KO.border_cloud()[1]) and lab[1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 0]
    if name == "blobs":                                                # a cloud alone against the same cloud in a batch
        one = net.cluster_dbscan(dev(pts[5:6]), KO.EPS, 3).cpu().numpy()
        assert np.array_equal(one[0], lab[5]) and cnt.max() >= 2 and (lab == -1).any()


def test_dbscan_limits(net):
    import ifdefense_amd as I
    x = dev(np.random.default_rng(0).standard_normal((2, 300, 3)).astype(np.float32) * 0.1)
    with pytest.raises(I.IfdError, match="stride outside"):
        net.cluster_dbscan(x[:, :257].contiguous())
    lab, cnt = net.cluster_dbscan(x, n_pts=np.array([257, 256], np.int32), want_count=True)     # 257: left untouched
    assert np.all(lab[0].cpu().numpy() == -1) and cnt.tolist()[0] == 0 and cnt.tolist()[1] >= 1
    assert np.array_equal(lab[1, :256].cpu().numpy(), KO.dbscan(x[1, :256].cpu().numpy())[0])
    for kw in ({"eps": 0.}, {"eps": float("nan")}, {"min_samples": 0}):
        with pytest.raises(I.IfdError, match="eps|min_samples"):
            net.cluster_dbscan(x[:, :100].contiguous(), **kw)


def test_dbscan_gives_the_recorded_sklearn_labels(net):
    """tests/golden/cluster_golden.npz: the reference run's 128 critical points and the labels sklearn gave them there."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "cluster_golden.npz"))
    lab = net.cluster_dbscan(dev(g["cri"])).cpu().numpy()
    assert np.array_equal(lab, g["labels"])


# ---------------------------------------------------------------------------------------------- 2. one step, teacher-forced
WANT = ("dist_grad", "nn_ori", "far_i", "far_j", "far_val")


def run_step(net, case, sel=None, weight=None, want=WANT, use_counts=True):
    """One ifd_cluster_step on the clouds `sel` of a case -> dict of numpy arrays."""
    sel = np.arange(case["B"]) if sel is None else np.asarray(sel)
    A = case["A"]
    w = case["weight"] if weight is None else weight
    marker = np.full((len(sel), A, 3), 7.0, np.float32)
    st = make_state(net, len(sel), A, m=case["m"][sel], v=case["v"][sel], weight=np.asarray(w)[sel], o_bestattack=marker)
    cat, last = dev(case["cat"][sel]), dev(marker)
    out = net.cluster_step(st, dev(case["grad"][sel]), case["pred"][sel], case["target"][sel], cat, case["num_add"], case["cl_num_p"],
                           case["t"], KO.STEP_LR, KO.STEP_SCALE, last_input=last, n_ori=case["n_ori"][sel] if use_counts else None,
                           want_info=True, want=want)
    return {k: x.cpu().numpy() for k, x in dict(st, cat=cat, last=last, **out).items()}


def per_cloud(case, got):
    """The GPU's results in the oracle's form."""
    A = case["A"]
    return [{"adv": got["cat"][b, n:n + A], "m": got["m"][b], "v": got["v"][b], "dist": got["info"][b, 2], "dist_grad": got["dist_grad"][b],
             "far_val": got["far_val"][b], "far_i": got["far_i"][b], "far_j": got["far_j"][b]} for b, n in enumerate(case["n_ori"])]


_ORACLE = {}


def oracle_case(name, t):
    key = (name, t)
    if key not in _ORACLE:
        case = KO.make_step_case(name, t)
        r32, r64 = KO.run_step_case(case, torch.float32), KO.run_step_case(case, torch.float64)
        _ORACLE[key] = (case, r32, r64, KO.judge(case, r32, r64))
    return _ORACLE[key]


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("name", [c[0] for c in KO.STEP_CASES])
def test_step_parity_teacher_forced(net, name, t):
    """cluster_oracle.STEP_CASES: 17 x (64 + 3 x 32); 5 ragged clouds of up to 300 + 7 x 11 rows in a wider stride with NaN beyond; 3 x
    (128 + 96 x 1), where i* = j* everywhere; 2 x (1024 + 512 x 2); 1 x (2048 + 1 x 1024).  judge asserts the conditions from the oracle
    alone.  Measured ratios |GPU - f64| / e_32 are printed; DESIGN 7k records them."""
    case, r32, r64, J = oracle_case(name, t)
    got = run_step(net, case, use_counts=name == "ragged")
    B, A = case["B"], case["A"]
    for b in range(B):
        n, keep = int(case["n_ori"][b]), ~J["rows_out"][b]
        # original rows and rows beyond the cloud: untouched, bit for bit
        assert np.array_equal(bits(got["cat"][b, :n]), bits(case["cat"][b, :n])) and np.array_equal(bits(got["cat"][b, n + A:]), bits(case["cat"][b, n + A:]))
        assert np.array_equal(bits(got["last"][b]), bits(case["cat"][b, n:n + A]))          # input_val: the pre-update rows
        assert np.array_equal(got["nn_ori"][b][keep], r64[b]["nn"][keep]), (name, t, b)
        hit = case["pred"][b] == case["target"][b]
        assert got["bestscore"][b] == (case["pred"][b] if hit else -1) and got["bestdist"][b] == (got["info"][b, 2] if hit else np.float32(1e10))
        assert got["o_bestdist"][b] == got["bestdist"][b] and got["o_bestscore"][b] == got["bestscore"][b]
        assert np.array_equal(bits(got["o_bestattack"][b]), bits(case["cat"][b, n:n + A] if hit else np.full((A, 3), 7.0, np.float32)))
    gpu = per_cloud(case, got)
    pairs = KO.pairs_of(gpu)
    KO.check_pairs(case, pairs, r64, J["pair_out"], J["order_out"], "the GPU")
    yard = r64 if np.array_equal(pairs, KO.pairs_of(r64)) else KO.run_step_case(case, torch.float64, pairs)
    err = KO.errors(case, gpu, yard, r64, J["rows_out"])
    if case["cl_num_p"] == 1:
        assert np.array_equal(pairs[:, :, 0], pairs[:, :, 1])
    print("%s t=%d: e_norm %.2e, rows excluded %.2f %%, orders undecided %.0f %%, the GPU takes the float64 order in %.0f %% of the clusters, "
          % (name, t, J["e_norm"], 100 * J["share"], 100 * J["undecided"], 100 * np.mean((pairs == KO.pairs_of(r64)).all(2))) +
          ", ".join("%s |GPU - f64| %.2e = %.2f e_32" % (k, err[k], err[k] / J["e32"][k]) for k in err))
    for k in err:
        assert J["e32"][k] > 0 and err[k] <= 4 * J["e32"][k], (k, err[k], J["e32"][k])


# ---------------------------------------------------------------------------------------------- 3. exact
def test_a_cloud_alone_in_a_batch_and_permuted_gives_the_same_bits(net):
    case = KO.make_step_case("ragged", 7)
    full = run_step(net, case)
    one = run_step(net, case, sel=[2])
    perm = np.array([3, 0, 4, 2, 1])
    mixed = run_step(net, case, sel=perm)
    for k in ("cat", "m", "v", "info", "bestdist", "o_bestattack") + WANT:
        assert np.array_equal(bits(one[k][0]), bits(full[k][2])), k
        assert np.array_equal(bits(mixed[k]), bits(full[k])[perm]), k
    assert case["n_ori"][1] == 1 and not full["nn_ori"][1].any()      # one original: everybody's nearest


def test_clouds_outside_the_limits_are_left_untouched(net):
    """The step never blocks, so a count it cannot take (n_ori < 1, n_ori + A > cat_stride, n_ori > 2048) leaves the cloud as it was,
    in every array; its neighbours in the batch are served."""
    case = KO.make_step_case("ragged", 7)
    bad = dict(case, n_ori=case["n_ori"].copy())
    bad["n_ori"][[0, 2, 4]] = [0, case["stride"] - case["A"] + 1, 2049]
    ok, got = run_step(net, case), run_step(net, bad)
    for b in (0, 2, 4):
        assert np.array_equal(bits(got["cat"][b]), bits(case["cat"][b]))
        assert np.array_equal(bits(got["m"][b]), bits(case["m"][b])) and np.array_equal(bits(got["v"][b]), bits(case["v"][b]))
        assert got["bestdist"][b] == np.float32(1e10) and np.all(got["nn_ori"][b] == -1) and np.all(got["far_i"][b] == -1)
        assert np.all(got["far_j"][b] == -1) and np.isnan(got["far_val"][b]).all() and np.isnan(got["dist_grad"][b]).all()
        assert not (got["last"][b] != 7.0).any() and not (got["o_bestattack"][b] != 7.0).any()
    for b in (1, 3):
        assert np.array_equal(bits(got["cat"][b]), bits(ok["cat"][b]))


def _crafted(rows, num_add, P):
    """One cloud: 8 originals on a lattice of spacing 4 and the given added rows."""
    ori = np.array([[x, y, z] for x in (0., 4.) for y in (0., 4.) for z in (0., 4.)], np.float32)
    adv = np.asarray(rows, np.float32)
    A = len(adv)
    rng = np.random.default_rng(4)
    return {"name": "crafted", "t": 3, "B": 1, "A": A, "num_add": num_add, "cl_num_p": P, "stride": 8 + A, "n_ori": np.array([8], np.int32),
            "cat": np.concatenate([ori, adv])[None].copy(), "grad": (rng.standard_normal((1, 8 + A, 3)) * 0.01).astype(np.float32),
            "m": (rng.standard_normal((1, A, 3)) * 0.01).astype(np.float32), "v": (rng.random((1, A, 3)) * 1e-3 + 1e-8).astype(np.float32),
            "weight": np.array([20.]), "target": np.array([3], np.int32), "pred": np.array([3], np.int32)}


def test_crafted_ties_in_the_far_term_take_the_lowest_j_then_i(net):
    """Cluster 0: points at +1, -1, +1, -1 on the x axis (+ 2): the longest ordered pairs are (i, j) = (1, 0), (3, 0), (1, 2), (3, 2), all
    equal - j = 0, then i = 1.  Cluster 1: the rows 4 = 6 and 5 = 7 duplicated: (5, 4), (7, 4), (5, 6), (7, 6) tie - (5, 4).  The oracle
    (torch's CPU max) agrees; the rows that receive the far term are exactly i* and j*."""
    a, b_ = [3., 2, 2], [1., 2, 2]
    c, d = [2.5, 1.25, 2], [2., 1, 2]
    case = _crafted([a, b_, a, b_, c, d, c, d], 2, 4)
    got, zero = run_step(net, case), run_step(net, case, weight=np.array([0.]))
    assert got["far_i"][0].tolist() == [1, 5] and got["far_j"][0].tolist() == [0, 4]
    r32 = KO.run_step_case(case, torch.float32)[0]
    assert r32["far_i"].tolist() == [1, 5] and r32["far_j"].tolist() == [0, 4]
    assert np.array_equal(bits(got["far_val"][0]), bits(r32["far_val"]))
    far = np.float32(got["far_val"][0][0]) + np.float32(got["far_val"][0][1])
    cd = np.float32(np.float32(4 * 9.0 + 2 * 7.8125 + 2 * 9.0) / np.float32(8))      # every min_p is exact in float32
    assert got["info"][0, 2] == np.float32(far + np.float32(cd * np.float32(0.1)))
    w = np.float32(20.)
    assert got["info"][0, 1] == np.float32(np.float32(far * w) + np.float32(np.float32(cd * w) * np.float32(0.1)))
    cham = KO.closed_form_grad(case["cat"][0, 8:], case["cat"][0, :8], 2, 20., KO.STEP_SCALE, got["nn_ori"][0], [0, 0], [0, 0])
    extra = np.abs(got["dist_grad"][0] - cham).max(1) > 1e-3
    assert np.nonzero(extra)[0].tolist() == [0, 1, 4, 5]
    assert np.isfinite(got["cat"]).all() and not np.array_equal(bits(got["cat"]), bits(zero["cat"]))


_E = np.float32(1e-7)
DIAG = np.sqrt(np.float32(np.float32(_E * _E + _E * _E) + _E * _E))   # |(p_i - p_i) + 1e-7| in float32


def test_identical_rows_and_single_point_clusters_have_no_far_gradient(net):
    """A cluster of identical rows: the diagonal's sqrt(3) * 1e-7 is the maximum, i* = j* = its first row, the far term is exactly
    zero and everything stays finite.  With weight 0 the step is the plain Adam step on grad, bit for bit."""
    p, q = [2., 2, 2.5], [1., 2, 2]
    case = _crafted([p] * 4 + [q, [1.5, 2, 2], q, q], 2, 4)
    got = run_step(net, case)
    assert got["far_i"][0].tolist() == [0, 4] and got["far_j"][0].tolist() == [0, 5]
    assert got["far_val"][0][0] == DIAG and np.isfinite(got["cat"]).all() and np.isfinite(got["dist_grad"]).all()
    cham = np.float32(np.float32(np.float32(KO.STEP_SCALE) * np.float32(20.)) * np.float32(0.1)) * (np.float32(2.) / np.float32(8))
    d = case["cat"][0, 8:12] - case["cat"][0, got["nn_ori"][0][:4]]
    assert np.array_equal(bits(got["dist_grad"][0][:4]), bits((cham * d).astype(np.float32)))          # the Chamfer term alone
    single = KO.make_step_case("single", 7)
    g1, z1 = run_step(net, single), run_step(net, single, weight=np.zeros(3))
    assert np.array_equal(g1["far_i"], g1["far_j"]) and np.all(g1["far_val"] == DIAG)
    # weight 0: the plain Adam step on grad (torch.optim.Adam in float32 agrees to rounding; the bits: no distance term at all)
    assert not z1["dist_grad"].any() and not z1["info"][:, 1].any() and z1["info"][:, 2].all()
    n, A = 128, 96
    g, m, v, x = (single[k][:, n:n + A] if k in ("grad", "cat") else single[k] for k in ("grad", "m", "v", "cat"))
    f32 = np.float32
    step_size, bc2 = f32(KO.STEP_LR / (1 - 0.9 ** 7)), f32(np.sqrt(1 - 0.999 ** 7))
    m1 = (g.astype(np.float64) - m) * f32(1 - 0.9) + m
    assert np.abs(z1["m"] - m1).max() < 1e-8 and np.abs(z1["cat"][:, n:] - (x - step_size * z1["m"] / (np.sqrt(z1["v"]) / bc2 + f32(1e-8)))).max() < 1e-6
    ref = KO.make_step_case("ref", 7)
    other = dict(ref, cat=ref["cat"].copy())
    other["cat"][:, :64] = ref["cat"][:, :64][:, ::-1]                # other originals: with weight 0 they play no part
    za, zc = run_step(net, ref, weight=np.zeros(17)), run_step(net, other, weight=np.zeros(17))
    for k in ("m", "v"):
        assert np.array_equal(bits(za[k]), bits(zc[k]))
    assert np.array_equal(bits(za["cat"][:, 64:]), bits(zc["cat"][:, 64:])) and not np.array_equal(bits(za["cat"]), bits(ref["cat"]))
    # ... and they are the bits of the plain Adam step on grad: ifd_cw_step with adv == ori has no distance term either
    rows = ref["cat"][:, 64:64 + ref["A"]].copy()
    st = make_state(net, 17, ref["A"], m=ref["m"], v=ref["v"], weight=np.zeros(17))
    X = dev(rows)
    net.cw_step(st, dev(ref["grad"][:, 64:64 + ref["A"]].copy()), ref["pred"], ref["target"], X, dev(rows), ref["t"], KO.STEP_LR, KO.STEP_SCALE)
    assert np.array_equal(bits(X), bits(za["cat"][:, 64:])) and not np.array_equal(bits(X), bits(rows))
    assert np.array_equal(bits(st["m"]), bits(za["m"])) and np.array_equal(bits(st["v"]), bits(za["v"]))


def test_limits_are_refused_one_past_them(sd, net):
    import ifdefense_amd as I
    from ifdefense_amd import _lib, weights
    lib, ctx = net.lib, net.ctx
    f = lambda *s: torch.zeros(*s, device="cuda")                      # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")   # noqa: E731
    big = f(1, 10001, 3)
    tt = i(2)
    P, T = big.data_ptr(), tt.data_ptr()

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.ifd_last_error(ctx), (rc, word, lib.ifd_last_error(ctx))
    st = net.cw_state(2, 1024)
    S = C.byref(net._cw_struct(st, 2, 1024))
    step = lambda cat_stride, num_add, P_, n=None, t=1: lib.ifd_cluster_step(ctx, S, P, T, None, T, P, n, None, None, None, t, 0.01, 1.0, 1,   # noqa: E731
                                                                           cat_stride, num_add, P_, None)
    refused(step(4096, 1025, 1), "num_add * cl_num_p")
    refused(step(4096, 33, 32), "num_add * cl_num_p")
    refused(step(4096, 0, 32), "num_add")
    refused(step(4096, 3, 0), "cl_num_p")
    refused(step(96, 3, 32), "cat_stride")
    refused(step(10001, 3, 32, T), "cat_stride")
    refused(step(2049 + 96, 3, 32), "2048 original rows")
    refused(step(200, 3, 32, None, 0), "t >= 1")
    db = lambda B, stride, eps=0.2, ms=3, n=None: lib.ifd_cluster_dbscan(ctx, P, n, B, stride, eps, ms, tt.data_ptr(), None, None)   # noqa: E731
    refused(db(1, 257), "stride outside [1, 256]")
    refused(db(1, 10001, n=T), "stride outside [1, 10000]")
    refused(db(0, 2), "B >= 1")
    refused(db(1, 2, 0.0), "eps")
    refused(db(1, 2, 0.2, 0), "min_samples")
    o, best, ok, cl = f(2, 3100, 3), f(2), i(2), f(2, 1024, 3)

    def attack(stride=128, out_stride=224, num_add=3, P_=32, loss=0, steps=1, it=1, size=C.sizeof(_lib.IfdClusterParams), n=None, B=2, out=None,
               clusters=True):
        prm = _lib.IfdClusterParams(size, loss, steps, it, num_add, P_, 0.0, 0.5, 0.01, 5., 30.)
        return lib.ifd_cluster_attack(ctx, C.byref(prm), P, None if n is None else n.data_ptr(), T, cl.data_ptr() if clusters else None, None,
                                      B, stride, out_stride, o.data_ptr() if out is None else out, best.data_ptr(), ok.data_ptr(), None, None)
    refused(attack(size=40), "struct_size")
    refused(attack(loss=5), "loss_kind")
    refused(attack(steps=0), "binary_step")
    refused(attack(it=0), "num_iter")
    refused(attack(num_add=0), "num_add")
    refused(attack(num_add=33, out_stride=3100), "num_add * cl_num_p")
    refused(attack(stride=2049, out_stride=3100), "without n_points")
    refused(attack(out_stride=223), "without n_points")
    refused(attack(out_stride=10001), "out_stride")
    refused(attack(stride=10001), "stride outside")
    refused(attack(B=0), "B >= 1")
    refused(attack(clusters=False), "missing pointer")
    refused(attack(out=P), "overlaps")
    refused(attack(n=dev(np.array([128, 0], np.int32))), "n_points outside [1, 128]")
    refused(attack(n=dev(np.array([129, 5], np.int32))), "n_points outside [1, 128]")
    refused(attack(out_stride=200, n=dev(np.array([105, 104], np.int32))), "n_points outside [1, 104]")
    assert not o.any() and not ok.any() and not best.any()
    with pytest.raises(I.IfdError, match="clusters"):
        net.cluster_attack(torch.zeros(2, 8, 3), [0, 1], torch.zeros(2, 5, 3), 2, 2, binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="noise"):
        net.cluster_attack(torch.zeros(2, 8, 3), [0, 1], torch.zeros(2, 4, 3), 2, 2, torch.zeros(1, 2, 8, 3), binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="target"):
        net.cluster_attack(torch.zeros(2, 8, 3), [0, 40], torch.zeros(2, 4, 3), 2, 2, binary_step=1, num_iter=1)
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, True), "pointnet"), feature_transform=True, device="cuda:0") as ft:
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.cluster_attack(torch.zeros(2, 8, 3), [0, 1], torch.zeros(2, 4, 3), 2, 2, binary_step=1, num_iter=1)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.cluster_dbscan(torch.zeros(2, 8, 3))
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.cluster_step(ft.cw_state(2, 4), f(2, 12, 3), [0, 0], [0, 0], f(2, 12, 3), 2, 2, 1, 0.01)
    # the limits themselves work: one original row, 1024 added rows, the whole attack
    x = np.random.default_rng(0).standard_normal((2, 1, 3)).astype(np.float32)
    out, _, _ = net.cluster_attack(x, [0, 1], np.random.default_rng(1).standard_normal((2, 1024, 3)).astype(np.float32), 32, 32,
                                   binary_step=1, num_iter=2)
    assert np.array_equal(bits(out[:, :1]), bits(x)) and np.isfinite(out.cpu().numpy()).all() and tuple(out.shape) == (2, 1025, 3)


# ---------------------------------------------------------------------------------------------- 4. records and adjustment
def test_record_logic_and_adjustment_are_exact(net):
    """test_gpu_add's record table on this state (stride = A), then ifd_cw_adjust as it is: the <=."""
    rng = np.random.default_rng(5)
    B, n, A = 5, 48, 12
    case = KO.make_step_case("ref", 1)
    cat = case["cat"][:B, :n + A].copy()
    cat[:, n:] = cat[:, :A] + (0.05 * rng.standard_normal((B, A, 3))).astype(np.float32)
    adv = cat[:, n:].copy()
    marker = np.full((B, A, 3), 7.0, np.float32)
    #          hit, smaller     hit, larger      miss, smaller   (equal: below)   hit, smaller than bestdist only
    pred, target = np.array([3, 3, 4, 3, 3], np.int32), np.full(B, 3, np.int32)
    bestdist = np.array([10., 1e-9, 10., 1e10, 10.], np.float32)
    o_bestdist = np.array([10., 1e-9, 10., 1e10, 1e-9], np.float32)
    st = make_state(net, B, A, bestdist=bestdist, o_bestdist=o_bestdist, bestscore=np.full(B, -5), o_bestscore=np.full(B, -5),
                    o_bestattack=marker)
    grad = dev((0.01 * rng.standard_normal(cat.shape)).astype(np.float32))
    X = dev(cat)
    dist = net.cluster_step(st, grad, pred, target, X, 3, 4, 1, 1e-2, 0.2, want_info=True)["info"].cpu().numpy()[:, 2]
    assert np.all(dist > 1e-6) and np.all(dist < 20) and not np.array_equal(X.cpu().numpy()[:, n:], adv)
    g = {k: x.cpu().numpy() for k, x in st.items()}
    assert np.array_equal(g["bestdist"], np.array([dist[0], 1e-9, 10., dist[3], dist[4]], np.float32))
    assert np.array_equal(g["bestscore"], [3, -5, -5, 3, 3])
    assert np.array_equal(g["o_bestdist"], np.array([dist[0], 1e-9, 10., dist[3], 1e-9], np.float32))
    assert np.array_equal(g["o_bestscore"], [3, -5, -5, 3, -5])
    for b, written in enumerate([True, False, False, True, False]):    # o_bestattack: the pre-update added rows
        assert np.array_equal(bits(g["o_bestattack"][b]), bits(adv[b] if written else marker[b])), b
    # the same clouds through again: every dist equals its record bit for bit, and < is strict
    st["o_bestattack"].copy_(dev(marker))
    st["o_bestscore"].fill_(-9)
    st["bestscore"].fill_(-9)
    st["bestdist"][1] = float(dist[1])
    st["o_bestdist"][1] = float(dist[1])
    st["o_bestdist"][4] = float(dist[4])
    before = {k: st[k].clone() for k in ("bestdist", "o_bestdist")}
    dist2 = net.cluster_step(st, grad, pred, target, dev(cat), 3, 4, 1, 1e-2, 0.2, want_info=True)["info"].cpu().numpy()[:, 2]
    assert np.array_equal(bits(dist2), bits(dist))
    assert torch.equal(st["bestdist"], before["bestdist"]) and torch.equal(st["o_bestdist"], before["o_bestdist"])
    assert np.array_equal(bits(st["o_bestattack"]), bits(marker)) and np.array_equal(st["o_bestscore"].cpu().numpy(), np.full(B, -9))
    # the adjustment on this state: bestdist == o_bestdist with the right class is a success (<=), above it or the wrong class a failure
    st["bestscore"].copy_(dev(np.array([3, 3, 4, 3, -1], np.int32)))
    st["bestdist"].copy_(dev(np.array([0.5, 0.75, 0.25, 0.25, 1e10], np.float32)))
    st["o_bestdist"].copy_(dev(np.array([0.5, 0.5, 0.5, 0.5, 1e10], np.float32)))
    st["m"].fill_(1.0)
    net.cw_adjust(st, target)
    assert np.array_equal(st["lower"].cpu().numpy(), [5., 0, 0, 5., 0]) and np.array_equal(st["upper"].cpu().numpy(), [30., 5., 5., 30., 5.])
    assert np.array_equal(st["weight"].cpu().numpy(), [17.5, 2.5, 2.5, 17.5, 2.5]) and st["weight"].dtype == torch.float64
    assert not st["m"].any() and np.array_equal(st["bestscore"].cpu().numpy(), np.full(B, -1))


# ---------------------------------------------------------------------------------------------- 5. through the network
def test_loop_teacher_forced_through_the_network(net, sd, W64, clouds):
    """B = 17, 64 + 3 x 16 points, 3 iterations driven from the host from 3 critical points + 0.05 randn.  After each iteration the new
    added rows against the oracle's ONE step from the GPU's previous state, the GPU's own gradient and the GPU's order of every
    farthest pair (the bar of test 2; the unordered pair must be the float64 oracle's own), and the gradient of the concatenated
    cloud at that state by test_gpu_atk's row-wise rule under atk_oracle.case_conditions."""
    B, n, na, P, lr = 17, 64, 3, 16, 1e-2
    A = na * P
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    cri = net.add_critical_points(x, tg, na, 1.0 / B)
    start = cri.repeat_interleave(P, dim=1) + dev((np.random.default_rng(2).standard_normal((B, A, 3)) * 0.05).astype(np.float32))
    cat = torch.cat([dev(x), start], 1).contiguous()
    weight = 5.
    st = net.cw_state(B, A, weight, 30.)
    done = 0
    for k in (1, 2, 3):
        prev, m, v = cat.cpu().numpy(), st["m"].cpu().numpy(), st["v"].cpu().numpy()
        grad, aux = net.input_grad(cat, tg, scale=1.0 / B, want_aux=True)
        g, aux = grad.cpu().numpy(), {a: b.cpu().numpy() for a, b in aux.items()}
        d = net.cluster_step(st, grad, aux["pred"], tg, cat, na, P, k, lr, 1.0 / B, loss=aux["loss"], want=("far_i", "far_j"))
        pairs = np.stack([d["far_i"].cpu().numpy(), d["far_j"].cpu().numpy()], 2)
        new = cat.cpu().numpy()
        assert np.array_equal(bits(new[:, :n]), bits(x))
        a = lambda i: (g[i, n:], int(aux["pred"][i]), int(tg[i]), prev[i, n:], x[i], weight, m[i], v[i], k, lr, 1.0 / B, KO.fresh_record(A), na)   # noqa: E731
        s64 = [KO.step(*a(i)) for i in range(B)]
        s32 = [KO.step(*a(i), dtype=torch.float32) for i in range(B)]
        e_min = max(float(np.abs(q[6]["min_p"].astype(np.float64) - r[6]["min_p"]).max()) for q, r in zip(s32, s64))
        e_norm = max(float(np.abs(q[6]["norm"].astype(np.float64) - r[6]["norm"]).max()) for q, r in zip(s32, s64))
        e_gpu = e_32 = 0.0
        n_out = 0
        for i in range(B):
            rows_out, pair_out, _ = KO.exclusions(prev[i, n:], x[i], e_min, s64[i][6]["norm"], e_norm)
            assert not pair_out.any()
            want = np.stack([s64[i][6]["far_i"], s64[i][6]["far_j"]], 1)
            assert np.array_equal(np.sort(pairs[i], 1), np.sort(want, 1)), (k, i)
            n_out += int(rows_out.sum())
            p32 = np.stack([s32[i][6]["far_i"], s32[i][6]["far_j"]], 1)
            y_gpu = KO.step(*a(i), forced=pairs[i])[0]
            y_32 = KO.step(*a(i), forced=p32)[0]
            e_gpu = max(e_gpu, np.abs(new[i, n:] - y_gpu)[~rows_out].max())
            e_32 = max(e_32, np.abs(s32[i][0] - y_32)[~rows_out].max())
        assert n_out <= 0.05 * B * A
        print("iteration %d: adv |GPU - f64| %.3e = %.2f e_32, %d rows excluded" % (k, e_gpu, e_gpu / e_32, n_out))
        assert e_32 > 0 and e_gpu <= 4 * e_32, (k, e_gpu, e_32)
        r32, r64, e, e32, ex = AO.run_case(sd, [c for c in prev], tg, scale=1.0 / B)
        AO.case_conditions(r64, e)
        for i in range(B):
            why, rows_out = AO.row_exclusion(r64[i], e)
            if why:
                continue
            f = AO.run_cloud(W64, prev[i], tg[i], scale=1.0 / B, force_feat=aux["win_feat"][i], force_stn=aux["win_stn"][i])
            AO.check_grad(g[i], f["grad"], e32, "iteration %d cloud %d" % (k, i), rows_out)
            done += 1
    assert done >= 0.9 * 3 * B


# ---------------------------------------------------------------------------------------------- 6. fused = host-driven
def test_fused_and_host_driven_loops_give_the_same_bits(net, W64, clouds, capsys):
    """16 clouds x (192 + 3 x 32) points, 2 search steps x 20 iterations, targets (prediction + 1) % 40, the reference script's
    weights.  The count beside the float64 oracle's free-running count is a sanity figure, printed, not a parity bar."""
    from ifdefense_amd import attack as A
    B, n, na, P = 16, 192, 3, 32
    add = na * P
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    kw = dict(binary_step=2, num_iter=20, num_add=na, cl_num_p=P, seed=3)
    a = A.CWAddClusters(net, **kw).attack(x, tg)
    out = capsys.readouterr().out
    b = A.CWAddClusters(net, verbose=False, **kw).attack(x, tg)
    quiet = capsys.readouterr().out
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[1].shape == (B, n + add, 3) and a[1].dtype == np.float32 and np.array_equal(bits(a[1][:, :n]), bits(x))
    for s in range(2):
        for it in (0, 4, 8, 12, 16):
            assert out.count("Step %d, iteration %d, success" % (s, it)) == 1
    assert out.count("adv_loss: ") == 10 and "time" not in out and "total" not in out
    assert out.count("Successfully attack %d/%d" % (a[2], B)) == 1 and quiet == "Successfully attack %d/%d\n" % (a[2], B)
    # the library call itself: the same clusters and noise, the same bits, success = lower > 0, the records
    atk = A.CWAddClusters(net, **kw)
    clusters = atk._init_centers(torch.from_numpy(x), torch.from_numpy(tg))
    noise = atk.noise(torch.from_numpy(x))
    cri = net.add_critical_points(x, tg, 128, 1.0 / B).cpu().numpy()
    for i in range(B):                                                 # every start row is one of the cloud's 128 critical points
        assert (clusters[i].numpy()[:, None] == cri[i][None]).all(2).any(1).all()
    args = dict(scale=1.0 / B, binary_step=2, num_iter=20, want_bounds=True)
    o1 = net.cluster_attack(x, tg, clusters, na, P, noise, **args)
    pc, best, ok, lower = o1[0].cpu().numpy(), o1[1].cpu().numpy(), o1[2].cpu().numpy(), o1[3]["lower"].cpu().numpy()
    assert np.array_equal(bits(pc), bits(b[1])) and np.array_equal(best.astype(np.float64), b[0])
    assert np.array_equal(ok, lower > 0) and ok.sum() == a[2]
    assert np.all(best[ok] < 1e10) and np.all(best[ok] >= 0)
    pred = net.predict(o1[0]).cpu().numpy()
    assert np.array_equal(pred[ok], tg[ok])                             # exact: the forward pass is batch-independent
    # clouds that never succeeded carry the last forwarded rows: after ONE iteration those are the start itself, clusters + noise
    s1 = net.cluster_attack(x, tg, clusters, na, P, noise[:1], **dict(args, binary_step=1, num_iter=1))
    fail = ~s1[2].cpu().numpy()
    assert fail.sum() >= 1 and np.all(s1[1].cpu().numpy()[fail] == np.float32(1e10))
    assert np.array_equal(bits(s1[0][:, n:])[fail], bits(clusters.cuda() + noise[0].cuda())[fail])
    # a padded, ragged, permuted batch gives the same per-cloud bits
    p = np.array([4, 0, 5, 2, 1, 3])
    xr = np.full((6, n + 5, 3), np.nan, np.float32)
    counts = np.array([n, n - 7, n, 1, n - 1, 64], np.int32)
    for j, i in enumerate(p):
        xr[j, :counts[j]] = x[i, :counts[j]]
    o2 = net.cluster_attack(xr, tg[p], clusters[p], na, P, noise[:, p], n_points=counts, out_stride=n + add + 3, **args)
    same = [j for j in range(6) if counts[j] == n]
    o3 = net.cluster_attack(x[p][same], tg[p][same], clusters[p][same], na, P, noise[:, p][:, same], **args)
    pc2, pc3 = o2[0].cpu().numpy(), o3[0].cpu().numpy()
    for k, j in enumerate(same):
        assert np.array_equal(bits(pc2[j, :n + add]), bits(pc3[k])) and np.array_equal(bits(pc3[k]), bits(pc[p[j]]))
        assert o2[1][j] == o3[1][k] == o1[1][p[j]]
    for j in range(6):
        c = int(counts[j])
        assert np.array_equal(bits(pc2[j, :c]), bits(xr[j, :c])) and np.isfinite(pc2[j, c:c + add]).all() and not pc2[j, c + add:].any()
    ref = KO.attack(W64, x, tg, clusters.numpy(), noise.numpy(), na, P, torch.float64, binary_step=2, num_iter=20)
    print("CW Add-Cluster: %d/%d clouds attacked, mean best_dist %.3e; the float64 oracle, free-running: %d/%d, %.3e"
          % (ok.sum(), B, best[ok].mean() if ok.any() else np.nan, ref["success_num"], B,
             ref["o_bestdist"][ref["success"]].mean() if ref["success_num"] else np.nan))


# ---------------------------------------------------------------------------------------------- 7. the CLI
def test_cli_end_to_end(net, sd, tmp_path, capsys):
    from ifdefense_amd import inference as Inf, cluster_attack as CA
    import bench
    ck, src = str(tmp_path / "pointnet.npz"), str(tmp_path / "attack_data.npz")
    np.savez(ck, **sd)
    pcs = bench.synth_clouds(20, seed=5)[:, :192]
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pcs])).cpu().numpy()
    label, target = pred.astype(np.uint8), ((pred + 1) % 40).astype(np.uint8)
    np.savez(src, test_pc=pcs, test_label=label, target_label=target)
    assert CA.main(["--data_root", src, "--num_points", "192", "--binary_step", "2", "--num_iter", "20", "--batch_size", "16",
                    "--model_path", ck, "--out_dir", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Successfully attack")]
    counts = [int(l.split()[-1].split("/")[0]) for l in lines]
    assert [l.split("/")[-1] for l in lines] == ["16", "4"]
    d = tmp_path / "attack" / "results" / "mn40_192" / "Cluster" / "3-32"
    (name,) = os.listdir(d)
    assert name == "Cluster-pointnet-logits_kappa=0.0-success_%.4f-rank_0.npz" % (sum(counts) / 20.0)
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (20, 288, 3) and np.isfinite(z["test_pc"]).all()
    assert np.array_equal(z["test_pc"][:, :192], np.stack([Inf.normalize_points_np(c) for c in pcs]))
    assert np.array_equal(z["test_label"], label) and np.array_equal(z["target_label"], target)
    assert Inf.main(["--data_root", str(d / name), "--mode", "target", "--model", "pointnet", "--model_path", ck, "--num_points", "288"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    rate = float(line.split("attack success rate:")[1])
    print("cluster_attack's rate %.4f, inference's rate on the written file %.4f" % (sum(counts) / 20.0, rate))
    assert rate >= sum(counts) / 20.0 - 1e-4                            # every recorded cloud reached its target when it was forwarded
