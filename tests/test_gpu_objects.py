"""GPU checks of the CW object-adding attack (include/ifd_object.h) against tests/objects_oracle.py.

The step is judged teacher-forced: one iteration from a given state against the float64 oracle's one iteration from the same state,
at 4 x the float32 oracle's own error per quantity (maximum over the case).  The nearest original of every world row is read from
ifd_object_step's diagnostics: it must be the float64 oracle's on every row the oracles alone call decidable, and on the others the
float64 yardstick takes the GPU's (objects_oracle.judge / yardstick).  Parity starts from the template + 0.05 randn, never from the
reference's 1e-7 start.  Everything discrete or defined bit for bit - the placement at angle 0 and in y, the integer gradient sums,
the remainder, the records, the weight's binary search, batching, fused against host-driven - is exact."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import atk_oracle as AO
import objects_oracle as OO
import pointnet_oracle as PO

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "objects_golden.npz")
DIAG = ("obj_grad", "nn_ori", "g_shift", "g_angle", "l2", "cd")
TWO_PI32 = np.float32(OO.TWO_PI)


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
        assert all(hasattr(c, k) for k in ("object_place", "object_step", "object_attack"))
        yield c


@pytest.fixture(scope="module")
def clouds():
    import bench
    return bench.synth_clouds(64, seed=91)


@pytest.fixture(scope="module")
def airplane():
    return np.load(GOLDEN)["object_raw"]


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64 if a.dtype == np.float64 else a.dtype)


def make_state(net, case, sel=None, **over):
    """The device state of a case (the clouds ``sel``), its concatenated cloud with the placement done on the GPU, the gradient."""
    sel = np.arange(case["B"]) if sel is None else np.asarray(sel)
    B, na, P, A = len(sel), case["num_add"], case["obj_num_p"], case["A"]
    st = net.object_state(B, na, P, 5., 40.)
    st["weight"].copy_(dev(case["weight"][sel]))
    st["obj"].copy_(dev(case["obj"][sel].reshape(B, A, 3)))
    for k in ("shift", "angle", "shift_m", "shift_v", "angle_m", "angle_v"):
        st[k].copy_(dev(case[k][sel]))
    st["m"].copy_(dev(case["m"][sel].reshape(B, A, 3)))
    st["v"].copy_(dev(case["v"][sel].reshape(B, A, 3)))
    for k, v in over.items():
        st[k].copy_(dev(np.asarray(v), st[k].dtype).reshape(st[k].shape))
    cat = np.full((B, case["stride"], 3), np.nan, np.float32)
    for j, b in enumerate(sel):
        n = int(case["n_ori"][b])
        cat[j, :n] = case["ori"][b, :n]
    cat = dev(cat)
    n_ori = dev(case["n_ori"][sel])
    net.object_place(st["obj"], st["angle"], st["shift"], cat, na, P, n_ori=n_ori)
    return st, cat, n_ori, dev(case["grad"][sel])


def gpu_step(net, case, sel=None, last=False, **over):
    """One ifd_object_step on a case -> (list of per-cloud dicts in the oracle's names, the raw pieces)."""
    sel = np.arange(case["B"]) if sel is None else np.asarray(sel)
    st, cat, n_ori, grad = make_state(net, case, sel, **over)
    before = cat.cpu().numpy()
    li = torch.full((len(sel), case["A"], 3), 7.0, device="cuda") if last else None
    d = net.object_step(st, case["objects"], grad, case["pred"][sel], case["target"][sel], cat, case["num_add"], case["obj_num_p"],
                        case["t"], OO.STEP_LR, OO.STEP_SCALE, n_ori=n_ori, last_input=li, want_info=True, want=DIAG)
    after = cat.cpu().numpy()
    g = {k: v.cpu().numpy() for k, v in list(st.items()) + list(d.items())}
    out = []
    for j, b in enumerate(sel):
        n, A = int(case["n_ori"][b]), case["A"]
        r = {k: g[k][j] for k in ("obj", "shift", "angle") + OO.MOMENTS + ("obj_grad", "g_shift", "g_angle", "l2", "cd")}
        r.update(dist=g["info"][j, 2], nn=g["nn_ori"][j], world=after[j, n:n + A], forwarded=before[j, n:n + A])
        out.append(r)
    return out, {"state": st, "before": before, "after": after, "got": g, "last": li}


# ---------------------------------------------------------------------------------------------- 1. step parity
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("name", [c[0] for c in OO.STEP_CASES])
def test_step_parity_teacher_forced(net, name, t):
    case = OO.make_step_case(name, t)
    r32, r64 = OO.run_step_case(case, torch.float32), OO.run_step_case(case, torch.float64)
    J = OO.judge(case, r32, r64)
    got, raw = gpu_step(net, case)
    for g, y, ro in zip(got, r64, J["rows_out"]):
        assert np.array_equal(g["nn"][~ro], y["nn"][~ro]), "%s: the GPU takes another nearest original on a judged row" % name
    yard = OO.yardstick(case, [g["nn"] for g in got], r64, J["rows_out"])
    err = OO.errors(got, yard)
    ratios = {k: err[k] / J["e32"][k] if J["e32"][k] > 0 else (0.0 if err[k] == 0 else np.inf) for k in OO.QUANTITIES}
    print("%s t=%d: %.2f %% rows excluded, e_min %.2e; |GPU - f64| / e_32: %s" % (
        name, t, 100 * J["share"], J["e_min"], ", ".join("%s %.2f (%.1e)" % (k, ratios[k], err[k]) for k in OO.QUANTITIES)))
    for k in OO.QUANTITIES:
        assert err[k] <= 4 * J["e32"][k], (name, t, k, err[k], J["e32"][k])
    # rows beyond a cloud and the originals are untouched; the new world rows are the placement of the new state, bit for bit
    st, cat2 = raw["state"], dev(raw["before"])
    net.object_place(st["obj"], st["angle"], st["shift"], cat2, case["num_add"], case["obj_num_p"], n_ori=dev(case["n_ori"]))
    assert np.array_equal(bits(cat2), bits(raw["after"]))
    for b in range(case["B"]):
        n = int(case["n_ori"][b])
        assert np.array_equal(bits(raw["after"][b, :n]), bits(case["ori"][b, :n]))
        assert np.array_equal(bits(raw["after"][b, n + case["A"]:]), bits(raw["before"][b, n + case["A"]:]))


# ---------------------------------------------------------------------------------------------- 2. exact pieces
def test_placement_is_exact(net):
    rng = np.random.default_rng(11)
    B, n, na, P = 3, 20, 5, 7
    A = na * P
    obj = rng.standard_normal((B, A, 3)).astype(np.float32)
    shift = rng.standard_normal((B, na, 3)).astype(np.float32)
    angle = rng.uniform(0, OO.TWO_PI, (B, na)).astype(np.float32)
    ori = rng.standard_normal((B, n, 3)).astype(np.float32)
    cat = np.concatenate([ori, np.full((B, A + 2, 3), np.nan, np.float32)], 1)
    zero = net.object_place(obj, np.zeros_like(angle), shift, dev(cat), na, P, n_ori=np.full(B, n)).cpu().numpy()
    want = obj + np.repeat(shift, P, axis=1)
    assert np.array_equal(bits(zero[:, n:n + A]), bits(want))
    assert np.array_equal(bits(zero[:, :n]), bits(ori)) and np.isnan(zero[:, n + A:]).all()
    turned = net.object_place(obj, angle, shift, dev(cat), na, P, n_ori=np.full(B, n)).cpu().numpy()
    assert np.array_equal(bits(turned[:, n:n + A, 1]), bits(want[:, :, 1]))
    c, s = np.cos(angle.astype(np.float64)), np.sin(angle.astype(np.float64))
    c, s = np.repeat(c, P, 1), np.repeat(s, P, 1)
    x64 = obj[..., 0] * c - obj[..., 2] * s + np.repeat(shift, P, 1)[..., 0]
    z64 = obj[..., 0] * s + obj[..., 2] * c + np.repeat(shift, P, 1)[..., 2]
    assert np.abs(turned[:, n:n + A, 0] - x64).max() < 2e-6 and np.abs(turned[:, n:n + A, 2] - z64).max() < 2e-6
    assert not np.array_equal(turned[:, n:n + A, 0], zero[:, n:n + A, 0])


def integer_case(angle0):
    """A 'ragged' case with weight 0, small-integer gradient rows and (with angle0) angle 0 and object points on a 1/8 grid."""
    case = OO.make_step_case("ragged", 1)
    rng = np.random.default_rng(3)
    case["weight"] = np.zeros(case["B"])
    for b in range(case["B"]):
        n = int(case["n_ori"][b])
        case["grad"][b, n:n + case["A"]] = rng.integers(-8, 9, (case["A"], 3)).astype(np.float32)
    if angle0:
        case["angle"] = np.zeros_like(case["angle"])
        case["obj"] = (rng.integers(-16, 17, case["obj"].shape) / 8.0).astype(np.float32)
    return case


def test_gradient_sums_are_the_integer_sums(net):
    for angle0 in (False, True):
        case = integer_case(angle0)
        got, _ = gpu_step(net, case)
        for b, g in enumerate(got):
            n, na, P = int(case["n_ori"][b]), case["num_add"], case["obj_num_p"]
            gw = case["grad"][b, n:n + case["A"]].astype(np.float64).reshape(na, P, 3)
            assert np.array_equal(g["g_shift"], gw.sum(1).astype(np.float32)), (angle0, b)
            if angle0:
                o = case["obj"][b].astype(np.float64)
                assert np.array_equal(g["g_angle"], (gw[..., 2] * o[..., 0] - gw[..., 0] * o[..., 2]).sum(1).astype(np.float32)), b
                assert np.array_equal(bits(g["obj_grad"]), bits(gw.reshape(-1, 3).astype(np.float32)))      # the transposed rotation at 0


def test_remainder_is_torchs_and_nothing_else_moves(net):
    """Weight 0, zero gradient, zero moments: Adam's step is 0 / (0 + 1e-8) = 0, so the only thing that happens is the remainder."""
    case = OO.make_step_case("ref", 1)
    crafted = np.array([-0.5, 7.0, OO.TWO_PI + 0.5, -0.0, TWO_PI32, 5e-4, TWO_PI32 - np.float32(5e-4), -1e-3, 100.0, 0.0, 3.0, -7.0],
                       np.float32)
    case["angle"] = np.resize(crafted, case["angle"].shape).astype(np.float32)
    case["weight"] = np.zeros(case["B"])
    case["grad"] = np.where(np.isnan(case["grad"]), np.nan, 0).astype(np.float32)
    got, raw = gpu_step(net, case)
    want = torch.remainder(torch.from_numpy(case["angle"]), OO.TWO_PI).numpy()
    assert np.array_equal(bits(want), bits(OO.remainder32(case["angle"])))
    new = np.stack([g["angle"] for g in got])
    assert np.array_equal(bits(new), bits(want)) and (new >= 0).all() and (new < TWO_PI32).all()
    assert np.array_equal(bits(np.stack([g["obj"] for g in got])), bits(case["obj"].reshape(case["B"], -1, 3)))
    assert np.array_equal(bits(np.stack([g["shift"] for g in got])), bits(case["shift"]))


# ---------------------------------------------------------------------------------------------- 3. batching, untouched data, limits
def test_a_cloud_alone_in_a_batch_and_permuted_gives_the_same_bits(net):
    case = OO.make_step_case("ragged", 7)
    case["pred"] = case["target"].copy()
    keys = ("obj", "shift", "angle") + OO.MOMENTS + DIAG + ("info", "o_bestattack", "o_bestdist", "bestdist")
    full, raw = gpu_step(net, case, last=True)
    perm = np.array([3, 0, 4, 1, 2])
    _, rawp = gpu_step(net, case, perm, last=True)
    for j, b in enumerate(perm):
        _, raw1 = gpu_step(net, case, [b], last=True)
        for k in keys:
            assert np.array_equal(bits(raw["got"][k][b]), bits(rawp["got"][k][j])), (k, b)
            assert np.array_equal(bits(raw["got"][k][b]), bits(raw1["got"][k][0])), (k, b)
        assert np.array_equal(bits(raw["after"][b]), bits(rawp["after"][j])) and np.array_equal(bits(raw["after"][b]), bits(raw1["after"][0]))
    # last_input and o_bestattack are the forwarded world rows (every cloud hits its target, every record is fresh)
    for b in range(case["B"]):
        n, A = int(case["n_ori"][b]), case["A"]
        fwd = raw["before"][b, n:n + A]
        assert np.array_equal(bits(raw["last"][b]), bits(fwd)) and np.array_equal(bits(raw["got"]["o_bestattack"][b]), bits(fwd))
        assert not np.array_equal(raw["after"][b, n:n + A], fwd)


def test_clouds_outside_the_limits_are_left_untouched(net):
    case = OO.make_step_case("ragged", 7)
    case["n_ori"] = np.array([300, 0, 150, 304, -5], np.int32)         # stride 380 = 300 + 77 + 3: 304 + 77 > 380
    case["ori"] = np.nan_to_num(case["ori"], nan=0.25)
    case["grad"] = np.nan_to_num(case["grad"], nan=0.5)
    sel = np.arange(5)
    B, A, na, P = 5, case["A"], case["num_add"], case["obj_num_p"]
    st = net.object_state(B, na, P)
    for k in st:
        if st[k].dtype == torch.float32:
            st[k].fill_(3.0)
    st["obj"].copy_(dev(case["obj"].reshape(B, A, 3)))
    cat = torch.full((B, case["stride"], 3), 0.125, device="cuda")
    placed = net.object_place(st["obj"], st["angle"], st["shift"], cat.clone(), na, P, n_ori=case["n_ori"])
    snap = {k: v.clone() for k, v in st.items()}
    li = torch.full((B, A, 3), 7.0, device="cuda")
    work = placed.clone()
    d = net.object_step(st, case["objects"], dev(case["grad"]), case["target"], case["target"], work, na, P, 2, 1e-2, 0.25,
                        n_ori=case["n_ori"], last_input=li, want_info=False, want=DIAG)
    for b in (1, 3, 4):
        assert torch.equal(placed[b], cat[b]) and torch.equal(work[b], cat[b]) and (li[b] == 7.0).all()
        for k in st:
            assert torch.equal(st[k][b], snap[k][b]), (k, b)
        for k in DIAG:
            x = d[k][b]
            assert (x == -1).all() if x.dtype == torch.int32 else torch.isnan(x).all(), (k, b)
    for b in (0, 2):
        assert not torch.equal(work[b], placed[b]) and not torch.equal(st["obj"][b], snap["obj"][b]) and torch.isfinite(d["l2"][b])


def test_limits_are_refused_one_past_them(sd, net):
    import ifdefense_amd as I
    from ifdefense_amd import _lib, weights
    lib, ctx = net.lib, net.ctx
    f = lambda *s: torch.zeros(*s, device="cuda")                      # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")   # noqa: E731
    big, tt = f(1, 10001, 3), i(2)
    P, T = big.data_ptr(), tt.data_ptr()

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.ifd_last_error(ctx), (rc, word, lib.ifd_last_error(ctx))
    st = net.object_state(2, 32, 32)
    S = C.byref(net._object_struct(st, 2, 32, 1024))
    step = lambda cat_stride, num_add, P_, n=None, t=1, objects=P: lib.ifd_object_step(    # noqa: E731
        ctx, S, objects, P, T, None, T, P, n, None, None, None, t, 0.01, 1.0, 1, cat_stride, num_add, P_, None)
    refused(step(4096, 1025, 1), "num_add * obj_num_p")
    refused(step(4096, 33, 32), "num_add * obj_num_p")
    refused(step(4096, 0, 32), "num_add")
    refused(step(4096, 3, 0), "obj_num_p")
    refused(step(192, 3, 64), "cat_stride")
    refused(step(10001, 3, 64, T), "cat_stride")
    refused(step(2049 + 192, 3, 64), "2048 original rows")
    refused(step(400, 3, 64, None, 0), "t >= 1")
    refused(step(400, 3, 64, None, 1, None), "objects")
    broken = _lib.IfdObjectState(net._cw_struct(st, 2, 1024), st["obj"].data_ptr(), st["shift"].data_ptr(), None, *[P] * 4)
    assert lib.ifd_object_step(ctx, C.byref(broken), P, P, T, None, T, P, None, None, None, None, 1, 0.01, 1.0, 1, 400, 3, 64, None) == -1
    assert b"state missing" in lib.ifd_last_error(ctx)
    place = lambda cat_stride, num_add, P_, n=None, B=1, obj=P: lib.ifd_object_place(ctx, obj, P, P, P, n, B, cat_stride, num_add, P_, None)   # noqa: E731
    refused(place(4096, 33, 32), "num_add * obj_num_p")
    refused(place(192, 3, 64), "cat_stride")
    refused(place(10001, 3, 64, T), "cat_stride")
    refused(place(2049 + 192, 3, 64), "2048 original rows")
    refused(place(400, 3, 64, None, 0), "B >= 1")
    refused(place(400, 3, 64, None, 1, None), "obj")
    o, best, ok = f(2, 3100, 3), f(2), i(2)

    def attack(stride=128, out_stride=320, num_add=3, P_=64, loss=0, steps=1, it=1, size=C.sizeof(_lib.IfdObjectParams), n=None, B=2, out=None,
               centers=True, angles=True):
        prm = _lib.IfdObjectParams(size, loss, steps, it, num_add, P_, 0.0, 0.5, 0.01, 5., 40.)
        return lib.ifd_object_attack(ctx, C.byref(prm), P, None if n is None else n.data_ptr(), T, P, P if centers else None, None, None,
                                     P if angles else None, B, stride, out_stride, o.data_ptr() if out is None else out, best.data_ptr(),
                                     ok.data_ptr(), None, None)
    refused(attack(size=40), "struct_size")
    refused(attack(loss=5), "loss_kind")
    refused(attack(steps=0), "binary_step")
    refused(attack(it=0), "num_iter")
    refused(attack(num_add=0), "num_add")
    refused(attack(P_=0), "obj_num_p")
    refused(attack(num_add=17, out_stride=3100), "num_add * obj_num_p")
    refused(attack(stride=2049, out_stride=3100), "without n_points")
    refused(attack(out_stride=319), "without n_points")
    refused(attack(out_stride=10001), "out_stride")
    refused(attack(stride=10001), "stride outside")
    refused(attack(B=0), "B >= 1")
    refused(attack(centers=False), "missing pointer")
    refused(attack(angles=False), "missing pointer")
    refused(attack(out=P), "overlaps")
    refused(attack(n=dev(np.array([128, 0], np.int32))), "n_points outside [1, 128]")
    refused(attack(n=dev(np.array([129, 5], np.int32))), "n_points outside [1, 128]")
    refused(attack(out_stride=300, n=dev(np.array([109, 108], np.int32))), "n_points outside [1, 108]")
    assert not o.any() and not ok.any() and not best.any()
    z = torch.zeros
    with pytest.raises(I.IfdError, match="centers"):
        net.object_attack(z(2, 8, 3), [0, 1], z(2, 2, 3), z(2, 3, 3), z(1, 2, 2), binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="angles0"):
        net.object_attack(z(2, 8, 3), [0, 1], z(2, 2, 3), z(2, 2, 3), z(2, 2, 2), binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="noise_obj"):
        net.object_attack(z(2, 8, 3), [0, 1], z(2, 2, 3), z(2, 2, 3), z(1, 2, 2), z(1, 2, 5, 3), binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="target"):
        net.object_attack(z(2, 8, 3), [0, 40], z(2, 2, 3), z(2, 2, 3), z(1, 2, 2), binary_step=1, num_iter=1)
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, True), "pointnet"), feature_transform=True, device="cuda:0") as ft:
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.object_attack(z(2, 8, 3), [0, 1], z(2, 2, 3), z(2, 2, 3), z(1, 2, 2), binary_step=1, num_iter=1)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.object_place(z(2, 4, 3), z(2, 2), z(2, 2, 3), f(2, 12, 3), 2, 2)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.object_step(ft.object_state(2, 2, 2), z(2, 2, 3), f(2, 12, 3), [0, 0], [0, 0], f(2, 12, 3), 2, 2, 1, 0.01)
    # the limits themselves work: one original row, 1024 added rows, the whole attack
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2, 1, 3)).astype(np.float32)
    out, _, _ = net.object_attack(x, [0, 1], 0.3 * rng.standard_normal((32, 32, 3)).astype(np.float32),
                                  rng.standard_normal((2, 32, 3)).astype(np.float32), rng.uniform(0, 3, (1, 2, 32)).astype(np.float32),
                                  binary_step=1, num_iter=2)
    assert np.array_equal(bits(out[:, :1]), bits(x)) and np.isfinite(out.cpu().numpy()).all() and tuple(out.shape) == (2, 1025, 3)


# ---------------------------------------------------------------------------------------------- 4. records and the distance
def test_record_logic_and_adjustment_are_exact(net):
    """test_gpu_add's record table on this state, then ifd_cw_adjust as it is: the <=."""
    case = OO.make_step_case("ref", 1)
    B, A = 5, case["A"]
    sel = np.arange(B)
    marker = np.full((B, A, 3), 7.0, np.float32)
    #          hit, smaller     hit, larger      miss, smaller   (equal: below)   hit, smaller than bestdist only
    case["pred"][:B], case["target"][:B] = np.array([3, 3, 4, 3, 3], np.int32), 3
    over = dict(bestdist=np.array([10., 1e-9, 10., 1e10, 10.], np.float32), o_bestdist=np.array([10., 1e-9, 10., 1e10, 1e-9], np.float32),
                bestscore=np.full(B, -5), o_bestscore=np.full(B, -5), o_bestattack=marker)
    got, raw = gpu_step(net, case, sel, **over)
    dist = np.array([g["dist"] for g in got], np.float32)
    l2, cd = np.array([g["l2"] for g in got]), np.array([g["cd"] for g in got])
    assert np.array_equal(bits(dist), bits((l2 + (cd * np.float32(0.2)).astype(np.float32)).astype(np.float32))) and np.all(dist > 1e-3)
    w = case["weight"][:B].astype(np.float32)
    assert np.array_equal(bits(raw["got"]["info"][:, 1]), bits(((l2 * w).astype(np.float32) + ((cd * w).astype(np.float32) * np.float32(0.2))
                                                                 .astype(np.float32)).astype(np.float32)))
    g = raw["got"]
    assert np.array_equal(g["bestdist"], np.array([dist[0], 1e-9, 10., dist[3], dist[4]], np.float32))
    assert np.array_equal(g["bestscore"], [3, -5, -5, 3, 3])
    assert np.array_equal(g["o_bestdist"], np.array([dist[0], 1e-9, 10., dist[3], 1e-9], np.float32))
    assert np.array_equal(g["o_bestscore"], [3, -5, -5, 3, -5])
    for b, written in enumerate([True, False, False, True, False]):    # o_bestattack: the forwarded world rows
        assert np.array_equal(bits(g["o_bestattack"][b]), bits(raw["before"][b, 64:64 + A] if written else marker[b])), b
    # the same clouds through again with the records AT the distances: < is strict, nothing is written
    over2 = dict(over, bestdist=dist, o_bestdist=dist, bestscore=np.full(B, -9), o_bestscore=np.full(B, -9))
    got2, raw2 = gpu_step(net, case, sel, **over2)
    assert np.array_equal(bits(np.array([x["dist"] for x in got2], np.float32)), bits(dist))
    assert np.array_equal(bits(raw2["got"]["bestdist"]), bits(dist)) and np.array_equal(bits(raw2["got"]["o_bestdist"]), bits(dist))
    assert np.array_equal(bits(raw2["got"]["o_bestattack"]), bits(marker)) and np.array_equal(raw2["got"]["o_bestscore"], np.full(B, -9))
    # the adjustment on this state: bestdist == o_bestdist with the right class is a success (<=), above it or the wrong class a failure
    st, target = raw2["state"], case["target"][:B]
    st["weight"].fill_(5.0)
    st["bestscore"].copy_(dev(np.array([3, 3, 4, 3, -1], np.int32)))
    st["bestdist"].copy_(dev(np.array([0.5, 0.75, 0.25, 0.25, 1e10], np.float32)))
    st["o_bestdist"].copy_(dev(np.array([0.5, 0.5, 0.5, 0.5, 1e10], np.float32)))
    st["m"].fill_(1.0)
    net.cw_adjust(st, target)
    assert np.array_equal(st["lower"].cpu().numpy(), [5., 0, 0, 5., 0]) and np.array_equal(st["upper"].cpu().numpy(), [40., 5., 5., 40., 5.])
    assert np.array_equal(st["weight"].cpu().numpy(), [22.5, 2.5, 2.5, 22.5, 2.5]) and st["weight"].dtype == torch.float64
    assert not st["m"].any() and np.array_equal(st["bestscore"].cpu().numpy(), np.full(B, -1))


def test_zero_l2_is_finite_and_weight_zero_ignores_the_distance(net):
    case = OO.make_step_case("ref", 1)
    case["obj"] = np.broadcast_to(case["objects"][None], case["obj"].shape).copy()         # no noise: l2 == 0
    got, _ = gpu_step(net, case)
    y = OO.run_step_case(case, torch.float64)
    for g, r in zip(got, y):
        assert g["l2"] == 0 and all(np.isfinite(g[k]).all() for k in ("obj", "shift", "angle", "obj_grad", "world", "dist"))
        assert g["dist"] == np.float32(g["cd"] * np.float32(0.2))
        ro = g["nn"] != r["nn"]
        assert ro.mean() <= 0.05 and np.abs(g["obj_grad"] - r["obj_grad"].reshape(-1, 3))[~ro].max() < 1e-6      # no L2 gradient, no NaN
    # weight 0: another cloud of originals changes the distance and the nearest originals, and no other bit
    case = OO.make_step_case("ref", 7)
    case["weight"] = np.zeros(case["B"])
    a, ra = gpu_step(net, case)
    other = dict(case, ori=np.roll(case["ori"], 1, axis=0) * np.float32(0.5))
    b, rb = gpu_step(net, other)
    for k in ("obj", "shift", "angle") + OO.MOMENTS + ("obj_grad", "g_shift", "g_angle"):
        assert np.array_equal(bits(ra["got"][k]), bits(rb["got"][k])), k
    assert np.array_equal(bits(ra["after"][:, 64:]), bits(rb["after"][:, 64:])) and not np.array_equal(ra["got"]["cd"], rb["got"]["cd"])
    assert not ra["got"]["info"][:, 1].any()


# ---------------------------------------------------------------------------------------------- 5. through the network
def test_loop_teacher_forced_through_the_network(net, sd, W64, clouds, airplane):
    """B = 17, 64 + 3 x 16 points, 3 iterations driven from the host from the object + 0.05 randn at 3 critical points.  After each
    iteration every array of the new state against the oracle's ONE step from the GPU's previous state with the GPU's own gradient
    (the bar of test 1), and the gradient of the concatenated cloud at that state by test_gpu_atk's row-wise rule."""
    from ifdefense_amd import attack as Atk
    B, n, na, P, lr = 17, 64, 3, 16, 1e-2
    A = na * P
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    objects = Atk.prepare_objects(airplane, 0.3, na, P, np.random.RandomState(0)).astype(np.float32)
    rng = np.random.default_rng(2)
    weight = 5.
    st = net.object_state(B, na, P, weight, 40.)
    st["obj"].copy_(dev((objects.reshape(1, A, 3) + 0.05 * rng.standard_normal((B, A, 3))).astype(np.float32)))
    st["shift"].copy_(net.add_critical_points(x, tg, na, 1.0 / B))
    st["angle"].copy_(dev(rng.uniform(0, np.pi, (B, na)).astype(np.float32)))
    cat = torch.cat([dev(x), torch.zeros(B, A, 3, device="cuda")], 1).contiguous()
    net.object_place(st["obj"], st["angle"], st["shift"], cat, na, P)
    keys = ("obj", "shift", "angle") + OO.MOMENTS
    done = 0
    for k in (1, 2, 3):
        prev = {q: st[q].cpu().numpy() for q in keys}
        before = cat.cpu().numpy()
        grad, aux = net.input_grad(cat, tg, scale=1.0 / B, want_aux=True)
        g, aux = grad.cpu().numpy(), {a: b.cpu().numpy() for a, b in aux.items()}
        d = net.object_step(st, objects, grad, aux["pred"], tg, cat, na, P, k, lr, 1.0 / B, loss=aux["loss"], want=("nn_ori",))
        nn = d["nn_ori"].cpu().numpy()
        new = {q: st[q].cpu().numpy() for q in keys}
        after = cat.cpu().numpy()
        assert np.array_equal(bits(after[:, :n]), bits(x))

        def one(i, dtype, forced=None):
            npdt = np.float32 if dtype == torch.float32 else np.float64
            mom = {q: prev[q][i].reshape(na, P, 3).astype(npdt) if q in ("m", "v") else prev[q][i].astype(npdt) for q in OO.MOMENTS}
            return OO.step(g[i, n:].astype(npdt), int(aux["pred"][i]), int(tg[i]), prev["obj"][i].reshape(na, P, 3).astype(npdt),
                           prev["shift"][i].astype(npdt), prev["angle"][i].astype(npdt), objects.astype(npdt), x[i].astype(npdt), weight,
                           mom, k, lr, 1.0 / B, OO.fresh_record(A, npdt), dtype, forced)
        s64, s32 = [one(i, torch.float64) for i in range(B)], [one(i, torch.float32) for i in range(B)]
        e_min = max(float(np.abs(q["min_p"].astype(np.float64) - r["min_p"]).max()) for q, r in zip(s32, s64))
        e_gpu, e_32 = {q: 0.0 for q in keys + ("world",)}, {q: 0.0 for q in keys + ("world",)}
        n_out = 0
        for i in range(B):
            ro = OO.DO.exclusions(s64[i]["forwarded"], x[i], e_min, "chamfer")[0]
            n_out += int(ro.sum())
            assert np.array_equal(nn[i][~ro], s64[i]["nn"][~ro]) and np.array_equal(s32[i]["nn"][~ro], s64[i]["nn"][~ro]), (k, i)
            y_gpu = one(i, torch.float64, np.where(ro, nn[i], s64[i]["nn"])) if ro.any() else s64[i]
            y_32 = one(i, torch.float64, np.where(ro, s32[i]["nn"], s64[i]["nn"])) if ro.any() else s64[i]
            for q in keys + ("world",):
                mine = after[i, n:] if q == "world" else new[q][i]
                e_gpu[q] = max(e_gpu[q], float(np.abs(mine.reshape(-1) - y_gpu[q].reshape(-1)).max()))
                e_32[q] = max(e_32[q], float(np.abs(s32[i][q].astype(np.float64).reshape(-1) - y_32[q].reshape(-1)).max()))
        assert n_out <= 0.05 * B * A
        print("iteration %d: |GPU - f64| / e_32: %s; %d rows excluded" % (
            k, ", ".join("%s %.2f" % (q, e_gpu[q] / e_32[q] if e_32[q] else 0.0) for q in e_gpu), n_out))
        for q in e_gpu:
            assert e_gpu[q] <= 4 * e_32[q], (k, q, e_gpu[q], e_32[q])
        r32, r64, e, e32, ex = AO.run_case(sd, [c for c in before], tg, scale=1.0 / B)
        AO.case_conditions(r64, e)
        for i in range(B):
            why, rows_out = AO.row_exclusion(r64[i], e)
            if why:
                continue
            f = AO.run_cloud(W64, before[i], tg[i], scale=1.0 / B, force_feat=aux["win_feat"][i], force_stn=aux["win_stn"][i])
            AO.check_grad(g[i], f["grad"], e32, "iteration %d cloud %d" % (k, i), rows_out)
            done += 1
    assert done >= 0.9 * 3 * B


# ---------------------------------------------------------------------------------------------- 6. fused = host-driven
def test_fused_and_host_driven_loops_give_the_same_bits(net, clouds, airplane, capsys):
    """16 clouds x (192 + 3 x 32) points, 2 search steps x 20 iterations, targets (prediction + 1) % 40, the reference script's weights."""
    from ifdefense_amd import attack as A
    B, n, na, P = 16, 192, 3, 32
    add = na * P
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    kw = dict(binary_step=2, num_iter=20, num_add=na, obj_num_p=P, seed=3)
    a = A.CWAddObjects(net, airplane, **kw).attack(x, tg)
    out = capsys.readouterr().out
    b = A.CWAddObjects(net, airplane, verbose=False, **kw).attack(x, tg)
    quiet = capsys.readouterr().out
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[1].shape == (B, n + add, 3) and a[1].dtype == np.float32 and np.array_equal(bits(a[1][:, :n]), bits(x))
    for s in range(2):
        for it in (0, 4, 8, 12, 16):
            assert out.count("Step %d, iteration %d, success" % (s, it)) == 1
    assert out.count("adv_loss: ") == 10 and "time" not in out and "total" not in out
    assert out.count("Successfully attack %d/%d" % (a[2], B)) == 1 and quiet == "Successfully attack %d/%d\n" % (a[2], B)
    # the library call itself: the same objects, centres and draws, the same bits, success = lower > 0, the records
    atk = A.CWAddObjects(net, airplane, **kw)
    objects = torch.from_numpy(atk.object_pc).float()
    centers = atk._init_centers(torch.from_numpy(x), torch.from_numpy(tg))
    no, ns, an = atk.draws(torch.from_numpy(x))
    cri = net.add_critical_points(x, tg, 128, 1.0 / B).cpu().numpy()
    for i in range(B):                                                 # every centre is one of the cloud's 128 critical points
        assert (centers[i].numpy()[:, None] == cri[i][None]).all(2).any(1).all()
    args = dict(scale=1.0 / B, binary_step=2, num_iter=20, want_bounds=True)
    o1 = net.object_attack(x, tg, objects, centers, an, no, ns, **args)
    pc, best, ok, lower = o1[0].cpu().numpy(), o1[1].cpu().numpy(), o1[2].cpu().numpy(), o1[3]["lower"].cpu().numpy()
    assert np.array_equal(bits(pc), bits(b[1])) and np.array_equal(best.astype(np.float64), b[0])
    assert np.array_equal(ok, lower > 0) and ok.sum() == a[2]
    assert np.all(best[ok] < 1e10) and np.all(best[ok] >= 0)
    pred = net.predict(o1[0]).cpu().numpy()
    assert np.array_equal(pred[ok], tg[ok])                             # exact: the forward pass is batch-independent
    # clouds that never succeeded carry the last forwarded rows: after ONE iteration those are the placement of the start itself
    s1 = net.object_attack(x, tg, objects, centers, an[:1], no[:1], ns[:1], **dict(args, binary_step=1, num_iter=1))
    fail = ~s1[2].cpu().numpy()
    assert fail.sum() >= 1 and np.all(s1[1].cpu().numpy()[fail] == np.float32(1e10))
    start = torch.zeros(B, n + add, 3, device="cuda")
    net.object_place(objects.reshape(1, add, 3).cuda() + no[0].cuda(), an[0], centers.cuda() + ns[0].cuda(), start, na, P)
    assert np.array_equal(bits(s1[0][:, n:])[fail], bits(start[:, n:])[fail])
    # a padded, ragged, permuted batch gives the same per-cloud bits
    p = np.array([4, 0, 5, 2, 1, 3])
    xr = np.full((6, n + 5, 3), np.nan, np.float32)
    counts = np.array([n, n - 7, n, 1, n - 1, 64], np.int32)
    for j, i in enumerate(p):
        xr[j, :counts[j]] = x[i, :counts[j]]
    o2 = net.object_attack(xr, tg[p], objects, centers[p], an[:, p], no[:, p], ns[:, p], n_points=counts, out_stride=n + add + 3, **args)
    same = [j for j in range(6) if counts[j] == n]
    o3 = net.object_attack(x[p][same], tg[p][same], objects, centers[p][same], an[:, p][:, same], no[:, p][:, same], ns[:, p][:, same], **args)
    pc2, pc3 = o2[0].cpu().numpy(), o3[0].cpu().numpy()
    for k, j in enumerate(same):
        assert np.array_equal(bits(pc2[j, :n + add]), bits(pc3[k])) and np.array_equal(bits(pc3[k]), bits(pc[p[j]]))
        assert o2[1][j] == o3[1][k] == o1[1][p[j]]
    for j in range(6):
        c = int(counts[j])
        assert np.array_equal(bits(pc2[j, :c]), bits(xr[j, :c])) and np.isfinite(pc2[j, c:c + add]).all() and not pc2[j, c + add:].any()
    print("CW Add-Objects: %d/%d clouds attacked, mean best_dist %.3e" % (ok.sum(), B, best[ok].mean() if ok.any() else np.nan))


# ---------------------------------------------------------------------------------------------- 7. the CLI
def test_cli_end_to_end(net, sd, airplane, tmp_path, capsys):
    from ifdefense_amd import inference as Inf, object_attack as OA
    import bench
    ck, src, obj = str(tmp_path / "pointnet.npz"), str(tmp_path / "attack_data.npz"), str(tmp_path / "airplane.npy")
    np.savez(ck, **sd)
    np.save(obj, airplane)
    pcs = bench.synth_clouds(20, seed=5)[:, :192]
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pcs])).cpu().numpy()
    label, target = pred.astype(np.uint8), ((pred + 1) % 40).astype(np.uint8)
    np.savez(src, test_pc=pcs, test_label=label, target_label=target)
    assert OA.main(["--data_root", src, "--obj_root", obj, "--num_points", "192", "--num_add", "3", "--obj_num_p", "16", "--binary_step", "2",
                    "--num_iter", "20", "--batch_size", "16", "--model_path", ck, "--out_dir", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Successfully attack")]
    counts = [int(l.split()[-1].split("/")[0]) for l in lines]
    assert [l.split("/")[-1] for l in lines] == ["16", "4"]
    d = tmp_path / "attack" / "results" / "mn40_192" / "Object" / "3-16"
    (name,) = os.listdir(d)
    assert name == "Object-pointnet-logits_kappa=0.0-success_%.4f-rank_0.npz" % (sum(counts) / 20.0)
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (20, 240, 3) and np.isfinite(z["test_pc"]).all()
    assert np.array_equal(z["test_pc"][:, :192], np.stack([Inf.normalize_points_np(c) for c in pcs]))
    assert np.array_equal(z["test_label"], label) and np.array_equal(z["target_label"], target)
    assert Inf.main(["--data_root", str(d / name), "--mode", "target", "--model", "pointnet", "--model_path", ck, "--num_points", "240"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    rate = float(line.split("attack success rate:")[1])
    print("object_attack's rate %.4f, inference's rate on the written file %.4f" % (sum(counts) / 20.0, rate))
    assert abs(rate - sum(counts) / 20.0) < 5e-5                        # the rate in the file name, to its four decimals
