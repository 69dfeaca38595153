"""GPU checks of the CW point-adding attack (include/ifd_add.h) against tests/add_oracle.py.

The selection is exact: its total order (descending score, lowest index first) leaves no bit open.  The step is judged
teacher-forced: one iteration from a given state against the float64 oracle's one iteration from the same state, at 4 x the float32
oracle's own error per quantity (maximum over the case), outside the rows the oracle alone calls undecidable at float32
(add_oracle.exclusions); the nearest original and the Hausdorff arg-max are read from ifd_add_step's optional diagnostics and must
equal the float64 oracle's there.  Parity always starts from critical points + 0.02 randn, never from the reference's 1e-7 start,
where its distances are rounding noise.  Everything discrete - ties, the records, the weight's binary search, batching, fused
against host-driven - is exact."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import add_oracle as DO
import atk_oracle as AO
import pointnet_oracle as PO

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")


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
        assert all(hasattr(c, k) for k in ("add_select", "add_critical_points", "add_step", "add_attack"))
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
    st = net.cw_state(B, A, 5e3, 4e4)
    for k, v in over.items():
        st[k] = dev(np.asarray(v), st[k].dtype).reshape(st[k].shape).contiguous()
    return st


# ---------------------------------------------------------------------------------------------- 1. the selection
def _select_case(name):
    """-> (grad [B,stride,3], pc, n_points or None, num_add list)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    mk = lambda B, s: (rng.standard_normal((B, s, 3)).astype(np.float32), rng.standard_normal((B, s, 3)).astype(np.float32))   # noqa: E731
    if name == "n64":
        g, p = mk(3, 64)
        return g, p, None, [1, 16, 64]
    if name == "ragged300":                                            # stride 320, NaN beyond each cloud's rows
        g, p = mk(3, 320)
        n = np.array([300, 77, 256], np.int32)
        for b in range(3):
            g[b, n[b]:] = np.nan
            p[b, n[b]:] = np.nan
        return g, p, n, [77]
    if name == "zeros1024":                                            # the measured worst case: 212 live rows, 512 wanted
        g, p = mk(2, 1024)
        for b, live in enumerate((212, 335)):
            dead = rng.permutation(1024)[live:]
            g[b, dead] = 0.
        return g, p, None, [512]
    if name == "n2048":
        g, p = mk(2, 2048)
        g[1, rng.permutation(2048)[:1500]] = 0.
        return g, p, None, [1024]
    if name == "ties":                                                 # equal non-zero scores straddling the boundary
        g, p = mk(2, 100)
        g[:] = 0.
        vals = np.repeat(np.array([4., 3., 3., 2., 2., 2., 1.], np.float32), [5, 10, 10, 10, 10, 10, 45])
        for b in range(2):
            g[b, :, b] = vals[rng.permutation(100)]                    # sign and axis do not matter to the score
            g[b, ::2, b] *= -1
        return g, p, None, [3, 5, 6, 20, 26, 40, 55, 56]
    assert name == "allzero"
    g, p = mk(2, 80)
    return np.zeros_like(g), p, None, [1, 33, 80]


@pytest.mark.parametrize("name", ["n64", "ragged300", "zeros1024", "n2048", "ties", "allzero"])
def test_select_is_the_stable_descending_sort_bit_for_bit(net, name):
    grad, pc, n_points, adds = _select_case(name)
    for num_add in adds:
        cri, idx = net.add_select(dev(grad), dev(pc), num_add, n_points=n_points, want_idx=True)
        cri, idx = cri.cpu().numpy(), idx.cpu().numpy()
        for b in range(len(pc)):
            n = pc.shape[1] if n_points is None else int(n_points[b])
            want = DO.select(grad[b, :n], num_add)
            assert np.array_equal(idx[b], want), (name, num_add, b)
            assert np.array_equal(bits(cri[b]), bits(pc[b, want])), (name, num_add, b)
    if name == "allzero":
        assert np.array_equal(idx[0], np.arange(80))
    if name == "zeros1024":
        assert not DO.scores(grad[0])[idx[0, 212:]].any() and np.all(np.diff(idx[0, 212:]) > 0)     # the zero rows in index order


def test_critical_points_is_select_on_input_grads_own_output(net, clouds):
    x = clouds[:6, :96].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    big = net.add_critical_points(clouds[:8, :512].copy(), np.arange(8), 128, 0.125)     # leaves a larger workspace behind
    assert tuple(big.shape) == (8, 128, 3)
    for n_points in (None, np.array([96, 40, 64, 33, 95, 32], np.int32)):
        grad = net.input_grad(x, tg, "cross_entropy", 0., 1.0 / 6, n_points=n_points)
        a = net.add_select(grad, x, 32, n_points=n_points, want_idx=True)
        b = net.add_critical_points(x, tg, 32, 1.0 / 6, n_points=n_points, want_idx=True)
        assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
        assert len(set(a[1][0].tolist())) == 32


# ---------------------------------------------------------------------------------------------- 2. one step, teacher-forced
def run_step(net, case, sel=None, weight=None, want=("dist_grad", "nn_ori", "far"), use_counts=True):
    """One ifd_add_step on the clouds `sel` of a case -> dict of numpy arrays."""
    sel = np.arange(case["B"]) if sel is None else np.asarray(sel)
    A = case["A"]
    w = case["weight"] if weight is None else weight
    marker = np.full((len(sel), A, 3), 7.0, np.float32)
    st = make_state(net, len(sel), A, m=case["m"][sel], v=case["v"][sel], weight=np.asarray(w)[sel], o_bestattack=marker)
    cat, last = dev(case["cat"][sel]), dev(marker)
    out = net.add_step(case["kind"], st, dev(case["grad"][sel]), case["pred"][sel], case["target"][sel], cat, A, case["t"], DO.STEP_LR,
                       DO.STEP_SCALE, last_input=last, n_ori=case["n_ori"][sel] if use_counts else None, want_info=True, want=want)
    return {k: x.cpu().numpy() for k, x in dict(st, cat=cat, last=last, **out).items()}


_ORACLE = {}


def oracle_case(name, kind, t):
    key = (name, kind, t)
    if key not in _ORACLE:
        case = DO.make_step_case(name, kind, t)
        r32, r64 = DO.run_step_case(case, torch.float32), DO.run_step_case(case, torch.float64)
        _ORACLE[key] = (case, r32, r64, DO.judge_step_case(case, r32, r64))
    return _ORACLE[key]


@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("kind", DO.KINDS)
@pytest.mark.parametrize("name", [c[0] for c in DO.STEP_CASES])
def test_step_parity_teacher_forced(net, name, kind, t):
    """add_oracle.STEP_CASES: 5 ragged clouds of up to 300 + 77 rows in a stride of 380 with NaN beyond, 17 x (64 + 16), 2 x (1024 +
    512), 1 x (2048 + 1024), from ori[idx] + 0.02 randn.  judge_step_case asserts the conditions from the oracle alone (at most
    5 % of the rows excluded, no Hausdorff cloud excluded).  Measured ratios |GPU - f64| / e_32 are printed; DESIGN 7g records them."""
    case, r32, r64, (e, rows_out, _, e32, share) = oracle_case(name, kind, t)
    got = run_step(net, case, use_counts=name == "ragged")
    B, A = case["B"], case["A"]
    err = {k: 0.0 for k in e32}
    for b in range(B):
        n, keep = int(case["n_ori"][b]), ~rows_out[b]
        # original rows and rows beyond the cloud: untouched, bit for bit
        assert np.array_equal(bits(got["cat"][b, :n]), bits(case["cat"][b, :n])) and np.array_equal(bits(got["cat"][b, n + A:]), bits(case["cat"][b, n + A:]))
        assert np.array_equal(bits(got["last"][b]), bits(case["cat"][b, n:n + A]))          # input_val: the pre-update rows
        assert np.array_equal(got["nn_ori"][b][keep], r64[b]["nn"][keep]), (name, kind, t, b)
        assert got["far"][b] == r64[b]["far"], (name, kind, t, b)
        for k, g in (("adv", got["cat"][b, n:n + A]), ("m", got["m"][b]), ("v", got["v"][b]), ("dist_grad", got["dist_grad"][b])):
            err[k] = max(err[k], float(np.abs(g.astype(np.float64) - r64[b][k])[keep].max()))
        err["dist"] = max(err["dist"], abs(float(got["info"][b, 2]) - float(r64[b]["dist"])))
        hit = case["pred"][b] == case["target"][b]
        assert got["bestscore"][b] == (case["pred"][b] if hit else -1) and got["bestdist"][b] == (got["info"][b, 2] if hit else np.float32(1e10))
        assert np.array_equal(bits(got["o_bestattack"][b]), bits(case["cat"][b, n:n + A] if hit else np.full((A, 3), 7.0, np.float32)))
    assert np.array_equal(got["info"][:, 1], got["info"][:, 2] * case["weight"].astype(np.float32))
    print("%s %s t=%d: e %.2e, excluded %.2f %%, " % (name, kind, t, e, 100 * share) +
          ", ".join("%s |GPU - f64| %.2e = %.2f e_32" % (k, err[k], err[k] / e32[k]) for k in err))
    for k in err:
        assert e32[k] > 0 and err[k] <= 4 * e32[k], (k, err[k], e32[k])


# ---------------------------------------------------------------------------------------------- 3. exact
@pytest.mark.parametrize("kind", DO.KINDS)
def test_a_cloud_alone_in_a_batch_and_permuted_gives_the_same_bits(net, kind):
    case = DO.make_step_case("ragged", kind, 7)
    full = run_step(net, case)
    one = run_step(net, case, sel=[2])
    perm = np.array([3, 0, 4, 2, 1])
    mixed = run_step(net, case, sel=perm)
    for k in ("cat", "m", "v", "info", "bestdist", "o_bestattack", "dist_grad", "nn_ori", "far"):
        assert np.array_equal(bits(one[k][0]), bits(full[k][2])), k
        assert np.array_equal(bits(mixed[k]), bits(full[k])[perm]), k
    # cloud 1 has num_add == n_ori
    assert case["n_ori"][1] == case["A"] and full["nn_ori"][1].min() >= 0 and full["nn_ori"][1].max() < case["A"]


@pytest.mark.parametrize("kind", DO.KINDS)
def test_clouds_outside_the_limits_are_left_untouched(net, kind):
    """The step never blocks, so a count it cannot take (n_ori < num_add, n_ori + num_add > cat_stride, n_ori > 2048) leaves the
    cloud as it was, in every array; its neighbours in the batch are served."""
    case = DO.make_step_case("ragged", kind, 7)
    bad = dict(case, n_ori=case["n_ori"].copy())
    bad["n_ori"][[0, 2, 4]] = [case["A"] - 1, case["stride"] - case["A"] + 1, 2049]
    ok, got = run_step(net, case), run_step(net, bad)
    for b in (0, 2, 4):
        assert np.array_equal(bits(got["cat"][b]), bits(case["cat"][b]))
        assert np.array_equal(bits(got["m"][b]), bits(case["m"][b])) and np.array_equal(bits(got["v"][b]), bits(case["v"][b]))
        assert got["bestdist"][b] == np.float32(1e10) and got["far"][b] == -1 and np.all(got["nn_ori"][b] == -1)
        assert not (got["last"][b] != 7.0).any() and not (got["o_bestattack"][b] != 7.0).any()
    for b in (1, 3):
        assert np.array_equal(bits(got["cat"][b]), bits(ok["cat"][b]))


def _crafted(kind):
    """One cloud: 8 originals on a lattice of spacing 4 - 0 and 5 swapped, so the lower INDEX is not the one met first in space -
    and 4 added points:
      p0  midway between ori 1 and ori 3: equidistant (4 each), must take index 1
      p1  ori 2 + (0.5, 0, 0), p2  ori 6 + (0, 0.5, 0): equal min_p 0.25; p3 on ori 7 exactly (min_p 0)
    Hausdorff: arg-max p0 (4).  All coordinates are small integers and halves: every distance is exact in float32."""
    ori = np.array([[x, y, z] for x in (0., 4.) for y in (0., 4.) for z in (0., 4.)], np.float32)
    ori[[0, 5]] = ori[[5, 0]]
    adv = np.stack([(ori[1] + ori[3]) / 2, ori[2] + np.float32([0.5, 0, 0]), ori[6] + np.float32([0, 0.5, 0]), ori[7]]).astype(np.float32)
    rng = np.random.default_rng(4)
    grad = (rng.standard_normal((1, 12, 3)) * 0.01).astype(np.float32)
    return {"name": "crafted", "kind": kind, "t": 3, "B": 1, "A": 4, "stride": 12, "n_ori": np.array([8], np.int32),
            "cat": np.concatenate([ori, adv])[None].copy(), "grad": grad, "m": (rng.standard_normal((1, 4, 3)) * 0.01).astype(np.float32),
            "v": (rng.random((1, 4, 3)) * 1e-3 + 1e-8).astype(np.float32), "weight": np.array([300.]), "target": np.array([3], np.int32),
            "pred": np.array([3], np.int32)}


@pytest.mark.parametrize("kind", DO.KINDS)
def test_crafted_ties_take_the_lower_index(net, kind):
    case = _crafted(kind)
    got, zero = run_step(net, case), run_step(net, case, weight=np.array([0.]))
    assert np.array_equal(got["nn_ori"][0], [1, 2, 6, 7])
    if kind == "chamfer":
        assert got["info"][0, 2] == np.float32((4 + 0.25 + 0.25 + 0) / 4) and got["far"][0] == -1
        moved = [0, 1, 2]
    else:
        assert got["info"][0, 2] == 4 and got["far"][0] == 0
        moved = [0]
    new, new0 = got["cat"][0, 8:], zero["cat"][0, 8:]
    for p in range(4):
        same = np.array_equal(bits(new[p]), bits(new0[p])) and np.array_equal(bits(got["m"][0, p]), bits(zero["m"][0, p]))
        assert same == (p not in moved), (kind, p)
        assert (got["dist_grad"][0, p] != 0).any() == (p in moved)
    # two added points with equal min_p under Hausdorff: the lower index receives the term, the other has the bits of weight 0
    if kind == "hausdorff":
        case["cat"][0, 8] = case["cat"][0, 7]                          # p0 onto ori 7: the maximum is now the pair p1, p2
        got, zero = run_step(net, case), run_step(net, case, weight=np.array([0.]))
        assert got["info"][0, 2] == 0.25 and got["far"][0] == 1
        assert (got["dist_grad"][0, 1] != 0).any() and not got["dist_grad"][0, [0, 2, 3]].any()
        assert not np.array_equal(bits(got["cat"][0, 9]), bits(zero["cat"][0, 9]))
        for k in ("cat", "m", "v"):
            assert np.array_equal(bits(np.delete(got[k][0], 9 if k == "cat" else 1, 0)), bits(np.delete(zero[k][0], 9 if k == "cat" else 1, 0))), k


@pytest.mark.parametrize("kind", DO.KINDS)
def test_coincident_points_have_distance_zero_and_the_bits_of_weight_zero(net, kind):
    case = DO.make_step_case("small", kind, 7)
    for b in range(case["B"]):
        idx = np.random.default_rng(b).permutation(64)[:16]
        case["cat"][b, 64:] = case["cat"][b, idx]
    got, zero = run_step(net, case), run_step(net, case, weight=np.zeros(case["B"]))
    assert not got["info"][:, 2].any() and not got["info"][:, 1].any() and not got["dist_grad"].any()
    assert np.isfinite(got["cat"]).all() and np.isfinite(got["m"]).all() and np.isfinite(got["v"]).all()
    for k in ("cat", "m", "v", "bestdist", "o_bestattack"):
        assert np.array_equal(bits(got[k]), bits(zero[k])), k
    assert not np.array_equal(bits(got["cat"]), bits(case["cat"]))      # Adam still moves them along the adversarial gradient
    if kind == "hausdorff":
        assert not got["far"].any()                                     # all equal: the lowest added point


def test_limits_are_refused_one_past_them(sd, net):
    import ifdefense_amd as I
    from ifdefense_amd import _lib, weights
    lib, ctx = net.lib, net.ctx
    f = lambda *s: torch.zeros(*s, device="cuda")                      # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")   # noqa: E731
    big = f(1, 10001, 3)
    tt, cri, idx = i(2), f(2, 1025, 3), i(2, 1025)
    P, T = big.data_ptr(), tt.data_ptr()

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.ifd_last_error(ctx), (rc, word, lib.ifd_last_error(ctx))
    sel = lambda B, stride, num_add, n=None: lib.ifd_add_select(ctx, P, P, n, B, stride, num_add, cri.data_ptr(), idx.data_ptr(), None)   # noqa: E731
    refused(sel(1, 2048, 1025), "num_add")
    refused(sel(1, 2048, 0), "num_add")
    refused(sel(1, 2049, 16), "stride outside [num_add, 2048]")
    refused(sel(1, 15, 16), "stride outside [num_add, 2048]")
    refused(sel(1, 10001, 16, T), "stride outside [1, 10000]")
    refused(sel(0, 64, 16), "B >= 1")
    assert sel(1, 2048, 1024) == 0 and sel(1, 10000, 16, T) == 0       # at the limits; n_points 0 < num_add: left untouched
    crit = lambda stride, num_add: lib.ifd_add_critical_points(ctx, P, None, T, 1, stride, num_add, 1.0, cri.data_ptr(), None, None)   # noqa: E731
    refused(crit(2049, 16), "stride outside [num_add, 2048]")
    refused(crit(64, 1025), "num_add")
    st = net.cw_state(2, 1024)
    S = C.byref(net._cw_struct(st, 2, 1024))
    step = lambda kind, cat_stride, num_add, n=None, t=1: lib.ifd_add_step(ctx, kind, S, P, T, None, T, P, n, None, None, None, t, 0.01, 1.0, 1,   # noqa: E731
                                                                        cat_stride, num_add, None)
    refused(step(2, 64, 16), "kind")
    refused(step(0, 4096, 1025), "num_add")
    refused(step(0, 31, 16), "cat_stride")
    refused(step(0, 10001, 16, T), "cat_stride")
    refused(step(0, 2049 + 16, 16), "2048 original rows")
    refused(step(0, 64, 16, None, 0), "t >= 1")
    o, best, ok = f(2, 3100, 3), f(2), i(2)

    def attack(stride=64, out_stride=80, num_add=16, kind=0, loss=0, steps=1, it=1, size=C.sizeof(_lib.IfdAddParams), n=None, B=2, out=None):
        prm = _lib.IfdAddParams(size, kind, loss, steps, it, num_add, 0.0, 0.5, 0.01, 5e3, 4e4)
        return lib.ifd_add_attack(ctx, C.byref(prm), P, None if n is None else n.data_ptr(), T, None, B, stride, out_stride,
                                  o.data_ptr() if out is None else out, best.data_ptr(), ok.data_ptr(), None, None)
    refused(attack(size=40), "struct_size")
    refused(attack(kind=2), "kind")
    refused(attack(loss=5), "loss_kind")
    refused(attack(steps=0), "binary_step")
    refused(attack(it=0), "num_iter")
    refused(attack(num_add=0), "num_add")
    refused(attack(stride=2048, out_stride=3100, num_add=1025), "num_add")
    refused(attack(stride=2049, out_stride=3100), "without n_points")
    refused(attack(stride=15), "without n_points")
    refused(attack(out_stride=79), "without n_points")
    refused(attack(out_stride=10001), "out_stride")
    refused(attack(stride=10001), "stride outside")
    refused(attack(B=0), "B >= 1")
    refused(attack(out=P), "overlaps")
    refused(attack(out=P + 12), "overlaps")
    for counts, word in (([64, 15], "n_points outside [16, 64]"), ([65, 64], "n_points outside [16, 64]")):
        refused(attack(n=dev(np.array(counts, np.int32))), word)
    refused(attack(stride=3000, out_stride=3100, n=dev(np.array([2049, 64], np.int32))), "n_points outside [16, 2048]")
    refused(attack(out_stride=70, n=dev(np.array([55, 54], np.int32))), "n_points outside [16, 54]")
    assert not o.any() and not ok.any() and not best.any()
    with pytest.raises(I.IfdError, match="target"):
        net.add_attack("chamfer", torch.zeros(2, 8, 3), [0, 40], 4, binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="noise"):
        net.add_attack("chamfer", torch.zeros(2, 8, 3), [0, 1], 4, torch.zeros(1, 2, 8, 3), binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="chamfer"):
        net.add_attack("l2", torch.zeros(2, 8, 3), [0, 1], 4)
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, True), "pointnet"), feature_transform=True, device="cuda:0") as ft:
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.add_attack("chamfer", torch.zeros(2, 8, 3), [0, 1], 4, binary_step=1, num_iter=1)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.add_select(torch.zeros(2, 8, 3), torch.zeros(2, 8, 3), 4)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.add_critical_points(torch.zeros(2, 8, 3), [0, 1], 4)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.add_step("chamfer", ft.cw_state(2, 4), f(2, 12, 3), [0, 0], [0, 0], f(2, 12, 3), 4, 1, 0.01)
    # the limits themselves work: num_add == n_ori, the whole attack
    x = np.random.default_rng(0).standard_normal((2, 8, 3)).astype(np.float32)
    out, _, _ = net.add_attack("hausdorff", x, [0, 1], 8, binary_step=1, num_iter=2)
    assert np.array_equal(bits(out[:, :8]), bits(x)) and np.isfinite(out.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------- 4. records and adjustment
@pytest.mark.parametrize("kind", DO.KINDS)
def test_record_logic_and_adjustment_are_exact(net, kind):
    """test_gpu_cw's record table on this state (stride = num_add), then ifd_cw_adjust as it is: the <=."""
    rng = np.random.default_rng(5)
    B, n, A = 5, 48, 12
    case = DO.make_step_case("small", kind, 1)
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
    dist = net.add_step(kind, st, grad, pred, target, X, A, 1, 1e-2, 0.2, want_info=True)["info"].cpu().numpy()[:, 2]
    assert np.all(dist > 1e-6) and np.all(dist < 1) and not np.array_equal(X.cpu().numpy()[:, n:], adv)
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
    dist2 = net.add_step(kind, st, grad, pred, target, dev(cat), A, 1, 1e-2, 0.2, want_info=True)["info"].cpu().numpy()[:, 2]
    assert np.array_equal(bits(dist2), bits(dist))
    assert torch.equal(st["bestdist"], before["bestdist"]) and torch.equal(st["o_bestdist"], before["o_bestdist"])
    assert np.array_equal(bits(st["o_bestattack"]), bits(marker)) and np.array_equal(st["o_bestscore"].cpu().numpy(), np.full(B, -9))
    # the adjustment on this state: bestdist == o_bestdist with the right class is a success (<=), above it or the wrong class a failure
    st["bestscore"].copy_(dev(np.array([3, 3, 4, 3, -1], np.int32)))
    st["bestdist"].copy_(dev(np.array([0.5, 0.75, 0.25, 0.25, 1e10], np.float32)))
    st["o_bestdist"].copy_(dev(np.array([0.5, 0.5, 0.5, 0.5, 1e10], np.float32)))
    st["m"].fill_(1.0)
    net.cw_adjust(st, target)
    assert np.array_equal(st["lower"].cpu().numpy(), [5e3, 0, 0, 5e3, 0]) and np.array_equal(st["upper"].cpu().numpy(), [4e4, 5e3, 5e3, 4e4, 5e3])
    assert np.array_equal(st["weight"].cpu().numpy(), [22500., 2500., 2500., 22500., 2500.]) and st["weight"].dtype == torch.float64
    assert not st["m"].any() and np.array_equal(st["bestscore"].cpu().numpy(), np.full(B, -1))


# ---------------------------------------------------------------------------------------------- 5. through the network
@pytest.mark.parametrize("kind", DO.KINDS)
def test_loop_teacher_forced_through_the_network(net, sd, W64, clouds, kind):
    """B = 17, 64 + 16 points, 3 iterations driven from the host from cri + 0.02 randn.  After each iteration the new added rows
    against the oracle's ONE step from the GPU's previous state and the GPU's own gradient (the bar of test 2), and the gradient of
    the concatenated cloud at that state by test_gpu_atk's row-wise rule under atk_oracle.case_conditions."""
    B, n, A, lr = 17, 64, 16, 1e-2
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    cri = net.add_critical_points(x, tg, A, 1.0 / B)
    start = cri + dev((np.random.default_rng(2).standard_normal((B, A, 3)) * 0.02).astype(np.float32))
    cat = torch.cat([dev(x), start], 1).contiguous()
    weight = 5e3 if kind == "chamfer" else 2e2
    st = net.cw_state(B, A, weight, 4e4)
    done = 0
    for k in (1, 2, 3):
        prev, m, v = cat.cpu().numpy(), st["m"].cpu().numpy(), st["v"].cpu().numpy()
        grad, aux = net.input_grad(cat, tg, scale=1.0 / B, want_aux=True)
        g, aux = grad.cpu().numpy(), {a: b.cpu().numpy() for a, b in aux.items()}
        net.add_step(kind, st, grad, aux["pred"], tg, cat, A, k, lr, 1.0 / B, loss=aux["loss"])
        new = cat.cpu().numpy()
        assert np.array_equal(bits(new[:, :n]), bits(x))
        e_gpu = e_32 = e_min = 0.0
        steps = []
        for i in range(B):
            a = (kind, g[i, n:], int(aux["pred"][i]), int(tg[i]), prev[i, n:], x[i], weight, m[i], v[i], k, lr, 1.0 / B, DO.fresh_record(A))
            steps.append((DO.step(*a), DO.step(*a, dtype=torch.float32)))
            e_min = max(e_min, float(np.abs(steps[-1][1][6]["min_p"].astype(np.float64) - steps[-1][0][6]["min_p"]).max()))
        n_out = 0
        for i, (s64, s32) in enumerate(steps):
            rows_out, cloud_out = DO.exclusions(prev[i, n:], x[i], e_min, kind)
            assert not cloud_out
            n_out += int(rows_out.sum())
            e_gpu = max(e_gpu, np.abs(new[i, n:] - s64[0])[~rows_out].max())
            e_32 = max(e_32, np.abs(s32[0] - s64[0])[~rows_out].max())
        assert n_out <= 0.05 * B * A
        print("%s iteration %d: adv |GPU - f64| %.3e = %.2f e_32, %d rows excluded" % (kind, k, e_gpu, e_gpu / e_32, n_out))
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
@pytest.mark.parametrize("kind", DO.KINDS)
def test_fused_and_host_driven_loops_give_the_same_bits(net, W64, clouds, capsys, kind):
    """16 clouds x (128 + 32) points, 2 search steps x 20 iterations, targets (prediction + 1) % 40, the reference script's weights.
    The count beside the float64 oracle's free-running count is a sanity figure, printed, not a parity bar (the trajectories part at
    the first discrete decision that float32 and float64 take differently)."""
    from ifdefense_amd import add_attack as AA, attack as A
    B, n, add = 16, 128, 32
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    w0, w1 = AA.WEIGHTS[kind]
    kw = dict(dist_func=kind, init_weight=w0, max_weight=w1, binary_step=2, num_iter=20, num_add=add, seed=3)
    a = A.CWAdd(net, **kw).attack(x, tg)
    out = capsys.readouterr().out
    b = A.CWAdd(net, verbose=False, **kw).attack(x, tg)
    quiet = capsys.readouterr().out
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[1].shape == (B, n + add, 3) and a[1].dtype == np.float32 and np.array_equal(bits(a[1][:, :n]), bits(x))
    for s in range(2):
        for it in (0, 4, 8, 12, 16):
            assert out.count("Step %d, iteration %d, success" % (s, it)) == 1
    assert out.count("adv_loss: ") == 10 and "time" not in out
    assert out.count("Successfully attack %d/%d" % (a[2], B)) == 1 and quiet == "Successfully attack %d/%d\n" % (a[2], B)
    # the library call itself: the same bits, success = lower > 0, the records
    noise = A.CWAdd(net, **kw).noise(torch.from_numpy(x))
    args = dict(scale=1.0 / B, init_weight=w0, max_weight=w1, binary_step=2, num_iter=20, want_bounds=True)
    o1 = net.add_attack(kind, x, tg, add, noise, **args)
    pc, best, ok, lower = o1[0].cpu().numpy(), o1[1].cpu().numpy(), o1[2].cpu().numpy(), o1[3]["lower"].cpu().numpy()
    assert np.array_equal(bits(pc), bits(b[1])) and np.array_equal(best.astype(np.float64), b[0])
    assert np.array_equal(ok, lower > 0) and ok.sum() == a[2]
    assert np.all(best[ok] < 1e10) and np.all(best[ok] >= 0)
    pred = net.predict(o1[0]).cpu().numpy()
    assert np.array_equal(pred[ok], tg[ok])                             # exact: the forward pass is batch-independent
    # clouds that never succeeded carry the last forwarded rows: after ONE iteration those are the start itself, cri + noise
    cri = net.add_critical_points(x, tg, add, 1.0 / B)
    s1 = net.add_attack(kind, x, tg, add, noise[:1], **dict(args, binary_step=1, num_iter=1))
    fail = ~s1[2].cpu().numpy()
    assert fail.sum() >= B // 2 and np.all(s1[1].cpu().numpy()[fail] == np.float32(1e10))
    assert np.array_equal(bits(s1[0][:, n:])[fail], bits(cri + noise[0].cuda())[fail])
    # a padded, ragged, permuted batch gives the same per-cloud bits
    p = np.array([4, 0, 5, 2, 1, 3])
    xr = np.full((6, n + 5, 3), np.nan, np.float32)
    counts = np.array([n, n - 7, n, add, n - 1, 64], np.int32)
    for j, i in enumerate(p):
        xr[j, :counts[j]] = x[i, :counts[j]]
    o2 = net.add_attack(kind, xr, tg[p], add, noise[:, p], n_points=counts, out_stride=n + add + 3, **dict(args, scale=1.0 / B))
    same = [j for j in range(6) if counts[j] == n]
    o3 = net.add_attack(kind, x[p][same], tg[p][same], add, noise[:, p][:, same], **args)
    pc2, pc3 = o2[0].cpu().numpy(), o3[0].cpu().numpy()
    for k, j in enumerate(same):
        assert np.array_equal(bits(pc2[j, :n + add]), bits(pc3[k])) and np.array_equal(bits(pc3[k]), bits(pc[p[j]]))
        assert o2[1][j] == o3[1][k] == o1[1][p[j]]
    for j in range(6):
        c = int(counts[j])
        assert np.array_equal(bits(pc2[j, :c]), bits(xr[j, :c])) and np.isfinite(pc2[j, c:c + add]).all() and not pc2[j, c + add:].any()
    ref = DO.attack(W64, x, tg, noise.numpy(), kind, add, torch.float64, binary_step=2, num_iter=20, init_weight=w0, max_weight=w1)
    print("CW Add %s: %d/%d clouds attacked, mean best_dist %.3e; the float64 oracle, free-running: %d/%d, %.3e"
          % (kind, ok.sum(), B, best[ok].mean() if ok.any() else np.nan, ref["success_num"], B,
             ref["o_bestdist"][ref["success"]].mean() if ref["success_num"] else np.nan))


# ---------------------------------------------------------------------------------------------- 7. the CLI
def test_cli_end_to_end(net, sd, tmp_path, capsys):
    from ifdefense_amd import inference as Inf, add_attack as AA
    import bench
    ck, src = str(tmp_path / "pointnet.npz"), str(tmp_path / "attack_data.npz")
    np.savez(ck, **sd)
    pcs = bench.synth_clouds(20, seed=5)[:, :128]
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pcs])).cpu().numpy()
    label, target = pred.astype(np.uint8), ((pred + 1) % 40).astype(np.uint8)
    np.savez(src, test_pc=pcs, test_label=label, target_label=target)
    assert AA.main(["--data_root", src, "--num_points", "128", "--num_add", "32", "--dist_func", "hausdorff", "--binary_step", "2",
                    "--num_iter", "20", "--batch_size", "16", "--model_path", ck, "--out_dir", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Successfully attack")]
    counts = [int(l.split()[-1].split("/")[0]) for l in lines]
    assert [l.split("/")[-1] for l in lines] == ["16", "4"]
    d = tmp_path / "attack" / "results" / "mn40_128" / "Add" / "hausdorff"
    (name,) = os.listdir(d)
    assert name == "Add-pointnet-logits_kappa=0.0-success_%.4f-rank_0.npz" % (sum(counts) / 20.0)
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (20, 160, 3) and np.isfinite(z["test_pc"]).all()
    assert np.array_equal(z["test_pc"][:, :128], np.stack([Inf.normalize_points_np(c) for c in pcs]))
    assert np.array_equal(z["test_label"], label) and np.array_equal(z["target_label"], target)
    assert Inf.main(["--data_root", str(d / name), "--mode", "target", "--model", "pointnet", "--model_path", ck, "--num_points", "160"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    rate = float(line.split("attack success rate:")[1])
    print("add_attack's rate %.4f, inference's rate on the written file %.4f" % (sum(counts) / 20.0, rate))
    assert rate >= sum(counts) / 20.0 - 1e-4                            # every recorded cloud reached its target when it was forwarded
