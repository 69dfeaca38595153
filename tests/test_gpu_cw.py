"""GPU checks of the CW point-perturbation attack (include/ifd_cw.h) against tests/cw_oracle.py.

The step is judged teacher-forced: one iteration from a given state against the float64 oracle's one iteration from the same state,
at 4 x the float32 oracle's own error per quantity (maximum over the batch).  Everything discrete - the records, the weight's binary
search, batching, fused against host-driven - is exact.  The gradient inside the loop keeps test_gpu_atk's row-wise rule."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import atk_oracle as AO
import cw_oracle as CO
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
        assert hasattr(c, "cw_step") and hasattr(c, "cw_adjust") and hasattr(c, "cw_perturb_attack")
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


def make_state(net, B, stride, **over):
    st = net.cw_state(B, stride)
    for k, v in over.items():
        st[k] = dev(np.asarray(v), st[k].dtype).reshape(st[k].shape).contiguous()
    return st


# ---------------------------------------------------------------------------------------------- 1. one step
@pytest.mark.parametrize("t", [1, 7])
def test_step_parity_teacher_forced(net, t):
    """B = 5, 300 points at stride 320 with NaN in the rows beyond; random gradient, m and positive v, so the network plays no
    part.  Cloud 4 has adv == ori exactly (dist == 0: finite, and the same bits as with weight 0 - the distance term is zero)."""
    rng = np.random.default_rng(11)
    B, n, stride, lr, scale = 5, 300, 320, 1e-2, 1.0 / 5
    weight = np.array([0., 10., 45., 10., 45.])
    adv, grad, m = (rng.standard_normal((B, stride, 3)).astype(np.float32) for _ in range(3))
    grad *= 0.05
    v = (rng.random((B, stride, 3)) * 0.01 + 1e-6).astype(np.float32)
    ori = (adv + 0.02 * rng.standard_normal(adv.shape)).astype(np.float32)
    ori[4] = adv[4]
    arrays = {"adv": adv, "ori": ori, "grad": grad, "m": m, "v": v}
    for a in arrays.values():
        a[:, n:] = np.nan
    pred, target = np.array([3, 3, 4, 5, 6], np.int32), np.array([3, 3, 3, 5, 6], np.int32)
    loss = rng.random(B).astype(np.float32)
    marker = np.full((B, stride, 3), 7.0, np.float32)

    def run(sel):
        st = make_state(net, len(sel), stride, m=m[sel], v=v[sel], weight=weight[sel], o_bestattack=marker[sel])
        A, LI = dev(adv[sel]), dev(marker[sel])
        info = net.cw_step(st, dev(grad[sel]), pred[sel], target[sel], A, dev(ori[sel]), t, lr, scale, loss=loss[sel], last_input=LI,
                           n_points=np.full(len(sel), n), want_info=True)
        return {k: x.cpu().numpy() for k, x in dict(st, adv=A, last=LI, info=info).items()}
    got = run(np.arange(B))
    # rows beyond the cloud: untouched in every array, bit for bit
    for k, before in (("adv", adv), ("m", m), ("v", v), ("o_bestattack", marker), ("last", marker)):
        assert np.array_equal(bits(got[k][:, n:]), bits(before[:, n:])), k
    assert np.array_equal(bits(got["last"][:, :n]), bits(adv[:, :n]))                     # input_val: the pre-update cloud
    assert np.array_equal(got["info"][:, 0], loss)
    err = {k: [0.0, 0.0] for k in ("adv", "m", "v", "dist")}                 # [GPU - f64, f32 - f64], maxima over the batch
    for b in range(B):
        a = (grad[b, :n], int(pred[b]), int(target[b]), adv[b, :n], ori[b, :n], weight[b], m[b, :n], v[b, :n], t, lr, scale, CO.fresh_record(n))
        p64, m64, v64, _, d64, _ = CO.step(*a)
        p32, m32, v32, _, d32, _ = CO.step(*a, dtype=torch.float32)
        for k, g, x32, x64 in (("adv", got["adv"][b, :n], p32, p64), ("m", got["m"][b, :n], m32, m64), ("v", got["v"][b, :n], v32, v64),
                               ("dist", got["info"][b, 2], d32, d64)):
            err[k][0] = max(err[k][0], float(np.abs(np.asarray(g, np.float64) - x64).max()))
            err[k][1] = max(err[k][1], float(np.abs(np.asarray(x32, np.float64) - x64).max()))
    print("t=%d: " % t + ", ".join("%s |GPU - f64| %.3e = %.2f e_32" % (k, a, a / e) for k, (a, e) in err.items()))
    for k, (a, e) in err.items():
        assert e > 0 and a <= 4 * e, (k, a, e)
    assert np.isfinite(got["adv"][4, :n]).all() and got["info"][4, 2] == 0 and got["info"][4, 1] == 0
    assert np.array_equal(got["info"][:, 1], got["info"][:, 2] * weight.astype(np.float32))   # dist * weight.float(): one float32 product
    # the record: clouds 0, 1, 3, 4 predicted their target
    hit = pred == target
    assert np.array_equal(got["bestscore"], np.where(hit, pred, -1)) and np.array_equal(got["o_bestscore"], np.where(hit, pred, -1))
    assert np.array_equal(got["bestdist"], np.where(hit, got["info"][:, 2], np.float32(1e10)))
    assert np.array_equal(bits(got["o_bestattack"][:, :n]), bits(np.where(hit[:, None, None], adv, marker)[:, :n]))
    # the same cloud alone gives the same bits; dist == 0 gives the bits of weight 0
    one = run(np.array([2]))
    for k in ("adv", "m", "v", "info", "bestdist"):
        assert np.array_equal(bits(one[k][0]), bits(got[k][2])), k
    weight[4] = 0.
    zero = run(np.array([4]))
    assert np.array_equal(bits(zero["adv"][0]), bits(got["adv"][4])) and np.array_equal(bits(zero["m"][0]), bits(got["m"][4]))


# ---------------------------------------------------------------------------------------------- 2. the record
def test_record_logic_is_exact(net):
    rng = np.random.default_rng(5)
    B, n = 5, 64
    ori = rng.standard_normal((B, n, 3)).astype(np.float32)
    adv = (ori + 0.05 * rng.standard_normal(ori.shape)).astype(np.float32)
    d = np.sqrt(((adv.astype(np.float64) - ori) ** 2).sum((1, 2)))                        # about 0.69
    marker = np.full((B, n, 3), 7.0, np.float32)
    #          hit, smaller     hit, larger      miss, smaller   (equal: below)   hit, smaller than bestdist only
    pred = np.array([3, 3, 4, 3, 3], np.int32)
    target = np.full(B, 3, np.int32)
    bestdist = np.array([10., 1e-3, 10., 1e10, 10.], np.float32)
    o_bestdist = np.array([10., 1e-3, 10., 1e10, 1e-3], np.float32)
    st = make_state(net, B, n, bestdist=bestdist, o_bestdist=o_bestdist, bestscore=np.full(B, -5), o_bestscore=np.full(B, -5),
                    o_bestattack=marker)
    grad = dev(0.01 * rng.standard_normal(ori.shape).astype(np.float32))
    A = dev(adv)
    info = net.cw_step(st, grad, pred, target, A, dev(ori), 1, 1e-2, 0.2, want_info=True).cpu().numpy()
    dist = info[:, 2]
    assert np.allclose(dist, d, rtol=1e-6) and not np.array_equal(A.cpu().numpy(), adv)
    g = {k: x.cpu().numpy() for k, x in st.items()}
    assert np.array_equal(g["bestdist"], np.array([dist[0], 1e-3, 10., dist[3], dist[4]], np.float32))
    assert np.array_equal(g["bestscore"], [3, -5, -5, 3, 3])
    assert np.array_equal(g["o_bestdist"], np.array([dist[0], 1e-3, 10., dist[3], 1e-3], np.float32))
    assert np.array_equal(g["o_bestscore"], [3, -5, -5, 3, -5])
    for b, written in enumerate([True, False, False, True, False]):
        assert np.array_equal(bits(g["o_bestattack"][b]), bits(adv[b] if written else marker[b])), b
    # the same clouds through again without the update: every dist equals its record bit for bit, and < is strict
    st["o_bestattack"].copy_(dev(marker))
    st["o_bestscore"].fill_(-9)
    st["bestscore"].fill_(-9)
    st["bestdist"][1] = float(dist[1])                                                       # equal on every cloud that hit
    st["o_bestdist"][1] = float(dist[1])
    st["o_bestdist"][4] = float(dist[4])
    before = {k: st[k].clone() for k in ("bestdist", "o_bestdist")}
    info2 = net.cw_step(st, grad, pred, target, dev(adv), dev(ori), 1, 1e-2, 0.2, want_info=True).cpu().numpy()
    assert np.array_equal(bits(info2[:, 2]), bits(dist))
    assert torch.equal(st["bestdist"], before["bestdist"]) and torch.equal(st["o_bestdist"], before["o_bestdist"])
    assert np.array_equal(bits(st["o_bestattack"]), bits(marker))
    assert np.array_equal(st["o_bestscore"].cpu().numpy(), np.full(B, -9)) and np.array_equal(st["bestscore"].cpu().numpy(), np.full(B, -9))


# ---------------------------------------------------------------------------------------------- 3. the adjustment
def test_adjust_is_exact(net):
    """12 clouds over every branch of Perturb.py:154-162, ten successive calls with a new record before each: success, the wrong
    class, no class at all (-1, also where the target is 0 and where the target itself is -1: the guard), bestdist == o_bestdist (success: <=), bestdist >
    o_bestdist with the right class (failure), bestdist < o_bestdist with the wrong class."""
    rng = np.random.default_rng(9)
    B, n, stride = 12, 20, 24
    target = np.array([3, 3, 3, 3, 0, 0, 7, 7, 39, 39, 1, -1], np.int32)      # -1: no class; only the guard keeps it a failure
    weight, lower, upper = np.full(B, 10.), np.zeros(B), np.full(B, 80.)
    m0 = rng.standard_normal((B, stride, 3)).astype(np.float32)
    st = make_state(net, B, stride)
    for call in range(10):
        kind = (np.arange(B) + call * 5 + rng.integers(0, 2, B)) % 6
        o_bestdist = rng.random(B).astype(np.float32) + 0.5
        bestscore = np.where(kind == 1, (target + 1) % 40, np.where(kind == 2, -1, target)).astype(np.int32)
        bestscore[kind == 5] = (target[kind == 5] + 39) % 40
        bestdist = np.where(kind == 3, o_bestdist, np.where(kind == 4, o_bestdist + np.float32(0.25), o_bestdist - np.float32(0.25)))
        bestdist = np.where(kind == 2, np.float32(1e10), bestdist).astype(np.float32)
        for k, a in (("bestscore", bestscore), ("bestdist", bestdist), ("o_bestdist", o_bestdist), ("m", m0), ("v", np.abs(m0))):
            st[k].copy_(dev(a))
        net.cw_adjust(st, target, n_points=np.full(B, n))
        for e in range(B):                                               # Perturb.py:154-162
            if bestscore[e] == target[e] and bestscore[e] != -1 and bestdist[e] <= o_bestdist[e]:
                lower[e] = max(lower[e], weight[e])
            else:
                upper[e] = min(upper[e], weight[e])
            weight[e] = (lower[e] + upper[e]) / 2.
        for k, a in (("weight", weight), ("lower", lower), ("upper", upper)):
            assert st[k].dtype == torch.float64 and np.array_equal(st[k].cpu().numpy(), a), (call, k)
        assert np.array_equal(st["bestdist"].cpu().numpy(), np.full(B, 1e10, np.float32)) and np.array_equal(st["bestscore"].cpu().numpy(), np.full(B, -1))
        assert np.array_equal(st["o_bestdist"].cpu().numpy(), o_bestdist)
        mm, vv = st["m"].cpu().numpy(), st["v"].cpu().numpy()
        assert not mm[:, :n].any() and not vv[:, :n].any()
        assert np.array_equal(mm[:, n:], m0[:, n:]) and np.array_equal(vv[:, n:], np.abs(m0)[:, n:])
    assert len(set(weight.tolist())) > 6 and (lower > 0).sum() >= 6 and (upper < 80).sum() >= 6


# ---------------------------------------------------------------------------------------------- 4. the loop, teacher-forced
def test_loop_teacher_forced_through_the_network(net, sd, W64, clouds):
    """B = 17, 64 points, 3 iterations driven from the host.  After each iteration the new adv against the oracle's ONE step from the
    GPU's previous state and the GPU's own gradient (the bar of test 1), and the gradient at that state by test_gpu_atk's row-wise
    rule under atk_oracle.case_conditions."""
    B, n, lr = 17, 64, 1e-2
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    ori = dev(x)
    adv = ori + dev((np.random.default_rng(2).standard_normal(x.shape) * 1e-7).astype(np.float32))
    st = make_state(net, B, n)
    done = 0
    for k in (1, 2, 3):
        prev, m, v = adv.cpu().numpy(), st["m"].cpu().numpy(), st["v"].cpu().numpy()
        grad, aux = net.input_grad(adv, tg, scale=1.0 / B, want_aux=True)
        g, aux = grad.cpu().numpy(), {a: b.cpu().numpy() for a, b in aux.items()}
        net.cw_step(st, grad, aux["pred"], tg, adv, ori, k, lr, 1.0 / B, loss=aux["loss"])
        new = adv.cpu().numpy()
        e_gpu = e_32 = 0.0
        for i in range(B):
            a = (g[i], int(aux["pred"][i]), int(tg[i]), prev[i], x[i], 10., m[i], v[i], k, lr, 1.0 / B, CO.fresh_record(n))
            p64, p32 = CO.step(*a)[0], CO.step(*a, dtype=torch.float32)[0]
            e_gpu, e_32 = max(e_gpu, np.abs(new[i] - p64).max()), max(e_32, np.abs(p32 - p64).max())
        print("iteration %d: adv |GPU - f64| %.3e = %.2f e_32" % (k, e_gpu, e_gpu / e_32))
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


# ---------------------------------------------------------------------------------------------- 5. fused = host-driven
def test_fused_and_host_driven_loops_give_the_same_bits(net, clouds, capsys):
    from ifdefense_amd import attack as A
    x, tg = clouds[:6, :128].copy(), np.array([1, 2, 3, 4, 5, 6])
    kw = dict(binary_step=3, num_iter=7, seed=3)
    a = A.CWPerturb(net, **kw).attack(x, tg)
    out = capsys.readouterr().out
    b = A.CWPerturb(net, verbose=False, **kw).attack(x, tg)
    quiet = capsys.readouterr().out
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])) and a[2] == b[2]
    assert a[0].shape == (6,) and a[1].shape == (6, 128, 3) and np.abs(a[1] - x).max() > 0
    # num_iter // 5 = 1: a line pair for every iteration of every search step, each once
    for s in range(3):
        for it in range(7):
            assert out.count("Step %d, iteration %d, success" % (s, it)) == 1
    lines = out.splitlines()
    assert out.count("adv_loss: ") == 21
    assert all(lines[lines.index("Step %d, iteration 0, success 0/6" % s) + 1] == "adv_loss: 0.0000, dist_loss: 0.0000" for s in range(3))
    assert out.count("Successfully attack %d/6" % a[2]) == 1 and quiet == "Successfully attack %d/6\n" % a[2]
    # a permuted batch gives the permuted outputs, bit for bit
    noise = A.CWPerturb(net, **kw).noise(torch.from_numpy(x))
    p = np.array([4, 0, 5, 2, 1, 3])
    args = dict(scale=1.0 / 6, binary_step=3, num_iter=7, want_bounds=True)
    o1 = net.cw_perturb_attack(x, tg, noise, **args)
    o2 = net.cw_perturb_attack(x[p], tg[p], noise[:, p], **args)
    assert np.array_equal(bits(o1[0]), bits(b[1])) and np.array_equal(o1[1].cpu().numpy().astype(np.float64), b[0])
    assert np.array_equal(bits(o2[0]), bits(o1[0])[p]) and np.array_equal(bits(o2[1]), bits(o1[1])[p])
    assert torch.equal(o2[2].cpu(), o1[2].cpu()[p]) and all(torch.equal(o2[3][k].cpu(), o1[3][k].cpu()[p]) for k in o1[3])


# ---------------------------------------------------------------------------------------------- 6. the attack as a whole
WHOLE_NUM_ITER = 10


def test_attack_as_a_whole(net, W64, clouds):
    """16 clouds x 128 points, targets (prediction + 1) % 40, binary_step 3, lr 0.01.  num_iter = 10 was chosen on the CPU from the
    float64 oracle alone (cw_oracle.attack, free-running, the same clouds and noise, targets from its own predictions): it reaches
    the target on 11 of the 16 clouds, 6 of them already in search step 0 (20 and 30 iterations: 14 of 16).  That count is printed beside the GPU's: a sanity
    figure, not a parity bar (the trajectories diverge at the first routing decision that float32 and float64 take differently, see
    test_gpu_atk.test_attack_as_a_whole)."""
    from ifdefense_amd import attack as A
    B, n = 16, 128
    x = clouds[:B, :n].copy()
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    noise = A.CWPerturb(net, binary_step=3, seed=1).noise(torch.from_numpy(x))
    kw = dict(scale=1.0 / B, attack_lr=1e-2, num_iter=WHOLE_NUM_ITER, want_bounds=True)
    out, best, ok, bounds = net.cw_perturb_attack(x, tg, noise, binary_step=3, **kw)
    out1, best1, ok1, _ = net.cw_perturb_attack(x, tg, noise[:1], binary_step=1, **kw)
    pred = net.predict(out).cpu().numpy()
    out, best, ok, best1, ok1 = out.cpu().numpy(), best.cpu().numpy(), ok.cpu().numpy(), best1.cpu().numpy(), ok1.cpu().numpy()
    lower = bounds["lower"].cpu().numpy()
    assert np.array_equal(pred[ok], tg[ok])                             # exact: the forward pass is batch-independent
    d = np.sqrt(((out.astype(np.float64) - x) ** 2).sum((1, 2)))
    assert np.all(best[ok] < 1e10) and np.all(np.abs(best[ok] - d[ok]) <= 1e-6 * d[ok])
    assert np.all(best[~ok] == np.float32(1e10))
    assert np.array_equal(ok, lower > 0)
    assert ok.sum() >= 1
    # the record only ever shrinks: the three-step run never ends above what search step 0 alone found (the one-step run's record,
    # itself at most the distance of the first state of that step that reached the target)
    assert np.all(best[ok1] <= best1[ok1]) and np.all(ok[ok1])
    ref = CO.attack(W64, x, tg, noise.numpy(), torch.float64, binary_step=3, num_iter=WHOLE_NUM_ITER)
    print("CW Perturb: %d/%d clouds attacked (%d within search step 0), mean best_dist %.4f; the float64 oracle, free-running: %d/%d, %.4f"
          % (ok.sum(), B, ok1.sum(), best[ok].mean(), ref["success_num"], B, ref["o_bestdist"][ref["success"]].mean()))
    assert ref["success_num"] >= B // 2


# ---------------------------------------------------------------------------------------------- 7. bad arguments
def test_bad_arguments(sd, net):
    import ifdefense_amd as I
    from ifdefense_amd import _lib, weights
    lib, ctx = net.lib, net.ctx
    d = torch.zeros(2, 8, 3, device="cuda")
    o, best = torch.zeros_like(d), torch.zeros(2, device="cuda")
    t, ok = torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    P, O, T, K, D = d.data_ptr(), o.data_ptr(), t.data_ptr(), ok.data_ptr(), best.data_ptr()

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.ifd_last_error(ctx), (rc, word, lib.ifd_last_error(ctx))

    def params(size=C.sizeof(_lib.IfdCwParams), loss=0, steps=2, it=3):
        return C.byref(_lib.IfdCwParams(size, loss, steps, it, 0.0, 1.0, 0.01, 10.0, 80.0))
    call = lambda p, B=2, stride=8, out=O: lib.ifd_cw_perturb_attack(ctx, p, P, None, T, None, B, stride, out, D, K, None, None)   # noqa: E731
    refused(call(params(size=32)), "struct_size")
    refused(call(None), "struct_size")
    refused(call(params(steps=0)), "binary_step")
    refused(call(params(it=0)), "num_iter")
    refused(call(params(loss=5)), "loss_kind")
    refused(call(params(), stride=10001), "stride")
    refused(call(params(), B=0), "B >= 1")
    refused(call(params(), out=P), "pc_out")
    refused(call(params(), out=P + 12), "pc_out")                      # overlapping, not only equal
    assert not o.any() and not ok.any() and not best.any()
    # the wrappers: state of the wrong type, targets outside the classes, a model with feature_transform
    st = net.cw_state(2, 8)
    with pytest.raises(I.IfdError, match="weight"):
        net.cw_step(dict(st, weight=st["weight"].float()), d, [0, 0], [0, 0], o, d, 1, 0.01)
    with pytest.raises(I.IfdError, match="target"):
        net.cw_perturb_attack(torch.zeros(2, 8, 3), [0, 40], binary_step=1, num_iter=1)
    with pytest.raises(I.IfdError, match="noise"):
        net.cw_perturb_attack(torch.zeros(2, 8, 3), [0, 1], torch.zeros(2, 2, 8, 3), binary_step=1, num_iter=1)
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, True), "pointnet"), feature_transform=True, device="cuda:0") as ft:
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.cw_perturb_attack(torch.zeros(2, 8, 3), [0, 1], binary_step=1, num_iter=1)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.cw_adjust(ft.cw_state(2, 8), [0, 1])
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.cw_step(ft.cw_state(2, 8), d, [0, 0], [0, 0], o, d, 1, 0.01)
    assert not o.any()


# ---------------------------------------------------------------------------------------------- 8. the CLI
def test_cli_end_to_end(net, sd, tmp_path, capsys):
    from ifdefense_amd import inference as Inf, perturb_attack as PA
    import bench
    ck, src = str(tmp_path / "pointnet.npz"), str(tmp_path / "attack_data.npz")
    np.savez(ck, **sd)
    pcs = bench.synth_clouds(70, seed=5)[:, :256]
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pcs])).cpu().numpy()
    label, target = pred.astype(np.uint8), ((pred + 1) % 40).astype(np.uint8)
    np.savez(src, test_pc=pcs, test_label=label, target_label=target)
    assert PA.main(["--data_root", src, "--num_points", "256", "--binary_step", "2", "--num_iter", "20", "--batch_size", "32",
                    "--model_path", ck, "--out_dir", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    counts = [int(l.split()[-1].split("/")[0]) for l in out.splitlines() if l.startswith("Successfully attack")]
    assert len(counts) == 3 and [l.split("/")[-1] for l in out.splitlines() if l.startswith("Successfully attack")] == ["32", "32", "6"]
    d = tmp_path / "attack" / "results" / "mn40_256" / "Perturb"
    (name,) = os.listdir(d)
    assert name == "Perturb-pointnet-logits_kappa=0.0-success_%.4f-rank_0.npz" % (sum(counts) / 70.0)
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (70, 256, 3) and np.isfinite(z["test_pc"]).all()
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8
    assert np.array_equal(z["test_label"], label) and np.array_equal(z["target_label"], target)
    assert Inf.main(["--data_root", str(d / name), "--mode", "target", "--model", "pointnet", "--model_path", ck, "--num_points", "256"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    rate = float(line.split("attack success rate:")[1])
    print("perturb_attack's rate %.4f, inference's rate on the written file %.4f" % (sum(counts) / 70.0, rate))
    assert 0.0 <= rate <= 1.0
