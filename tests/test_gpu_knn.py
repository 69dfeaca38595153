"""GPU checks of the kNN attack (include/ifd_knn.h) against tests/knn_oracle.py.

The step is judged teacher-forced: one iteration from a given state against the float64 oracle's one iteration from the same state.
Its discrete decisions - the Chamfer nearest, the five neighbours, the mask - are EXACT outside the rows the oracle's exclusion rule
leaves out (knn_oracle.rows_out: from the float64 oracle and the float32 oracle's measured errors alone); everything continuous is
held to 4 x the float32 oracle's own error, the maximum over the case.  Batching, permutation, fused against host-driven and a
stale workspace are bit for bit.  The gradient inside the loop keeps test_gpu_atk's row-wise rule."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import atk_oracle as AO
import knn_oracle as KO
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
        assert hasattr(c, "knn_step") and hasattr(c, "knn_project_clip") and hasattr(c, "knn_attack")
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


DIAG = ("info", "dist_grad", "nn_ori", "nn5", "mask")


def step_inputs(clouds, B, n, stride, seed=11):
    """Unit-sphere synthetic clouds, adv = ori + 0.02 randn, unit normals, a random gradient, m and positive v (so the network plays
    no part; the momentum of every seventh row is large enough to carry it over the budget), NaN in the rows beyond n.  n = 2048 is two synthetic clouds side by side."""
    rng = np.random.default_rng(seed)
    if n > clouds.shape[1]:
        x = np.concatenate([clouds[:B], clouds[B:2 * B] * 0.8 + 0.1], axis=1)[:, :n]
    else:
        x = clouds[:B, :n]
    arr = {"ori": np.full((B, stride, 3), np.nan, np.float32)}
    arr["ori"][:, :n] = KO.unit_sphere(x)
    for k in ("adv", "normal", "grad", "m", "v"):
        arr[k] = np.full((B, stride, 3), np.nan, np.float32)
    arr["adv"][:, :n] = arr["ori"][:, :n] + (0.02 * rng.standard_normal((B, n, 3))).astype(np.float32)
    arr["normal"][:, :n] = KO.synth_normals(arr["ori"][:, :n], seed)
    arr["grad"][:, :n] = 0.05 * rng.standard_normal((B, n, 3))
    arr["m"][:, :n] = 0.1 * rng.standard_normal((B, n, 3))
    arr["m"][:, :n:7] *= 30.                                             # every seventh row is carried far over the budget at any t
    arr["v"][:, :n] = rng.random((B, n, 3)) * 0.01 + 1e-6
    return arr


def run_step(net, arr, sel, n, t, lr, scale, normal=True, want=DIAG, **hyper):
    sel = np.asarray(sel)
    A, M, V = dev(arr["adv"][sel]), dev(arr["m"][sel]), dev(arr["v"][sel])
    loss = np.arange(len(sel), dtype=np.float32) + 0.5
    out = net.knn_step(dev(arr["grad"][sel]), A, dev(arr["ori"][sel]), M, V, t, lr, scale, normal=dev(arr["normal"][sel]) if normal else None,
                       loss=loss, n_points=None if n is None else np.full(len(sel), n) if np.isscalar(n) else np.asarray(n)[sel], want=want,
                       **hyper)
    return dict({k: x.cpu().numpy() for k, x in out.items()}, adv=A.cpu().numpy(), m=M.cpu().numpy(), v=V.cpu().numpy())


def oracle_step(arr, b, n, t, lr, scale, dtype, normal=True):
    return KO.step(arr["grad"][b, :n], arr["adv"][b, :n], arr["ori"][b, :n], arr["normal"][b, :n] if normal else None, arr["m"][b, :n],
                   arr["v"][b, :n], t, lr, scale, dtype)


def judge_step(got, arr, B, n, t, lr, scale, what, r64=None, r32=None):
    """The bars of test 1 on the first n rows of every cloud of `got` against the two oracles -> the share of rows left out."""
    r64 = r64 or [oracle_step(arr, b, n, t, lr, scale, torch.float64) for b in range(B)]
    r32 = r32 or [oracle_step(arr, b, n, t, lr, scale, torch.float32) for b in range(B)]
    assert all(r["self_ok"] for r in r64)
    E = KO.errors(r32, r64)
    outs, share = KO.case_rows(r64, [arr["adv"][b, :n] for b in range(B)], [arr["ori"][b, :n] for b in range(B)], E)
    err = {k: [0.0, 0.0] for k in ("dist_grad", "adv", "m", "v", "cd", "knn")}      # [GPU - f64, f32 - f64], maxima over the case
    masked = 0
    for b in range(B):
        out, clip = outs[b]
        keep = ~out
        assert np.array_equal(got["nn_ori"][b, :n][keep], r64[b]["nn_ori"][keep]), (what, b, "nn_ori")
        assert np.array_equal(got["mask"][b, :n][keep], r64[b]["mask"][keep].astype(np.int32)), (what, b, "mask")
        assert np.array_equal(np.sort(got["nn5"][b, :n][keep], 1), np.sort(r64[b]["nn5"][keep], 1)), (what, b, "nn5")
        masked += int(got["mask"][b, :n].sum())
        for k, o, rows in (("dist_grad", "g_dist", keep), ("adv", "adv", ~clip), ("m", "m", keep), ("v", "v", keep)):
            err[k][0] = max(err[k][0], float(np.abs(got[k][b, :n][rows].astype(np.float64) - r64[b][o][rows]).max()))
            err[k][1] = max(err[k][1], float(np.abs(r32[b][o][rows].astype(np.float64) - r64[b][o][rows]).max()))
        for k, col in (("cd", 1), ("knn", 2)):
            err[k][0] = max(err[k][0], abs(float(got["info"][b, col]) - r64[b][k]))
            err[k][1] = max(err[k][1], abs(r32[b][k] - r64[b][k]))
    print("%s: %.2f %% of the rows out, %d masked; " % (what, 100 * share, masked)
          + ", ".join("%s |GPU - f64| %.3e = %.2f e_32" % (k, a, a / e if e else np.inf) for k, (a, e) in err.items()))
    for k, (a, e) in err.items():
        assert e > 0 and a <= 4 * e, (what, k, a, e)
    assert masked > 0
    return share


# ---------------------------------------------------------------------------------------------- 1. decisions and gradient
@pytest.mark.parametrize("t", [1, 7])
@pytest.mark.parametrize("B,n,stride", [(5, 300, 320), (17, 64, 64), (2, 1024, 1024), (1, 2048, 2048)])
def test_step_decisions_and_gradient(net, clouds, B, n, stride, t):
    """No network: a random gradient and Adam state.  300 of 320: threads own 1 or 2 points, NaN beyond; 64: fewer points than
    threads; 1024: the workload's shape; 2048: the LDS limit."""
    lr, scale = 1e-2, 1.0 / B
    arr = step_inputs(clouds, B, n, stride)
    got = run_step(net, arr, np.arange(B), n if stride != n else None, t, lr, scale)
    judge_step(got, arr, B, n, t, lr, scale, "B=%d n=%d t=%d" % (B, n, t))
    assert np.array_equal(got["info"][:, 0], np.arange(B, dtype=np.float32) + 0.5)
    want3 = np.float32(n) * (np.float32(5) * got["info"][:, 1] + np.float32(3) * got["info"][:, 2])
    assert np.allclose(got["info"][:, 3], want3, rtol=1e-6, atol=0)
    # rows beyond the cloud: untouched in every array, bit for bit (the diagnostics were allocated as NaN / -1)
    for k in ("adv", "m", "v"):
        assert np.array_equal(bits(got[k][:, n:]), bits(arr[k][:, n:])), k
    assert np.isnan(got["dist_grad"][:, n:]).all() and (got["nn_ori"][:, n:] == -1).all() and (got["nn5"][:, n:] == -1).all()
    assert (got["mask"][:, n:] == -1).all()
    # nn5 is ascending in (distance, index), and never the point itself
    a = arr["adv"][:, :n].astype(np.float64)
    for b in range(B):
        d = ((a[b][:, None] - a[b][got["nn5"][b, :n]]) ** 2).sum(-1)
        assert (np.diff(d, axis=1) >= -1e-9).all() and (got["nn5"][b, :n] != np.arange(n)[:, None]).all()
    # some rows are clipped onto the budget, some are not, and nothing ends beyond it
    disp = np.sqrt(((got["adv"][:, :n].astype(np.float64) - arr["ori"][:, :n]) ** 2).sum(-1))
    assert disp.max() <= 0.1 * (1 + 1e-6) and (disp > 0.0999).sum() > 0 and (disp < 0.09).sum() > 0


# ---------------------------------------------------------------------------------------------- 2. edges
def test_step_edges(net, clouds):
    rng = np.random.default_rng(4)
    lr, scale = 1e-2, 0.5
    # n = 6, the minimum: every point's five neighbours are all the others
    arr = step_inputs(clouds, 2, 6, 8)
    got = run_step(net, arr, [0, 1], 6, 1, lr, scale)
    for b in range(2):
        assert np.array_equal(np.sort(got["nn5"][b, :6], 1), np.array([[j for j in range(6) if j != i] for i in range(6)]))
        r64 = oracle_step(arr, b, 6, 1, lr, scale, torch.float64)
        assert np.array_equal(got["nn_ori"][b, :6], r64["nn_ori"]) and np.array_equal(got["mask"][b, :6], r64["mask"].astype(np.int32))
        assert np.allclose(got["dist_grad"][b, :6], r64["g_dist"], rtol=0, atol=1e-5) and np.allclose(got["adv"][b, :6], r64["adv"], rtol=0, atol=1e-5)
    for k in ("adv", "m", "v"):
        assert np.array_equal(bits(got[k][:, 6:]), bits(arr[k][:, 6:])), k
    # 4 distinct points repeated to 64, adv == ori: every value 0, no mask, dist_grad exactly zero, the bits of zero weights
    arr = step_inputs(clouds, 1, 64, 64)
    arr["ori"][0] = np.tile(arr["ori"][0, :4], (16, 1))
    arr["adv"][0] = arr["ori"][0]
    got = run_step(net, arr, [0], None, 3, lr, scale)
    zero = run_step(net, arr, [0], None, 3, lr, scale, chamfer_weight=0., knn_weight=0.)
    assert not got["mask"].any() and not got["dist_grad"].any() and got["info"][0, 1] == 0 and got["info"][0, 2] == 0
    assert (got["nn_ori"][0] == np.arange(64) % 4).all()                 # the lowest index among the coincident originals
    assert (got["nn5"][0][:, 0] % 4 == np.arange(64) % 4).all()           # the nearest are the point's own copies
    for k in ("adv", "m", "v"):
        assert np.isfinite(got[k]).all() and np.array_equal(bits(got[k]), bits(zero[k])), k
    # two coincident adversarial points among distinct ones: finite
    arr = step_inputs(clouds, 1, 64, 64)
    arr["adv"][0, 9] = arr["adv"][0, 40]
    got = run_step(net, arr, [0], None, 1, lr, scale)
    assert all(np.isfinite(got[k]).all() for k in ("adv", "m", "v", "dist_grad", "info"))
    assert got["nn5"][0, 9, 0] == 40 and got["nn5"][0, 40, 0] == 9
    # a cloud of 5 points in a batch is left untouched, in every array; its neighbour of 6 points is not
    arr = step_inputs(clouds, 2, 6, 8)
    got = run_step(net, arr, [0, 1], np.array([5, 6]), 1, lr, scale)
    for k in ("adv", "m", "v"):
        assert np.array_equal(bits(got[k][0]), bits(arr[k][0])), k
    assert np.isnan(got["dist_grad"][0]).all() and (got["mask"][0] == -1).all() and np.isnan(got["info"][0]).all()
    assert not np.array_equal(bits(got["adv"][1, :6]), bits(arr["adv"][1, :6])) and (got["mask"][1, :6] >= 0).all()
    del rng


# ---------------------------------------------------------------------------------------------- 3. project / clip alone
def test_project_clip(net):
    """The crafted rows of the CPU test and 300 random ones (displacements from far inside the budget to far beyond it, on either side
    of the tangent plane), against the float64 oracle at 4 e_32 outside the rows with |d.n| < 8 e_dn."""
    rng = np.random.default_rng(8)
    c_adv, c_ori, c_nrm = KO.crafted_rows()
    ori = np.concatenate([c_ori, rng.uniform(-0.6, 0.6, (300, 3))]).astype(np.float32)
    nrm = rng.standard_normal((300, 3))
    nrm = np.concatenate([c_nrm, nrm / np.sqrt((nrm ** 2).sum(-1, keepdims=True))]).astype(np.float32)
    d = rng.standard_normal((300, 3)) * rng.choice([0.01, 0.05, 0.3], (300, 1))
    adv = np.concatenate([c_adv, ori[7:] + d]).astype(np.float32)
    n, stride = len(adv), 320

    def padded(a):
        out = np.full((2, stride, 3), np.nan, np.float32)
        out[:, :n] = a
        return out
    A = dev(padded(adv))
    net.knn_project_clip(A, dev(padded(ori)), dev(padded(nrm)), 0.1, n_points=[n, n])
    got = A.cpu().numpy()
    assert np.array_equal(bits(got[0]), bits(got[1])) and np.isnan(got[:, n:]).all()
    p64, dn64 = KO.project_clip_rows(adv, ori, nrm)
    p32, dn32 = KO.project_clip_rows(adv, ori, nrm, dtype=torch.float32)
    e_dn = np.abs(dn32.astype(np.float64) - dn64).max()
    keep = np.abs(dn64) >= 8 * e_dn
    e_gpu, e_32 = np.abs(got[0, :n][keep] - p64[keep]).max(), np.abs(p32[keep].astype(np.float64) - p64[keep]).max()
    print("project / clip: %d of %d rows out, |GPU - f64| %.3e = %.2f e_32; %d inward, %d clipped" % ((~keep).sum(), n, e_gpu, e_gpu / e_32,
          (dn64 < 0).sum(), (np.sqrt(((adv.astype(np.float64) - ori) ** 2).sum(-1)) > 0.1).sum()))
    assert e_32 > 0 and e_gpu <= 4 * e_32 and (~keep).sum() <= 0.05 * n
    row = {k: i for i, k in enumerate(KO.CRAFTED)}
    assert np.array_equal(bits(got[0, row["zero"]]), bits(ori[row["zero"]]))
    assert np.array_equal(bits(got[0, row["anti-parallel"]]), bits(ori[row["anti-parallel"]]))
    assert (np.sqrt(((got[0, :n].astype(np.float64) - ori) ** 2).sum(-1)) <= 0.1 * (1 + 1e-6)).all()
    # normal = None is the clip only
    A = dev(padded(adv))
    net.knn_project_clip(A, dev(padded(ori)), None, 0.1, n_points=[n, n])
    got = A.cpu().numpy()
    c64, c32 = KO.project_clip_rows(adv, ori, None)[0], KO.project_clip_rows(adv, ori, None, dtype=torch.float32)[0]
    e_gpu, e_32 = np.abs(got[0, :n] - c64).max(), np.abs(c32.astype(np.float64) - c64).max()
    print("clip alone: |GPU - f64| %.3e = %.2f e_32" % (e_gpu, e_gpu / e_32))
    assert e_32 > 0 and e_gpu <= 4 * e_32 and np.isnan(got[:, n:]).all()
    assert (np.sqrt(((got[0, :n].astype(np.float64) - ori) ** 2).sum(-1)) <= 0.1 * (1 + 1e-6)).all()
    assert not np.allclose(got[0, row["inward"]], p64[row["inward"]], atol=1e-4)


# ---------------------------------------------------------------------------------------------- 4. bitwise rules
def attack_inputs(clouds, B, n, seed=6):
    pts = KO.unit_sphere(clouds[:B, :n])
    return pts, KO.synth_normals(pts, seed)


def test_bitwise_rules(net, clouds, capsys):
    from ifdefense_amd import attack as A
    B, n, stride = 6, 300, 320
    arr = step_inputs(clouds, B, n, stride, seed=21)
    keys = ("adv", "m", "v") + DIAG
    full = run_step(net, arr, np.arange(B), n, 2, 1e-2, 0.25)
    one = run_step(net, arr, [3], n, 2, 1e-2, 0.25)
    p = np.array([4, 0, 5, 2, 1, 3])
    perm = run_step(net, arr, p, n, 2, 1e-2, 0.25)
    for k in keys:
        if k == "info":                                                  # column 0 is the loss the caller passed per position
            assert np.array_equal(bits(one[k][0, 1:]), bits(full[k][3, 1:])) and np.array_equal(bits(perm[k][:, 1:]), bits(full[k][p][:, 1:]))
        else:
            assert np.array_equal(bits(one[k][0]), bits(full[k][3])), k
            assert np.array_equal(bits(perm[k]), bits(full[k][p])), k
    bare = run_step(net, arr, np.arange(B), n, 2, 1e-2, 0.25, want=())     # the diagnostics change nothing
    assert all(np.array_equal(bits(bare[k]), bits(full[k])) for k in ("adv", "m", "v"))
    # the whole attack: permuted batch, a cloud alone (at the batch's scale), a second call behind a larger batch (stale workspace)
    pts, nrm = attack_inputs(clouds, 12, 128)
    tg = (net.predict(pts).cpu().numpy() + 1) % 40
    noise = A.CWKNN(net, seed=3).noise(torch.from_numpy(pts))
    kw = dict(kappa=0., scale=1.0 / 6, attack_lr=1e-2, num_iter=5)
    o1 = net.knn_attack(pts[:6], tg[:6], nrm[:6], noise[:6], **kw)
    o2 = net.knn_attack(pts[:6][p], tg[:6][p], nrm[:6][p], noise[:6][p], **kw)
    assert np.array_equal(bits(o2[0]), bits(o1[0])[p]) and torch.equal(o2[1], o1[1][p]) and torch.equal(o2[2], o1[2][p])
    net.knn_attack(pts, tg, nrm, noise, **kw)                             # grows the workspace and leaves it dirty
    o3 = net.knn_attack(pts[:6], tg[:6], nrm[:6], noise[:6], **kw)
    o4 = net.knn_attack(pts[2:3], tg[2:3], nrm[2:3], noise[2:3], **kw)
    assert np.array_equal(bits(o3[0]), bits(o1[0])) and torch.equal(o3[1], o1[1]) and torch.equal(o3[2], o1[2])
    assert np.array_equal(bits(o4[0][0]), bits(o1[0][2])) and np.abs(o1[0].cpu().numpy() - pts[:6]).max() > 1e-3
    # fused equals host-driven, through CWKNN verbose and quiet
    capsys.readouterr()
    data = np.concatenate([pts[:6], nrm[:6]], axis=2)
    a = A.CWKNN(net, attack_lr=1e-2, num_iter=7, kappa=0., seed=3).attack(data, tg[:6])
    out = capsys.readouterr().out
    b = A.CWKNN(net, attack_lr=1e-2, num_iter=7, kappa=0., seed=3, verbose=False).attack(data, tg[:6])
    quiet = capsys.readouterr().out
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1] and a[0].shape == (6, 128, 3)
    lines = out.splitlines()
    assert [l.split(",")[0] for l in lines if l.startswith("Iteration")] == ["Iteration %d/7" % it for it in range(7)]
    assert out.count("adv_loss: ") == 7
    assert lines[1] == "adv_loss: 0.0000, dist_loss: 0.0000" and lines[3] != lines[1]
    assert lines[-1] == "Successfully attack %d/6" % a[1] and quiet == "Successfully attack %d/6\n" % a[1]
    # [B,K,3] data runs the clip alone: another result than with normals, the same in both loop forms
    c = A.CWKNN(net, attack_lr=1e-2, num_iter=7, kappa=0., seed=3).attack(pts[:6], tg[:6])
    d = A.CWKNN(net, attack_lr=1e-2, num_iter=7, kappa=0., seed=3, verbose=False).attack(pts[:6], tg[:6])
    assert np.array_equal(bits(c[0]), bits(d[0])) and not np.array_equal(bits(c[0]), bits(a[0]))
    capsys.readouterr()


# ---------------------------------------------------------------------------------------------- 5. the loop, teacher-forced
def test_loop_teacher_forced_through_the_network(net, sd, W64, clouds):
    """B = 17, 64 points, 3 iterations driven from the host.  After each iteration the new adv (and everything else) against the
    oracle's ONE step from the GPU's previous state and the GPU's own gradient at the bars of test 1, and the gradient at that state by
    test_gpu_atk's row-wise rule under atk_oracle.case_conditions.  The loop starts from ori + 0.02 randn, test 1's perturbation, not from
    the attack's randn * 1e-7: there the float32 oracle's expanded-form distance gradient is noise of the size of the true one (5e-7
    against 1e-6), Adam's first steps are sign steps that blow that up to e_dn = 6e-3, and the oracle's rule leaves out 100 %, 99 % and
    84 % of the rows of the three iterations - the 5 % condition on the inputs is not met.  From 0.02 it leaves out 0.09 %, 0 % and 0 %."""
    B, n, lr = 17, 64, 1e-2
    x, nrm = attack_inputs(clouds, B, n)
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    ori, normal = dev(x), dev(nrm)
    adv = ori + dev((np.random.default_rng(2).standard_normal(x.shape) * 0.02).astype(np.float32))
    m, v = torch.zeros_like(ori), torch.zeros_like(ori)
    done = 0
    for k in (1, 2, 3):
        grad, aux = net.input_grad(adv, tg, kappa=0., scale=1.0 / B, want_aux=True)
        arr = {"adv": adv.cpu().numpy(), "ori": x, "normal": nrm, "grad": grad.cpu().numpy(), "m": m.cpu().numpy(), "v": v.cpu().numpy()}
        aux = {a: b.cpu().numpy() for a, b in aux.items()}
        got = net.knn_step(grad, adv, ori, m, v, k, lr, 1.0 / B, normal=normal, loss=aux["loss"], want=DIAG)
        got = dict({a: b.cpu().numpy() for a, b in got.items()}, adv=adv.cpu().numpy(), m=m.cpu().numpy(), v=v.cpu().numpy())
        judge_step(got, arr, B, n, k, lr, 1.0 / B, "iteration %d" % k)
        assert np.array_equal(got["info"][:, 0], aux["loss"])
        r32, r64, e, e32, ex = AO.run_case(sd, [c for c in arr["adv"]], tg, kappa=0., scale=1.0 / B)
        AO.case_conditions(r64, e)
        for i in range(B):
            why, rows_out = AO.row_exclusion(r64[i], e)
            if why:
                continue
            f = AO.run_cloud(W64, arr["adv"][i], tg[i], kappa=0., scale=1.0 / B, force_feat=aux["win_feat"][i], force_stn=aux["win_stn"][i])
            AO.check_grad(arr["grad"][i], f["grad"], e32, "iteration %d cloud %d" % (k, i), rows_out)
            done += 1
    assert done >= 0.9 * 3 * B


# ---------------------------------------------------------------------------------------------- 6. the attack as a whole
WHOLE = dict(num_iter=20, attack_lr=1e-2, kappa=15.)


def test_attack_as_a_whole(net, W64, clouds):
    """16 clouds x 128 points with normals (synthetic clouds 16 to 31), targets (prediction + 1) % 40.  num_iter = 20, lr = 0.01 and
    kappa = 15 were chosen on the CPU from the float64 oracle alone (knn_oracle.attack, free-running, the same clouds and noise,
    targets from its own predictions): it reaches the target on 10 of the 16 clouds.  (On clouds 0 to 15 it stays at 7 of 16 for
    every num_iter in 15 .. 40, lr in 0.005 .. 0.02 and kappa in 15 .. 100 that was tried: the 0.1 budget decides there, not the
    optimiser; hence the other clouds, not a lower bar.)  The oracle's count is printed beside the GPU's (measured: 9 of 16): a sanity figure, not a
    parity bar (the trajectories diverge at the first decision that float32 and float64 take differently)."""
    from ifdefense_amd import attack as A
    B, n = 16, 128
    x, nrm = attack_inputs(clouds[16:], B, n)
    tg = (net.predict(torch.from_numpy(x)).cpu().numpy() + 1) % 40
    noise = A.CWKNN(net, seed=1).noise(torch.from_numpy(x))
    out, pred, ok = net.knn_attack(x, tg, nrm, noise, scale=1.0 / B, **WHOLE)
    again = net.predict(out).cpu().numpy()
    out, pred, ok = out.cpu().numpy(), pred.cpu().numpy(), ok.cpu().numpy()
    assert np.array_equal(pred, again) and np.array_equal(ok, again == tg)      # exact: the forward pass is batch-independent
    disp = np.sqrt(((out.astype(np.float64) - x) ** 2).sum(-1))
    assert np.isfinite(out).all() and disp.max() <= 0.1 * (1 + 1e-6)
    assert ok.sum() >= 1
    ref = KO.attack(W64, x, nrm, tg, noise.numpy(), torch.float64, num_iter=WHOLE["num_iter"], lr=WHOLE["attack_lr"], kappa=WHOLE["kappa"])
    print("kNN: %d/%d clouds attacked, largest displacement %.4f, %d rows on the budget; the float64 oracle, free-running: %d/%d"
          % (ok.sum(), B, disp.max(), (disp > 0.0999).sum(), ref["success_num"], B))
    assert ref["success_num"] >= B // 2


# ---------------------------------------------------------------------------------------------- 7. bad arguments
def test_bad_arguments(sd, net):
    import ifdefense_amd as I
    from ifdefense_amd import _lib, weights
    lib, ctx = net.lib, net.ctx
    d = torch.zeros(2, 8, 3, device="cuda")
    o, m, v = torch.zeros_like(d), torch.zeros_like(d), torch.zeros_like(d)
    t, ok, pr = (torch.zeros(2, dtype=torch.int32, device="cuda") for _ in range(3))
    P, O, M, V, T, K, R = d.data_ptr(), o.data_ptr(), m.data_ptr(), v.data_ptr(), t.data_ptr(), ok.data_ptr(), pr.data_ptr()

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.ifd_last_error(ctx), (rc, word, lib.ifd_last_error(ctx))

    def params(size=C.sizeof(_lib.IfdKnnParams), loss=0, it=3):
        return C.byref(_lib.IfdKnnParams(size, loss, it, 0.0, 1.0, 0.001, 5.0, 3.0, 1.05, 0.1))
    call = lambda p, B=2, stride=8, out=O, pc=P, tg=T: lib.ifd_knn_attack(ctx, p, pc, None, None, tg, None, B, stride, out, R, K, None)   # noqa: E731
    refused(call(params(size=36)), "struct_size")
    refused(call(None), "struct_size")
    refused(call(params(it=0)), "num_iter")
    refused(call(params(loss=5)), "loss_kind")
    refused(call(params(), B=0), "B >= 1")
    refused(call(params(), pc=None), "missing pointer")
    refused(call(params(), tg=None), "missing pointer")
    refused(call(params(), out=P), "pc_out")
    refused(call(params(), out=P + 12), "pc_out")                      # overlapping, not only equal
    refused(call(params(), stride=5), "stride")
    refused(call(params(), stride=2049), "stride")
    step = lambda p, B=2, stride=8, adv=O, tt=1: lib.ifd_knn_step(ctx, p, P, None, adv, P, None, M, V, tt, 0.001, 1.0, None, None, B, stride, None)   # noqa: E731
    refused(step(params(size=36)), "struct_size")
    refused(step(None), "struct_size")
    refused(step(params(), B=0), "B >= 1")
    refused(step(params(), stride=5), "stride")
    refused(step(params(), stride=2049), "stride")
    refused(step(params(), adv=None), "missing pointer")
    refused(step(params(), tt=0), "t < 1")
    clip = lambda B=2, stride=8, adv=O: lib.ifd_knn_project_clip(ctx, adv, P, None, 0.1, None, B, stride, None)   # noqa: E731
    refused(clip(B=0), "B >= 1")
    refused(clip(stride=0), "stride")
    refused(clip(adv=None), "missing pointer")
    assert not o.any() and not ok.any() and not m.any() and not v.any()
    # the wrappers name the argument: tensors of the wrong kind, counts and targets at the one blocking check, feature_transform
    z = torch.zeros(2, 8, 3)
    with pytest.raises(I.IfdError, match="adv"):
        net.knn_step(d, o.double(), d, m, v, 1, 0.001)
    with pytest.raises(I.IfdError, match="normal"):
        net.knn_step(d, o, d, m, v, 1, 0.001, normal=z)
    with pytest.raises(I.IfdError, match="m is missing"):
        net.knn_step(d, o, d, None, v, 1, 0.001)
    with pytest.raises(I.IfdError, match="diagnostic"):
        net.knn_step(d, o, d, m, v, 1, 0.001, want=("values",))
    with pytest.raises(I.IfdError, match="ori"):
        net.knn_project_clip(o, z)
    with pytest.raises(I.IfdError, match="target"):
        net.knn_attack(z, [0, 40], num_iter=1)
    with pytest.raises(I.IfdError, match="n_points"):
        net.knn_attack(z, [0, 1], num_iter=1, n_points=[8, 5])
    with pytest.raises(I.IfdError, match="noise"):
        net.knn_attack(z, [0, 1], noise=torch.zeros(2, 7, 3), num_iter=1)
    with pytest.raises(I.IfdError, match="normal"):
        net.knn_attack(z, [0, 1], normal=torch.zeros(1, 8, 3), num_iter=1)
    with pytest.raises(I.IfdError, match="stride"):
        net.knn_attack(torch.zeros(2, 5, 3), [0, 1], num_iter=1)
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, True), "pointnet"), feature_transform=True, device="cuda:0") as ft:
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.knn_attack(z, [0, 1], num_iter=1)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.knn_step(d, o, d, m, v, 1, 0.001)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.knn_project_clip(o, d)
    assert not o.any() and not m.any()


# ---------------------------------------------------------------------------------------------- 8. the CLI
def test_cli_end_to_end(net, sd, tmp_path, capsys):
    from ifdefense_amd import inference as Inf, knn_attack as KA
    import bench
    ck, src = str(tmp_path / "pointnet.npz"), str(tmp_path / "attack_data.npz")
    np.savez(ck, **sd)
    pts = bench.synth_clouds(20, seed=5)[:, :128]
    pcs = np.concatenate([pts, KO.synth_normals(pts, 5)], axis=2)
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pts])).cpu().numpy()
    label, target = pred.astype(np.uint8), ((pred + 1) % 40).astype(np.uint8)
    np.savez(src, test_pc=pcs, test_label=label, target_label=target)
    assert KA.main(["--data_root", src, "--num_points", "128", "--num_iter", "20", "--attack_lr", "0.01", "--kappa", "0", "--batch_size", "8",
                    "--model_path", ck, "--out_dir", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    ends = [l for l in out.splitlines() if l.startswith("Successfully attack")]
    counts = [int(l.split()[-1].split("/")[0]) for l in ends]
    assert [l.split("/")[-1] for l in ends] == ["8", "8", "4"] and "no normals" not in out
    d = tmp_path / "attack" / "results" / "mn40_128" / "kNN"
    (name,) = os.listdir(d)
    assert name == "kNN-pointnet-logits_kappa=0.0-success_%.4f-rank_0.npz" % (sum(counts) / 20.0)
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (20, 128, 3) and np.isfinite(z["test_pc"]).all()
    assert np.array_equal(z["test_label"], label) and np.array_equal(z["target_label"], target)
    x = np.stack([Inf.normalize_points_np(c) for c in pts])
    assert np.sqrt(((z["test_pc"].astype(np.float64) - x) ** 2).sum(-1)).max() <= 0.1 * (1 + 1e-6)
    assert Inf.main(["--data_root", str(d / name), "--mode", "target", "--model", "pointnet", "--model_path", ck, "--num_points", "128"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    rate = float(line.split("attack success rate:")[1])
    print("knn_attack's rate %.4f, inference's rate on the written file %.4f" % (sum(counts) / 20.0, rate))
    assert 0.0 <= rate <= 1.0
