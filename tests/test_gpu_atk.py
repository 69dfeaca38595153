"""GPU checks of the attack primitives (include/ifd_atk.h) against tests/atk_oracle.py.

The gradient is discontinuous in its inputs (max-pool routing, ReLU gates), so the yardstick is the float64 oracle run with the
GPU's own winners forced, the winners are held against the float64 activations on their own (8 e_act), and the clouds whose
gates sit within rounding of zero in float64 are left out by the oracle alone.  Bar: |GPU - f64| <= 4 e_32, e_32 = the float32
oracle's own error on the case.  By whole clouds that rule leaves out 25 - 80 % of the clouds from 64 points on, so it is applied
row by row (atk_oracle.row_exclusion: only the rows a near-zero gate can reach are left out), and every case must meet
atk_oracle.case_conditions from the oracle alone: at most 10 % of its clouds wholly out, at least half of its gradient-receiving
rows judged.  Everything about batching is bitwise."""
import os
import warnings

import numpy as np
import pytest
import torch

import atk_oracle as AO
import pointnet_oracle as PO
from test_atk_cpu import CASES, case_inputs

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
        yield c


@pytest.fixture(scope="module")
def clouds():
    import bench
    return bench.synth_clouds(64, seed=91)


def gpu_grad(net, pcs, tg, **kw):
    g, aux = net.input_grad(pcs, torch.as_tensor(np.asarray(tg)), want_aux=True, **kw)
    return g.cpu().numpy(), {k: v.cpu().numpy() for k, v in aux.items()}


def compare_case(net, sd, W64, cl, tg, what, loss="logits", stride=None, first=None):
    """first: the GPU runs only the first `first` clouds of the case; e_32, e_act and the case's conditions stay the whole case's."""
    r32, r64, e, e32, ex = AO.run_case(sd, cl, tg, loss)
    whole, judged, live = AO.case_conditions(r64, e, loss)
    if first is not None:
        cl, tg, r64 = cl[:first], tg[:first], r64[:first]
    if stride is None:
        g, aux = gpu_grad(net, cl if len({len(c) for c in cl}) > 1 else np.stack(cl), tg, loss=loss)
    else:
        pad = np.full((len(cl), stride, 3), np.nan, np.float32)
        for i, c in enumerate(cl):
            pad[i, :len(c)] = c
        g, aux = gpu_grad(net, pad, tg, loss=loss, n_points=[len(c) for c in cl])
    ratios, wr = [], []
    for i, c in enumerate(cl):
        wr.append(AO.winners_valid(aux["win_feat"][i], r64[i]["pre"]["c3"], e["c3"], "%s cloud %d trunk" % (what, i)))
        wr.append(AO.winners_valid(aux["win_stn"][i], np.maximum(r64[i]["pre"]["stn3"], 0), e["stn3"], "%s cloud %d stn" % (what, i)))
        assert not g[i, len(c):].any()
        why, rows_out = AO.row_exclusion(r64[i], e, loss)
        if why:
            continue
        f = AO.run_cloud(W64, c, tg[i], loss, force_feat=aux["win_feat"][i], force_stn=aux["win_stn"][i])
        ratios.append(AO.check_grad(g[i], f["grad"], e32, "%s cloud %d" % (what, i), rows_out))
    print("%s: e_32 %.3e, e_act c3 %.1e stn3 %.1e, clouds wholly out %d/%d, rows judged %d/%d, GPU/e_32 max %.2f, winners short by <= %.2f e_act"
          % (what, e32, e["c3"], e["stn3"], whole, len(r64) if first is None else len(ex), judged, live, max(ratios), max(wr)))
    assert ratios


@pytest.mark.parametrize("n,B", CASES)
def test_gradient_parity(net, sd, W64, n, B):
    cl, tg = case_inputs(sd, n, B)
    compare_case(net, sd, W64, cl, tg, "N=%d B=%d" % (n, B))


def test_gradient_parity_cross_entropy(net, sd, W64):
    cl, tg = case_inputs(sd, 5, 33)
    compare_case(net, sd, W64, cl, tg, "CE N=5 B=33", loss="cross_entropy")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("loss", ["logits", "cross_entropy"])
def test_gradient_parity_small_batches(net, sd, W64, B, loss):
    """Batches of 1 and 3 clouds: the first clouds of the 33-cloud case, held to that case's e_32.  e_32 is a maximum over clouds,
    and the float32 oracle's own error spreads by a factor of 50 from cloud to cloud (cross-entropy, 5 points, 33 clouds: 0.26 to
    6.7 10^-6 of a cloud's largest entry, 1.6 10^-6 on the first three; the calibrated fc3 has weights of several hundred, so logits
    of order 10 carry an error of 2 - 4 10^-5 that the softmax passes on): a maximum over one or three clouds is not the reference's
    error, the maximum over the case they are taken from is."""
    cl, tg = case_inputs(sd, 5, 33)
    compare_case(net, sd, W64, cl, tg, "%s N=5 B=%d" % (loss, B), loss=loss, first=B)


def test_gradient_parity_ragged_at_stride_320(net, sd, W64, clouds):
    sizes = [1, 5, 64, 255, 256, 257, 320, 17, 2, 100, 300, 33]
    cl = [clouds[i][:n] for i, n in enumerate(sizes)]
    lo = np.concatenate([PO.forward(W64, c[None], dtype=torch.float64)[0].numpy() for c in cl])
    compare_case(net, sd, W64, cl, (lo.argmax(1) + 1) % 40, "ragged stride 320", stride=320)


def test_forward_outputs_are_the_classifiers_bits(net, clouds):
    x = torch.from_numpy(clouds[:33, :300])
    lo, a = net.logits(x, want_aux=True)
    _, b = gpu_grad(net, x, np.arange(33) % 40)
    assert np.array_equal(lo.cpu().numpy(), b["logits"]) and np.array_equal(a["pred"].cpu().numpy(), b["pred"])
    assert np.array_equal(a["global_feat"].cpu().numpy(), b["global_feat"])


def test_batching_is_bitwise(net, clouds):
    x = clouds[:33, :300].copy()
    tg = (np.arange(33) * 7) % 40
    g, aux = gpu_grad(net, x, tg)
    assert np.abs(g).max() > 0
    perm = np.random.default_rng(0).permutation(33)
    for p in (np.roll(np.arange(33), 5), perm):
        gp, ap = gpu_grad(net, x[p], tg[p])
        assert np.array_equal(gp, g[p]) and np.array_equal(ap["win_feat"], aux["win_feat"][p]) and np.array_equal(ap["loss"], aux["loss"][p])
    for B in (1, 15):
        assert np.array_equal(gpu_grad(net, x[:B], tg[:B])[0], g[:B])
    big = np.concatenate([x] * 8)[:257]
    gb = gpu_grad(net, big, np.concatenate([tg] * 8)[:257])[0]
    assert np.array_equal(gb, np.concatenate([g] * 8)[:257])
    # NaN padding and another stride
    pad = np.full((33, 512, 3), np.nan, np.float32)
    pad[:, :300] = x
    gp = gpu_grad(net, pad, tg, n_points=np.full(33, 300))[0]
    assert np.array_equal(gp[:, :300], g) and not gp[:, 300:].any()


def test_chunked_batch_equals_its_pieces(net, clouds):
    B = 4097
    x = np.tile(clouds[:64, :8], (65, 1, 1))[:B].copy()
    x[:, 0, 0] += np.arange(B, dtype=np.float32) * 1e-4
    tg = np.arange(B) % 40
    g = gpu_grad(net, x, tg)[0]
    for a, b in ((0, 40), (2030, 2070), (4060, 4097)):                 # around the chunk boundary (2049) and both ends
        assert np.array_equal(gpu_grad(net, x[a:b], tg[a:b])[0], g[a:b])


def test_stale_workspace_is_not_read(net, sd, clouds):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    x, tg = clouds[:4, :40], np.array([1, 2, 3, 4])
    gpu_grad(net, clouds[:40, :600] * 50, np.arange(40))
    got = gpu_grad(net, x, tg)[0]
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as fresh:
        assert np.array_equal(gpu_grad(fresh, x, tg)[0], got)


def test_degenerate_clouds(net, sd, W64, clouds):
    same = np.tile(np.array([[0.3, -0.2, 0.5]], np.float32), (1, 70, 1))
    g, aux = gpu_grad(net, same, [1])
    assert not aux["win_feat"].any() and not aux["win_stn"].any() and np.abs(g[0, 0]).max() > 0 and not g[0, 1:].any()
    f = AO.run_cloud(W64, same[0], 1)
    r32 = AO.run_cloud(PO.to_torch(sd, torch.float32), same[0], 1, dtype=torch.float32)
    e32 = max(np.abs(r32["grad"] - f["grad"]).max() / np.abs(f["grad"]).max(), 1e-7)
    AO.check_grad(g[0], f["grad"], e32, "all points equal")
    dup = np.repeat(clouds[:3, :20], 2, axis=1)                        # every point twice: the first copy takes the gradient
    g, aux = gpu_grad(net, dup, [5, 6, 7])
    assert not (aux["win_feat"] % 2).any() and not (aux["win_stn"] % 2).any() and not g[:, 1::2].any()
    # target == prediction, kappa 0: the hinge is closed, the gradient is exactly zero and plain FGM moves nothing
    x = torch.from_numpy(clouds[:9, :100]).cuda()
    pred = net.predict(x)
    g = net.input_grad(x, pred)
    assert not g.cpu().numpy().any()
    before = x.clone()
    out, ok = net.fgm_attack("fgm", x, pred, 1.0, 1.0)
    assert torch.equal(out, before) and bool(ok.all())


def test_bad_arguments(sd, net):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    x = torch.zeros(2, 8, 3)
    with pytest.raises(I.IfdError, match="target"):
        net.input_grad(x, [0, 40])
    with pytest.raises(I.IfdError, match="n_points"):
        net.input_grad(x, [0, 1], n_points=[8, 9])
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, True), "pointnet"), feature_transform=True, device="cuda:0") as ft:
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.input_grad(x, [0, 1])
    # the host-side refusals of the C ABI, each before anything is enqueued
    import ctypes as C
    from ifdefense_amd import _lib
    lib, ctx = net.lib, net.ctx
    d = torch.zeros(2, 8, 3, device="cuda")
    o, t, ok = torch.zeros_like(d), torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    P, T, K = d.data_ptr(), t.data_ptr(), ok.data_ptr()

    def refused(rc, word):
        assert rc == -1 and word.encode() in lib.ifd_last_error(ctx), (rc, lib.ifd_last_error(ctx))
    refused(lib.ifd_cls_input_grad(ctx, P, None, 2, 8, T, 2, 0.0, 1.0, o.data_ptr(), None, None), "loss_kind")
    refused(lib.ifd_cls_input_grad(ctx, P, None, 2, 10001, T, 0, 0.0, 1.0, o.data_ptr(), None, None), "stride")
    refused(lib.ifd_cls_input_grad(ctx, P, None, 0, 8, T, 0, 0.0, 1.0, o.data_ptr(), None, None), "B >= 1")
    refused(lib.ifd_fgm_update(ctx, 4, P, o.data_ptr(), P, None, 0.1, 1.0, 1.0, None, 2, 8, None), "kind")
    refused(lib.ifd_fgm_update(ctx, _lib.FGM_IFGM, P, o.data_ptr(), None, None, 0.1, 1.0, 1.0, None, 2, 8, None), "ori_pc")
    refused(lib.ifd_fgm_update(ctx, _lib.FGM_MIFGM, P, o.data_ptr(), P, None, 0.1, 1.0, 1.0, None, 2, 8, None), "momentum")

    def params(size=C.sizeof(_lib.IfdFgmParams), kind=_lib.FGM_IFGM, loss=0, it=3):
        return C.byref(_lib.IfdFgmParams(size, kind, loss, it, 0.0, 1.0, 0.1, 1.0, 1.0))
    refused(lib.ifd_fgm_attack(ctx, params(size=32), P, None, T, 2, 8, o.data_ptr(), K, None), "struct_size")
    refused(lib.ifd_fgm_attack(ctx, params(it=0), P, None, T, 2, 8, o.data_ptr(), K, None), "num_iter")
    refused(lib.ifd_fgm_attack(ctx, params(kind=9), P, None, T, 2, 8, o.data_ptr(), K, None), "kind")
    refused(lib.ifd_fgm_attack(ctx, params(loss=5), P, None, T, 2, 8, o.data_ptr(), K, None), "loss_kind")
    refused(lib.ifd_fgm_attack(ctx, params(), P, None, T, 2, 8, P, K, None), "pc_out")
    refused(lib.ifd_fgm_attack(ctx, params(), P, None, T, 2, 10001, o.data_ptr(), K, None), "stride")
    assert not o.any() and not ok.any()


@pytest.mark.parametrize("budget", [0.9, 0.25], ids=["inside", "clipped"])
@pytest.mark.parametrize("kind", ["fgm", "ifgm", "mifgm", "pgd"])
def test_fgm_update(net, kind, budget):
    """||pc - ori|| is about 0.6 before and 0.67 after the step: inside the budget of 0.9 (scale factor 1), far outside 0.25 (scale
    factor about 0.37: the clip's own branch, where the result must sit ON the sphere)."""
    rng = np.random.default_rng(4)
    B, n, stride, step, mu = 5, 300, 320, 0.3, 0.8
    grad, pc, mom = (rng.standard_normal((B, stride, 3)).astype(np.float32) for _ in range(3))
    ori = (pc + 0.02 * rng.standard_normal(pc.shape)).astype(np.float32)
    d = lambda a: torch.from_numpy(a.copy()).cuda()                    # noqa: E731
    P, M = d(pc), d(mom)
    net.fgm_update(kind, d(grad), P, d(ori), M, step, budget, mu, n_points=np.full(B, n))
    P, M = P.cpu().numpy(), M.cpu().numpy()
    assert np.array_equal(P[:, n:], pc[:, n:]) and np.array_equal(M[:, n:], mom[:, n:])
    worst = 0.0
    for b in range(B):
        a = [x[b, :n] for x in (grad, pc, ori, mom)]
        p64, m64 = AO.update(kind, *a, step, budget, mu)
        p32, m32 = AO.update(kind, *a, step, budget, mu, dtype=torch.float32)
        e32 = np.abs(p32 - p64).max()
        worst = max(worst, np.abs(P[b, :n] - p64).max() / e32)
        if kind == "mifgm":
            assert np.abs(M[b, :n] - m64).max() <= 4 * np.abs(m32 - m64).max()
        if kind != "fgm":
            dist = np.sqrt(((P[b, :n].astype(np.float64) - ori[b, :n]) ** 2).sum())
            assert dist <= budget * (1 + 1e-6)
            u = AO.update("mifgm" if kind == "mifgm" else "ifgm", *a, step, 1e9, mu)[0]      # the same step without a clip
            unclipped = np.sqrt(((u - ori[b, :n]) ** 2).sum())
            assert (unclipped > 2 * budget and dist >= budget * (1 - 1e-6)) if budget < 0.5 else unclipped < budget
    print("%s update: |GPU - f64| = %.2f e_32" % (kind, worst))
    assert worst <= 4
    P1, M1 = d(pc[2:3]), d(mom[2:3])                                   # bitwise independent of the batch
    net.fgm_update(kind, d(grad[2:3]), P1, d(ori[2:3]), M1, step, budget, mu, n_points=[n])
    assert np.array_equal(P1.cpu().numpy()[0], P[2]) and np.array_equal(M1.cpu().numpy()[0], M[2])


def test_loop_teacher_forced(net, sd, W64, clouds):
    """The state after k iterations against ONE step from the GPU's own state after k - 1 (free-running trajectories amplify the
    discontinuities): the gradient at that state at the bar of the parity tests, and the new state against the oracle's update of
    that gradient at the bar of test_fgm_update.  I-FGM: its state is the cloud alone."""
    B, n, budget = 33, 64, 0.5
    x = torch.from_numpy(clouds[:B, :n].copy())
    tg = (net.predict(x).cpu().numpy() + 1) % 40
    step = budget / 3
    state = [x.numpy()] + [net.fgm_attack("ifgm", x, tg, budget, step, k, scale=1.0 / B)[0].cpu().numpy() for k in (1, 2, 3)]
    done = 0
    for k in (1, 2, 3):
        prev = [c for c in state[k - 1]]
        r32, r64, e, e32, ex = AO.run_case(sd, prev, tg, scale=1.0 / B)
        g, aux = gpu_grad(net, state[k - 1], tg, scale=1.0 / B)
        for i in range(B):
            p64, _ = AO.update("ifgm", g[i], prev[i], state[0][i], None, step, budget, 1.0)
            p32, _ = AO.update("ifgm", g[i], prev[i], state[0][i], None, step, budget, 1.0, dtype=torch.float32)
            assert np.abs(state[k][i] - p64).max() <= 4 * np.abs(p32 - p64).max(), (k, i)
            why, rows_out = AO.row_exclusion(r64[i], e)
            if why:
                continue
            f = AO.run_cloud(W64, prev[i], tg[i], scale=1.0 / B, force_feat=aux["win_feat"][i], force_stn=aux["win_stn"][i])
            AO.check_grad(g[i], f["grad"], e32, "iteration %d cloud %d" % (k, i), rows_out)
            done += 1
        AO.case_conditions(r64, e)
    assert done >= 0.9 * 3 * B


def oracle_attack(W64, kind, x, tg, budget, step, iters, mu, scale):
    """The float64 oracle free-running: FGM.py's loop one cloud at a time -> success count."""
    ok = 0
    for c, t in zip(x, tg):
        ori = c.astype(np.float64)
        cur, mom = ori.copy(), np.zeros_like(ori)
        for _ in range(iters):
            cur, mom = AO.update(kind, AO.run_cloud(W64, cur, t, scale=scale)["grad"], cur, ori, mom, step, budget, mu)
        ok += int(AO.run_cloud(W64, cur, t)["logits"].argmax() == t)
    return ok


@pytest.mark.parametrize("kind", ["ifgm", "mifgm"])
def test_attack_as_a_whole(net, W64, clouds, kind):
    """The float64 oracle's free-running count is printed beside the GPU's: a sanity check, not a parity bar (the trajectories
    diverge at the first routing decision that float32 and float64 take differently)."""
    B, n, budget, iters = 64, 256, 0.08 * np.sqrt(256 * 3), 10
    x = torch.from_numpy(clouds[:B, :n].copy())
    x = x + torch.randn(x.shape, generator=torch.Generator().manual_seed(1)) * 1e-7
    tg = torch.from_numpy((net.predict(x).cpu().numpy() + 1) % 40)
    before = int((net.predict(x).cpu() == tg).sum())
    out, ok = net.fgm_attack(kind, x, tg, budget, budget / iters, iters, 1.0, scale=1.0 / B)
    assert torch.equal(ok.cpu(), net.predict(out).cpu() == tg)
    d = (out.cpu().double() - x.double()).pow(2).sum(dim=[1, 2]).sqrt()
    assert float(d.max()) <= budget * (1 + 1e-6) and float(d.min()) > 0
    ref = oracle_attack(W64, kind, x.numpy(), tg.numpy(), budget, budget / iters, iters, 1.0, 1.0 / B)
    print("%s: %d/%d clouds reach their target after %d iterations (%d before); the float64 oracle, free-running: %d/%d"
          % (kind, int(ok.sum()), B, iters, before, ref, B))
    assert int(ok.sum()) > before and ref > before


def test_verbose_and_fused_loops_give_the_same_bits(net, clouds, capsys):
    from ifdefense_amd import attack as A
    x, tg = clouds[:6, :128], np.array([1, 2, 3, 4, 5, 6])
    for cls in (A.IFGM, A.MIFGM, A.PGD):
        a = cls(net, "logits", None, 0.6, 0.1, 5, seed=3).attack(x, tg)
        b = cls(net, "logits", None, 0.6, 0.1, 5, seed=3, verbose=False).attack(x, tg)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert capsys.readouterr().out.count("iter 0/5") == 3


def test_cli_end_to_end(net, sd, clouds, tmp_path, capsys):
    from ifdefense_amd import fgm_attack as FA, inference as Inf
    ck, src = str(tmp_path / "pointnet.npz"), str(tmp_path / "attack_data.npz")
    np.savez(ck, **sd)
    import bench
    pcs = bench.synth_clouds(70, seed=5)[:, :256]
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pcs])).cpu().numpy()
    np.savez(src, test_pc=pcs, test_label=pred.astype(np.uint8), target_label=((pred + 1) % 40).astype(np.uint8))
    assert FA.main(["--data_root", src, "--num_points", "256", "--attack_type", "mifgm", "--num_iter", "10", "--model_path", ck,
                    "--out_dir", str(tmp_path), "--batch_size", "32"]) == 0
    capsys.readouterr()
    d = tmp_path / "attack" / "results" / "mn40_256" / "FGM" / "pointnet"
    (name,) = os.listdir(d)
    rate = name.split("-success_")[1].split("-rank")[0]
    assert Inf.main(["--data_root", str(d / name), "--mode", "target", "--model", "pointnet", "--model_path", ck, "--num_points", "256"]) == 0
    line = capsys.readouterr().out.strip()
    assert line.endswith("attack success rate: " + rate) and float(rate) > 0, (line, name)
