"""GPU tests of the DGCNN input gradient and its FGM family (include/ifd_dgcnn_atk.h) against tests/dgcnn_grad_oracle.py.

Parity: the float64 explicit-choice oracle, fed the GPU's own discrete choices (neighbour tables, winners, signs) once those have
been held against the float64 reference-form run (choices_valid), at the project's bar |GPU - f64| <= 4 e_32 max |grad|, e_32 the
float32 explicit-choice oracle's own distance from the float64 one on the same choices, floored at 1e-7.  A cloud whose head gates
(fc1, fc2, hinge, runner-up), which cannot be forced, are within 8 e_act of flipping is left out whole; at most 10 % of a case.
The cases and their inputs are tests/test_dgcnn_grad_cpu.py's, which shows on the CPU that the oracle alone keeps them within that."""
import os

import numpy as np
import pytest
import torch

import atk_oracle as AO
import dgcnn_grad_oracle as GO
import dgcnn_oracle as DO
from test_dgcnn_grad_cpu import CASES, MAX_OUT, case_inputs

pytestmark = pytest.mark.gpu

IFD_ERR_ARG = -1


def make_net(sd, k=20):
    import ifdefense_amd as I
    return I.DgcnnClassifier(I.weights.pack_state_dict(sd, "dgcnn"), k=k, device="cuda:0")


@pytest.fixture(scope="module")
def sd():
    return DO.make_calibrated_weights(0)


@pytest.fixture(scope="module")
def net(sd):
    with make_net(sd) as c:
        yield c


@pytest.fixture(scope="module")
def net4(sd):
    with make_net(sd, 4) as c:
        yield c


@pytest.fixture(scope="module")
def pool():
    import bench
    return bench.synth_clouds(40, seed=77)


def padded(clouds, stride=None, fill=np.nan):
    """-> (pc [B,stride,3] with `fill` beyond every cloud, n_points [B] int32 or None where no cloud is shorter than stride)."""
    counts = np.array([len(c) for c in clouds], np.int32)
    stride = int(stride or counts.max())
    pc = np.full((len(clouds), stride, 3), fill, np.float32)
    for i, c in enumerate(clouds):
        pc[i, :len(c)] = c
    return pc, (None if (counts == stride).all() else counts)


def gpu_grad(net, clouds, targets, loss="logits", kappa=0., scale=1., stride=None):
    pc, n = padded(clouds, stride)
    g, aux = net.input_grad(pc, np.asarray(targets), loss, kappa, scale, n_points=n, want_aux=True)
    torch.cuda.synchronize()
    return g.cpu().numpy(), aux


def bits(net, clouds, targets, stride=None, **kw):
    """The gradient rows of every cloud, as a list of arrays (the rows beyond a cloud must be zero)."""
    pc, n = padded(clouds, stride)
    g = net.input_grad(pc, np.asarray(targets), n_points=n, **kw).cpu().numpy()
    for i, c in enumerate(clouds):
        assert not g[i, len(c):].any()
    return [g[i, :len(c)].copy() for i, c in enumerate(clouds)]


def check_parity(sd, k, clouds, targets, g, aux, loss="logits", kappa=0., scale=1., what="", max_out=MAX_OUT):
    """The whole judgement of one call (module docstring) -> (clouds judged, worst |GPU - f64| / e_32 max |grad|)."""
    W32, W64 = DO.to_torch(sd, torch.float32), DO.to_torch(sd, torch.float64)
    F32, F64 = GO.folded(sd, torch.float32), GO.folded(sd, torch.float64)
    ch = [GO.gpu_choices(aux, b, len(c)) for b, c in enumerate(clouds)]
    r32 = [GO.run_cloud(W32, c, t, loss, kappa, scale, k, h["idx"], torch.float32) for c, t, h in zip(clouds, targets, ch)]
    r64 = [GO.run_cloud(W64, c, t, loss, kappa, scale, k, h["idx"], torch.float64) for c, t, h in zip(clouds, targets, ch)]
    e = GO.layer_errors(r32, r64)
    for b, (h, r) in enumerate(zip(ch, r64)):
        GO.choices_valid(h, r, e, "%s cloud %d" % (what, b))
    keep = [b for b, r in enumerate(r64) if not GO.head_exclusion(r, e, loss)]
    assert len(clouds) - len(keep) <= max_out * len(clouds), "%s: %d of %d clouds left out" % (what, len(clouds) - len(keep), len(clouds))
    kw = dict(loss=loss, kappa=kappa, scale=scale)
    x64 = {b: GO.explicit_from(F64, clouds[b], targets[b], ch[b], **kw)["grad"] for b in keep}
    x32 = {b: GO.explicit_from(F32, clouds[b], targets[b], ch[b], dtype=torch.float32, **kw)["grad"] for b in keep}
    e32 = GO.grad_e32([x32[b] for b in keep], [x64[b] for b in keep])
    worst = 0.0
    for b in keep:
        worst = max(worst, AO.check_grad(g[b], x64[b], e32, "%s cloud %d" % (what, b)))
        lo = aux["logits"][b].cpu().numpy()
        assert np.abs(lo - r64[b]["logits"]).max() <= 8 * max(e["logits"], 1e-6), (what, b)
    print("%s: judged %d of %d, e_32 %.3e, worst |GPU - f64| = %.2f e_32" % (what, len(keep), len(clouds), e32, worst))
    return len(keep), worst


# ---------------------------------------------------------------------------------------------- parity with float64
@pytest.fixture(scope="module")
def nets():
    made = {}
    yield lambda sd, k: made.setdefault(k, make_net(sd, k))
    for c in made.values():
        c.close()


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_against_f64(nets, name):
    sd, clouds, targets, k, loss, stride = case_inputs(name)
    net = nets(sd, k)
    scale = 1.0 / len(clouds)
    g, aux = gpu_grad(net, clouds, targets, loss, 0., scale, stride)
    assert np.abs(g[np.isfinite(g)]).max() > 0 and np.isfinite(g).all()
    check_parity(sd, k, clouds, targets, g, aux, loss, 0., scale, name)
    want = AO.adv_loss(aux["logits"].cpu().double(), torch.as_tensor(targets), loss, 0.)[0].numpy()
    assert np.abs(aux["loss"].cpu().numpy() - want).max() <= 1e-5 * max(1.0, np.abs(want).max())


# ---------------------------------------------------------------------------------------------- bits
def test_forward_half_is_the_forward_call_bit_for_bit(net, pool):
    clouds = [pool[0][:300], pool[1][:64], pool[2][:131], pool[3][:20], pool[4][:257]]
    pc, n = padded(clouds, 320)
    lo, fw = net.logits(pc, n, want_aux=True)
    _, aux = net.input_grad(pc, np.arange(5), n_points=n, want_aux=True)
    assert torch.equal(lo, aux["logits"])
    for k in ("pred", "global_feat", "feat"):
        assert torch.equal(fw[k], aux[k]), k
    for a, b in zip(fw["idx"], aux["idx"]):
        assert torch.equal(a, b)
    for b, c in enumerate(clouds):                                          # rows beyond a cloud are left as they were
        assert (aux["win_edge"][3][b, len(c):] == -1).all() and not aux["act5"][b, len(c):].any()
        assert int(aux["win_pool"][b].min()) >= 0 and int(aux["win_pool"][b].max()) < len(c)


def test_a_clouds_gradient_does_not_depend_on_its_batch(net, pool):
    sizes = [40, 64, 65, 130, 20, 200, 77]
    clouds = [pool[i][:m] for i, m in enumerate(sizes)]
    tg = np.array([3, 9, 1, 30, 22, 17, 5])
    base = bits(net, clouds, tg)
    assert all(np.abs(b).max() > 0 for b in base)
    perm = [4, 2, 6, 0, 5, 1, 3]
    for order in (list(np.roll(np.arange(7), 3)), perm):
        got = bits(net, [clouds[i] for i in order], tg[order])
        for j, i in enumerate(order):
            assert np.array_equal(got[j], base[i]), ("order", order, i)
    for i in (0, 3):                                                        # alone, alone at another stride, and among 33
        assert np.array_equal(bits(net, [clouds[i]], tg[i:i + 1])[0], base[i])
        assert np.array_equal(bits(net, [clouds[i]], tg[i:i + 1], stride=333)[0], base[i])
    many = [pool[(3 * j) % 40][:50 + j] for j in range(33)]
    many[17], many[32] = clouds[3], clouds[0]
    t33 = np.arange(33) % 40
    t33[17], t33[32] = tg[3], tg[0]
    got = bits(net, many, t33, stride=256)
    assert np.array_equal(got[17], base[3]) and np.array_equal(got[32], base[0])
    # zeros instead of NaN behind the clouds: the padding takes no part
    pc, n = padded(clouds, fill=0.0)
    g0 = net.input_grad(pc, tg, n_points=n).cpu().numpy()
    assert all(np.array_equal(g0[i, :m], base[i]) for i, m in enumerate(sizes))


def test_chunk_boundaries_and_stale_workspace(net4, pool):
    n = 24
    src = [pool[j % 40][(j // 40) * n:(j // 40) * n + n] for j in range(257)]
    tg = np.arange(257) % 40
    whole = bits(net4, src, tg)                                             # three chunks of 86, 86 and 85 clouds
    part = bits(net4, src[:129], tg[:129])                                  # two chunks of 65 and 64, on workspace the larger call left
    assert all(np.array_equal(a, b) for a, b in zip(part, whole))
    for i in (0, 64, 65, 85, 86, 128, 171, 172, 256):
        assert np.array_equal(bits(net4, [src[i]], tg[i:i + 1])[0], whole[i]), i
    assert sum(np.abs(w).max() > 0 for w in whole) > 200


def test_a_2048_point_cloud_runs_and_repeats(net, pool):
    c = np.concatenate([pool[20][:1024], 0.8 * pool[21][:1024] + 0.1]).astype(np.float32)
    a = bits(net, [c], [7])[0]
    b = bits(net, [c], [7])[0]
    assert a.shape == (2048, 3) and np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- ties
def test_ties_go_to_the_lowest_index(net, sd, pool):
    m = 40
    twice = np.concatenate([pool[5][:m], pool[5][:m]]).astype(np.float32)   # every point twice: i and i + 40, across the tile edge at 64
    g, aux = gpu_grad(net, [twice], [6])
    for l in range(4):
        w = aux["win_edge"][l][0].cpu().numpy()
        assert w.min() >= 0 and w.max() < m, "edge %d: a second copy won" % (l + 1)
    wp = aux["win_pool"][0].cpu().numpy()
    assert wp.min() >= 0 and wp.max() < m
    assert np.abs(g).max() > 0


def test_all_points_equal(net, sd, pool):
    c = np.repeat(pool[6][3:4], 20, axis=0).astype(np.float32)              # n = k = 20 copies of one point
    lo = DO.forward(DO.to_torch(sd, torch.float64), [c], dtype=torch.float64)["logits"].numpy()
    tg = (lo.argmax(1) + 1) % 40
    g, aux = gpu_grad(net, [c], tg)
    assert all(int(t.max()) == 0 for t in aux["win_edge"]) and int(aux["win_pool"].max()) == 0
    check_parity(sd, 20, [c], tg, g, aux, what="all equal", max_out=0)
    assert np.abs(g).max() > 0


def test_target_equal_to_the_prediction_gives_exactly_zero(net, pool):
    x = torch.from_numpy(np.stack([pool[i][:96] for i in range(4)]))
    pred = net.predict(x)
    g, aux = net.input_grad(x, pred, "logits", 0., 1., want_aux=True)
    assert not g.any() and not aux["loss"].any()
    adv, ok = net.fgm_attack("fgm", x, pred, 0.5, 0.5)
    assert torch.equal(adv.cpu(), x) and bool(ok.all())


# ---------------------------------------------------------------------------------------------- the FGM family
def test_fgm_update_is_the_pointnet_contexts(net, pool):
    import ifdefense_amd as I
    rng = np.random.default_rng(2)
    pc0 = torch.from_numpy(np.stack([pool[i][:100] for i in range(5)])).cuda()
    grad = torch.from_numpy(rng.standard_normal((5, 100, 3)).astype(np.float32)).cuda()
    n = np.array([100, 64, 99, 20, 100], np.int32)
    with I.Classifier(I.weights.pack_state_dict(I.weights.pointnet_random_state_dict(0), "pointnet"), device="cuda:0") as pn:
        for kind in ("fgm", "ifgm", "mifgm", "pgd"):
            out = []
            for c in (net, pn):
                pc, mom = (pc0 + 0.01).contiguous(), torch.full_like(pc0, 0.001)
                c.fgm_update(kind, grad, pc, pc0, mom, 0.05, 0.3, 0.9, n_points=n)
                out.append((pc.cpu(), mom.cpu()))
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), kind
            assert not torch.equal(out[0][0], (pc0 + 0.01).cpu())


@pytest.mark.parametrize("kind", ["ifgm", "mifgm"])
def test_loop_teacher_forced(net, sd, pool, kind):
    """At each of 5 iterations the GPU's gradient at ITS OWN current cloud passes the parity bar (free-running trajectories amplify
    the discontinuities), and the cloud it moves to is the oracle's update of that gradient."""
    B, n, budget, iters = 3, 65, 0.4, 5
    x = np.stack([pool[10 + i][:n] for i in range(B)]).astype(np.float32)
    tg = (net.predict(x).cpu().numpy() + 1) % 40
    step, scale, mu = budget / iters, 1.0 / B, 0.8
    ori = torch.from_numpy(x).cuda()
    cur = ori.clone()
    mom = torch.zeros_like(cur) if kind == "mifgm" else None
    judged = 0
    for it in range(iters):
        before, mom_before = cur.cpu().numpy(), None if mom is None else mom.cpu().numpy()
        g, aux = net.input_grad(cur, tg, "logits", 0., scale, want_aux=True)
        gh = g.cpu().numpy()
        judged += check_parity(sd, 20, list(before), tg, gh, aux, scale=scale, what="%s iteration %d" % (kind, it), max_out=1 / 3)[0]
        net.fgm_update(kind, g, cur, ori, mom, step, budget, mu)
        after = cur.cpu().numpy()
        for b in range(B):
            p64, _ = AO.update(kind, gh[b], before[b], x[b], None if mom is None else mom_before[b], step, budget, mu)
            p32, _ = AO.update(kind, gh[b], before[b], x[b], None if mom is None else mom_before[b], step, budget, mu, dtype=torch.float32)
            assert np.abs(after[b] - p64).max() <= 4 * max(np.abs(p32 - p64).max(), 1e-7), (kind, it, b)
    assert judged >= 0.8 * B * iters
    fused = net.fgm_attack(kind, x, tg, budget, step, iters, mu, scale=scale)[0]
    assert torch.equal(fused, cur)


def test_verbose_and_fused_loops_give_the_same_bits(net, pool, capsys):
    from ifdefense_amd import attack as A
    x, tg = np.stack([pool[i][:128] for i in range(4)]), np.array([1, 2, 3, 4])
    for cls in (A.IFGM, A.MIFGM, A.PGD):
        a = cls(net, "logits", None, 0.6, 0.1, 5, seed=3).attack(x, tg)
        b = cls(net, "logits", None, 0.6, 0.1, 5, seed=3, verbose=False).attack(x, tg)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1]
        assert not np.array_equal(a[0], x)
    f = A.FGM(net, "cross_entropy", 0.3).attack(x, tg)
    assert f[0].shape == x.shape and np.isfinite(f[0]).all()
    assert capsys.readouterr().out.count("iter 0/5") == 3


def test_cli_end_to_end(net, sd, tmp_path, capsys):
    from ifdefense_amd import dgcnn_fgm_attack as DA, dgcnn_inference as DI, inference as Inf
    import bench
    ck, src = str(tmp_path / "dgcnn.npz"), str(tmp_path / "attack_data.npz")
    np.savez(ck, **sd)
    pcs = bench.synth_clouds(16, seed=5)[:, :128]
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pcs])).cpu().numpy()
    np.savez(src, test_pc=pcs, test_label=pred.astype(np.uint8), target_label=((pred + 1) % 40).astype(np.uint8))
    assert DA.main(["--data_root", src, "--num_points", "128", "--attack_type", "ifgm", "--num_iter", "10", "--model_path", ck,
                    "--out_dir", str(tmp_path), "--batch_size", "8"]) == 0
    capsys.readouterr()
    d = tmp_path / "attack" / "results" / "mn40_128" / "FGM" / "dgcnn"
    (name,) = os.listdir(d)
    rate = name.split("-success_")[1].split("-rank")[0]
    assert DI.main(["--data_root", str(d / name), "--mode", "target", "--model", "dgcnn", "--model_path", ck, "--num_points", "128"]) == 0
    line = capsys.readouterr().out.strip()
    assert line.endswith("attack success rate: " + rate), (line, name)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_contexts_usable(net, pool):
    import ifdefense_amd as I
    x = np.stack([pool[i][:64] for i in range(2)])
    good = net.input_grad(x, [1, 2]).cpu()
    for bad, word in ((lambda: net.input_grad(x[:, :19], [1, 2]), "stride"),
                      (lambda: net.input_grad(x, [1, 2], n_points=[64, 19]), "n_points"),
                      (lambda: net.input_grad(np.zeros((1, 2049, 3), np.float32), [1]), "stride"),
                      (lambda: net.input_grad(x, [1, 40]), "target"),
                      (lambda: net.fgm_attack("ifgm", x, [1, 40], 0.1, 0.1, 2), "target"),
                      (lambda: net.fgm_attack("ifgm", x[:, :19], [1, 2], 0.1, 0.1, 2), "stride")):
        with pytest.raises(I.IfdError, match=word):
            bad()
    # the PointNet calls keep refusing a DGCNN context, and the DGCNN calls a PointNet context
    f32 = dict(device="cuda:0", dtype=torch.float32)
    pc, tg, g = torch.from_numpy(x).cuda(), torch.tensor([1, 2], dtype=torch.int32, device="cuda:0"), torch.empty(2, 64, 3, **f32)
    rc = net.lib.ifd_cls_input_grad(net.ctx, pc.data_ptr(), None, 2, 64, tg.data_ptr(), 0, 0.0, 1.0, g.data_ptr(), None, None)
    assert rc == IFD_ERR_ARG and b"not a classifier context" in net.lib.ifd_last_error(net.ctx)
    assert net.lib.ifd_fgm_update(net.ctx, 0, g.data_ptr(), pc.data_ptr(), None, None, 0.1, 0.1, 1.0, None, 2, 64, None) == IFD_ERR_ARG
    with I.Classifier(I.weights.pack_state_dict(I.weights.pointnet_random_state_dict(0), "pointnet"), device="cuda:0") as pn:
        rc = pn.lib.ifd_dgcnn_input_grad(pn.ctx, pc.data_ptr(), None, 2, 64, tg.data_ptr(), 0, 0.0, 1.0, g.data_ptr(), None, None)
        assert rc == IFD_ERR_ARG and b"not a DGCNN context" in pn.lib.ifd_last_error(pn.ctx)
        assert pn.lib.ifd_dgcnn_fgm_update(pn.ctx, 0, g.data_ptr(), pc.data_ptr(), None, None, 0.1, 0.1, 1.0, None, 2, 64, None) == IFD_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(net.input_grad(x, [1, 2]).cpu(), good)
