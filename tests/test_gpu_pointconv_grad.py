"""GPU tests of the PointConv input gradient and its FGM family (include/ifd_pc_atk.h) against tests/pointconv_grad_oracle.py.

Parity: the float64 explicit-choice oracle, fed the GPU's own discrete choices (index tables and every gate of the three levels)
once those have been held against the float64 reference-form run (choices_valid) and the tables against the header's selection
rules, at the project's bar |GPU - f64| <= 4 e_32 max |grad|, e_32 the float32 explicit-choice oracle's own distance from the
float64 one on the same choices, floored at 1e-7.  A cloud whose head gates (fc1, fc2, hinge, runner-up), which cannot be forced,
are within 8 e_act of flipping is left out whole; at most 10 % of a case.  The cases and their inputs are
tests/test_pointconv_grad_cpu.py's, which shows on the CPU that the oracle alone keeps them within that, and that each of the five
paths of the coordinates moves the gradient of cases "100" and "1024" by more than 100 e_32.  PointConv always runs 512 x 32 +
128 x 64 + 128 rows a cloud, so small clouds cost what large ones cost."""
import os

import numpy as np
import pytest
import torch

import atk_oracle as AO
import pointconv_grad_oracle as GO
import pointconv_oracle as PCO
from test_pointconv_grad_cpu import CASES, DEGENERATE, MAX_OUT, case_inputs, degenerate_inputs, source_clouds

pytestmark = pytest.mark.gpu

IFD_ERR_ARG = -1
FWD = ("fps1", "fps2", "knn1", "knn2", "dens1", "dens2", "dens3", "l1_feat", "l2_feat", "global_feat")


def make_net(sd):
    import ifdefense_amd as I
    return I.PointConvClassifier(I.weights.pack_state_dict(sd, "pointconv"), device="cuda:0")


@pytest.fixture(scope="module")
def sd():
    return PCO.make_calibrated_weights(0)


@pytest.fixture(scope="module")
def net(sd):
    with make_net(sd) as c:
        yield c


@pytest.fixture(scope="module")
def pool():
    return source_clouds()[0]


def padded(clouds, stride=None, fill=np.nan):
    """-> (pc [B,stride,3] with `fill` beyond every cloud, n_points [B] int32 or None where no cloud is shorter than stride)."""
    counts = np.array([len(c) for c in clouds], np.int32)
    stride = int(stride or counts.max())
    pc = np.full((len(clouds), stride, 3), fill, np.float32)
    for i, c in enumerate(clouds):
        pc[i, :len(c)] = c
    return pc, (None if (counts == stride).all() else counts)


def gpu_grad(net, clouds, targets, loss="logits", kappa=0., scale=1., stride=None, starts=None):
    pc, n = padded(clouds, stride)
    g, aux = net.input_grad(pc, np.asarray(targets), loss, kappa, scale, n_points=n, want_aux=True, fps_start=starts)
    torch.cuda.synchronize()
    return g.cpu().numpy(), aux


def bits(net, clouds, targets, stride=None, fill=np.nan, starts=None, **kw):
    """The gradient rows of every cloud, as a list of arrays (the rows beyond a cloud must be zero)."""
    pc, n = padded(clouds, stride, fill)
    g = net.input_grad(pc, np.asarray(targets), n_points=n, fps_start=starts, **kw).cpu().numpy()
    for i, c in enumerate(clouds):
        assert not g[i, len(c):].any()
    return [g[i, :len(c)].copy() for i, c in enumerate(clouds)]


def check_parity(sd, clouds, targets, g, aux, loss="logits", kappa=0., scale=1., what="", max_out=MAX_OUT, starts=None):
    """The whole judgement of one call (module docstring) -> (clouds judged, worst |GPU - f64| / e_32 max |grad|, e_32)."""
    W32, W64 = PCO.to_torch(sd, torch.float32), PCO.to_torch(sd, torch.float64)
    F32, F64 = GO.folded(sd, torch.float32), GO.folded(sd, torch.float64)
    ch = [GO.gpu_choices(aux, b, len(c)) for b, c in enumerate(clouds)]
    for b, (c, h) in enumerate(zip(clouds, ch)):
        PCO.check_tables(c, h["tables"], (0, 0) if starts is None else tuple(int(v) for v in starts[b]), "%s cloud %d" % (what, b))
    r32 = [GO.run_cloud(W32, c, t, h["tables"], loss, kappa, scale, torch.float32) for c, t, h in zip(clouds, targets, ch)]
    r64 = [GO.run_cloud(W64, c, t, h["tables"], loss, kappa, scale, torch.float64) for c, t, h in zip(clouds, targets, ch)]
    e = GO.layer_errors(r32, r64)
    for b, (h, r) in enumerate(zip(ch, r64)):
        GO.choices_valid(h, r, e, "%s cloud %d" % (what, b))
    keep = [b for b, r in enumerate(r64) if not GO.head_exclusion(r, e, loss)]
    assert len(clouds) - len(keep) <= max_out * len(clouds), "%s: %d of %d clouds left out" % (what, len(clouds) - len(keep), len(clouds))
    kw = dict(loss=loss, kappa=kappa, scale=scale)
    x64 = {b: GO.explicit_from(F64, clouds[b], targets[b], ch[b], **kw)["grad"] for b in keep}
    x32 = {b: GO.explicit_from(F32, clouds[b], targets[b], ch[b], dtype=torch.float32, **kw)["grad"] for b in keep}
    e32 = GO.grad_e32([x32[b] for b in keep], [x64[b] for b in keep])
    ratios = {b: float(np.abs(g[b][:len(clouds[b])] - x64[b]).max() / (e32 * max(np.abs(x64[b]).max(), 1e-30))) for b in keep}
    print("%s: judged %d of %d, e_32 %.3e, |GPU - f64| / (e_32 max |grad|) per cloud: %s" %
          (what, len(keep), len(clouds), e32, ", ".join("%.2f" % ratios[b] for b in keep)))
    worst = 0.0
    for b in keep:
        worst = max(worst, AO.check_grad(g[b][:len(clouds[b])], x64[b], e32, "%s cloud %d" % (what, b)))
        lo = aux["logits"][b].cpu().numpy()
        assert np.abs(lo - r64[b]["logits"]).max() <= 8 * max(e["logits"], 1e-6), (what, b)
    return len(keep), worst, e32


# ---------------------------------------------------------------------------------------------- parity with float64
@pytest.mark.parametrize("name", list(CASES))
def test_gradient_against_f64(net, name):
    sd, clouds, targets, loss, stride, starts = case_inputs(name)
    scale = 1.0 / len(clouds)
    g, aux = gpu_grad(net, clouds, targets, loss, 0., scale, stride, starts)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    check_parity(sd, clouds, targets, g, aux, loss, 0., scale, name, starts=starts)
    want = AO.adv_loss(aux["logits"].cpu().double(), torch.as_tensor(targets), loss, 0.)[0].numpy()
    assert np.abs(aux["loss"].cpu().numpy() - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    if starts is not None:
        assert np.array_equal(aux["fps1"][:, 0].cpu().numpy(), starts[:, 0]) and np.array_equal(aux["fps2"][:, 0].cpu().numpy(), starts[:, 1])


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_clouds(net, name):
    """32 identical points, every point twice, two far clusters: finite, zero beyond the cloud, and parity with no cloud left out
    (the CPU test shows that the oracle alone admits all three)."""
    sd, clouds, targets = degenerate_inputs(name)
    g, aux = gpu_grad(net, clouds, targets, stride=len(clouds[0]) + 5)
    assert np.isfinite(g).all() and not g[0, len(clouds[0]):].any()
    check_parity(sd, clouds, targets, g, aux, what=name, max_out=0)


# ---------------------------------------------------------------------------------------------- the forward half
def test_forward_half_is_the_forward_call_bit_for_bit(net, pool):
    clouds = [np.ascontiguousarray(pool[i][:m], dtype=np.float32) for i, m in enumerate((300, 32, 64, 513, 40))]
    pc, n = padded(clouds, 520)
    starts = np.array([[17, 3], [0, 500], [63, 0], [512, 255], [5, 77]], np.int32)
    lo, fw = net.logits(pc, n, fps_start=starts, want_aux=True)
    _, aux = net.input_grad(pc, np.arange(5), n_points=n, want_aux=True, fps_start=starts)
    assert torch.equal(lo, aux["logits"]) and torch.equal(fw["pred"], aux["pred"])
    for k in FWD:
        assert torch.equal(fw[k], aux[k]), k
    assert not aux["dgate1"][1, 32:].any() and bool(aux["dgate1"][1, :32].any())


def test_the_gradient_call_writes_nothing_beyond_a_cloud(net, pool):
    """Rows beyond a cloud: zeros in grad, and the cloud's own padding is never read (NaN there changes nothing)."""
    clouds = [np.ascontiguousarray(pool[i][:m], dtype=np.float32) for i, m in enumerate((70, 33))]
    a = bits(net, clouds, [1, 2], stride=100, fill=np.nan)
    b = bits(net, clouds, [1, 2], stride=100, fill=0.0)
    assert all(np.array_equal(x, y) and np.abs(x).max() > 0 for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------- bits
def test_a_clouds_gradient_does_not_depend_on_its_batch(net, pool):
    n = 40
    me = np.ascontiguousarray(pool[3][:n], dtype=np.float32)
    st = np.array([[11, 200]], np.int32)
    base = bits(net, [me], [9], starts=st)[0]
    assert np.abs(base).max() > 0
    assert np.array_equal(bits(net, [me], [9], starts=st)[0], base)                         # two calls in a row
    # at positions 0, 16 and 32 of a batch of 33 clouds of 32 points: two chunks, the last cloud behind the 32-cloud chunk edge
    many = [np.ascontiguousarray(pool[(3 * j) % 24][j % 7:j % 7 + 32], dtype=np.float32) for j in range(33)]
    tg = np.arange(33) % 40
    s33 = np.stack([np.arange(33) % 20, (np.arange(33) * 5) % 512], 1).astype(np.int32)
    for at in (0, 16, 32):
        many[at], tg[at], s33[at] = me, 9, st[0]
    got = bits(net, many, tg, starts=s33)
    for at in (0, 16, 32):
        assert np.array_equal(got[at], base), at
    assert sum(np.abs(g).max() > 0 for g in got) > 25
    # the same context right after the larger call (a stale workspace), at stride n and at another stride, NaN and zero padding
    assert np.array_equal(bits(net, [me], [9], starts=st)[0], base)
    for fill in (np.nan, 0.0):
        assert np.array_equal(bits(net, [me], [9], stride=2048, fill=fill, starts=st)[0], base), fill
    # inside a ragged batch, with other neighbours
    other = [np.ascontiguousarray(pool[7][:600], dtype=np.float32), me, np.ascontiguousarray(pool[8][:32], dtype=np.float32)]
    got = bits(net, other, [1, 9, 3], starts=np.array([[5, 5], st[0], [1, 0]], np.int32))
    assert np.array_equal(got[1], base)


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
    n = np.array([100, 64, 99, 32, 100], np.int32)
    with I.Classifier(I.weights.pack_state_dict(I.weights.pointnet_random_state_dict(0), "pointnet"), device="cuda:0") as pn:
        for kind in ("fgm", "ifgm", "mifgm", "pgd"):
            out = []
            for c in (net, pn):
                pc, mom = (pc0 + 0.01).contiguous(), torch.full_like(pc0, 0.001)
                c.fgm_update(kind, grad, pc, pc0, mom, 0.05, 0.3, 0.9, n_points=n)
                out.append((pc.cpu(), mom.cpu()))
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), kind
            assert not torch.equal(out[0][0], (pc0 + 0.01).cpu())


@pytest.mark.parametrize("kind", ["fgm", "ifgm", "mifgm", "pgd"])
def test_fused_loop_equals_the_host_driven_loop(net, pool, kind, capsys):
    """fgm_attack (one library call) against attack.py's loop from the host, 3 iterations on 3 clouds of 100 points, bit for bit."""
    from ifdefense_amd import attack as A
    x = np.stack([pool[i][:100] for i in range(3)]).astype(np.float32)
    tg = (net.predict(x).cpu().numpy() + 1) % 40
    if kind == "fgm":
        a = A.FGM(net, "logits", 0.3).attack(x, tg)
        g = net.input_grad(x, tg, "logits", 0., 1.0 / 3)
        cur = torch.from_numpy(x).cuda()
        net.fgm_update("fgm", g, cur, None, None, 0.3, 0.3, 1.0)
        b = (cur.cpu().numpy(), int((net.predict(cur).cpu().numpy() == tg).sum()))
    else:
        cls = {"ifgm": A.IFGM, "mifgm": A.MIFGM, "pgd": A.PGD}[kind]
        a = cls(net, "logits", None, 0.6, 0.2, 3, seed=3).attack(x, tg)
        b = cls(net, "logits", None, 0.6, 0.2, 3, seed=3, verbose=False).attack(x, tg)
        assert capsys.readouterr().out.count("iter 0/3") == 1
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert not np.array_equal(a[0], x) and np.isfinite(a[0]).all()


@pytest.mark.parametrize("kind", ["ifgm", "mifgm"])
def test_loop_teacher_forced(net, sd, pool, kind):
    """At each of 3 iterations the GPU's gradient at ITS OWN current cloud passes the parity bar (free-running trajectories amplify
    the discontinuities), and the cloud it moves to is the oracle's update of that gradient."""
    B, n, budget, iters = 3, 65, 0.4, 3
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
        judged += check_parity(sd, list(before), tg, gh, aux, scale=scale, what="%s iteration %d" % (kind, it), max_out=1 / 3)[0]
        net.fgm_update(kind, g, cur, ori, mom, step, budget, mu)
        after = cur.cpu().numpy()
        for b in range(B):
            p64, _ = AO.update(kind, gh[b], before[b], x[b], None if mom is None else mom_before[b], step, budget, mu)
            p32, _ = AO.update(kind, gh[b], before[b], x[b], None if mom is None else mom_before[b], step, budget, mu, dtype=torch.float32)
            assert np.abs(after[b] - p64).max() <= 4 * max(np.abs(p32 - p64).max(), 1e-7), (kind, it, b)
    assert judged >= 0.8 * B * iters
    fused = net.fgm_attack(kind, x, tg, budget, step, iters, mu, scale=scale)[0]
    assert torch.equal(fused, cur)


@pytest.fixture(scope="module")
def cli_runs(net, sd, tmp_path_factory):
    """pointconv_fgm_attack on a file of 6 clouds x 64 points, I-FGM, 3 iterations, with --batch_size 4 and with -1 ->
    {batch size: (file name, its arrays)}, the file's starts."""
    from ifdefense_amd import pointconv_fgm_attack as PA, inference as Inf
    from ifdefense_amd.pointnet2_inference import fps_starts
    import bench
    tmp = tmp_path_factory.mktemp("pc_cli")
    ck, src = str(tmp / "pointconv.npz"), str(tmp / "attack_data.npz")
    np.savez(ck, **sd)
    pcs = bench.synth_clouds(6, seed=5)[:, :64]
    st = fps_starts(4, [64] * 6)
    pred = net.predict(np.stack([Inf.normalize_points_np(c) for c in pcs]), fps_start=st).cpu().numpy()
    np.savez(src, test_pc=pcs, test_label=pred.astype(np.uint8), target_label=((pred + 1) % 40).astype(np.uint8))
    runs = {}
    for bs in (4, -1):
        out = tmp / ("bs%d" % bs)
        assert PA.main(["--data_root", src, "--num_points", "64", "--attack_type", "ifgm", "--num_iter", "3", "--model_path", ck,
                        "--out_dir", str(out), "--batch_size", str(bs), "--fps_seed", "4"]) == 0
        d = out / "attack" / "results" / "mn40_64" / "FGM" / "pointconv"
        (name,) = os.listdir(d)
        runs[bs] = (name, dict(np.load(d / name)), str(d / name))
    return runs, st, pcs, ck


def test_cli_success_rate_is_what_the_inference_cli_reports(net, cli_runs, capsys):
    """The rate in the file's name is predict(test_pc, fps_start = fps_starts(seed, sizes)) == target, however the file was batched,
    and it is what pointconv_inference --fps_seed reports on that file."""
    from ifdefense_amd import pointconv_inference as PI
    runs, st, pcs, ck = cli_runs
    for bs, (name, z, path) in runs.items():
        rate = float((net.predict(z["test_pc"], fps_start=st).cpu().numpy() == z["target_label"]).mean())
        assert name.split("-success_")[1].split("-rank")[0] == "%.4f" % rate, (bs, name, rate)
        assert z["test_pc"].shape == (6, 64, 3) and np.isfinite(z["test_pc"]).all() and not np.array_equal(z["test_pc"], pcs)
    capsys.readouterr()
    name, z, path = runs[4]
    assert PI.main(["--data_root", path, "--num_points", "64", "--model_path", ck, "--fps_seed", "4", "--mode", "target"]) == 0
    out = capsys.readouterr().out
    rate = float(name.split("-success_")[1].split("-rank")[0])
    assert "attack success rate: %.4f" % rate in out, out


def test_cli_clouds_do_not_depend_on_the_batch_size(cli_runs):
    """With --batch_size 4 and with -1 the clouds written are equal bit for bit: starts, loss scale and start noise are the
    file's (attack_file(by_file=True)), and the library's gradient and update do not depend on the batch."""
    runs = cli_runs[0]
    a, b = runs[4][1]["test_pc"], runs[-1][1]["test_pc"]
    print("clouds differing: %d of %d elements, max |difference| %.3e" % (int((a != b).sum()), a.size, float(np.abs(a - b).max())))
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_contexts_usable(net, pool):
    import ctypes as C
    import ifdefense_amd as I
    import pointnet2_oracle as PO
    x = np.stack([pool[i][:64] for i in range(2)]).astype(np.float32)
    good = net.input_grad(x, [1, 2]).cpu()
    for bad, word in ((lambda: net.input_grad(x, [1, 2], n_points=[64, 31]), "n_points"),
                      (lambda: net.input_grad(x, [1, 2], n_points=[65, 64]), "n_points"),
                      (lambda: net.input_grad(np.zeros((1, 2049, 3), np.float32), [1]), "stride"),
                      (lambda: net.input_grad(np.zeros((1, 31, 3), np.float32), [1]), "stride"),
                      (lambda: net.input_grad(x, [1, 40]), "target"),
                      (lambda: net.input_grad(x, [-1, 2]), "target"),
                      (lambda: net.input_grad(x, [1, 2], fps_start=[[64, 0], [0, 0]]), "fps_start"),
                      (lambda: net.input_grad(x, [1, 2], fps_start=[[0, 512], [0, 0]]), "fps_start"),
                      (lambda: net.fgm_attack("ifgm", x, [1, 40], 0.1, 0.1, 2), "target"),
                      (lambda: net.fgm_attack("ifgm", x, [1, 2], 0.1, 0.1, 2, fps_start=[[0, 0], [0, -1]]), "fps_start"),
                      (lambda: net.fgm_attack("ifgm", np.zeros((1, 2049, 3), np.float32), [1], 0.1, 0.1, 2), "stride")):
        with pytest.raises(I.IfdError, match=word):
            bad()
        assert torch.equal(net.input_grad(x, [1, 2]).cpu(), good)              # the next valid call gives the same bits as before
    f32 = dict(device="cuda:0", dtype=torch.float32)
    pc, tg, g = torch.from_numpy(x).cuda(), torch.tensor([1, 2], dtype=torch.int32, device="cuda:0"), torch.empty(2, 64, 3, **f32)
    ok = torch.empty(2, dtype=torch.int32, device="cuda:0")
    lib, P = net.lib, I._lib.IfdFgmParams
    prm = P(C.sizeof(P), 1, 0, 2, 0.0, 1.0, 0.1, 0.1, 1.0)
    assert lib.ifd_pc_input_grad(net.ctx, pc.data_ptr(), None, None, 2, 64, tg.data_ptr(), 0, 0.0, 1.0, None, None, None) == IFD_ERR_ARG
    assert lib.ifd_pc_input_grad(net.ctx, pc.data_ptr(), None, None, 2, 64, tg.data_ptr(), 7, 0.0, 1.0, g.data_ptr(), None, None) == IFD_ERR_ARG
    assert lib.ifd_pc_fgm_attack(net.ctx, C.byref(prm), pc.data_ptr(), None, None, tg.data_ptr(), 2, 64, pc.data_ptr(), ok.data_ptr(),
                                 None) == IFD_ERR_ARG
    assert lib.ifd_pc_fgm_update(net.ctx, 1, g.data_ptr(), pc.data_ptr(), pc.data_ptr(), None, 0.1, 0.1, 1.0, None, 2, 2049, None) == IFD_ERR_ARG
    assert lib.ifd_pc_fgm_update(net.ctx, 1, g.data_ptr(), pc.data_ptr(), pc.data_ptr(), None, 0.1, 0.1, 1.0, None, 2, 31, None) == IFD_ERR_ARG
    # the calls of the three existing attack headers keep refusing a PointConv context, and the PointConv calls every other context
    rc = lib.ifd_cls_input_grad(net.ctx, pc.data_ptr(), None, 2, 64, tg.data_ptr(), 0, 0.0, 1.0, g.data_ptr(), None, None)
    assert rc == IFD_ERR_ARG and b"not a classifier context" in lib.ifd_last_error(net.ctx)
    rc = lib.ifd_dgcnn_input_grad(net.ctx, pc.data_ptr(), None, 2, 64, tg.data_ptr(), 0, 0.0, 1.0, g.data_ptr(), None, None)
    assert rc == IFD_ERR_ARG and b"not a DGCNN context" in lib.ifd_last_error(net.ctx)
    rc = lib.ifd_pn2_input_grad(net.ctx, pc.data_ptr(), None, None, 2, 64, tg.data_ptr(), 0, 0.0, 1.0, g.data_ptr(), None, None)
    assert rc == IFD_ERR_ARG and b"not a PointNet++ context" in lib.ifd_last_error(net.ctx)
    with I.Classifier(I.weights.pack_state_dict(I.weights.pointnet_random_state_dict(0), "pointnet"), device="cuda:0") as pn, \
            I.PointNet2Classifier(I.weights.pack_state_dict(PO.make_weights(0), "pointnet2"), device="cuda:0") as p2:
        for other in (pn, p2):
            rc = lib.ifd_pc_input_grad(other.ctx, pc.data_ptr(), None, None, 2, 64, tg.data_ptr(), 0, 0.0, 1.0, g.data_ptr(), None, None)
            assert rc == IFD_ERR_ARG and b"not a PointConv context" in lib.ifd_last_error(other.ctx)
            assert lib.ifd_pc_fgm_update(other.ctx, 0, g.data_ptr(), pc.data_ptr(), None, None, 0.1, 0.1, 1.0, None, 2, 64, None) == IFD_ERR_ARG
            assert lib.ifd_pc_fgm_attack(other.ctx, C.byref(prm), pc.data_ptr(), None, None, tg.data_ptr(), 2, 64, g.data_ptr(),
                                         ok.data_ptr(), None) == IFD_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(pc.cpu(), torch.from_numpy(x))                        # nothing was enqueued on the refused calls' clouds
    assert torch.equal(net.input_grad(x, [1, 2]).cpu(), good)
