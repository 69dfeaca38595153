"""GPU tests of the Perturb, kNN and Drop attacks on the DGCNN, PointNet++ and PointConv victims (include/ifd_victim_atk.h).

No float64 parity bar of their own: each victim's gradient is held to float64 in its own test file, and the step kernels are held
to cw_oracle / knn_oracle / drop_oracle and to the recorded reference runs on PointNet.  These tests show that the new loops are
exactly those two parts composed: the step calls do not depend on the victim (1), the loops on a PointNet context give the old
calls' bits (2), fused = host-driven on every victim (3), a cloud's result does not depend on its batch (4), the outputs mean what
the headers say (5), the refusals (6) and the three CLIs end to end (7).  Clouds have 48 points: PointConv's minimum plus room to
drop, and the sampled victims cost the same at any size.  DGCNN runs with k = 8."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch

from test_victim_atk_cpu import DG_K, MEANING_LR, MEANING_STEPS, N_POINTS, NUM_ITER, VICTIMS, meaning_inputs, state_dict

pytestmark = pytest.mark.gpu

IFD_ERR_ARG = -1
CHUNK = {"dgcnn": 128, "pointnet2": 128, "pointconv": 32}      # most clouds of one chunk of the victim's forward and gradient
DEV = "cuda:0"


def make(victim, sd=None):
    import ifdefense_amd as I
    sd = state_dict(victim) if sd is None else sd
    w = I.weights.pack_state_dict(sd, victim)
    if victim == "dgcnn":
        return I.DgcnnClassifier(w, k=DG_K, device=DEV)
    return {"pointnet2": I.PointNet2Classifier, "pointconv": I.PointConvClassifier}[victim](w, device=DEV)


def pointnet_weights(feature_transform=False):
    import ifdefense_amd as I
    import pointnet_oracle as PNO
    return I.weights.pack_state_dict(PNO.make_calibrated_weights(0, feature_transform), "pointnet")


@pytest.fixture(scope="module")
def nets():
    """{victim: classifier}, "pointnet": the PointNet victim through its own entry points, "pointnet-victim": the same weights
    through the ifd_victim_* entry points."""
    import ifdefense_amd as I

    class ThroughVictimCalls(I.Classifier):
        LOOP_FNS = I.Classifier.VICTIM_LOOP_FNS

        def _loop_starts(self, fps_start, B):
            return super()._loop_starts(fps_start, B) + [None]

    out = {v: make(v) for v in VICTIMS}
    out["pointnet"] = I.Classifier(pointnet_weights(), device=DEV)
    out["pointnet-victim"] = ThroughVictimCalls(pointnet_weights(), device=DEV)
    yield out
    for n in out.values():
        n.close()


def clouds_of(B, n=N_POINTS, seed=21):
    import bench
    from ifdefense_amd.inference import normalize_points_np
    return np.stack([normalize_points_np(c[:n]) for c in bench.synth_clouds(B, seed=seed)]).astype(np.float32)


def starts_of(victim, B, n=N_POINTS):
    if victim in ("dgcnn", "pointnet", "pointnet-victim"):
        return None
    return np.stack([(5 * np.arange(B) + 2) % n, (13 * np.arange(B) + 7) % 512], axis=1).astype(np.int32)


def skw(starts, idx=None):
    """fps_start as a keyword of a runtime call; nothing for a victim that does not sample."""
    return {} if starts is None else {"fps_start": starts if idx is None else starts[idx]}


def normals_of(B, n=N_POINTS, seed=5):
    v = np.random.default_rng(seed).standard_normal((B, n, 3)).astype(np.float32)
    return v / np.linalg.norm(v, axis=2, keepdims=True)


def noise_of(shape, seed=3):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 1e-7).numpy()


def same(a, b, what=""):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
        "%s: %d of %d elements differ" % (what, int((a != b).sum()), a.size)


# The three fused attacks through the runtime -> a tuple of arrays with the batch in front
P_KW = dict(loss="logits", kappa=0., attack_lr=1e-2, init_weight=10., max_weight=80.)


def run_perturb(net, pc, tgt, noise, starts, n_points=None, binary_step=2, num_iter=3, scale=None):
    out, best, ok, bounds = net.cw_perturb_attack(pc, tgt, noise, scale=scale or 1.0 / len(pc), binary_step=binary_step, num_iter=num_iter,
                                                  n_points=n_points, want_bounds=True, **P_KW, **skw(starts))
    return out, best, ok, bounds["weight"], bounds["lower"], bounds["upper"]


def run_knn(net, pc, tgt, noise, starts, normal=None, n_points=None, num_iter=3, scale=None):
    return net.knn_attack(pc, tgt, normal, noise, "logits", 15., scale or 1.0 / len(pc), 1e-3, num_iter, n_points=n_points, **skw(starts))


def run_drop(net, pc, label, starts, num_drop=12, k=5, n_points=None, scale=None):
    return net.drop_attack(pc, label, num_drop, k, 1., scale or 1.0 / len(pc), n_points=n_points, want_kept=True, **skw(starts))


def valid_rows(t, counts):
    t = t.detach().cpu().numpy()
    return [t[b, :n].copy() for b, n in enumerate(counts)]


# ---------------------------------------------------------------------------------------------- 1. the steps do not depend on the victim
STEP_COUNTS = (70, 69, 64, 33, 32)


def run_steps(net):
    """The five step calls on fixed random inputs, B = 5, stride 70, NaN beyond every cloud's count -> {name: bytes}."""
    B, S = 5, 70
    g = torch.Generator().manual_seed(17)
    n = torch.tensor(STEP_COUNTS, dtype=torch.int32, device=DEV)
    beyond = (torch.arange(S)[None, :] >= torch.tensor(STEP_COUNTS)[:, None])[:, :, None].expand(B, S, 3)

    def cloud(scale=1.0, positive=False):
        t = torch.randn(B, S, 3, generator=g) * scale
        t = t.abs() if positive else t
        return torch.where(beyond, torch.full_like(t, float("nan")), t).to(DEV).contiguous()
    ori = cloud()
    adv0 = (ori + cloud(0.01)).contiguous()
    grad, normal = cloud(0.1), cloud()
    pred = torch.tensor([3, 7, 7, 1, 0], dtype=torch.int32, device=DEV)
    tgt = torch.tensor([3, 7, 2, 1, 5], dtype=torch.int32, device=DEV)
    loss = torch.rand(B, generator=g).to(DEV)
    out = {}
    # Perturb: a state in mid-attack
    st = net.cw_state(B, S, 10., 80.)
    st["m"], st["v"], st["o_bestattack"] = cloud(0.01), cloud(0.001, positive=True), cloud()
    st["bestdist"] = torch.tensor([1e10, 0.01, 1e10, 5.0, 1e10], device=DEV)
    st["bestscore"] = torch.tensor([-1, 7, -1, 1, -1], dtype=torch.int32, device=DEV)
    st["o_bestdist"] = torch.tensor([1e10, 0.01, 1e10, 0.2, 1e10], device=DEV)
    st["o_bestscore"] = st["bestscore"].clone()
    adv, last = adv0.clone(), torch.full_like(adv0, float("nan"))
    out["cw_info"] = net.cw_step(st, grad, pred, tgt, adv, ori, 3, 1e-2, 0.2, loss=loss, last_input=last, n_points=n, want_info=True)
    out.update(cw_adv=adv, cw_last=last, **{"cw1_" + k: v.clone() for k, v in st.items()})
    net.cw_adjust(st, tgt, n_points=n)
    out.update({"cw2_" + k: v.clone() for k, v in st.items()})
    # kNN
    adv, m, v = adv0.clone(), cloud(0.01), cloud(0.001, positive=True)
    d = net.knn_step(grad, adv, ori, m, v, 2, 1e-3, 0.2, normal=normal, loss=loss, n_points=n, want=("info", "dist_grad", "nn_ori", "nn5", "mask"))
    out.update(knn_adv=adv, knn_m=m, knn_v=v, **{"knn_" + k: t for k, t in d.items()})
    adv = (ori + cloud(0.2)).contiguous()
    out["clip_adv"] = net.knn_project_clip(adv, ori, normal, 0.1, n_points=n)
    # Drop
    pc, cnt = ori.clone(), n.clone()
    index = torch.arange(S, dtype=torch.int32, device=DEV)[None].repeat(B, 1).contiguous()
    d = net.drop_step(grad, pc, cnt, 3, 1., index=index, want=("saliency", "center", "dropped"))
    out.update(drop_pc=pc, drop_n=cnt, drop_index=index, **{"drop_" + k: t for k, t in d.items()})
    torch.cuda.synchronize()
    for name in ("cw_adv", "cw_last", "cw1_m", "cw1_v", "knn_adv", "knn_m", "knn_v", "clip_adv"):
        assert bool(torch.isnan(out[name].cpu()[beyond]).all()), name        # rows beyond a cloud's count come back untouched
        assert not bool(torch.isnan(out[name].cpu()[~beyond]).any()), name
    assert out["drop_n"].cpu().tolist() == [c - 3 for c in STEP_COUNTS]
    return {k: t.detach().cpu().numpy().tobytes() for k, t in out.items()}


@pytest.fixture(scope="module")
def pointnet_steps(nets):
    return run_steps(nets["pointnet"])


@pytest.mark.parametrize("victim", ("pointnet-victim",) + VICTIMS)
def test_steps_do_not_depend_on_the_victim(nets, pointnet_steps, victim):
    got = run_steps(nets[victim])
    assert sorted(got) == sorted(pointnet_steps)
    for k in got:
        assert got[k] == pointnet_steps[k], k


# ---------------------------------------------------------------------------------------------- 2. PointNet contexts: the old calls' bits
def test_pointnet_context_gives_the_old_calls_bits(nets):
    old, new = nets["pointnet"], nets["pointnet-victim"]
    B, n = 4, 64
    pc = clouds_of(B, n)
    tgt = (old.predict(pc).cpu().numpy() + 1) % 40
    label = old.predict(pc).cpu().numpy()
    noise = noise_of((2, B, n, 3))
    for a, b in zip(run_perturb(old, pc, tgt, noise, None), run_perturb(new, pc, tgt, noise, None)):
        same(a, b, "perturb")
    for a, b in zip(run_knn(old, pc, tgt, noise[0], None, normals_of(B, n)), run_knn(new, pc, tgt, noise[0], None, normals_of(B, n))):
        same(a, b, "knn")
    r_old, r_new = run_drop(old, pc, label, None, num_drop=7), run_drop(new, pc, label, None, num_drop=7)      # rounds of 5 and 2
    assert tuple(r_old[0].shape) == (B, n - 7, 3)
    for a, b in zip(r_old, r_new):
        same(a, b, "drop")


# ---------------------------------------------------------------------------------------------- 3. fused = host-driven
def bound(victim, net, starts, B):
    from ifdefense_amd.victim_atk_cli import BoundLoopStarts
    if starts is None:
        return net
    w = BoundLoopStarts(net, starts)
    w.at(0, B)
    return w


@pytest.mark.parametrize("victim", VICTIMS)
@pytest.mark.parametrize("kind", ("perturb", "knn", "drop"))
def test_fused_is_host_driven_through_the_attack_classes(nets, victim, kind, capsys):
    from ifdefense_amd import attack as A
    B = 3
    pc, starts = clouds_of(B), starts_of(victim, B, N_POINTS - 12)
    model = bound(victim, nets[victim], starts, B)
    pred = nets[victim].predict(pc, **skw(starts)).cpu().numpy()
    got = {}
    for verbose in (True, False):
        if kind == "perturb":
            atk = A.CWPerturb(model, "logits", "l2", attack_lr=1e-2, binary_step=2, num_iter=3, seed=4, verbose=verbose)
            got[verbose] = atk.attack(pc, (pred + 1) % 40)
        elif kind == "knn":
            atk = A.CWKNN(model, "logits", attack_lr=1e-3, num_iter=3, kappa=15., seed=4, verbose=verbose)
            got[verbose] = atk.attack(np.concatenate([pc, normals_of(B)], axis=2), (pred + 1) % 40)
        else:
            atk = A.SaliencyDrop(model, num_drop=12, alpha=1, k=5, verbose=verbose)          # three rounds, the last of 2; 36 points left
            got[verbose] = atk.attack(pc, pred)
            assert got[verbose][0].shape == (B, N_POINTS - 12, 3)
    lines = capsys.readouterr().out
    assert ("Iteration 0/" in lines or "Step 0, iteration 0" in lines)
    for a, b in zip(got[True], got[False]):
        same(np.asarray(a), np.asarray(b), "%s %s" % (victim, kind))


RAGGED = (48, 40, 33)


def ragged_batch(seed=31):
    pc = np.full((3, N_POINTS, 3), np.nan, np.float32)
    for b, n in enumerate(RAGGED):
        pc[b, :n] = clouds_of(3, n, seed)[b]
    return pc, np.array(RAGGED, np.int32)


@pytest.mark.parametrize("victim", VICTIMS)
def test_fused_is_host_driven_on_ragged_counts(nets, victim):
    """The raw runtime calls with counts {48, 40, 33} and NaN beyond them: Perturb (2 x 3), kNN (3) and Drop (one point)."""
    net = nets[victim]
    pc, n = ragged_batch()
    starts = starts_of(victim, 3, 30)
    kw = skw(starts)
    pred = net.predict(pc, n, **kw).cpu().numpy()
    tgt = torch.as_tensor((pred + 1) % 40).to(DEV)
    noise = np.nan_to_num(noise_of((2, 3, N_POINTS, 3)))
    x = torch.from_numpy(pc).to(DEV)
    nd = torch.from_numpy(n).to(DEV)
    # Perturb
    fused = run_perturb(net, pc, tgt, noise, starts, n_points=n)
    st = net.cw_state(3, N_POINTS, 10., 80.)
    last = torch.full_like(x, float("nan"))
    for step in range(2):
        adv = (x + torch.from_numpy(noise[step]).to(DEV)).contiguous()
        for it in range(3):
            grad, aux = net.input_grad(adv, tgt, "logits", 0., 1.0 / 3, n_points=nd, want_aux=("pred", "loss"), **kw)
            assert sorted(aux) == ["loss", "pred"]
            net.cw_step(st, grad, aux["pred"], tgt, adv, x, it + 1, 1e-2, 1.0 / 3, loss=aux["loss"], n_points=nd,
                        last_input=last if (step, it) == (1, 2) else None)
        net.cw_adjust(st, tgt, n_points=nd)
    ok = st["lower"] > 0
    host = (torch.where(ok[:, None, None], st["o_bestattack"], last), st["o_bestdist"], ok, st["weight"], st["lower"], st["upper"])
    for a, b in zip(valid_rows(fused[0], RAGGED), valid_rows(host[0], RAGGED)):
        same(a, b, "perturb clouds")
    for a, b in zip(fused[1:], host[1:]):
        same(a, b, "perturb records")
    # kNN
    normal = normals_of(3)
    fo, fp, fok = run_knn(net, pc, tgt, noise[0], starts, normal, n_points=n)
    adv = (x + torch.from_numpy(noise[0]).to(DEV)).contiguous()
    m, v, nrm = torch.zeros_like(x), torch.zeros_like(x), torch.from_numpy(normal).to(DEV)
    for it in range(3):
        grad, aux = net.input_grad(adv, tgt, "logits", 15., 1.0 / 3, n_points=nd, want_aux=("loss",), **kw)
        net.knn_step(grad, adv, x, m, v, it + 1, 1e-3, 1.0 / 3, normal=nrm, loss=aux["loss"], n_points=nd)
    for a, b in zip(valid_rows(fo, RAGGED), valid_rows(adv, RAGGED)):
        same(a, b, "knn clouds")
    same(fp, net.predict(adv, nd, **kw), "knn pred")
    # Drop, one point
    label = torch.as_tensor(pred).to(DEV)
    do, dok, dkept = run_drop(net, pc, label, starts, num_drop=1, n_points=n)
    cur, cnt = x.clone(), nd.clone()
    index = torch.arange(N_POINTS, dtype=torch.int32, device=DEV)[None].repeat(3, 1).contiguous()
    grad = net.input_grad(cur, label, "cross_entropy", 0., 1.0 / 3, n_points=cnt, **kw)
    net.drop_step(grad, cur, cnt, 1, 1., index=index)
    left = [c - 1 for c in RAGGED]
    assert cnt.cpu().tolist() == left
    for a, b in zip(valid_rows(do, left), valid_rows(cur, left)):
        same(a, b, "drop clouds")
    for a, b in zip(valid_rows(dkept, left), valid_rows(index, left)):
        same(a, b, "drop kept")
    same(dok, net.predict(cur, cnt, **kw).to(DEV) == label.long(), "drop correct")


# ---------------------------------------------------------------------------------------------- 4. a cloud's result does not depend on its batch
def all_three(net, pc, tgt, label, noise, starts, normal, idx=None, **kw):
    """Perturb, kNN and Drop on the clouds idx of a batch (all of it: None) -> a list of arrays, the batch in front."""
    i = slice(None) if idx is None else idx
    st = None if starts is None else starts[i]
    scale = 1.0 / len(pc)                                                       # the whole batch's, whatever part of it runs
    out = list(run_perturb(net, pc[i], tgt[i], noise[:, i], st, scale=scale, **kw))
    out += list(run_knn(net, pc[i], tgt[i], noise[0][i], st, normal[i], scale=scale))
    out += list(run_drop(net, pc[i], label[i], st, scale=scale))
    return out


@pytest.mark.parametrize("victim", VICTIMS)
def test_permuted_and_single_clouds_give_the_same_bits(nets, victim):
    net, B = nets[victim], 3
    pc, starts, normal = clouds_of(B, seed=41), starts_of(victim, B, N_POINTS - 12), normals_of(B)
    label = net.predict(pc, **skw(starts)).cpu().numpy()
    tgt = (label + 1) % 40
    noise = noise_of((2, B, N_POINTS, 3))
    whole = all_three(net, pc, tgt, label, noise, starts, normal)
    perm = [2, 0, 1]
    for k, (a, b) in enumerate(zip(whole, all_three(net, pc, tgt, label, noise, starts, normal, idx=perm))):
        same(a[perm], b, "permuted, output %d" % k)
    for k, (a, b) in enumerate(zip(whole, all_three(net, pc, tgt, label, noise, starts, normal, idx=[1]))):
        same(a[1:2], b, "alone, output %d" % k)


@pytest.mark.parametrize("victim", VICTIMS)
def test_clouds_beyond_the_chunk_equal_their_single_runs(nets, victim):
    """B = the victim's chunk + 1: Perturb with 1 search step x 2 iterations, Drop with one round."""
    net, B = nets[victim], CHUNK[victim] + 1
    base = clouds_of(8, seed=51)
    rng = np.random.default_rng(8)
    pc = np.stack([base[b % 8] * np.float32(1.0 - 0.001 * (b // 8)) for b in range(B)]).astype(np.float32)
    starts = starts_of(victim, B, N_POINTS - 5)
    label = rng.integers(0, 40, B)
    tgt = (label + 1) % 40
    noise = noise_of((1, B, N_POINTS, 3))
    scale = 1.0 / B
    big_p = run_perturb(net, pc, tgt, noise, starts, binary_step=1, num_iter=2, scale=scale)
    big_d = run_drop(net, pc, label, starts, num_drop=5, scale=scale)
    for b in (0, CHUNK[victim] - 1, CHUNK[victim]):
        i = [b]
        st = None if starts is None else starts[i]
        for k, (a, c) in enumerate(zip(big_p, run_perturb(net, pc[i], tgt[i], noise[:, i], st, binary_step=1, num_iter=2, scale=scale))):
            same(a[b:b + 1], c, "perturb cloud %d output %d" % (b, k))
        for k, (a, c) in enumerate(zip(big_d, run_drop(net, pc[i], label[i], st, num_drop=5, scale=scale))):
            same(a[b:b + 1], c, "drop cloud %d output %d" % (b, k))


# ---------------------------------------------------------------------------------------------- 5. meaning
@pytest.mark.parametrize("victim", VICTIMS)
def test_perturb_meaning(nets, victim):
    """The run test_victim_atk_cpu.py::test_oracle_perturb_reaches_the_target chose num_iter for: at least one cloud succeeds."""
    net = nets[victim]
    pc, tgt, starts, noise = meaning_inputs(victim)
    starts = None if victim == "dgcnn" else starts
    out, best, ok, weight, lower, upper = run_perturb(net, pc, tgt, noise, starts, binary_step=MEANING_STEPS, num_iter=NUM_ITER[victim])
    assert P_KW["attack_lr"] == MEANING_LR
    ok, best, out = ok.cpu().numpy(), best.cpu().numpy(), out.cpu().numpy()
    print("%s: %d of %d clouds reach their target in %d x %d iterations" % (victim, int(ok.sum()), len(ok), MEANING_STEPS, NUM_ITER[victim]))
    assert np.array_equal(ok, lower.cpu().numpy() > 0)
    assert int(ok.sum()) >= 1
    pred = net.predict(out, **skw(starts)).cpu().numpy()
    assert np.array_equal(pred[ok], np.asarray(tgt)[ok])
    dist = np.sqrt(((out.astype(np.float64) - pc.astype(np.float64)) ** 2).sum(axis=(1, 2)))
    assert (np.abs(best[ok] - dist[ok]) <= 1e-6 * dist[ok]).all(), (best[ok], dist[ok])
    assert (best[~ok] == np.float32(1e10)).all()
    assert np.isfinite(out).all()


@pytest.mark.parametrize("victim", VICTIMS)
def test_knn_and_drop_meaning(nets, victim):
    net, B = nets[victim], 3
    pc, starts, normal = clouds_of(B, seed=61), starts_of(victim, B, N_POINTS - 12), normals_of(B)
    label = net.predict(pc, **skw(starts)).cpu().numpy()
    tgt = (label + 1) % 40
    out, pred, ok = run_knn(net, pc, tgt, noise_of((B, N_POINTS, 3)), starts, normal, num_iter=5)
    out = out.cpu().numpy()
    # |adv - ori| <= budget per point (the clip's norm), so per component too; one float32 rounding of ori + d on top
    assert (np.abs(out.astype(np.float64) - pc) <= 0.1 + np.spacing(np.float32(1.1))).all()
    same(pred, net.predict(out, **skw(starts)), "knn pred")
    assert np.array_equal(ok.cpu().numpy(), pred.cpu().numpy() == tgt)
    # Drop: 12 points in rounds of 5, 5 and 2
    full, _, _ = net.drop_attack(pc, label, 12, 5, 1., 1.0 / B, **skw(starts)), None, None
    dout, correct, kept = run_drop(net, pc, label, starts)
    same(full[0], dout, "drop without kept")
    dout, kept = dout.cpu().numpy(), kept.cpu().numpy()
    assert dout.shape == (B, N_POINTS - 12, 3) and kept.shape == (B, N_POINTS - 12)
    for b in range(B):
        assert (np.diff(kept[b]) > 0).all() and kept[b].min() >= 0 and kept[b].max() < N_POINTS
        assert np.array_equal(dout[b], pc[b][kept[b]])
    assert np.array_equal(correct.cpu().numpy(), net.predict(dout, **skw(starts)).cpu().numpy() == label)
    # the raw call: n_out and the zeros behind the survivors
    P = _params("drop", num_drop=12, k=5, scale=1.0 / B)
    bufs = _drop_buffers(pc, label, starts)
    rc = net.lib.ifd_victim_drop_attack(net.ctx, C.byref(P), *_ptrs(bufs, "pc", "n", "starts", "label"), B, N_POINTS,
                                        *_ptrs(bufs, "out", "n_out", "kept", "correct"), None)
    assert rc == 0, net.lib.ifd_last_error(net.ctx)
    torch.cuda.synchronize()
    assert bufs["n_out"].cpu().tolist() == [N_POINTS - 12] * B
    raw = bufs["out"].cpu().numpy()
    assert np.array_equal(raw[:, :N_POINTS - 12], dout) and not raw[:, N_POINTS - 12:].any()
    assert (bufs["kept"].cpu().numpy()[:, N_POINTS - 12:] == -1).all()


# ---------------------------------------------------------------------------------------------- 6. refusals
def _params(kind, **kw):
    from ifdefense_amd import _lib
    if kind == "perturb":
        return _lib.IfdCwParams(kw.get("struct_size", C.sizeof(_lib.IfdCwParams)), 0, 1, 1, 0., 1., 1e-2, 10., 80.)
    if kind == "knn":
        return _lib.IfdKnnParams(kw.get("struct_size", C.sizeof(_lib.IfdKnnParams)), 0, 1, 15., 1., 1e-3, 5., 3., 1.05, 0.1)
    return _lib.IfdDropParams(kw.get("struct_size", C.sizeof(_lib.IfdDropParams)), kw.get("num_drop", 5), kw.get("k", 5), 1., kw.get("scale", 1.))


def _drop_buffers(pc, label, starts, n=None):
    B, S = pc.shape[:2]
    i32 = dict(dtype=torch.int32, device=DEV)
    return {"pc": torch.from_numpy(np.ascontiguousarray(pc)).to(DEV), "label": torch.as_tensor(np.asarray(label)).to(**i32),
            "n": None if n is None else torch.as_tensor(np.asarray(n)).to(**i32),
            "starts": None if starts is None else torch.as_tensor(np.asarray(starts)).to(**i32).contiguous(),
            "out": torch.full((B, S, 3), 7.0, device=DEV), "n_out": torch.full((B,), -7, **i32), "kept": torch.full((B, S), -7, **i32),
            "correct": torch.full((B,), -7, **i32), "best": torch.full((B,), 7.0, device=DEV), "pred": torch.full((B,), -7, **i32)}


def _ptrs(bufs, *names):
    return [None if bufs[n] is None else bufs[n].data_ptr() for n in names]


def raw_call(net, kind, bufs, B, S, P, pc_out="out"):
    """The raw ifd_victim_*_attack call -> (status, message)."""
    lib = net.lib
    if kind == "perturb":
        rc = lib.ifd_victim_cw_perturb_attack(net.ctx, None if P is None else C.byref(P), *_ptrs(bufs, "pc", "n", "starts", "label"), None, B, S,
                                              *_ptrs(bufs, pc_out, "best", "correct"), None, None)
    elif kind == "knn":
        rc = lib.ifd_victim_knn_attack(net.ctx, None if P is None else C.byref(P), bufs["pc"].data_ptr(), None, *_ptrs(bufs, "n", "starts", "label"),
                                       None, B, S, *_ptrs(bufs, pc_out, "pred", "correct"), None)
    else:
        rc = lib.ifd_victim_drop_attack(net.ctx, None if P is None else C.byref(P), *_ptrs(bufs, "pc", "n", "starts", "label"), B, S,
                                        *_ptrs(bufs, pc_out, "n_out", "kept", "correct"), None)
    return rc, (lib.ifd_last_error(net.ctx) or b"").decode()


CALL = {"perturb": "ifd_victim_cw_perturb_attack", "knn": "ifd_victim_knn_attack", "drop": "ifd_victim_drop_attack"}


def refused(net, kind, bufs, P, word, B=2, S=N_POINTS, pc_out="out"):
    rc, msg = raw_call(net, kind, bufs, B, S, P, pc_out)
    torch.cuda.synchronize()
    assert rc == IFD_ERR_ARG and msg.startswith(CALL[kind] + ":") and word in msg, (kind, rc, msg)
    for name, fill in (("out", 7.0), ("n_out", -7), ("kept", -7), ("correct", -7), ("best", 7.0), ("pred", -7)):
        assert bool((bufs[name] == fill).all()), (kind, name)               # nothing was enqueued on the outputs


def test_refusals(nets):
    import ifdefense_amd as I
    pc, label = clouds_of(2, seed=71), [1, 2]
    some = np.array([[1, 2], [3, 4]], np.int32)
    for kind in ("perturb", "knn", "drop"):
        # a victim that does not sample takes no starts
        for victim in ("pointnet", "dgcnn"):
            refused(nets[victim], kind, _drop_buffers(pc, label, some), _params(kind), "fps_start must be NULL")
        for victim in VICTIMS:
            net, st = nets[victim], starts_of(victim, 2, N_POINTS - 12)
            good = _drop_buffers(pc, label, st)
            refused(net, kind, good, _params(kind, struct_size=4), "struct_size")
            refused(net, kind, good, None, "params missing")
            refused(net, kind, good, _params(kind), "overlaps", pc_out="pc")
            big = _drop_buffers(np.zeros((1, 2049, 3), np.float32), [1], None)
            refused(net, kind, big, _params(kind), "stride", B=1, S=2049)
            refused(net, kind, _drop_buffers(pc, [1, 40], st), _params(kind), "outside [0, 40)")
    # kNN below 6 points
    for victim in ("pointnet2", "pointnet"):
        refused(nets[victim], "knn", _drop_buffers(pc, label, None, n=[5, N_POINTS]), _params("knn"), "1 cloud(s) with n_points outside [6, stride]")
    refused(nets["pointnet2"], "knn", _drop_buffers(pc[:, :5], label, None), _params("knn"), "stride outside [6, 2048]", S=5)
    # Drop: what is left must be a cloud the victim takes ...
    refused(nets["pointconv"], "drop", _drop_buffers(pc, label, None), _params("drop", num_drop=N_POINTS - 31), "without n_points, stride outside")
    refused(nets["pointconv"], "drop", _drop_buffers(pc, label, None, n=[N_POINTS, N_POINTS - 1]), _params("drop", num_drop=N_POINTS - 32),
            "1 cloud(s) with n_points outside [%d, %d]" % (N_POINTS, N_POINTS))
    refused(nets["dgcnn"], "drop", _drop_buffers(pc, label, None), _params("drop", num_drop=N_POINTS - DG_K + 1), "without n_points, stride outside")
    refused(nets["dgcnn"], "drop", _drop_buffers(pc, label, None, n=[N_POINTS, N_POINTS - 1]), _params("drop", num_drop=N_POINTS - DG_K),
            "1 cloud(s) with n_points outside")
    # ... and its start a row that every round still has: [n - num_drop, n) is refused, n - num_drop - 1 is taken
    for victim in ("pointnet2", "pointconv"):
        net = nets[victim]
        for s0 in (N_POINTS - 12, N_POINTS - 1):
            refused(net, "drop", _drop_buffers(pc, label, np.array([[0, 0], [s0, 0]], np.int32)), _params("drop", num_drop=12),
                    "1 cloud(s) with fps_start outside [0, n_points - 12) x [0, 512)")
        refused(net, "drop", _drop_buffers(pc, label, np.array([[0, 512], [0, 0]], np.int32)), _params("drop", num_drop=12), "fps_start outside")
        refused(net, "perturb", _drop_buffers(pc, label, np.array([[N_POINTS, 0], [0, 0]], np.int32)), _params("perturb"),
                "1 cloud(s) with fps_start outside [0, n_points) x [0, 512)")
        ok = _drop_buffers(pc, label, np.array([[0, 0], [N_POINTS - 13, 511]], np.int32))
        rc, msg = raw_call(net, "drop", ok, 2, N_POINTS, _params("drop", num_drop=12))
        torch.cuda.synchronize()
        assert rc == 0 and ok["n_out"].cpu().tolist() == [N_POINTS - 12] * 2, msg
        # the ragged form of the same rule: the start is held against the cloud's own count
        refused(net, "drop", _drop_buffers(pc, label, np.array([[0, 0], [N_POINTS - 14, 0]], np.int32), n=[N_POINTS, N_POINTS - 2]),
                _params("drop", num_drop=12), "fps_start outside")
    # a PointNet context with feature_transform keeps its refusal, in the new calls' names
    with I.Classifier(pointnet_weights(True), feature_transform=True, device=DEV) as ft:
        for kind in ("perturb", "knn", "drop"):
            refused(ft, kind, _drop_buffers(pc, label, None), _params(kind), "input gradients are not built for a model with feature_transform")
        x = torch.zeros(2, N_POINTS, 3, device=DEV)
        n = torch.full((2,), N_POINTS, dtype=torch.int32, device=DEV)
        rc = ft.lib.ifd_victim_drop_step(ft.ctx, x.data_ptr(), x.data_ptr(), n.data_ptr(), None, 2, N_POINTS, 1, 1.0, None, None)
        assert rc == IFD_ERR_ARG and b"ifd_victim_drop_step: input gradients are not built" in ft.lib.ifd_last_error(ft.ctx)
        rc = ft.lib.ifd_victim_knn_project_clip(ft.ctx, x.data_ptr(), x.data_ptr(), None, 0.1, None, 2, N_POINTS, None)
        assert rc == IFD_ERR_ARG and b"ifd_victim_knn_project_clip: input gradients are not built" in ft.lib.ifd_last_error(ft.ctx)
    # the refused contexts go on working
    net = nets["pointconv"]
    a = run_drop(net, pc, label, None)
    b = run_drop(net, pc, label, None)
    same(a[0], b[0], "after the refusals")


# ---------------------------------------------------------------------------------------------- 7. the CLIs end to end
def _stdout_of(main, argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert main(argv) == 0
    return buf.getvalue()


@pytest.mark.parametrize("victim", VICTIMS)
def test_clis_end_to_end(nets, victim, tmp_path):
    """A 5-cloud file through the three CLIs: the result lands under the reference's path, the victim's inference CLI with the same
    --fps_seed / --k prints the rate (Drop: the accuracy) in the file's name, and --batch_size 2 and -1 write the same bytes."""
    import importlib
    from ifdefense_amd import victim_drop_attack, victim_knn_attack, victim_perturb_attack
    from ifdefense_amd.pointnet2_inference import fps_starts
    inference = importlib.import_module("ifdefense_amd.%s_inference" % victim)
    net = nets[victim]
    ck, src, src6 = str(tmp_path / ("%s.npz" % victim)), str(tmp_path / "attack_data.npz"), str(tmp_path / "attack_data_normals.npz")
    np.savez(ck, **state_dict(victim))
    pcs = clouds_of(5, seed=81)
    st = None if victim == "dgcnn" else fps_starts(4, [N_POINTS] * 5)
    pred = net.predict(pcs, **skw(st)).cpu().numpy()
    labels = dict(test_label=pred.astype(np.uint8), target_label=((pred + 1) % 40).astype(np.uint8))
    np.savez(src, test_pc=pcs, **labels)
    np.savez(src6, test_pc=np.concatenate([pcs, normals_of(5)], axis=2), **labels)
    common = ["--model", victim, "--num_points", str(N_POINTS), "--model_path", ck, "--fps_seed", "4", "--k", str(DG_K)]
    runs = (("perturb", victim_perturb_attack, src, ["--binary_step", "2", "--num_iter", "3"], "Perturb", "success_"),
            ("knn", victim_knn_attack, src6, ["--num_iter", "3"], "kNN", "success_"),
            ("drop", victim_drop_attack, src, ["--num_drop", "12"], "Drop_12", "acc_"))
    for kind, cli, data, flags, sub, key in runs:
        files = {}
        for bs in (2, -1):
            out = tmp_path / ("%s_bs%d" % (kind, bs))
            _stdout_of(cli.main, common + flags + ["--data_root", data, "--out_dir", str(out), "--batch_size", str(bs)])
            d = out / "attack" / "results" / ("mn40_%d" % N_POINTS) / sub
            (name,) = os.listdir(d)
            assert name.startswith({"perturb": "Perturb-", "knn": "kNN-", "drop": "Drop-"}[kind] + victim + "-")
            files[bs] = (str(d / name), np.load(d / name))
        a, b = files[2][1]["test_pc"], files[-1][1]["test_pc"]
        assert a.shape == (5, N_POINTS - (12 if kind == "drop" else 0), 3) and a.dtype == np.float32 and np.isfinite(a).all()
        assert a.tobytes() == b.tobytes(), "%s: --batch_size changes %d elements" % (kind, int((a != b).sum()))
        path = files[-1][0]
        said = _stdout_of(inference.main, ["--data_root", path, "--model", victim, "--mode", "target", "--model_path", ck, "--k", str(DG_K)] +
                          ([] if victim == "dgcnn" else ["--fps_seed", "4"]))
        rate = os.path.basename(path).split(key)[1][:6]
        word = "Overall accuracy: " if kind == "drop" else "attack success rate: "
        assert word + rate in said, (kind, path, said)
