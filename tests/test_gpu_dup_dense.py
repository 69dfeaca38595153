"""GPU parity of ifd_punet_forward, ifd_srs and ifd_dup_fill where the shipped checkpoint and the golden clouds cannot see:
dense seeded weights (punet_oracle.make_weights: a third of the checkpoint's channels are dead, and a dead channel hides a
wrong column map), every golden cloud and synthetic ones against float64, every differing decision attributed to a float64
near-tie, degenerate clouds, the 512-cloud chunk loop, the library's own draws, and the K = 10000 / K = 1 size edges.

Arithmetic bar: max |GPU - f64| <= 4 * e_32 with e_32 = max |f32 oracle - f64 oracle| per cloud group, both oracle runs fed
the GPU's decisions and float32 distances (dist_dtype): the expanded form's float32 noise at coinciding points, which the
kernel reproduces on purpose, is then on both sides and the bar measures arithmetic only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dup_golden.npz")
DEC = ("fps_idx", "ball_idx", "knn_idx")
SEEDS = (1, 2)
WEIGHT_SETS = ("shipped",) + tuple("dense%d" % s for s in SEEDS)
# golden clouds by what the DUP fill did to them: 7 repeats input rows, 11-13 are 2-3 whole copies plus a remainder draw
GOLDEN_GROUPS = {"golden plain": [0, 1, 2, 3, 4, 5, 6, 8, 9, 10, 14, 15], "golden repeated": [7, 11, 12, 13]}


def state_dict(name):
    import punet_oracle as PO
    return PO.load_weights() if name == "shipped" else PO.make_weights(int(name[5:]))


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def nets():
    import ifdefense_amd as I
    from ifdefense_amd import weights
    made = {n: I.DupNet(weights.pack_state_dict(state_dict(n), "punet"), device="cuda:0", seed=3) for n in WEIGHT_SETS}
    yield made
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def synth():
    import bench
    x = torch.from_numpy(bench.synth_clouds(16, seed=21))
    st = torch.from_numpy(np.random.default_rng(21).integers(0, (1024, 1024, 512, 256), (16, 4)).astype(np.int32))
    return x, st


def run_gpu(net, x, st):
    out, aux = net.pu_net(x, fps_start=st, want_aux=True)
    torch.cuda.synchronize()
    return out.cpu(), {k: v.cpu() for k, v in aux.items()}


def check_arithmetic(name, out, aux, x, groups, chunk=8):
    """The bar of the module docstring on `out` = the GPU's result for clouds x under weight set `name`, per group of rows."""
    import punet_oracle as PO
    sd = state_dict(name)
    W64, W32 = PO.to_torch(sd, torch.float64), PO.to_torch(sd)
    assert torch.isfinite(out).all()
    ratios = {}
    for gname, sel in groups.items():
        r64, r32 = [], []
        for a in range(0, len(sel), chunk):
            s = sel[a:a + chunk]
            dec = {k: aux[k][s] for k in DEC}
            r64.append(PO.forward(W64, x[s], dtype=torch.float64, dist_dtype=torch.float32, **dec)[0])
            r32.append(PO.forward(W32, x[s], dist_dtype=torch.float32, **dec)[0])
        r64, r32 = torch.cat(r64), torch.cat(r32)
        assert torch.isfinite(r32).all()
        e_gpu = float((out[sel].double() - r64).abs().max())
        e_32 = float((r32.double() - r64).abs().max())
        print("%s, %s (%d clouds): max |GPU - f64| %.3e, max |f32 oracle - f64| %.3e, ratio %.2f" % (
            name, gname, len(sel), e_gpu, e_32, e_gpu / e_32))
        ratios[gname] = e_gpu / e_32
    for gname, r in ratios.items():
        assert r <= 4, (name, gname, r)


def check_decisions(aux, x, st, what):
    """FPS identical to the float32 oracle; every ball-query and 3-NN row that differs from it attributed to a float64
    near-tie (punet_oracle.attribute_decisions, band measured per cloud from the oracle; indices of coinciding centroids
    count as one, see there); at most 1 % of rows differ."""
    import punet_oracle as PO
    ref = PO.decisions(x, st)
    assert torch.equal(aux["fps_idx"], ref["fps_idx"]), what
    exact = PO.exact_distances(ref["l_xyz"])
    band = PO.distance_band(ref["l_xyz"], exact)
    nb, nk, bad = PO.attribute_decisions(aux, ref, exact, band, ref["l_xyz"])
    rows_b, rows_k = aux["ball_idx"][..., 0].numel(), aux["knn_idx"][..., 0].numel()
    print("%s: ball-query rows differing %d of %d, 3-NN rows differing %d of %d, not attributable %d; band %.2e .. %.2e" % (
        what, nb, rows_b, nk, rows_k, len(bad), float(band.min()), float(band.max())))
    assert not bad, "\n".join(bad[:20])
    assert nb <= 0.01 * rows_b and nk <= 0.01 * rows_k
    return ref


# ---------------------------------------------------------------------------------------------- C.1 - C.3
@pytest.fixture(scope="module")
def golden_runs(nets, g):
    x, st = torch.from_numpy(g["filled"]), torch.from_numpy(g["fps_start"])
    return x, st, {n: run_gpu(nets[n], x, st) for n in WEIGHT_SETS}


@pytest.fixture(scope="module")
def synth_runs(nets, synth):
    x, st = synth
    return x, st, {n: run_gpu(nets[n], x, st) for n in WEIGHT_SETS}


@pytest.mark.parametrize("name", WEIGHT_SETS)
def test_golden_clouds_against_float64(golden_runs, name):
    """All 16 golden clouds, the duplicate-heavy ones in a group of their own, under the shipped and both dense weight sets."""
    x, _, runs = golden_runs
    out, aux = runs[name]
    check_arithmetic(name, out, aux, x, GOLDEN_GROUPS)


@pytest.mark.parametrize("name", WEIGHT_SETS)
def test_synthetic_clouds_against_float64(synth_runs, name):
    x, _, runs = synth_runs
    out, aux = runs[name]
    check_arithmetic(name, out, aux, x, {"synthetic": list(range(16))})


def test_decisions_do_not_depend_on_the_weights(golden_runs, synth_runs):
    for _, _, runs in (golden_runs, synth_runs):
        for n in WEIGHT_SETS[1:]:
            assert all(torch.equal(runs[n][1][k], runs["shipped"][1][k]) for k in DEC), n


def test_decisions_attributed_on_golden_and_synthetic_clouds(golden_runs, synth_runs, g):
    x, st, runs = golden_runs
    check_decisions(runs["dense1"][1], x, st, "golden")
    assert np.array_equal(runs["dense1"][1]["fps_idx"].numpy(), g["fps_idx"])
    x, st, runs = synth_runs
    check_decisions(runs["dense1"][1], x, st, "synthetic")


# ---------------------------------------------------------------------------------------------- C.4 degenerate clouds
def cluster_cloud():
    """18 tight clusters (0.02 wide, 0.6 apart: every level-0 ball is exactly its centroid's cluster).  A: 32 points, all
    inside the scan's first 64 indices (fills at its last member there); B: 16 + 16 across the first two 64-index steps
    (fills exactly at the end of the second); C: 16 + 40 (overflows inside the second); D: 31 points (one short: first-member
    fill); the rest 64 or 41 points spread over indices 128..1023."""
    rng = np.random.default_rng(5)
    lab = np.empty(1024, np.int64)
    lab[:64] = [0] * 32 + [1] * 16 + [2] * 16
    lab[64:128] = [1] * 16 + [2] * 40 + [3] * 8
    rest = [3] * 23 + [4 + k for k in range(13) for _ in range(64)] + [17] * 41
    lab[128:] = rng.permutation(np.asarray(rest))
    centres = np.array([[0.6 * (i - 1), 0.6 * (j - 1), 0.6 * k - 0.3] for i in range(3) for j in range(3) for k in range(2)])
    pts = centres[lab] + rng.uniform(-0.01, 0.01, (1024, 3))
    return pts.astype(np.float32), lab


def degenerate_clouds(g):
    rng = np.random.default_rng(9)
    base = rng.uniform(-0.8, 0.8, (40, 3)).astype(np.float32)
    clouds = {"%d distinct" % n: base[np.arange(1024) % n] for n in (1, 2, 31, 33)}
    clouds["inside one ball"] = (np.float32([0.31, -0.22, 0.4]) + rng.uniform(-0.01, 0.01, (1024, 3))).astype(np.float32)
    clouds["clusters"] = cluster_cloud()[0]
    clouds["translated"] = g["filled"][0] + np.float32(0.5)
    return clouds


@pytest.fixture(scope="module")
def degenerate_runs(nets, g):
    clouds = degenerate_clouds(g)
    x = torch.from_numpy(np.stack(list(clouds.values())))
    st = torch.tensor([[17, 900, 300, 100]], dtype=torch.int32).repeat(len(clouds), 1)
    return list(clouds), x, st, {n: run_gpu(nets[n], x, st) for n in WEIGHT_SETS}


def test_degenerate_clouds_are_in_the_reference_domain(g):
    """CPU side, before anything is asserted about the GPU: the float32 oracle is finite on each cloud (none was dropped) and
    no ball is empty (each centroid is a point of its own level, so its own distance, rounding noise, is below r^2)."""
    import punet_oracle as PO
    clouds = degenerate_clouds(g)
    x = torch.from_numpy(np.stack(list(clouds.values())))
    st = torch.tensor([[17, 900, 300, 100]], dtype=torch.int32).repeat(len(clouds), 1)
    for n in WEIGHT_SETS:
        out, rec = PO.forward(PO.to_torch(state_dict(n)), x, st)
        assert torch.isfinite(out).all(), n
    for q, c, r in PO.level_inputs(PO.decisions(x, st)["l_xyz"])[:4]:
        assert bool((PO.square_distance(q, c) <= r ** 2).any(-1).all())


def test_degenerate_clouds_decisions(degenerate_runs):
    names, x, st, runs = degenerate_runs
    aux = runs["dense1"][1]
    assert all(torch.equal(runs[n][1][k], aux[k]) for n in WEIGHT_SETS for k in DEC)
    for i, name in enumerate(names):
        check_decisions({k: aux[k][i:i + 1] for k in DEC}, x[i:i + 1], st[i:i + 1], name)
    ball = aux["ball_idx"].numpy()
    # every ball holds every point of its level: the members are the first 32 indices
    assert (ball[names.index("1 distinct")] == np.arange(32)).all() and (ball[names.index("inside one ball")] == np.arange(32)).all()
    # level 0 of the cluster cloud in closed form: the first 32 indices of the centroid's cluster, the first one filling up
    _, lab = cluster_cloud()
    ci = names.index("clusters")
    fps0 = aux["fps_idx"][ci, :1024].numpy()
    seen = set()
    for w in range(1024):
        mem = np.flatnonzero(lab == lab[fps0[w]])[:32]
        want = np.concatenate([mem, np.full(32 - len(mem), mem[0])])
        assert np.array_equal(ball[ci, w], want), (w, lab[fps0[w]])
        seen.add(int(lab[fps0[w]]))
    assert seen == set(range(18))


@pytest.mark.parametrize("name", WEIGHT_SETS)
def test_degenerate_clouds_against_float64(degenerate_runs, name):
    names, x, _, runs = degenerate_runs
    out, aux = runs[name]
    check_arithmetic(name, out, aux, x, {n: [i] for i, n in enumerate(names)})


# ---------------------------------------------------------------------------------------------- C.5 chunk edges
EDGE = (0, 511, 512, 513, 1023, 1024)


def test_chunk_loop_of_punet_forward(nets):
    """ifd_punet_forward splits a batch into chunks of 512 clouds itself (runtime.DupNet also splits at `chunk`, 512 by
    default, so only a DupNet with a larger chunk reaches that loop).  B = 1025 is chunks of 512, 512 and 1: the clouds
    either side of each boundary, run alone with the matching start row / cloud_index_base, give the same bits."""
    import bench
    import ifdefense_amd as I
    from ifdefense_amd import weights
    x = torch.from_numpy(bench.synth_clouds(1025, seed=31))
    st = torch.from_numpy(np.random.default_rng(31).integers(0, (1024, 1024, 512, 256), (1025, 4)).astype(np.int32))
    small = nets["dense1"]
    big = I.DupNet(weights.pack_state_dict(state_dict("dense1"), "punet"), device="cuda:0", seed=3, chunk=4096)
    try:
        for kw, base in (({"fps_start": st}, 0), ({}, 1000)):
            def alone(i):
                o, a = small.pu_net(x[i:i + 1], fps_start=st[i:i + 1] if kw else None, cloud_index_base=base + i, want_aux=True)
                return o.cpu(), {k: v.cpu() for k, v in a.items()}
            singles = {i: alone(i) for i in EDGE}
            if not kw:                     # the library's FPS starts depend on the global cloud index
                assert not torch.equal(singles[0][1]["fps_idx"], small.pu_net(x[:1], cloud_index_base=0, want_aux=True)[1]["fps_idx"].cpu())
            for B in (1025, 512, 513):     # 513 after 512 after 1025 on one context: the workspace is kept and re-laid
                o, a = big.pu_net(x[:B], cloud_index_base=base, want_aux=True, **({"fps_start": st[:B]} if kw else {}))
                o, a = o.cpu(), {k: v.cpu() for k, v in a.items()}
                assert torch.isfinite(o).all()
                for i in [i for i in EDGE if i < B]:
                    assert torch.equal(o[i:i + 1], singles[i][0]), (B, i, base)
                    assert all(torch.equal(a[k][i:i + 1], singles[i][1][k]) for k in DEC), (B, i, base)
            o2 = small.pu_net(x, cloud_index_base=base, **kw).cpu()    # the Python-side split agrees with the library's
            assert torch.equal(o2, big.pu_net(x, cloud_index_base=base, **kw).cpu())
    finally:
        big.close()


# ---------------------------------------------------------------------------------------------- C.6 draws and size edges
def fill_restated(pc, keep, draws):
    """DUPNet.process_data in numpy (include/ifd_dup.h): the kept rows padded or trimmed to 1024 with explicit draws."""
    rows = pc[keep.astype(bool)]
    N = len(rows)
    if N == 1024:
        return rows
    if N > 1024:
        return rows[draws[:1024]]
    q = 1024 // N
    return np.concatenate([rows] * q + [rows[draws[:1024 - q * N]]])


def tuples(a):
    return [tuple(r) for r in np.asarray(a).tolist()]


def test_fill_library_draws(nets):
    import ifdefense_amd as I
    net = nets["shipped"]
    rng = np.random.default_rng(41)
    kept = [1500, 700, 300, 1024, 1, 512]           # N > 1024; q = 1; q = 3; N = 1024; q = 1024 and q = 2 with no remainder
    pc = rng.standard_normal((len(kept), 2048, 3)).astype(np.float32)
    keep = np.zeros((len(kept), 2048), np.uint8)
    for i, n in enumerate(kept):
        keep[i, rng.permutation(2048)[:n]] = 1
    tp, tk = torch.from_numpy(pc), torch.from_numpy(keep)
    out, n = net.process_data(tp, tk)
    out = out.cpu().numpy()
    assert n.cpu().tolist() == kept
    for i, N in enumerate(kept):
        rows = tuples(pc[i][keep[i].astype(bool)])
        got = tuples(out[i])
        assert set(got) <= set(rows), i
        if N > 1024:
            assert len(set(got)) == 1024
            assert got != rows[:1024]                                   # a draw, not a truncation
        elif N == 1024:
            assert got == rows
        else:
            q = 1024 // N
            assert got[:q * N] == rows * q, i
            rest = got[q * N:]
            assert len(rest) == 1024 - q * N and len(set(rest)) == len(rest), i
            assert not rest or rest != rows[:len(rest)]
    a, _ = net.process_data(tp[:2], tk[:2])
    b, _ = net.process_data(tp[2:], tk[2:], cloud_index_base=2)
    assert np.array_equal(torch.cat([a, b]).cpu().numpy(), out)
    assert np.array_equal(net.process_data(tp, tk)[0].cpu().numpy(), out)
    shifted, _ = net.process_data(tp, tk, cloud_index_base=1)
    other = I.DupNet(None, device="cuda:0", seed=4)
    try:
        seeded = other.process_data(tp, tk)[0].cpu().numpy()
    finally:
        other.close()
    for i in (0, 1, 2):                                                 # the clouds that draw
        assert not np.array_equal(seeded[i], out[i]) and not np.array_equal(shifted[i].cpu().numpy(), out[i])
    for i in (3, 4, 5):
        assert np.array_equal(seeded[i], out[i])


def test_size_edges_of_srs_and_fill(nets):
    """K = 10000 (the largest the ABI takes: 80 KB and 120 KB of dynamic LDS) and K = 1, explicit draws against numpy and
    the library's own draws as properties."""
    net = nets["shipped"]
    rng = np.random.default_rng(43)
    K = 10000
    pc = rng.standard_normal((3, K, 3)).astype(np.float32)
    tp = torch.from_numpy(pc)
    for drop in (1, K - 1):
        m = K - drop
        idx = np.stack([rng.permutation(K)[:m] for _ in range(3)]).astype(np.int32)
        got = net.srs(tp, drop, idx=torch.from_numpy(idx)).cpu().numpy()
        assert np.array_equal(got, np.stack([pc[b][idx[b]] for b in range(3)])), drop
        lib = net.srs(tp, drop).cpu().numpy()
        assert lib.shape == (3, m, 3)
        for b in range(3):
            rows = tuples(lib[b])
            assert len(set(rows)) == m and set(rows) <= set(tuples(pc[b])), (drop, b)
        assert np.array_equal(lib[1:], net.srs(tp[1:], drop, cloud_index_base=1).cpu().numpy())
    first = net.srs(tp, K - 1).cpu().numpy()[:, 0]
    assert len({tuples(pc[b]).index(tuple(first[b])) for b in range(3)}) > 1          # three clouds, not one draw
    keep = np.ones((3, K), np.uint8)
    keep[1] = 0
    keep[1, 7777] = 1                                                   # cloud 1: one kept row; clouds 0, 2: all kept
    draws = np.stack([rng.permutation(K)[:1024] for _ in range(3)]).astype(np.int32)
    out, n = net.process_data(tp, torch.from_numpy(keep), draws=torch.from_numpy(draws))
    assert n.cpu().tolist() == [K, 1, K]
    for b in range(3):
        assert np.array_equal(out[b].cpu().numpy(), fill_restated(pc[b], keep[b], draws[b])), b
    lib = net.process_data(tp, torch.from_numpy(keep))[0].cpu().numpy()
    assert np.array_equal(lib[1], np.repeat(pc[1, 7777][None], 1024, 0))
    for b in (0, 2):
        rows = tuples(lib[b])
        assert len(set(rows)) == 1024 and set(rows) <= set(tuples(pc[b]))
    one = torch.from_numpy(pc[:, :1].copy())
    assert np.array_equal(net.srs(one, 0).cpu().numpy(), pc[:, :1])
    assert np.array_equal(net.srs(one, 0, idx=torch.zeros(3, 1, dtype=torch.int32)).cpu().numpy(), pc[:, :1])
    out, n = net.process_data(one, torch.ones(3, 1, dtype=torch.uint8))
    assert n.cpu().tolist() == [1, 1, 1] and np.array_equal(out.cpu().numpy(), np.repeat(pc[:, :1], 1024, 1))


def test_first_srs_draw_is_uniform(nets):
    """The first draw of SRS over 65,536 cloud indices at K = 16: chi-square against the uniform law, 15 degrees of freedom,
    99.9 % quantile 37.7.  Philox is deterministic: seed 3 gives the statistic printed here, every run."""
    net = nets["shipped"]
    B, K = 65536, 16
    pc = torch.zeros(B, K, 3)
    pc[:, :, 0] = torch.arange(K, dtype=torch.float32)
    first = net.srs(pc, K - 1).cpu()[:, 0, 0].long()
    counts = torch.bincount(first, minlength=K).double()
    assert counts.numel() == K and int(counts.sum()) == B
    chi2 = float(((counts - B / K) ** 2 / (B / K)).sum())
    print("chi-square of the first SRS draw, 65536 clouds, K = 16, seed 3: %.2f (99.9 %% quantile 37.7)" % chi2)
    assert chi2 <= 37.7
    full = net.srs(pc[:4096], 0).cpu()[:, :, 0].long()                  # drop 0: each output is a permutation of the rows
    assert torch.equal(full.sort(1)[0], torch.arange(K).repeat(4096, 1))
    pos = torch.stack([torch.bincount(full[:, j], minlength=K) for j in range(K)]).double()
    chi2_pos = ((pos - 256) ** 2 / 256).sum(1)
    print("chi-square per output position over 4096 clouds: max %.2f" % float(chi2_pos.max()))
