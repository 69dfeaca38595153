"""GPU tests of the DGCNN victim (include/ifd_dgcnn.h) against tests/dgcnn_oracle.py.

The neighbour choice is judged on its own (exact float64 scores of the GPU's own layer inputs, a derived rounding bound, exact
ties on lattice clouds); the arithmetic is judged with the GPU's neighbour sets forced into the float32 and the float64 oracle,
every bar relative to e_32 = max |forced float32 oracle - forced float64 oracle| of the tensor in question, computed here.

Measured on an MI355X (worst e_gpu / e_32 over test_arithmetic_against_f64's cases): DESIGN 7m.
The neighbour choice is exact, not only within the bound: tests/test_gpu_dgcnn_exact.py holds it to the header bit for bit at n = 20
.. 2048, k = 1 .. 32, on queue-stressing row orders and on tied scores; the tolerance here stays as a second net."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ((0, 3), (0, 64), (64, 128), (128, 256))          # a layer's input: xyz, then these columns of feat
OUT_COLS = ((0, 64), (64, 128), (128, 256), (256, 512))  # x1 .. x4 in feat
IFD_ERR_ARG = -1
CHUNK = 128                                               # clouds per chunk of ifd_dgcnn_forward (include/ifd_dgcnn.h)


def make_net(sd, k=20):
    import ifdefense_amd as I
    return I.DgcnnClassifier(I.weights.pack_state_dict(sd, "dgcnn"), k=k, device="cuda:0")


@pytest.fixture(scope="module")
def sd():
    import dgcnn_oracle as DO
    return DO.make_weights(0)


@pytest.fixture(scope="module")
def net(sd):
    with make_net(sd) as c:
        yield c


@pytest.fixture(scope="module")
def pool():
    """Source clouds: 24 x 1024 points, and two of 2048 (two shapes side by side)."""
    import bench
    s = bench.synth_clouds(24, seed=77)
    big = [np.concatenate([s[20], 0.8 * s[21] + 0.1]), np.concatenate([s[22], 0.7 * s[23] - 0.2])]
    return s, [np.ascontiguousarray(b, dtype=np.float32) for b in big]


def cloud(pool, i, n):
    s, big = pool
    return np.ascontiguousarray(s[i][:n] if n <= 1024 else big[i % 2][:n], dtype=np.float32)


def run(net, clouds):
    """-> logits [B,40], aux (everything on the CPU), for a list of clouds or a [B,N,3] array."""
    lo, aux = net.logits(clouds, want_aux=True)
    torch.cuda.synchronize()
    return lo.cpu(), {"idx": [t.cpu() for t in aux["idx"]], "feat": aux["feat"].cpu(), "global_feat": aux["global_feat"].cpu(),
                      "pred": aux["pred"].cpu()}


def layer_input(c, feat_b, l):
    a, b = COLS[l]
    return np.asarray(c if l == 0 else feat_b[:len(c), a:b].numpy())


# ---- 1. neighbour validity ---------------------------------------------------------------------------------------------------
NEIGHBOUR_SIZES = (20, 21, 63, 64, 65, 255, 257, 1024)


def test_neighbours_are_the_k_best_in_every_layer(net, pool):
    import dgcnn_oracle as DO
    clouds = [cloud(pool, i, n) for i, n in enumerate(NEIGHBOUR_SIZES)]
    _, aux = run(net, clouds)
    for b, c in enumerate(clouds):
        for l in range(4):
            idx = aux["idx"][l][b, :len(c)].numpy()
            worst = DO.check_neighbours(layer_input(c, aux["feat"][b], l), idx, 20, "n = %d, layer %d" % (len(c), l + 1))
            print("n = %4d layer %d: worst (best left out - worst chosen) / 2 tau = %.3f" % (len(c), l + 1, worst))
            if len(c) == 20:
                assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(20), (20, 1)))


@pytest.mark.parametrize("k", [1, 32])
def test_neighbours_at_the_ends_of_k(sd, pool, k):
    import dgcnn_oracle as DO
    c = cloud(pool, 9, 65)
    with make_net(sd, k) as net:
        _, aux = run(net, [c])
    for l in range(4):
        DO.check_neighbours(layer_input(c, aux["feat"][0], l), aux["idx"][l][0].numpy(), k, "k = %d, layer %d" % (k, l + 1))


# ---- 2. exact ties -----------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_lowest_index(net):
    import dgcnn_oracle as DO
    rng = np.random.default_rng(5)
    lattice = (rng.integers(0, 5, size=(257, 3)) * 0.25).astype(np.float32)       # every layer-1 score is exact in f32, in any order
    half = (rng.integers(0, 5, size=(70, 3)) * 0.25 + rng.normal(0, 0.01, (70, 3))).astype(np.float32)
    twins = np.concatenate([half, half])                                         # point i + 70 is point i again
    inter = np.repeat(half, 2, axis=0)                                           # point 2 i + 1 is point 2 i again
    _, aux = run(net, [lattice, twins, inter])
    s = DO.exact_scores(lattice)
    got = np.sort(aux["idx"][0][0, :257].numpy(), axis=1)
    for i in range(257):
        want = np.lexsort((np.arange(257), -s[i]))[:20]                          # score descending, index ascending
        assert np.array_equal(got[i], np.sort(want)), (i, got[i], np.sort(want))
    for l in range(4):
        a = aux["idx"][l][1, :140].numpy()
        for i in range(140):
            row = set(a[i].tolist())
            assert all(j - 70 in row for j in row if j >= 70), ("twins", l, i, sorted(row))
        a = aux["idx"][l][2, :140].numpy()
        for i in range(140):
            row = set(a[i].tolist())
            assert all(j - 1 in row for j in row if j % 2 == 1), ("interleaved twins", l, i, sorted(row))
    f = aux["feat"][1, :140]
    assert torch.equal(f[:70], f[70:])                                           # twins stay twins through every layer


# ---- 3. arithmetic against float64, the GPU's neighbours forced ---------------------------------------------------------------
def forced_pair(sd, clouds, idx, k=20):
    import dgcnn_oracle as DO
    out = []
    for dt in (torch.float32, torch.float64):
        out.append(DO.forward(DO.to_torch(sd, dt), clouds, dtype=dt, k=k, idx=[t.numpy() for t in idx]))
    return out


def check_arithmetic(sd, clouds, lo, aux, what):
    r32, r64 = forced_pair(sd, clouds, aux["idx"])
    worst = {}

    def one(name, got, a32, a64):
        e32 = float((a32.double() - a64).abs().max())
        egpu = float((got.double() - a64).abs().max())
        assert e32 > 0, (what, name)
        worst[name] = max(worst.get(name, 0.0), egpu / e32)
        return egpu, e32

    bad = []
    for j, (a, b) in enumerate(OUT_COLS):
        for ci, c in enumerate(clouds):
            egpu, e32 = one("x%d" % (j + 1), aux["feat"][ci, :len(c), a:b], r32["feat"][ci][:, a:b], r64["feat"][ci][:, a:b])
            if egpu > 4 * e32:
                bad.append(("x%d" % (j + 1), ci, egpu, e32))
    for name, got in (("global_feat", aux["global_feat"]), ("logits", lo)):
        egpu, e32 = one(name, got, r32[name], r64[name])
        if egpu > 4 * e32:
            bad.append((name, egpu, e32))
    print("%s: worst e_gpu / e_32: %s" % (what, ", ".join("%s %.2f" % kv for kv in worst.items())))
    assert not bad, (what, bad)


@pytest.mark.parametrize("n,count", [(20, 2), (65, 2), (257, 2), (1024, 1), (1536, 1), (2048, 1)])
def test_arithmetic_against_f64(net, sd, pool, n, count):
    clouds = [cloud(pool, 3 + i, n) for i in range(count)]
    lo, aux = run(net, np.stack(clouds))
    check_arithmetic(sd, clouds, lo, aux, "%d x %d points" % (count, n))


def test_arithmetic_against_f64_ragged(net, sd, pool):
    clouds = [cloud(pool, 11 + i, n) for i, n in enumerate((20, 300, 65, 257))]
    lo, aux = run(net, clouds)
    check_arithmetic(sd, clouds, lo, aux, "ragged 20 / 300 / 65 / 257")


# ---- 4., 5. predictions ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def varied():
    import bench
    import dgcnn_oracle as DO
    sd = DO.make_calibrated_weights(0)
    x = np.ascontiguousarray(bench.synth_clouds(256, seed=23)[:, :128])
    with make_net(sd) as c:
        lo, aux = run(c, x)
    return sd, x, lo, aux


def test_predictions_against_f64(varied):
    import cls_checks
    import dgcnn_oracle as DO
    sd, x, lo, aux = varied
    lo32, lo64 = [], []
    for a in range(0, len(x), 32):
        idx = [t[a:a + 32].numpy() for t in aux["idx"]]
        lo32.append(DO.forward(DO.to_torch(sd), x[a:a + 32], idx=idx)["logits"])
        lo64.append(DO.forward(DO.to_torch(sd, torch.float64), x[a:a + 32], dtype=torch.float64, idx=idx)["logits"])
    lo32, lo64 = torch.cat(lo32), torch.cat(lo64)
    e_32 = cls_checks.e32_of(lo32, lo64)
    assert e_32 > 0
    e_gpu = float((lo.double() - lo64).abs().max())
    print("calibrated head: e_gpu %.3e, e_32 %.3e, ratio %.2f" % (e_gpu, e_32, e_gpu / e_32))
    assert e_gpu <= 4 * e_32
    cls_checks.check_pred_against_f64(aux["pred"].numpy(), lo64, e_32, "dgcnn, calibrated head, 256 x 128 points")
    # not asserted (the neighbour choice is the library's own, include/ifd_dgcnn.h): agreement with the oracle left to choose
    free = torch.cat([DO.forward(DO.to_torch(sd, torch.float64), x[a:a + 32], dtype=torch.float64)["logits"] for a in range(0, len(x), 32)])
    print("pred == argmax of the free-running float64 oracle on %.4f of the clouds; max |logits - free-running f64| %.3e"
          % (float((aux["pred"].long() == free.argmax(1)).float().mean()), float((lo.double() - free).abs().max())))


def test_pred_is_the_argmax_of_its_own_logits(varied, pool):
    import cls_checks
    import dgcnn_oracle as DO
    sd, x, lo, aux = varied
    cls_checks.check_pred_is_argmax(aux["pred"].numpy(), lo, "calibrated head")
    with make_net(DO.make_tied_weights(sd)) as c:
        lo_t, aux_t = run(c, x[:64])
    cls_checks.check_ties(lo_t, aux_t["pred"].numpy(), "tied head")
    assert torch.equal(lo_t[:, :20], lo[:64, :20])


# ---- 6. bitwise invariance ---------------------------------------------------------------------------------------------------
def same_cloud(a_lo, a_aux, ia, b_lo, b_aux, ib, n):
    assert torch.equal(a_lo[ia], b_lo[ib])
    assert torch.equal(a_aux["global_feat"][ia], b_aux["global_feat"][ib])
    assert torch.equal(a_aux["feat"][ia, :n], b_aux["feat"][ib, :n])
    assert a_aux["pred"][ia] == b_aux["pred"][ib]
    for l in range(4):
        assert torch.equal(torch.sort(a_aux["idx"][l][ia, :n], dim=1).values, torch.sort(b_aux["idx"][l][ib, :n], dim=1).values)


def test_a_cloud_does_not_depend_on_its_batch(net, pool):
    x = np.stack([cloud(pool, i, 200) for i in range(17)])
    lo17, aux17 = run(net, x)
    for B in (1, 2):
        lo, aux = run(net, x[:B])
        for b in range(B):
            same_cloud(lo, aux, b, lo17, aux17, b, 200)
    lo_r, aux_r = run(net, np.roll(x, 5, axis=0))
    for b in range(17):
        same_cloud(lo_r, aux_r, (b + 5) % 17, lo17, aux17, b, 200)
    # a larger stride, NaN beyond n_points
    pad = np.full((17, 333, 3), np.nan, np.float32)
    pad[:, :200] = x
    lo_p, aux_p = net.logits(pad, n_points=np.full(17, 200, np.int32), want_aux=True)
    torch.cuda.synchronize()
    aux_p = {"idx": [t.cpu() for t in aux_p["idx"]], "feat": aux_p["feat"].cpu(), "global_feat": aux_p["global_feat"].cpu(),
             "pred": aux_p["pred"].cpu()}
    for b in range(17):
        same_cloud(lo_p.cpu(), aux_p, b, lo17, aux17, b, 200)
    assert bool(torch.isfinite(lo_p).all())


def test_chunks_and_stale_workspace(net, pool):
    rng = np.random.default_rng(9)
    sizes = rng.integers(20, 65, size=CHUNK + 1)
    sizes[0], sizes[CHUNK] = 64, 20                            # the last cloud is alone in its chunk
    clouds = [cloud(pool, b % 24, int(n)) + np.float32(0.001 * b) for b, n in enumerate(sizes)]
    lo, aux = run(net, clouds)
    run(net, np.stack([cloud(pool, 1, 1024), cloud(pool, 2, 1024)]))        # a large call in between
    for b, c in enumerate(clouds):                             # ... then every cloud alone
        lo1, aux1 = run(net, [c])
        same_cloud(lo1, aux1, 0, lo, aux, b, len(c))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_runtime_refusals_leave_the_context_usable(net, pool):
    import ifdefense_amd as I
    x = np.stack([cloud(pool, 0, 64), cloud(pool, 1, 64)])
    want = net.logits(x).cpu()
    for bad_x, counts, words in ((x, [64, 19], "n_points outside"), (x, [65, 64], "n_points outside"),
                                 (np.zeros((1, 2049, 3), np.float32), None, "stride above 2048"),
                                 (x[:, :19], None, "fewer than k")):
        with pytest.raises(I.IfdError, match="libifd error %d: .*%s" % (IFD_ERR_ARG, words)):
            net.logits(bad_x, n_points=counts)
        assert torch.equal(net.logits(x).cpu(), want)


# ---- 8. the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(varied, tmp_path, capsys):
    from ifdefense_amd import dgcnn_inference
    sd, x, lo, aux = varied
    wpath = str(tmp_path / "dgcnn.npz")
    np.savez(wpath, **sd)
    pred = aux["pred"].numpy().astype(np.int64)
    label = pred.copy()
    label[::4] = (label[::4] + 1) % 40
    target = (pred + (np.arange(len(pred)) % 3 == 0)) % 40
    same = str(tmp_path / "kNN-dgcnn-same.npz")
    np.savez(same, test_pc=x[:48], test_label=label[:48], target_label=target[:48])
    assert dgcnn_inference.main(["--data_root", same, "--mode", "target", "--model_path", wpath, "--num_points", "128"]) == 0
    out = capsys.readouterr().out
    assert out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % ((pred[:48] == label[:48]).mean(), (pred[:48] == target[:48]).mean())
    sizes = [128, 100, 64, 20, 77, 128]
    rag = np.empty(len(sizes), dtype=object)
    for i, n in enumerate(sizes):
        rag[i] = x[100 + i, :n]
    with make_net(sd) as c:
        pr = c.predict([rag[i] for i in range(len(sizes))]).cpu().numpy()
    lab = pr.copy()
    lab[1] = (lab[1] + 3) % 40
    ragged = str(tmp_path / "sor-ragged.npz")
    np.savez(ragged, test_pc=rag, test_label=lab)
    assert dgcnn_inference.main(["--data_root", ragged, "--model", "dgcnn", "--model_path", wpath]) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f\n" % (5 / 6)
