"""The victim classifier (include/ifd_cls.h) under weights whose predictions vary from cloud to cloud
(pointnet_oracle.make_calibrated_weights: 22 / 25 classes on 512 clouds where make_weights gives one or two), so that what is built
on the prediction - argmax, the tie rule, which cloud gets which answer, the CLI's accuracy - is checked by more than one class.
Also the edges test_gpu_cls.py leaves out: batch sizes around fc_kernel's 16-cloud tiles and the 256-cloud blocks, the C ABI's
chunk loop (B > 4096), and workspace rows left by an earlier, longer call.

Bars: logits and aux outputs |GPU - f64| <= 4 e_32 (test_gpu_cls.check_against_f64, e_32 recomputed under these weights);
predictions equal the float64 oracle's wherever its top-2 margin is >= 8 e_32 (cls_checks: each of the two logits may move by
4 e_32), at most 1 % of the clouds below that; tests/test_cls_varied_cpu.py holds the reference alone to the same cap.  Everything
about batching is bitwise."""
import os

import numpy as np
import pytest
import torch

import cls_checks as CC
from test_gpu_cls import NAMES, check_against_f64, gpu_outputs, oracle_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cls_golden.npz")
CLS_CHUNK = 4096                                   # api.cpp: most clouds per chunk of ifd_cls_forward


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "feature_transform"])
def ft(request):
    return request.param


@pytest.fixture(scope="module")
def sd(g, ft):
    import pointnet_oracle as PO
    return PO.make_calibrated_weights(int(g["weight_seed"]), ft)


def make_net(sd, ft):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    return I.Classifier(weights.pack_state_dict(sd, "pointnet"), feature_transform=ft, device="cuda:0")


@pytest.fixture(scope="module")
def net(sd, ft):
    with make_net(sd, ft) as c:
        yield c


@pytest.fixture(scope="module")
def clouds512():
    import bench
    return bench.synth_clouds(512, seed=23)


@pytest.fixture(scope="module")
def ref512(sd, clouds512):
    """(float32 oracle, float64 oracle) outputs on the 512 evaluation clouds, once per mode; nothing writes to them."""
    return oracle_pair(sd, clouds512, chunk=4)


@pytest.fixture(scope="module")
def gpu512(net, clouds512):
    return gpu_outputs(net, torch.from_numpy(clouds512))


def run_all(net, x, n_points=None):
    """-> {"logits", "pred", "trans", "global_feat" (, "trans_feat")} on the CPU."""
    lo, aux = net.logits(x, n_points, want_aux=True)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in aux.items()}
    out["logits"] = lo.cpu()
    return out


def assert_rows_equal(part, whole, rows, what):
    assert set(part) == set(whole)
    for k in whole:
        assert torch.equal(part[k], whole[k][rows]), (what, k)


def check_rows_against_f64(sd, out, x, n_points, rows, what):
    """Clouds ``rows`` of a GPU result against the float64 oracle at the usual bar, and their predictions."""
    r32, r64 = oracle_pair(sd, [x[i] for i in rows], [int(n_points[i]) for i in rows])
    got = tuple(out[k][rows] if k in out else None for k in NAMES)
    worst = check_against_f64(got, r32, r64, what)
    e_32 = CC.e32_of(r32[0], r64[0])
    clear = CC.top2_margin(r64[0]) >= CC.MARGIN_FACTOR * e_32
    assert np.array_equal(out["pred"][rows].numpy()[clear], r64[0].argmax(1).numpy()[clear]), what
    print("%s: clouds %s, e_32 %.3e, worst e_gpu / e_32 %.2f, excluded %d" % (what, list(rows), e_32, worst, int((~clear).sum())))


def ragged_batch(x, n_points):
    """x [B,S,3] with every row at or beyond n_points[b] set to NaN: nothing beyond a cloud's count may be read into a result."""
    x = torch.from_numpy(np.ascontiguousarray(x)).clone()
    x[torch.arange(x.shape[1])[None, :] >= torch.as_tensor(n_points)[:, None].long()] = float("nan")
    return x


# ------------------------------------------------------------------------------------------------------- (a) arithmetic
def test_arithmetic_against_float64(net, sd, g):
    clouds = [g["pc_%d" % i] for i in range(int(g["n_clouds"]))]
    r32, r64 = oracle_pair(sd, clouds)
    got, pred = gpu_outputs(net, clouds)
    worst = check_against_f64(got, r32, r64, "golden clouds, calibrated weights")
    e_32, margin = CC.e32_of(r32[0], r64[0]), CC.top2_margin(r64[0])
    print("golden clouds: e_32 %.3e, worst e_gpu / e_32 %.2f, classes predicted %d, smallest top-2 margin %.0f e_32, excluded 0"
          % (e_32, worst, len(set(pred.tolist())), margin.min() / e_32))
    assert np.array_equal(pred.numpy(), r64[0].argmax(1).numpy())             # every golden cloud, no exclusions


# ------------------------------------------------------------------------------------------------------ (b) predictions
def test_predictions_on_512_clouds(ref512, gpu512):
    r32, r64 = ref512
    got, pred = gpu512
    worst = check_against_f64(got, r32, r64, "512 clouds")
    e_32 = CC.e32_of(r32[0], r64[0])
    excluded, classes = CC.check_pred_against_f64(pred.numpy(), r64[0], e_32, "512 clouds")
    print("512 clouds: e_32 %.3e, worst e_gpu / e_32 %.2f, classes predicted %d, excluded %d" % (e_32, worst, classes, excluded))


# ------------------------------------------------------------------------------------------- (c) pred belongs to its cloud
def test_pred_is_the_argmax_of_its_own_cloud(net, clouds512, gpu512):
    (logits, _, _, _), pred = gpu512
    x = torch.from_numpy(clouds512)
    CC.check_pred_is_argmax(pred, logits, "512 clouds")
    p = net.predict(x)
    assert p.dtype == torch.int64 and torch.equal(p.cpu(), pred.long())
    perm = torch.from_numpy(np.random.default_rng(41).permutation(len(x)))
    for what, idx in (("rolled by 37", torch.roll(torch.arange(len(x)), 37)), ("seeded permutation", perm)):
        moved = torch.roll(x, 37, 0) if what.startswith("rolled") else x[idx]
        assert torch.equal(moved, x[idx])
        out = run_all(net, moved)
        CC.check_same_permutation(logits, pred, idx, out["logits"], out["pred"], what)
        CC.check_pred_is_argmax(out["pred"], out["logits"], what)
    print("512 clouds: classes predicted %d, excluded 0" % len(set(pred.tolist())))


# ---------------------------------------------------------------------------------------------------------------- (d) ties
def test_equal_logits_give_the_lowest_class(sd, ft, clouds512):
    import pointnet_oracle as PO
    x = torch.from_numpy(clouds512[:64])
    with make_net(PO.make_tied_weights(sd), ft) as tied:
        out = run_all(tied, x)
        p = tied.predict(x).cpu()
    CC.check_ties(out["logits"], out["pred"], "64 clouds, classes 20..39 twins of 0..19")
    assert torch.equal(p, out["pred"].long())
    print("ties: 64 clouds, classes predicted %d, all below 20" % len(set(p.tolist())))
    assert len(set(p.tolist())) >= 5                                           # the rule is exercised at more than one pair


# --------------------------------------------------------------------------------------------------- (e) batch-size edges
EDGE_SIZES = [1, 15, 16, 17, 31, 32, 33, 255, 256]


@pytest.fixture(scope="module")
def edge_case(net):
    """257 clouds at stride 320 (two point tiles, the second partly filled), ragged counts in [1, 320] with 1, 256, 257 and 320
    at the clouds that are also checked against the oracle.  -> (x, n_points, the B = 257 result)."""
    import bench
    n = np.random.default_rng(43).integers(1, 321, 257).astype(np.int32)
    n[[0, 15, 16, 255]] = [1, 256, 257, 320]
    x = ragged_batch(bench.synth_clouds(257, seed=27)[:, :320], n)
    return x, n, run_all(net, x, torch.from_numpy(n))


def test_batch_edges_reference_run(net, sd, edge_case):
    x, n, whole = edge_case
    assert all(torch.isfinite(v).all() for k, v in whole.items() if k != "pred")
    CC.check_pred_is_argmax(whole["pred"], whole["logits"], "B = 257")
    check_rows_against_f64(sd, whole, x.numpy(), n, [0, 15, 16, 255, 256], "B = 257, stride 320")
    print("B = 257: classes predicted %d" % len(set(whole["pred"].tolist())))
    assert len(set(whole["pred"].tolist())) >= CC.MIN_CLASSES


@pytest.mark.parametrize("B", EDGE_SIZES)
def test_batch_edges_equal_the_large_batch(net, edge_case, B):
    x, n, whole = edge_case
    part = run_all(net, x[:B], torch.from_numpy(n[:B]))
    assert_rows_equal(part, whole, slice(0, B), "B = %d" % B)
    last = run_all(net, x[257 - B:], torch.from_numpy(n[257 - B:]))            # the same clouds at other positions of the tiles
    assert_rows_equal(last, whole, slice(257 - B, 257), "last %d" % B)


# ------------------------------------------------------------------------------------------------------ (f) the chunk loop
def chunk_clouds(B, base):
    """B distinct 64-point clouds: cloud i is a 64-row slice of base[i % len(base)] moved by 1e-5 i; ragged counts in [1, 64]."""
    i = np.arange(B)
    start = 64 * ((i // len(base)) % (base.shape[1] // 64))
    x = base[i % len(base)][np.arange(B)[:, None], start[:, None] + np.arange(64)[None, :]] + (1e-5 * i).astype(np.float32)[:, None, None]
    n = np.random.default_rng(47).integers(1, 65, B).astype(np.int32)
    n[[0, B - 1]] = [64, 1]
    return np.ascontiguousarray(x, dtype=np.float32), n


def chunk_bounds(B):
    n_chunks = (B + CLS_CHUNK - 1) // CLS_CHUNK
    chunk = (B + n_chunks - 1) // n_chunks
    return [(c0, min(c0 + chunk, B)) for c0 in range(0, B, chunk)]


@pytest.mark.parametrize("B", [4097, 8193])
def test_chunked_batches(net, sd, clouds512, B):
    """B > 4096 runs as balanced chunks (4097: 2049 + 2048; 8193: 3 x 2731), every output offset by the chunk's first cloud."""
    assert chunk_bounds(4097) == [(0, 2049), (2049, 4097)] and chunk_bounds(8193) == [(0, 2731), (2731, 5462), (5462, 8193)]
    x_np, n = chunk_clouds(B, clouds512)
    x, nt = ragged_batch(x_np, n), torch.from_numpy(n)
    whole = run_all(net, x, nt)
    assert all(torch.isfinite(v).all() for k, v in whole.items() if k != "pred")
    step = 3000                                                                # unchunked pieces whose seams are not the chunks' seams
    for a in range(0, B, step):
        b = min(a + step, B)
        assert_rows_equal(run_all(net, x[a:b], nt[a:b]), whole, slice(a, b), "B = %d, clouds %d:%d" % (B, a, b))
    CC.check_pred_is_argmax(whole["pred"], whole["logits"], "B = %d" % B)
    assert torch.equal(net.predict(x, nt).cpu(), whole["pred"].long())
    ends = sorted({i for c0, c1 in chunk_bounds(B) for i in (c0, c1 - 1)})
    check_rows_against_f64(sd, whole, x_np, n, ends, "B = %d, ends of the chunks" % B)
    classes = len(set(whole["pred"].tolist()))
    print("B = %d: classes predicted %d" % (B, classes))
    assert classes >= CC.MIN_CLASSES
    assert len(np.unique(whole["logits"].numpy(), axis=0)) == B                # no two clouds share a row of logits


# ----------------------------------------------------------------------------------------------------- (g) stale workspace
def test_stale_workspace_rows_are_not_read(net, sd, ft, clouds512):
    """`part` holds a [1024] row per 256-point tile and is reused from call to call.  A first call fills all 16 tiles of 8 clouds
    with large maxima (coordinates x 50); the second call's clouds have 1 ... 4 tiles, and must not see the rest."""
    big = torch.from_numpy(clouds512[:32].reshape(8, 4096, 3) * 50.0)
    n = np.array([1, 255, 256, 257, 1024], np.int32)
    x_np = np.ascontiguousarray(clouds512[40:60].reshape(5, 4096, 3))
    x = ragged_batch(x_np, n)
    with make_net(sd, ft) as used:
        first = run_all(used, big)
        assert float(first["global_feat"].abs().max()) > 10 * float(run_all(used, torch.from_numpy(x_np))["global_feat"].abs().max())
        run_all(used, big)
        second = run_all(used, x, torch.from_numpy(n))
    with make_net(sd, ft) as fresh:
        want = run_all(fresh, x, torch.from_numpy(n))
    assert_rows_equal(second, want, slice(0, 5), "after a longer call")
    assert all(torch.isfinite(v).all() for k, v in second.items() if k != "pred")
    check_rows_against_f64(sd, second, x_np, n, [0, 1, 2, 3, 4], "stride 4096 after 8 x 4096 points x 50")


# ------------------------------------------------------------------------------------------------------------- (h) the CLI
def test_cli_under_a_varied_checkpoint(net, sd, ft, tmp_path, capsys):
    """Labels are the float64 oracle's predictions with a known set changed; the same clouds in reversed order under the SAME
    labels must print the other accuracy the oracle predicts: the number depends on which cloud gets which label."""
    import bench
    import pointnet_oracle as PO
    import ifdefense_amd as I
    from ifdefense_amd import inference as Inf
    wp = str(tmp_path / "pointnet.pth")
    torch.save(PO.reference_state_dict(sd), wp)
    x = bench.synth_clouds(70, seed=25)
    lo32, lo64 = CC.oracle_logits_pair(sd, x)
    e_32 = CC.e32_of(lo32, lo64)
    assert CC.top2_margin(lo64).min() >= CC.MARGIN_FACTOR * e_32              # the reference leaves no cloud in doubt (also on the CPU)
    want = lo64.argmax(1).numpy()
    with capsys.disabled():                                                    # what the CLI prints is compared whole below
        print("CLI: 70 clouds, e_32 %.3e, classes predicted %d, smallest margin %.0f e_32, excluded 0"
              % (e_32, len(set(want.tolist())), CC.top2_margin(lo64).min() / e_32))
    wrong, hit = np.arange(0, 70, 5), np.arange(1, 70, 2)[:21]                  # 14 labels changed, 21 targets hit
    label, target = want.copy(), (want + 3) % 40
    label[wrong] = (label[wrong] + 1) % 40
    target[hit] = want[hit]
    p = str(tmp_path / "kNN-pointnet-adv.npz")
    np.savez(p, test_pc=x, test_label=label.astype(np.uint8), target_label=target.astype(np.uint8))
    r = I.evaluate_npz(p, net, "target", 1024, False)
    assert r["n"] == 70 and np.array_equal(r["pred"], want)
    assert r["accuracy"] == 56 / 70 and r["success_rate"] == 21 / 70
    common = ["--data_root", p, "--model_path", wp, "--feature_transform", str(ft)]
    assert Inf.main(common) == 0
    assert capsys.readouterr().out == "Overall accuracy: 0.8000\n"
    assert Inf.main(common + ["--mode", "target", "--model", "pointnet"]) == 0
    assert capsys.readouterr().out == "Overall accuracy: 0.8000, attack success rate: 0.3000\n"
    # reversed clouds, labels as they were
    acc, suc = float((want[::-1] == label).sum()) / 70, float((want[::-1] == target).sum()) / 70
    assert "%.4f" % acc != "0.8000" and "%.4f" % suc != "0.3000"
    d = tmp_path / "reversed"
    d.mkdir()
    p = str(d / "kNN-pointnet-adv.npz")
    np.savez(p, test_pc=np.ascontiguousarray(x[::-1]), test_label=label.astype(np.uint8), target_label=target.astype(np.uint8))
    assert np.array_equal(I.evaluate_npz(p, net, "normal", 1024, False)["pred"], want[::-1])
    assert Inf.main(["--data_root", p, "--model_path", wp, "--feature_transform", str(ft), "--mode", "target"]) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % (acc, suc)
