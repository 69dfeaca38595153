"""GPU tests of the PointNet++ victim (include/ifd_pn2.h) against tests/pointnet2_oracle.py.

The two selection steps (farthest point sampling, ball query) are held to the header's definitions bit for bit: the numpy float32
oracle's tables must equal the GPU's.  The arithmetic is judged with the GPU's tables forced into the float32 and the float64
oracle, every bar relative to e_32 = max |float32 oracle - float64 oracle| of the tensor in question, computed here.
Section 1b runs the clouds on which rounding decides the selection (certified in test_pointnet2_cpu.py).

Measured on an MI355X (worst e_gpu / e_32 over test_arithmetic_against_f64's cases): DESIGN 7n."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IFD_ERR_ARG = -1
CHUNK = 128                                               # clouds per chunk of ifd_pn2_forward (include/ifd_pn2.h)
TABLES = ("fps1", "fps2", "ball1", "ball2")
TENSORS = ("l1_feat", "l2_feat", "global_feat")
SIZES = (1, 31, 33, 100, 511, 512, 513, 1024, 1536, 2048)


def make_net(sd):
    import ifdefense_amd as I
    return I.PointNet2Classifier(I.weights.pack_state_dict(sd, "pointnet2"), device="cuda:0")


@pytest.fixture(scope="module")
def sd():
    import pointnet2_oracle as PO
    return PO.make_weights(0)


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
    return np.ascontiguousarray(s[i % 24][:n] if n <= 1024 else big[i % 2][:n], dtype=np.float32)


def to_cpu(lo, aux):
    torch.cuda.synchronize()
    return lo.cpu(), {k: v.cpu() for k, v in aux.items()}


def run(net, clouds, fps_start=None, n_points=None):
    """-> logits [B,40], aux (everything on the CPU), for a list of clouds or a [B,N,3] array."""
    return to_cpu(*net.logits(clouds, n_points=n_points, fps_start=fps_start, want_aux=True))


def assert_tables(clouds, starts, aux, what):
    """The GPU's four tables of every cloud equal the numpy oracle's."""
    import pointnet2_oracle as PO
    for b, c in enumerate(clouds):
        PO.check_tables(c, {k: aux[k][b].numpy() for k in TABLES}, (0, 0) if starts is None else starts[b], "%s, cloud %d (n = %d)" % (what, b, len(c)))


# ---- 1. selection, bit for bit ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized(net, pool):
    """One cloud of every size of SIZES, each alone in its call (stride = its size), with starts in the middle: shared by the
    selection and the arithmetic test."""
    rng = np.random.default_rng(3)
    out = []
    for i, n in enumerate(SIZES):
        c = cloud(pool, i, n)
        st = np.array([[rng.integers(0, n), rng.integers(0, 512)]], np.int32)
        lo, aux = run(net, c[None], fps_start=st)
        out.append((c, st, lo, aux))
    return out


def test_selection_equals_the_oracle_at_every_size(sized):
    for c, st, lo, aux in sized:
        assert_tables([c], st, aux, "alone")
        assert aux["fps1"][0, 0] == st[0, 0] and aux["fps2"][0, 0] == st[0, 1]
        if len(c) == 1:
            assert not aux["fps1"].any() and not aux["ball1"].any()


@pytest.mark.parametrize("n", [100, 513, 2048])
def test_selection_under_several_starts(net, pool, n):
    c = cloud(pool, 5, n)
    starts = np.array([[0, 0], [n - 1, 511], [n // 2, 255], [n - 1, 0]], np.int32)
    lo, aux = run(net, np.stack([c] * 4), fps_start=starts)
    assert_tables([c] * 4, starts, aux, "starts")
    assert not torch.equal(aux["fps1"][0], aux["fps1"][1])


def test_selection_in_a_ragged_batch_with_nan_rows(net, pool):
    sizes = (1, 31, 100, 513, 700, 64)
    clouds = [cloud(pool, 7 + i, n) for i, n in enumerate(sizes)]
    pad = np.full((len(sizes), 777, 3), np.nan, np.float32)
    for b, c in enumerate(clouds):
        pad[b, :len(c)] = c
    starts = np.array([[0, 5], [30, 511], [99, 0], [512, 17], [3, 300], [63, 63]], np.int32)
    lo, aux = run(net, pad, fps_start=starts, n_points=np.array(sizes, np.int32))
    assert_tables(clouds, starts, aux, "ragged, NaN beyond the counts")
    assert bool(torch.isfinite(lo).all())
    lo_l, aux_l = run(net, clouds, fps_start=starts)                           # the same clouds as a list, zero padding
    assert torch.equal(lo, lo_l) and all(torch.equal(aux[k], aux_l[k]) for k in aux)


# ---- 1b. selection where rounding decides --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [0, 1, 2])
def test_lattice_family_equals_the_oracle(net, cls):
    """The clouds of pointnet2_oracle.LATTICE_FAMILY, on which test_pointnet2_cpu.py certifies that a contracted, a re-associated,
    a matrix-form or a doubly precise distance, and each tie or edge rule turned round, changes every table in every stride class:
    equal tables here mean the header's distance and rules, which bench.synth_clouds, the tie lattice and twins cannot tell.  The
    settings (alone, mid-cloud starts, a ragged NaN-padded batch, 300 points at strides 600 and 1100): check_family."""
    import pointnet2_oracle as PO

    def call(x, fps_start, n_points):
        lo, aux = run(net, x, fps_start=fps_start, n_points=n_points)
        assert bool(torch.isfinite(lo).all())
        return {k: aux[k].numpy() for k in TABLES}
    PO.check_family(cls, PO, call)


# ---- 2. ties of the sampling --------------------------------------------------------------------------------------------------
def lattice_fps(q, npoint, start):
    """FPS on integer coordinates in exact integer arithmetic: the lowest index of the largest running distance."""
    q = np.asarray(q, np.int64)
    running = np.full(len(q), np.iinfo(np.int64).max)
    out, far = [], start
    for _ in range(npoint):
        out.append(far)
        running = np.minimum(running, ((q - q[far]) ** 2).sum(1))
        far = int(np.flatnonzero(running == running.max())[0])
    return np.array(out)


def test_fps_ties_go_to_the_lowest_index(net):
    rng = np.random.default_rng(5)
    q = rng.integers(0, 6, size=(700, 3))                                      # a 6^3 lattice: 216 places for 700 points
    lattice = (q * 0.25).astype(np.float32)                                    # every distance is exact in f32
    half = rng.normal(0, 0.3, (150, 3)).astype(np.float32)
    twins = np.concatenate([half, half])                                       # point i + 150 is point i again
    inter = np.repeat(half, 2, axis=0)                                         # point 2 i + 1 is point 2 i again
    starts = np.array([[699, 0], [299, 3], [1, 2]], np.int32)
    lo, aux = run(net, [lattice, twins, inter], fps_start=starts)
    assert_tables([lattice, twins, inter], starts, aux, "ties")
    f1 = aux["fps1"][0].numpy()
    assert np.array_equal(f1, lattice_fps(q, 512, 699))
    assert np.array_equal(aux["fps2"][0].numpy(), lattice_fps(q[f1], 128, 0))
    t = aux["fps1"][1].numpy()
    assert t[0] == 299 and (t[1:150] < 150).all() and (t[150:] == 0).all()     # after the start only first copies, then exhausted
    t = aux["fps1"][2].numpy()
    assert t[0] == 1 and (t[1:150] % 2 == 0).all() and (t[150:] == 0).all()


# ---- 3. the ball's edge -------------------------------------------------------------------------------------------------------
def neighbours(v, k):
    """The 2 k + 1 floats around v."""
    out = [np.float32(v)]
    for _ in range(k):
        out = [np.nextafter(out[0], np.float32(-np.inf))] + out + [np.nextafter(out[-1], np.float32(np.inf))]
    return np.array(out, np.float32)


def edge_points(c, r, rng):
    """Two points beside c [3]: the oracle's float32 distance of the first to c is exactly r2, of the second the next float
    above r2.  Found by a search over the neighbouring floats of a point on the sphere."""
    import pointnet2_oracle as PO
    r2 = PO.radius2(r)
    above = np.nextafter(r2, np.float32(1))
    found = {}
    for _ in range(200):
        u = rng.normal(size=3)
        p = (c + r * u / np.linalg.norm(u)).astype(np.float32)
        X, Y = np.meshgrid(neighbours(p[0], 48), neighbours(p[1], 48))
        cand = np.stack([X.ravel(), Y.ravel(), np.full(X.size, p[2], np.float32)], 1)
        d = PO.dist(cand, c)
        for want in (r2, above):
            hit = np.flatnonzero(d == want)
            if want not in found and hit.size:
                found[want] = cand[hit[0]]
        if len(found) == 2:
            return found[r2], found[above]
    raise AssertionError("no points at the edge found")


def test_ball_edges(net):
    import pointnet2_oracle as PO
    rng = np.random.default_rng(8)
    c = np.array([0.125, -0.25, 0.3125], np.float32)
    in1, out1 = edge_points(c, 0.2, rng)
    in2, out2 = edge_points(c, 0.4, rng)
    assert PO.dist(in1[None], c)[0] == PO.radius2(0.2) and PO.dist(out2[None], c)[0] > PO.radius2(0.4)
    crowd = (c + rng.normal(0, 0.02, (50, 3))).astype(np.float32)              # 50 more members of c's ball: more than 32
    lone = np.array([[3.0, 3.0, 3.0]], np.float32)                             # nobody within 0.4
    far = (rng.uniform(-1, 1, (40, 3)) + np.array([0, 0, -2.5])).astype(np.float32)
    x = np.concatenate([c[None], in1[None], out1[None], in2[None], out2[None], crowd, lone, far]).astype(np.float32)
    lo, aux = run(net, [x], fps_start=np.zeros((1, 2), np.int32))
    assert_tables([x], None, aux, "edges")
    f1, f2 = aux["fps1"][0].numpy(), aux["fps2"][0].numpy()
    b1, b2 = aux["ball1"][0].numpy(), aux["ball2"][0].numpy()
    assert f1[0] == 0 and f2[0] == 0
    assert np.array_equal(b1[0], [0, 1] + list(range(5, 35)))                  # the first 32 members by index: 2, 3, 4 are outside
    pos = {p: int(np.flatnonzero(f1 == p)[0]) for p in (1, 2, 3, 4)}           # where the edge points sit among the 512
    row = set(b2[0].tolist())
    assert len(x) < 512 and pos[1] in row and pos[2] in row and pos[3] in row and pos[4] not in row
    lone_i = 5 + len(crowd)
    k1 = int(np.flatnonzero(f1 == lone_i)[0])
    assert (b1[k1] == lone_i).all()                                            # one member: it pads with itself
    k2 = int(np.flatnonzero(f2 == k1)[0])
    assert (b2[k2] == k1).all()


# ---- 4. arithmetic against float64, the GPU's tables forced -------------------------------------------------------------------
def check_arithmetic(sd, clouds, lo, aux, what):
    import pointnet2_oracle as PO
    t = {k: aux[k].numpy() for k in TABLES}
    r32 = PO.forward(PO.to_torch(sd), clouds, tables=t)
    r64 = PO.forward(PO.to_torch(sd, torch.float64), clouds, dtype=torch.float64, tables=t)
    bad, ratio = [], {}
    for name, got in [(k, aux[k]) for k in TENSORS] + [("logits", lo)]:
        e32 = float((r32[name].double() - r64[name]).abs().max())
        egpu = float((got.double() - r64[name]).abs().max())
        assert e32 > 0, (what, name)
        ratio[name] = egpu / e32
        if egpu > 4 * e32:
            bad.append((name, egpu, e32))
    print("%s: e_gpu / e_32: %s" % (what, ", ".join("%s %.2f" % kv for kv in ratio.items())))
    assert not bad, (what, bad)
    return ratio


def test_arithmetic_against_f64(sd, sized):
    worst = {}
    for c, st, lo, aux in sized:
        for k, v in check_arithmetic(sd, [c], lo, aux, "n = %d" % len(c)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("worst e_gpu / e_32: %s" % ", ".join("%s %.2f" % kv for kv in worst.items()))


def test_arithmetic_against_f64_ragged(net, sd, pool):
    clouds = [cloud(pool, 11 + i, n) for i, n in enumerate((20, 300, 65, 257))]
    lo, aux = run(net, clouds)
    assert_tables(clouds, None, aux, "ragged")
    check_arithmetic(sd, clouds, lo, aux, "ragged 20 / 300 / 65 / 257")


# ---- 5. predictions ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def varied():
    import bench
    import pointnet2_oracle as PO
    sd = PO.make_calibrated_weights(0)
    x = np.ascontiguousarray(bench.synth_clouds(256, seed=23)[:, :128])
    with make_net(sd) as c:
        lo, aux = run(c, x)
    return sd, x, lo, aux


def test_predictions_against_f64(varied):
    import cls_checks
    import pointnet2_oracle as PO
    sd, x, lo, aux = varied
    t = {k: aux[k].numpy() for k in TABLES}
    lo32 = PO.forward(PO.to_torch(sd), x, tables=t)["logits"]
    lo64 = PO.forward(PO.to_torch(sd, torch.float64), x, dtype=torch.float64, tables=t)["logits"]
    e_32 = cls_checks.e32_of(lo32, lo64)
    assert e_32 > 0
    e_gpu = float((lo.double() - lo64).abs().max())
    print("calibrated head: e_gpu %.3e, e_32 %.3e, ratio %.2f" % (e_gpu, e_32, e_gpu / e_32))
    assert e_gpu <= 4 * e_32
    cls_checks.check_pred_against_f64(aux["pred"].numpy(), lo64, e_32, "pointnet2, calibrated head, 256 x 128 points")
    for b in (0, 100, 255):
        PO.check_tables(x[b], {k: t[k][b] for k in TABLES}, (0, 0), "calibrated, cloud %d" % b)


def test_pred_is_the_argmax_of_its_own_logits(varied):
    import cls_checks
    import pointnet2_oracle as PO
    sd, x, lo, aux = varied
    cls_checks.check_pred_is_argmax(aux["pred"].numpy(), lo, "calibrated head")
    with make_net(PO.make_tied_weights(sd)) as c:
        lo_t, aux_t = run(c, x[:64])
    cls_checks.check_ties(lo_t, aux_t["pred"].numpy(), "tied head")
    assert torch.equal(lo_t[:, :20], lo[:64, :20])


# ---- 6. bitwise independence -------------------------------------------------------------------------------------------------
def same_cloud(a_lo, a_aux, ia, b_lo, b_aux, ib):
    assert torch.equal(a_lo[ia], b_lo[ib])
    for k in a_aux:
        assert torch.equal(a_aux[k][ia], b_aux[k][ib]), k


def test_a_cloud_does_not_depend_on_its_batch(net, pool):
    rng = np.random.default_rng(12)
    B = CHUNK + 1
    x = np.stack([cloud(pool, i, 200) + np.float32(0.001 * i) for i in range(B)])
    starts = np.stack([rng.integers(0, 200, B), rng.integers(0, 512, B)], 1).astype(np.int32)
    lo_all, aux_all = run(net, x, fps_start=starts)                            # 129 clouds: chunks of 65 and 64
    for n in (1, 2, CHUNK):                                                    # ... one chunk of 1, of 2, of exactly 128
        lo, aux = run(net, x[:n], fps_start=starts[:n])
        for b in (range(n) if n <= 2 else (0, 64, 65, CHUNK - 1)):
            same_cloud(lo, aux, b, lo_all, aux_all, b)
    lo_r, aux_r = run(net, np.roll(x[:17], 5, axis=0), fps_start=np.roll(starts[:17], 5, axis=0))
    for b in range(17):
        same_cloud(lo_r, aux_r, (b + 5) % 17, lo_all, aux_all, b)
    # a larger stride, NaN beyond n_points
    pad = np.full((17, 333, 3), np.nan, np.float32)
    pad[:, :200] = x[:17]
    lo_p, aux_p = run(net, pad, fps_start=starts[:17], n_points=np.full(17, 200, np.int32))
    for b in range(17):
        same_cloud(lo_p, aux_p, b, lo_all, aux_all, b)
    # ... and one that changes the sampling kernel's points per thread (above 512 and above 1024 rows)
    for stride in (600, 1100):
        pad = np.zeros((3, stride, 3), np.float32)
        pad[:, :200] = x[:3]
        lo_p, aux_p = run(net, pad, fps_start=starts[:3], n_points=np.full(3, 200, np.int32))
        for b in range(3):
            same_cloud(lo_p, aux_p, b, lo_all, aux_all, b)


def test_stale_workspace(net, pool):
    clouds = [cloud(pool, b, n) for b, n in enumerate((40, 64, 20, 1, 300))]
    lo, aux = run(net, clouds)
    run(net, np.stack([cloud(pool, i, 2048) for i in range(40)]))              # a larger call in between
    for b, c in enumerate(clouds):                                             # ... then every cloud alone
        lo1, aux1 = run(net, [c])
        same_cloud(lo1, aux1, 0, lo, aux, b)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------
def test_runtime_refusals_leave_the_context_usable(net, pool):
    import ifdefense_amd as I
    x = np.stack([cloud(pool, 0, 64), cloud(pool, 1, 64)])
    want = net.logits(x).cpu()
    ok = [[0, 0], [63, 511]]
    for bad_x, counts, starts, words in ((x, [64, 0], None, "n_points outside"), (x, [65, 64], None, "n_points outside"),
                                         (np.zeros((1, 2049, 3), np.float32), None, None, "stride above 2048"),
                                         (x, None, [[0, 0], [64, 0]], "fps_start outside"), (x, [64, 10], [[0, 0], [10, 0]], "fps_start outside"),
                                         (x, None, [[0, 0], [0, 512]], "fps_start outside"), (x, None, [[-1, 0], [0, 0]], "fps_start outside")):
        with pytest.raises(I.IfdError, match="libifd error %d: .*%s" % (IFD_ERR_ARG, words)):
            net.logits(bad_x, n_points=counts, fps_start=starts)
        assert torch.equal(net.logits(x).cpu(), want)
    assert torch.equal(net.logits(x, fps_start=[[0, 0], [0, 0]]).cpu(), want)  # NULL starts mean 0, 0
    assert bool(torch.isfinite(net.logits(x, fps_start=ok)).all())             # the last valid starts are taken


# ---- 8. the CLI --------------------------------------------------------------------------------------------------------------
def test_cli_end_to_end(varied, tmp_path, capsys):
    import pointnet2_oracle as PO
    from ifdefense_amd import pointnet2_inference as Inf
    sd, x, lo, aux = varied
    wpath = str(tmp_path / "pointnet2.npz")
    np.savez(wpath, **sd)
    n = 48
    starts = Inf.fps_starts(1, [128] * n)
    t = PO.tables_of(x[:n], fps_start=starts)
    pred = PO.forward(PO.to_torch(sd, torch.float64), x[:n], dtype=torch.float64, tables=t)["logits"].argmax(1).numpy()
    with make_net(sd) as c:
        assert np.array_equal(c.predict(x[:n], fps_start=starts).cpu().numpy(), pred)     # margins of 8 e_32 and more: test_predictions_against_f64
    label = pred.copy()
    label[::4] = (label[::4] + 1) % 40
    target = (pred + (np.arange(n) % 3 == 0)) % 40
    same = str(tmp_path / "kNN-pointnet2-same.npz")
    np.savez(same, test_pc=x[:n], test_label=label, target_label=target)
    assert Inf.main(["--data_root", same, "--mode", "target", "--model_path", wpath, "--num_points", "128"]) == 0
    out = capsys.readouterr().out
    assert out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % ((pred == label).mean(), (pred == target).mean())
    sizes = [128, 100, 64, 1, 77, 128]
    rag = np.empty(len(sizes), dtype=object)
    for i, m in enumerate(sizes):
        rag[i] = x[100 + i, :m]
    st = Inf.fps_starts(7, sizes)
    with make_net(sd) as c:
        pr = c.predict([rag[i] for i in range(len(sizes))], fps_start=st).cpu().numpy()
    lab = pr.copy()
    lab[1] = (lab[1] + 3) % 40
    ragged = str(tmp_path / "sor-ragged.npz")
    np.savez(ragged, test_pc=rag, test_label=lab)
    assert Inf.main(["--data_root", ragged, "--model", "pointnet2", "--model_path", wpath, "--fps_seed", "7"]) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f\n" % (5 / 6)
