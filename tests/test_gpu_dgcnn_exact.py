"""GPU tests that hold the DGCNN victim's neighbour choice to include/ifd_dgcnn.h bit for bit.

Every check takes the GPU's own layer inputs (the cloud for layer 1, the columns of aux["feat"] for layers 2 to 4) and requires
aux["idx"][l], sorted, to EQUAL dgcnn_oracle.header_neighbours of them: the header's fused chains in float32 (fma32), the k
largest scores, the lowest index among equal ones.  Sizes from 20 to 2048 points, k from 1 to 32, row orders that keep the
kernel's candidate queues full and stale (certified on the CPU by tests/test_dgcnn_cpu.py from dgcnn_oracle.wave_trace), and
clouds whose scores tie.  Measured figures: DESIGN 7m."""
import numpy as np
import pytest
import torch

import test_gpu_dgcnn as T

pytestmark = pytest.mark.gpu

RAGGED_SIZES = (20, 21, 63, 64, 65, 127, 128, 129, 257, 513)
LARGE_SIZES = (1024, 1025, 1536, 2048)
KS = (1, 2, 3, 4, 5, 8, 9, 31, 32)


@pytest.fixture(scope="module")
def sd():
    import dgcnn_oracle as DO
    return DO.make_weights(0)


@pytest.fixture(scope="module")
def net(sd):
    with T.make_net(sd) as c:
        yield c


@pytest.fixture(scope="module")
def pool():
    import bench
    s = bench.synth_clouds(24, seed=77)
    big = [np.concatenate([s[20], 0.8 * s[21] + 0.1]), np.concatenate([s[22], 0.7 * s[23] - 0.2])]
    return s, [np.ascontiguousarray(b, dtype=np.float32) for b in big]


def check_layers(c, aux, b, k, what, rows=None):
    """All four layers of cloud b against the header; -> (tied rows of each layer, the scores of each layer for ``rows``)."""
    import dgcnn_oracle as DO
    ties, scores = [], []
    for l in range(4):
        x = np.asarray(T.layer_input(c, aux["feat"][b], l), dtype=np.float32)
        idx = aux["idx"][l][b, :len(c)].numpy()
        S = DO.header_scores(x, rows)
        ties.append(DO.check_neighbours_exact(x, idx if rows is None else idx[rows], k, rows, "%s, layer %d" % (what, l + 1), scores=S))
        scores.append(S)
    print("%s: rows tied at the k-th place, layers 1 .. 4: %s" % (what, ties))
    return ties, scores


# ---- a. sizes ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(net, pool):
    clouds = [T.cloud(pool, i, n) for i, n in enumerate(RAGGED_SIZES)]
    lo, aux = T.run(net, clouds)
    return clouds, lo, aux


@pytest.fixture(scope="module")
def ragged_tight(net, pool):
    """The same sizes, every cloud 1/16 the size and far from the origin (dgcnn_oracle.tight_cloud): near-ties in every row."""
    import dgcnn_oracle as DO
    clouds = [DO.tight_cloud(T.cloud(pool, i + 1, n)) for i, n in enumerate(RAGGED_SIZES)]
    lo, aux = T.run(net, clouds)
    return clouds, lo, aux


@pytest.mark.parametrize("which", ["natural", "tight"])
def test_every_row_of_a_ragged_batch(request, which):
    clouds, _, aux = request.getfixturevalue("ragged" if which == "natural" else "ragged_tight")
    for b, c in enumerate(clouds):
        check_layers(c, aux, b, 20, "n = %d, %s" % (len(c), which))
        if len(c) == 20:
            for l in range(4):
                assert np.array_equal(np.sort(aux["idx"][l][b, :20].numpy(), axis=1), np.tile(np.arange(20), (20, 1)))


@pytest.mark.parametrize("which", ["natural", "tight"])
def test_ragged_batch_again_at_stride_2048_with_nan_padding(request, net, which):
    clouds, lo, aux = request.getfixturevalue("ragged" if which == "natural" else "ragged_tight")
    pad = np.full((len(clouds), 2048, 3), np.nan, np.float32)
    for b, c in enumerate(clouds):
        pad[b, :len(c)] = c
    lo_p, aux_p = net.logits(pad, n_points=np.array([len(c) for c in clouds], np.int32), want_aux=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lo_p).all()) and torch.equal(lo_p.cpu(), lo)
    assert torch.equal(aux_p["global_feat"].cpu(), aux["global_feat"]) and torch.equal(aux_p["pred"].cpu(), aux["pred"])
    feat_p, idx_p = aux_p["feat"].cpu(), [t.cpu() for t in aux_p["idx"]]
    for b, c in enumerate(clouds):
        n = len(c)
        assert torch.equal(feat_p[b, :n], aux["feat"][b, :n]), n
        for l in range(4):
            assert torch.equal(idx_p[l][b, :n], aux["idx"][l][b, :n]), (n, l)


def large_rows(n):
    """The first 32 rows, the last 32 and 32 seeded random ones."""
    rng = np.random.default_rng(n)
    return np.concatenate([np.arange(32), np.arange(n - 32, n), np.sort(rng.choice(np.arange(32, n - 32), 32, replace=False))])


@pytest.mark.parametrize("which", ["natural", "tight"])
@pytest.mark.parametrize("n", LARGE_SIZES)
def test_first_last_and_random_rows_of_a_large_cloud(net, pool, n, which):
    import dgcnn_oracle as DO
    c = T.cloud(pool, 5, n)
    c = c if which == "natural" else DO.tight_cloud(c)
    _, aux = T.run(net, [c])
    check_layers(c, aux, 0, 20, "n = %d, %s, 96 rows" % (n, which), large_rows(n))


# ---- b. k --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_k(sd, pool, k):
    import dgcnn_oracle as DO
    clouds = [T.cloud(pool, 9, 65), T.cloud(pool, 10, k), DO.tight_cloud(T.cloud(pool, 9, 65))]
    clouds += [T.cloud(pool, 12, 33), DO.tight_cloud(T.cloud(pool, 12, 33))] if k == 32 else []
    with T.make_net(sd, k) as net:
        lo, aux = T.run(net, clouds)
        one = T.run(net, [clouds[1]]) if k == 1 else None
    for b, c in enumerate(clouds):
        check_layers(c, aux, b, k, "k = %d, n = %d%s" % (k, len(c), ", tight" if b in (2, 4) else ""))
    for l in range(4):                                                   # a cloud of exactly k points: every index in every row
        assert np.array_equal(np.sort(aux["idx"][l][1, :k].numpy(), axis=1), np.tile(np.arange(k), (k, 1))), l
    assert bool(torch.isfinite(lo).all())
    if k == 1:                                                           # the one-point cloud: its own neighbour, and the arithmetic bar
        lo1, aux1 = one
        assert all(int(aux1["idx"][l][0, 0, 0]) == 0 for l in range(4))
        r32, r64 = T.forced_pair(sd, [clouds[1]], aux1["idx"], k=1)
        e32 = float((r32["logits"].double() - r64["logits"]).abs().max())
        egpu = float((lo1.double() - r64["logits"]).abs().max())
        print("one point, k = 1: e_gpu %.3e, e_32 %.3e" % (egpu, e32))
        assert bool(torch.isfinite(lo1).all()) and e32 > 0 and egpu <= 4 * e32
        assert torch.equal(lo1[0], lo[1])


# ---- c. row orders that work the queues --------------------------------------------------------------------------------------
_stress_runs = {}


def stress_run(sd, name, reverse=False):
    import dgcnn_oracle as DO
    key = (name, reverse)
    if key not in _stress_runs:
        c, k = DO.stress_cloud(name)
        c = np.ascontiguousarray(c[::-1]) if reverse else c
        with T.make_net(sd, k) as net:
            _, aux = T.run(net, [c])
        ties, scores = check_layers(c, aux, 0, k, name + (", reversed" if reverse else ""))
        _stress_runs[key] = (c, k, aux, ties, scores)
    return _stress_runs[key]


STRESS_NAMES = ("approach, k = 20", "runs of 8, k = 1", "runs of 8, k = 5", "runs of 32, k = 20", "approach, k = 32", "runs of 48, k = 32")


@pytest.mark.parametrize("name", STRESS_NAMES)
def test_orders_that_keep_the_queues_busy(sd, name):
    import dgcnn_oracle as DO
    assert set(STRESS_NAMES) == set(DO.STRESS)
    c, k, aux, ties, scores = stress_run(sd, name)
    _, _, counter, floor = DO.STRESS[name]
    for l in range(4):
        tr = DO.wave_trace(scores[l][DO.STRESS_GROUP], k)
        print("%s, layer %d, queries 448 .. 511: queued %d .. %d (%.2f of n - k at least), stale %d .. %d, %d flushes"
              % (name, l + 1, tr["queued"].min(), tr["queued"].max(), tr["queued"].min() / (len(c) - k), tr["stale"].min(),
                 tr["stale"].max(), tr["flushes"]))
        if l == 0:                                                       # the input is the one the CPU test certified
            assert (tr[counter] >= floor).all(), (name, counter, int(tr[counter].min()), floor)


def test_receding_order_gives_the_mirrored_sets(sd):
    import dgcnn_oracle as DO
    name = "approach, k = 20"
    c, k, aux, _, scores = stress_run(sd, name)
    r, _, aux_r, _, scores_r = stress_run(sd, name, reverse=True)
    n = len(c)
    mirrored = 0
    for l in range(4):
        x, xr = T.layer_input(c, aux["feat"][0], l), T.layer_input(r, aux_r["feat"][0], l)
        same_input = np.array_equal(np.asarray(x)[::-1], np.asarray(xr))
        assert same_input or l > 0
        print("receding order, layer %d: the input is the approaching one's, mirrored: %s" % (l + 1, same_input))
        if not same_input:                                               # a tie upstream was broken the other way: nothing to compare
            continue
        free = ~(DO.tied_rows(x, k, scores=scores[l]) | DO.tied_rows(xr, k, scores=scores_r[l])[::-1])
        a = np.sort(aux["idx"][l][0, :n].numpy().astype(np.int64), axis=1)
        b = np.sort(n - 1 - aux_r["idx"][l][0, :n].numpy().astype(np.int64), axis=1)[::-1]
        assert np.array_equal(a[free], b[free]), (l, np.nonzero((a != b).any(1) & free)[0][:10])
        mirrored += int(free.sum())
    assert mirrored >= n - 64


# ---- d. equal scores ---------------------------------------------------------------------------------------------------------
def test_equal_scores_off_the_lattice(net):
    import dgcnn_oracle as DO
    p, q = np.array([0.3, -0.2, 0.5], np.float32), np.array([-0.4, 0.1, 0.25], np.float32)
    copies = np.tile(p, (100, 1))
    inter = np.tile(np.stack([p, q]), (50, 1))
    moved = DO.translated_cloud()
    clouds = [copies, inter, moved]
    _, aux = T.run(net, clouds)
    ties = [check_layers(c, aux, b, 20, what)[0] for b, (c, what) in enumerate(zip(clouds, ("100 copies", "two points, 50 and 50",
                                                                                            "cloud moved by (+8, -8, +8)")))]
    first = np.arange(20)
    for l in range(4):
        assert np.array_equal(np.sort(aux["idx"][l][0, :100].numpy(), axis=1), np.tile(first, (100, 1))), l
        got = np.sort(aux["idx"][l][1, :100].numpy(), axis=1)
        assert np.array_equal(got[0::2], np.tile(2 * first, (50, 1))) and np.array_equal(got[1::2], np.tile(2 * first + 1, (50, 1))), l
    assert ties[0] == [100] * 4 and ties[1] == [100] * 4
    assert sum(ties[2]) >= 1 and ties[2][0] >= 1                        # the lowest-index rule, seen at work on natural data
