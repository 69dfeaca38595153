"""GPU checks of the input gradient (include/ifd_atk.h) and of CW Add (include/ifd_add.h) above 1024 points, up to the 10000 rows
the ABI accepts: more than 4 point tiles for tile_max_win_kernel to choose between, up to 40 rows a thread in
stack_backward_kernel's ranking, a stride of 10000 with ragged counts.  The inputs are tests/atk_large_inputs.py's, which
tests/test_atk_large_cpu.py holds to atk_oracle.case_conditions on the CPU.  The bars are test_gpu_atk's (4 e_32 on the judged
rows, winners within 8 e_act of the float64 maximum, rows beyond a cloud exactly zero) and test_gpu_add's; everything else here is
bitwise, and two of the bitwise tests pin the winners of the high tiles without a tolerance: a cloud equals its own winner rows,
and repeated copies of a cloud leave everything in the first copy."""
import warnings

import numpy as np
import pytest
import torch

import add_oracle as DO
import atk_large_inputs as LI
import atk_oracle as AO
import pointnet_oracle as PO
from test_gpu_add import bits, dev
from test_gpu_atk import compare_case, gpu_grad
from test_gpu_cls import check_against_f64, gpu_outputs, oracle_pair

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def W64(sd):
    return PO.to_torch(sd, torch.float64)


def make_net(sd, ft=False):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    return I.Classifier(weights.pack_state_dict(sd, "pointnet"), feature_transform=ft, device="cuda:0")


@pytest.fixture(scope="module")
def net(sd):
    with make_net(sd) as c:
        yield c


# ---------------------------------------------------------------------------------------------- a. parity
@pytest.mark.parametrize("n,B", LI.LARGE_CASES)
def test_gradient_parity(net, sd, W64, n, B):
    cl, tg = LI.inputs(sd, (n, B))
    compare_case(net, sd, W64, cl, tg, "N=%d B=%d" % (n, B))


@pytest.mark.parametrize("n,B", LI.CE_CASES)
def test_gradient_parity_cross_entropy(net, sd, W64, n, B):
    cl, tg = LI.inputs(sd, (n, B))
    compare_case(net, sd, W64, cl, tg, "CE N=%d B=%d" % (n, B), loss="cross_entropy")


def test_gradient_parity_ragged_at_stride_10000(net, sd, W64):
    cl, tg = LI.inputs(sd, "ragged")
    compare_case(net, sd, W64, cl, tg, "ragged stride 10000", stride=LI.RAGGED_STRIDE)


# ---------------------------------------------------------------------------------------------- b. the forward at the limit
@pytest.mark.parametrize("ft", [False, True], ids=["plain", "feature_transform"])
@pytest.mark.parametrize("n", [4097, 9999, 10000])
def test_forward_at_the_limit(ft, n):
    w = PO.make_calibrated_weights(0, ft)
    x = np.stack([c[:n] for c in LI.cached(("big", 3), lambda: LI.big_clouds(3, 10000))])
    r32, r64 = oracle_pair(w, x)
    with make_net(w, ft) as c:
        got, _ = gpu_outputs(c, torch.from_numpy(x))
    check_against_f64(got, r32, r64, "%d points%s" % (n, ", feature_transform" if ft else ""))


def test_forward_outputs_are_the_classifiers_bits_at_10000_rows(net, sd):
    cl, tg = LI.inputs(sd, (10000, 4))
    x = torch.from_numpy(np.stack(cl))
    lo, a = net.logits(x, want_aux=True)
    _, b = gpu_grad(net, x, tg)
    assert np.array_equal(bits(lo), bits(b["logits"])) and np.array_equal(a["pred"].cpu().numpy(), b["pred"])
    assert np.array_equal(bits(a["global_feat"]), bits(b["global_feat"]))


# ---------------------------------------------------------------------------------------------- c. a cloud = its winner rows
@pytest.mark.parametrize("loss", ["logits", "cross_entropy"])
@pytest.mark.parametrize("n", [10000, 2561])
def test_a_cloud_equals_its_own_winner_rows_bit_for_bit(net, sd, n, loss):
    """U = the sorted union of the reported winners of both max-pools.  The maxima are exact, stack_backward_kernel visits the
    winner points in ascending order and sums a point's channels in ascending order: the cloud x[U] alone has the bits of x."""
    cl, tg = LI.inputs(sd, "ragged")
    i = LI.RAGGED_COUNTS.index(n)
    x, t = cl[i][None], tg[i:i + 1]
    g, a = gpu_grad(net, x, t, loss=loss)
    U = np.union1d(a["win_feat"][0], a["win_stn"][0])
    gs, s = gpu_grad(net, np.ascontiguousarray(x[:, U]), t, loss=loss)
    print("%d rows, %s: |U| = %d, highest winner row %d" % (n, loss, len(U), U[-1]))
    assert np.abs(g).max() > 0 and U[0] >= 0 and U[-1] < n
    if n == 10000:
        assert U[-1] > 1024
    for k in ("logits", "loss", "global_feat", "pred"):
        assert np.array_equal(bits(s[k]), bits(a[k])), k
    assert np.array_equal(s["win_feat"][0], np.searchsorted(U, a["win_feat"][0])) and np.array_equal(s["win_stn"][0], np.searchsorted(U, a["win_stn"][0]))
    assert np.array_equal(bits(gs[0]), bits(g[0, U]))
    assert not np.delete(g[0], U, 0).any()


# ---------------------------------------------------------------------------------------------- d. ties across waves and tiles
@pytest.mark.parametrize("base,n", [(300, 2500), (257, 10000)])
def test_repeated_copies_leave_everything_in_the_first(net, sd, base, n):
    """Copies of the base cloud start at rows base, 2 base, ... across wave (64 rows) and tile (256 rows) boundaries, and every
    channel's maximum is held by one row of every copy: the lowest wins."""
    x, t, tiled = LI.tiled_cloud(sd, base, n)
    g0, a0 = gpu_grad(net, x[None], [t])
    g, a = gpu_grad(net, tiled[None], [t])
    assert np.abs(g0).max() > 0
    assert a["win_feat"].max() < base and a["win_stn"].max() < base
    for k in ("win_feat", "win_stn", "logits", "loss", "global_feat"):
        assert np.array_equal(bits(a[k]), bits(a0[k])), k
    assert np.array_equal(bits(g[0, :base]), bits(g0[0])) and not g[0, base:].any()


# ---------------------------------------------------------------------------------------------- e. batching at size
def test_batching_is_bitwise_at_10000_rows(net, sd):
    cl, tg = LI.inputs(sd, (10000, 4))
    x = np.stack(cl)
    g, a = gpu_grad(net, x, tg)
    assert np.abs(g).max() > 0
    g1, a1 = gpu_grad(net, x[2:3], tg[2:3])
    p = np.array([3, 1, 0, 2])
    gp, ap = gpu_grad(net, x[p], tg[p])
    for k in ("win_feat", "win_stn", "loss", "logits"):
        assert np.array_equal(bits(a1[k][0]), bits(a[k][2])) and np.array_equal(bits(ap[k]), bits(a[k][p])), k
    assert np.array_equal(bits(g1[0]), bits(g[2])) and np.array_equal(bits(gp), bits(g[p]))


def test_a_short_cloud_of_the_ragged_call_equals_itself_alone(net, sd):
    cl, tg = LI.inputs(sd, "ragged")
    pad, counts = LI.padded(cl, LI.RAGGED_STRIDE)
    g, a = gpu_grad(net, pad, tg, n_points=counts)
    i = LI.RAGGED_COUNTS.index(257)
    g1, a1 = gpu_grad(net, cl[i][None], tg[i:i + 1])
    assert np.abs(g1).max() > 0 and np.array_equal(bits(g[i, :257]), bits(g1[0])) and not g[i, 257:].any()
    for k in ("win_feat", "win_stn", "loss", "logits", "global_feat"):
        assert np.array_equal(bits(a[k][i]), bits(a1[k][0])), k


def test_stale_workspace_of_a_10000_row_call_is_not_read(net, sd):
    cl, tg = LI.inputs(sd, (10000, 4))
    x = np.stack(cl)
    gpu_grad(net, x * np.float32(50.0), tg)                            # leaves 40 tiles of larger maxima and their winners behind
    small = np.ascontiguousarray(x[:, :1100])
    got, a = gpu_grad(net, small, tg)
    with make_net(sd) as fresh:
        want, b = gpu_grad(fresh, small, tg)
    assert np.abs(want).max() > 0 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(a["win_feat"], b["win_feat"]) and np.array_equal(a["win_stn"], b["win_stn"])


# ---------------------------------------------------------------------------------------------- f. CW Add at its real shape
def test_critical_points_is_select_on_input_grads_own_output_at_size(net, sd):
    cat, tg, ori = LI.cached(("add", "full"), lambda: LI.add_case(sd))
    B, A = len(ori), LI.ADD_NUM
    x, n_ori = LI.padded(ori, 1024)
    grad = net.input_grad(x, tg, "cross_entropy", 0., 1.0 / B, n_points=n_ori)
    a = net.add_select(grad, x, A, n_points=n_ori, want_idx=True)
    b = net.add_critical_points(x, tg, A, 1.0 / B, n_points=n_ori, want_idx=True)
    assert torch.equal(a[1], b[1]) and np.array_equal(bits(a[0]), bits(b[0]))
    idx = a[1].cpu().numpy()
    for i in range(B):
        assert len(set(idx[i].tolist())) == A and idx[i].min() >= 0 and idx[i].max() < n_ori[i]
        assert np.array_equal(bits(a[0][i]), bits(ori[i][idx[i]]))


@pytest.mark.parametrize("kind", DO.KINDS)
def test_add_loop_teacher_forced_through_the_network_at_size(net, sd, W64, kind):
    """test_gpu_add.test_loop_teacher_forced_through_the_network at 8 ragged clouds of up to 1024 + 512 rows in a stride of 1600 with
    NaN beyond, 2 iterations: the added rows against the oracle's ONE step from the GPU's previous state and the GPU's own gradient
    (4 x the float32 oracle's error outside add_oracle.exclusions, at most 5 % of the rows excluded), and the gradient of the
    concatenated cloud at that state by the row-wise rule under atk_oracle.case_conditions."""
    clouds, tg, ori = LI.cached(("add", "full"), lambda: LI.add_case(sd))
    B, A, lr = len(ori), LI.ADD_NUM, 1e-2
    start, counts = LI.padded(clouds, LI.ADD_STRIDE)
    n_ori = np.array(LI.ADD_N_ORI, np.int32)
    cat = dev(start)
    weight = 5e3 if kind == "chamfer" else 2e2
    st = net.cw_state(B, A, weight, 4e4)
    done = 0
    for k in (1, 2):
        prev, m, v = cat.cpu().numpy(), st["m"].cpu().numpy(), st["v"].cpu().numpy()
        grad, aux = net.input_grad(cat, tg, scale=1.0 / B, n_points=counts, want_aux=True)
        g, aux = grad.cpu().numpy(), {a: b.cpu().numpy() for a, b in aux.items()}
        net.add_step(kind, st, grad, aux["pred"], tg, cat, A, k, lr, 1.0 / B, loss=aux["loss"], n_ori=n_ori)
        new = cat.cpu().numpy()
        e_gpu = e_32 = e_min = 0.0
        steps = []
        for i in range(B):
            n = int(n_ori[i])
            # original rows and rows beyond the cloud: untouched, bit for bit
            assert np.array_equal(bits(new[i, :n]), bits(start[i, :n])) and np.array_equal(bits(new[i, n + A:]), bits(start[i, n + A:]))
            a = (kind, g[i, n:n + A], int(aux["pred"][i]), int(tg[i]), prev[i, n:n + A], ori[i], weight, m[i], v[i], k, lr, 1.0 / B, DO.fresh_record(A))
            steps.append((DO.step(*a), DO.step(*a, dtype=torch.float32)))
            e_min = max(e_min, float(np.abs(steps[-1][1][6]["min_p"].astype(np.float64) - steps[-1][0][6]["min_p"]).max()))
        n_out = 0
        for i, (s64, s32) in enumerate(steps):
            n = int(n_ori[i])
            rows_out, cloud_out = DO.exclusions(prev[i, n:n + A], ori[i], e_min, kind)
            assert not cloud_out
            n_out += int(rows_out.sum())
            e_gpu = max(e_gpu, np.abs(new[i, n:n + A] - s64[0])[~rows_out].max())
            e_32 = max(e_32, np.abs(s32[0] - s64[0])[~rows_out].max())
        assert n_out <= 0.05 * B * A
        print("%s iteration %d: adv |GPU - f64| %.3e = %.2f e_32, %d rows excluded" % (kind, k, e_gpu, e_gpu / e_32, n_out))
        assert e_32 > 0 and e_gpu <= 4 * e_32, (k, e_gpu, e_32)
        live = [prev[i, :counts[i]] for i in range(B)]
        r32, r64, e, e32, ex = AO.run_case(sd, live, tg, scale=1.0 / B)
        whole, judged, rows = AO.case_conditions(r64, e)
        ratios = []
        for i in range(B):
            AO.winners_valid(aux["win_feat"][i], r64[i]["pre"]["c3"], e["c3"], "iteration %d cloud %d trunk" % (k, i))
            AO.winners_valid(aux["win_stn"][i], np.maximum(r64[i]["pre"]["stn3"], 0), e["stn3"], "iteration %d cloud %d stn" % (k, i))
            why, rows_out = AO.row_exclusion(r64[i], e)
            if why:
                continue
            f = AO.run_cloud(W64, live[i], tg[i], scale=1.0 / B, force_feat=aux["win_feat"][i], force_stn=aux["win_stn"][i])
            ratios.append(AO.check_grad(g[i], f["grad"], e32, "iteration %d cloud %d" % (k, i), rows_out))
            done += 1
        print("%s iteration %d: gradient of the concatenated clouds: e_32 %.3e, clouds wholly out %d/%d, rows judged %d/%d, GPU/e_32 max %.2f"
              % (kind, k, e32, whole, B, judged, rows, max(ratios)))
    assert done >= 0.9 * 2 * B


# ---------------------------------------------------------------------------------------------- g. fused = host-driven at size
def test_fused_and_host_driven_ifgm_give_the_same_bits_at_3000_rows(net, sd):
    cl, tg = LI.inputs(sd, (3072, 8))
    x = np.stack([c[:3000] for c in cl[:2]])
    t = torch.as_tensor(tg[:2])
    budget, iters = 0.08 * np.sqrt(3000 * 3), 2
    out, ok = net.fgm_attack("ifgm", x, t, budget, budget / iters, iters, scale=0.5)
    ori = dev(x)
    cur = ori.clone()
    for _ in range(iters):
        cur = net.fgm_update("ifgm", net.input_grad(cur, t, scale=0.5), cur, ori, None, budget / iters, budget)
    assert np.array_equal(bits(out), bits(cur)) and not np.array_equal(bits(out), bits(x))
    assert torch.equal(ok.cpu(), net.predict(cur).cpu() == t)
