"""GPU checks of the saliency Drop attack (include/ifd_drop.h) against tests/drop_oracle.py.

One round on supplied gradients is exact: with alpha = 1 the header's formula, its lower median, its total order and its stable
compaction leave no bit open, so the saliencies, the centre, the dropped rows, the compacted cloud, the index rows and the counts
must equal the plain numpy restatement bit for bit.  Through the network the rounds are judged against the float64 oracle's free
run by the margin rule (drop_oracle.round_margin): in a round whose k-th and (k + 1)-th saliency lie further apart than 8 e_sal the
dropped SET must be the oracle's; a cloud that meets a round that is not clear is not judged further.  Everything else - ties,
untouched clouds, batching, the one-call form against the host-driven one - is exact."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import drop_oracle as DO
import pointnet_oracle as PO

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")
PAD = 7777                                                             # index rows beyond a cloud


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def net(sd):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as c:
        assert all(hasattr(c, k) for k in ("drop_step", "drop_attack"))
        yield c


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True))
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(a):
    a = np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def padded(clouds, stride, fill=np.nan):
    """A list of [n_b,3] arrays as [B,stride,3] with ``fill`` beyond each cloud."""
    out = np.full((len(clouds), stride, 3), fill, np.float32)
    for b, c in enumerate(clouds):
        out[b, :len(c)] = c
    return out


def gpu_step(net, pts, grads, stride, k, alpha=1., want=("saliency", "center", "dropped")):
    """One ifd_drop_step on ragged clouds -> (pc, n_points, index, diagnostics) as numpy arrays."""
    n = np.array([len(p) for p in pts], np.int32)
    idx = np.full((len(pts), stride), PAD, np.int32)
    for b in range(len(pts)):
        idx[b, :n[b]] = np.arange(n[b])
    pc, g, nn, ii = dev(padded(pts, stride)), dev(padded(grads, stride)), dev(n), dev(idx)
    out = net.drop_step(g, pc, nn, k, alpha, index=ii, want=want)
    torch.cuda.synchronize()
    return pc.cpu().numpy(), nn.cpu().numpy(), ii.cpu().numpy(), {k_: v.cpu().numpy() for k_, v in out.items()}


def check_step(pts, grads, stride, k, got, alpha=1.):
    """Everything ifd_drop_step writes against saliency_f32_plain + step, bit for bit; clouds outside the limits untouched."""
    pc, nn, ii, out = got
    before = padded(pts, stride)
    for b, (p, g) in enumerate(zip(pts, grads)):
        n = len(p)
        if not (k < n <= 2048):
            assert np.array_equal(bits(pc[b]), bits(before[b])) and nn[b] == n, "cloud %d is not untouched" % b
            assert list(ii[b, :n]) == list(range(n)) and (ii[b, n:] == PAD).all()
            assert np.isnan(out["saliency"][b]).all() and np.isnan(out["center"][b]).all() and (out["dropped"][b] == -1).all()
            continue
        s, c = DO.saliency_f32_plain(p, g, alpha)
        st = DO.step(p, s, k, np.arange(n))
        what = "cloud %d (n %d, k %d, stride %d)" % (b, n, k, stride)
        assert np.array_equal(bits(out["center"][b]), bits(c)), what
        assert np.array_equal(bits(out["saliency"][b, :n]), bits(s)), what
        assert np.isnan(out["saliency"][b, n:]).all(), what
        assert np.array_equal(out["dropped"][b], st["dropped"]), what
        assert nn[b] == n - k, what
        assert np.array_equal(bits(pc[b, :n - k]), bits(st["points"])), what
        assert not pc[b, n - k:n].any() and np.array_equal(bits(pc[b, n:]), bits(before[b, n:])), what
        assert np.array_equal(ii[b, :n - k], st["index"]) and (ii[b, n - k:n] == -1).all() and (ii[b, n:] == PAD).all(), what


# ---------------------------------------------------------------------------------------------- 1. one round, exact
@pytest.mark.parametrize("n", [2, 3, 64, 255, 256, 257, 1024, 2047, 2048])
def test_step_is_the_plain_restatement_bit_for_bit(net, n):
    """Dense random gradients, alpha = 1, k in {1, 5, n - 1}, stride == n and stride > n with NaN beyond the cloud (k = 5 at n <= 5
    leaves the cloud untouched, which is checked as such)."""
    rng = np.random.default_rng(n)
    pts = [rng.standard_normal((n, 3)).astype(np.float32) * np.float32(0.4) for _ in range(2)]
    grads = [rng.standard_normal((n, 3)).astype(np.float32) for _ in range(2)]
    for k in sorted({1, 5, n - 1}):
        for stride in (n, n + 37):
            check_step(pts, grads, stride, k, gpu_step(net, pts, grads, stride, k))


def test_step_ties_follow_the_total_order(net):
    """Duplicated rows (equal saliencies, equal coordinates for the median) and a gradient that is exactly zero in all but a few
    rows, with k reaching into the zeros: the lowest row goes first."""
    rng = np.random.default_rng(5)
    n = 300
    p = rng.standard_normal((n, 3)).astype(np.float32) * np.float32(0.4)
    p[100:200] = p[:100]                                               # every row of the first 100 twice
    p[250:] = p[249]
    dense = rng.standard_normal((n, 3)).astype(np.float32)
    dense[100:200] = dense[:100]
    sparse = np.zeros((n, 3), np.float32)
    sparse[[7, 107, 33, 260]] = dense[[7, 107, 33, 260]]
    zero = np.zeros((n, 3), np.float32)
    pts, grads = [p, p, p], [dense, sparse, zero]
    for k in (1, 4, 5, 150, 299):
        got = gpu_step(net, pts, grads, n + 3, k)
        check_step(pts, grads, n + 3, k, got)
        assert list(got[3]["dropped"][2]) == list(range(k))            # all saliencies equal (zero): rows 0 .. k - 1
    s, _ = DO.saliency_f32_plain(p, sparse)
    assert np.count_nonzero(s) <= 4 and len(np.unique(DO.saliency_f32_plain(p, dense)[0])) < n


def test_clouds_outside_the_limits_are_left_untouched(net):
    """A ragged batch, k = 5: clouds of 5 rows and fewer and one of 2049 rows are left as they are, counts included, next to
    clouds that are processed."""
    rng = np.random.default_rng(6)
    sizes = [10, 3, 2049, 5, 6, 1, 2048]
    pts = [rng.standard_normal((n, 3)).astype(np.float32) for n in sizes]
    grads = [rng.standard_normal((n, 3)).astype(np.float32) for n in sizes]
    got = gpu_step(net, pts, grads, 2100, 5)
    check_step(pts, grads, 2100, 5, got)
    assert list(got[1]) == [5, 3, 2049, 5, 1, 1, 2043]
    # a count above the stride
    pc, g = dev(padded(pts[:1], 10)), dev(padded(grads[:1], 10))
    nn = dev(np.array([11], np.int32))
    net.drop_step(g, pc, nn, 5)
    assert int(nn[0]) == 11 and np.array_equal(bits(pc), bits(padded(pts[:1], 10)))


def test_step_alpha_2_drops_the_float64_oracles_rows_on_clear_rounds(net):
    """alpha != 1 goes through powf: held to the float64 oracle by the margin rule."""
    rng = np.random.default_rng(7)
    pts = [rng.standard_normal((n, 3)).astype(np.float32) * np.float32(0.4) for n in (64, 100, 257, 33, 500, 64, 64, 1000)]
    grads = [rng.standard_normal(p.shape).astype(np.float32) for p in pts]
    got = gpu_step(net, pts, grads, 1000, 5, alpha=2.)
    clear = 0
    for b, (p, g) in enumerate(zip(pts, grads)):
        s64, _ = DO.saliency(p, g, torch.float64, 2)
        s32, _ = DO.saliency(p, g, torch.float32, 2)
        gap, e = DO.round_margin(s32, s64, 5)
        if DO.is_clear(gap, e):
            clear += 1
            assert set(got[3]["dropped"][b]) == set(DO.select(s64, 5)), b
    assert clear >= 7


# ---------------------------------------------------------------------------------------------- 2. through the network
def host_loop(net, pts, labels, num_drop, k, scale, n_points=None, want_dropped=False):
    """attack.SaliencyDrop's host-driven loop -> (cloud tensor [B,stride,3], counts, index, dropped per round)."""
    B, stride = pts.shape[:2]
    cur, tgt = dev(pts), dev(labels)
    n = torch.full((B,), stride, dtype=torch.int32, device="cuda") if n_points is None else dev(n_points, torch.int32)
    idx = torch.arange(stride, dtype=torch.int32, device="cuda")[None].repeat(B, 1).contiguous()
    if n_points is not None:
        idx[torch.arange(stride, device="cuda")[None] >= n[:, None]] = -1
    rounds = []
    for done in range(0, num_drop, k):
        grad = net.input_grad(cur, tgt, "cross_entropy", 0., scale, n_points=n)
        out = net.drop_step(grad, cur, n, min(k, num_drop - done), 1., index=idx, want=("dropped",) if want_dropped else ())
        if want_dropped:
            rounds.append(out["dropped"].cpu().numpy())
    return cur, n, idx, rounds


def raw_attack(net, pts, labels, num_drop, k, scale, n_points=None, alpha=1., size=None, out=None):
    """ifd_drop_attack itself -> (rc, pc_out, n_out, kept, correct): output arrays start as NaN / -7."""
    from ifdefense_amd import _lib
    pc = pts if torch.is_tensor(pts) else dev(pts)
    B, stride = pc.shape[:2]
    tgt = dev(np.asarray(labels), torch.int32)
    n = None if n_points is None else dev(np.asarray(n_points), torch.int32)
    o = torch.full_like(pc, float("nan")) if out is None else out
    n_out, kept, ok = (torch.full(s, -7, dtype=torch.int32, device="cuda") for s in ((B,), (B, stride), (B,)))
    P = _lib.IfdDropParams(C.sizeof(_lib.IfdDropParams) if size is None else size, num_drop, k, alpha, scale)
    rc = net.lib.ifd_drop_attack(net.ctx, C.byref(P), pc.data_ptr(), None if n is None else n.data_ptr(), tgt.data_ptr(), B, stride,
                                 o.data_ptr(), n_out.data_ptr(), kept.data_ptr(), ok.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, o, n_out, kept, ok


@pytest.mark.parametrize("case", [c for c in DO.CASES if c[0] <= 300], ids=lambda c: "n%d_B%d_drop%d_k%d" % c)
def test_attack_rounds_against_the_float64_oracle(net, case):
    n, B, num_drop, k = case
    pts, labels, _, runs = DO.case_run(case)
    cur, cnt, idx, rounds = host_loop(net, pts, labels, num_drop, k, 1. / B, want_dropped=True)
    judged = np.ones(B, bool)
    met = 0
    for i, got in enumerate(rounds):
        for b in range(B):
            r = runs[b]["rounds"][i]
            if judged[b] and not r["clear"]:
                judged[b] = False
            if not judged[b]:
                met += 1
                continue
            assert set(got[b, :r["k"]]) == set(r["dropped"]), "round %d cloud %d (gap %.2e, e_sal %.2e)" % (i, b, r["gap"], r["e_sal"])
    print("case %s: %d of %d cloud-rounds not judged" % (case, met, B * len(rounds)))
    assert met <= 0.1 * B * len(rounds)
    assert (cnt.cpu().numpy() == n - num_drop).all()
    correct = (net.predict(cur[:, :n - num_drop].contiguous()).cpu().numpy() == labels)
    for b in np.nonzero(judged)[0]:
        assert np.array_equal(idx[b, :n - num_drop].cpu().numpy(), runs[b]["kept"])
        assert np.array_equal(bits(cur[b, :n - num_drop]), bits(runs[b]["points"]))
        assert bool(correct[b]) == runs[b]["correct"], b


@pytest.mark.parametrize("case", [(64, 8, 12, 5), (33, 8, 7, 3), (2, 8, 1, 1)], ids=lambda c: "n%d_B%d_drop%d_k%d" % c)
def test_one_call_gives_the_bits_of_the_host_driven_loop(net, case):
    n, B, num_drop, k = case
    pts, labels, _ = DO.case_inputs(n, B)
    cur, cnt, idx, _ = host_loop(net, pts, labels, num_drop, k, 1. / B)
    rc, out, n_out, kept, ok = raw_attack(net, pts, labels, num_drop, k, 1. / B)
    assert rc == 0
    m = n - num_drop
    assert np.array_equal(bits(out), bits(cur)) and np.array_equal(n_out.cpu().numpy(), cnt.cpu().numpy()) and (n_out == m).all()
    assert np.array_equal(kept.cpu().numpy(), idx.cpu().numpy())
    want_ok = net.predict(cur[:, :m].contiguous()).cpu().numpy() == labels
    assert np.array_equal(ok.cpu().numpy().astype(bool), want_ok)
    kk = kept.cpu().numpy()
    for b in range(B):                                                 # kept indexes pc_in to exactly pc_out
        assert np.array_equal(bits(pts[b][kk[b, :m]]), bits(out[b, :m])) and (np.diff(kk[b, :m]) > 0).all() and (kk[b, m:] == -1).all()
        assert not out[b, m:].cpu().numpy().any()
    # the Python entry returns the same
    o2, ok2, k2 = net.drop_attack(pts, labels, num_drop, k, 1., 1. / B, want_kept=True)
    assert np.array_equal(bits(o2), bits(out[:, :m])) and np.array_equal(ok2.cpu().numpy(), want_ok) and np.array_equal(k2.cpu().numpy(), kk[:, :m])


def test_batching_is_bitwise(net):
    """A cloud's result does not depend on B, on its position, on stride or on the other clouds: roll, permutation, B in {1, 15,
    257}, another stride with NaN padding, ragged counts, and the chunked path (B = 4097) at a small n."""
    n, num_drop, k, scale = 64, 12, 5, 0.125
    pts, labels, _ = DO.case_inputs(n, 8)
    alone = []
    for b in range(8):                                                 # B = 1: the reference of everything below
        rc, out, n_out, kept, ok = raw_attack(net, pts[b:b + 1], labels[b:b + 1], num_drop, k, scale)
        assert rc == 0
        alone.append((out[0, :n - num_drop].cpu().numpy(), kept[0, :n - num_drop].cpu().numpy(), int(ok[0])))

    def same(order, stride=n, counts=None):
        order = np.asarray(order)
        x = padded([pts[b] for b in order], stride)
        rc, out, n_out, kept, ok = raw_attack(net, x, labels[order], num_drop, k, scale, n_points=counts)
        assert rc == 0
        for j, b in enumerate(order):
            m = n - num_drop
            assert np.array_equal(bits(out[j, :m]), bits(alone[b][0])) and np.array_equal(kept[j, :m].cpu().numpy(), alone[b][1])
            assert int(ok[j]) == alone[b][2] and int(n_out[j]) == m
            if stride > n:
                assert np.isnan(out[j, n:].cpu().numpy()).all() and not out[j, m:n].cpu().numpy().any()
    same(np.roll(np.arange(8), 3))
    same(np.random.default_rng(0).permutation(8))
    for B in (15, 257):
        same(np.arange(B) % 8)
    same(np.arange(8), stride=100, counts=np.full(8, n, np.int32))
    # ragged counts: cloud b truncated to n - 3 b rows, against its own B = 1 run
    counts = np.array([n - 3 * b for b in range(8)], np.int32)
    rc, out, n_out, kept, ok = raw_attack(net, padded([pts[b][:counts[b]] for b in range(8)], 70), labels, num_drop, k, scale, n_points=counts)
    assert rc == 0
    for b in range(8):
        r1 = raw_attack(net, np.ascontiguousarray(pts[b:b + 1, :counts[b]]), labels[b:b + 1], num_drop, k, scale)
        m = counts[b] - num_drop
        assert r1[0] == 0 and int(n_out[b]) == m and np.array_equal(bits(out[b, :m]), bits(r1[1][0, :m])) and int(ok[b]) == int(r1[4][0])
        assert np.array_equal(kept[b, :m].cpu().numpy(), r1[3][0, :m].cpu().numpy())
    # the chunked path: 4097 clouds of 8 points
    small, lab = np.ascontiguousarray(pts[:, :8]), labels
    base = [raw_attack(net, small[b:b + 1], lab[b:b + 1], 3, 2, scale) for b in range(8)]
    order = np.arange(4097) % 8
    rc, out, n_out, kept, ok = raw_attack(net, small[order], lab[order], 3, 2, scale)
    assert rc == 0 and (n_out == 5).all()
    o, kp, okn = out.cpu().numpy(), kept.cpu().numpy(), ok.cpu().numpy()
    for b in range(8):
        rows = np.nonzero(order == b)[0]
        assert (bits(o[rows, :5]) == bits(base[b][1][0, :5])[None]).all() and (kp[rows] == base[b][3].cpu().numpy()).all()
        assert (okn[rows] == int(base[b][4][0])).all()


def test_the_recorded_reference_run(net):
    """tests/golden/drop_golden.npz: on the all-clear clouds the GPU leaves the reference's set of rows, bit for bit, and the
    success counts agree."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "drop_golden.npz"))
    B = len(g["data"])
    out, ok = net.drop_attack(g["data"], g["label"], int(g["num_drop"]), int(g["k"]), float(g["alpha"]), 1. / B)
    out = out.cpu().numpy()
    assert out.shape == g["adv"].shape and g["all_clear"].sum() >= 3
    srt = lambda a: a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]         # noqa: E731
    for b in np.nonzero(g["all_clear"])[0]:
        assert np.array_equal(bits(srt(out[b])), bits(srt(g["adv"][b]))), b
    assert int(ok.sum()) == int(g["success_num"])


# ---------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_write_nothing_and_a_stale_workspace_changes_nothing(sd, net):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    pts, labels, _ = DO.case_inputs(64, 8)
    first = raw_attack(net, pts, labels, 12, 5, 0.125)
    assert first[0] == 0

    def refused(r, word):
        rc, out, n_out, kept, ok = r
        assert rc == -1 and word.encode() in net.lib.ifd_last_error(net.ctx), (rc, word, net.lib.ifd_last_error(net.ctx))
        assert np.isnan(out.cpu().numpy()).all() and (n_out == -7).all() and (kept == -7).all() and (ok == -7).all()
    refused(raw_attack(net, pts, labels, 64, 5, 0.125), "num_drop")                        # num_drop >= n
    refused(raw_attack(net, pts, labels, 65, 5, 0.125), "num_drop")
    refused(raw_attack(net, np.zeros((1, 2049, 3), np.float32), [0], 5, 5, 1.), "without n_points")
    refused(raw_attack(net, np.zeros((2, 2100, 3), np.float32), [0, 0], 5, 5, 1., n_points=[2048, 2049]), "n_points outside [6, 2048]")
    refused(raw_attack(net, pts, labels, 12, 5, 0.125, n_points=[64] * 7 + [12]), "n_points outside [13, 64]")
    bad = labels.copy()
    bad[3] = 40
    refused(raw_attack(net, pts, bad, 12, 5, 0.125), "outside [0, 40)")
    refused(raw_attack(net, pts, labels, 0, 5, 0.125), "num_drop")
    refused(raw_attack(net, pts, labels, 12, 0, 0.125), "k < 1")
    refused(raw_attack(net, pts, labels, 12, 5, 0.125, alpha=0.), "alpha")
    refused(raw_attack(net, pts, labels, 12, 5, 0.125, alpha=float("nan")), "alpha")
    refused(raw_attack(net, pts, labels, 12, 5, 0.125, size=16), "struct_size")
    x = dev(pts)
    rc = raw_attack(net, x, labels, 12, 5, 0.125, out=x)[0]
    assert rc == -1 and b"overlaps" in net.lib.ifd_last_error(net.ctx) and np.array_equal(bits(x), bits(pts))
    g, nn = torch.zeros(1, 8, 3, device="cuda"), torch.full((1,), 8, dtype=torch.int32, device="cuda")
    for k, alpha in ((0, 1.), (2, 0.), (2, -1.), (2, float("inf"))):
        with pytest.raises(I.IfdError, match="k < 1|alpha"):
            net.drop_step(g, g.clone(), nn, k, alpha)
    assert int(nn[0]) == 8
    with pytest.raises(I.IfdError, match="label|target"):
        net.drop_attack(pts, labels[:7], 12)
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, True), "pointnet"), feature_transform=True, device="cuda:0") as ft:
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.drop_attack(pts, labels, 12)
        with pytest.raises(I.IfdError, match="feature_transform"):
            ft.drop_step(g, g.clone(), nn, 2)
    # a larger workspace left by a bigger call changes nothing
    big, lab = DO.case_inputs(300, 40)[:2]
    assert raw_attack(net, big, lab, 10, 5, 1. / 40)[0] == 0
    again = raw_attack(net, pts, labels, 12, 5, 0.125)
    assert again[0] == 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(first[1:], again[1:]))


# ---------------------------------------------------------------------------------------------- 4. the CLI
def test_cli_end_to_end(net, sd, tmp_path, capsys):
    from ifdefense_amd import inference as Inf, drop_attack as DA
    import bench
    ck, src = str(tmp_path / "pointnet.npz"), str(tmp_path / "attack_data.npz")
    np.savez(ck, **sd)
    pcs = bench.synth_clouds(6, seed=5)[:, :64]
    norm = np.stack([Inf.normalize_points_np(c) for c in pcs])
    label = net.predict(norm).cpu().numpy().astype(np.uint8)
    target = ((label + 1) % 40).astype(np.uint8)
    np.savez(src, test_pc=pcs, test_label=label, target_label=target)
    assert DA.main(["--data_root", src, "--num_points", "64", "--num_drop", "10", "--batch_size", "4", "--model_path", ck,
                    "--out_dir", str(tmp_path)]) == 0
    out = capsys.readouterr().out
    lines = [l for l in out.splitlines() if l.startswith("Final success")]
    assert [l.split(",")[0].split("/")[-1] for l in lines] == ["4", "2"] and all(l.endswith("point num: 54/64") for l in lines)
    counts = [int(l.split()[2].split("/")[0]) for l in lines]
    d = tmp_path / "attack" / "results" / "mn40_64" / "Drop_10"
    (name,) = os.listdir(d)
    assert name == "Drop-pointnet-acc_%.4f.npz" % (sum(counts) / 6.0)
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 54, 3) and np.isfinite(z["test_pc"]).all()
    assert np.array_equal(z["test_label"], label) and np.array_equal(z["target_label"], target)
    for b in range(6):                                                 # every written row is a row of the normalised input, in its order
        rows = [int(np.nonzero((norm[b] == r).all(1))[0][0]) for r in z["test_pc"][b]]
        assert rows == sorted(rows) and len(set(rows)) == 54
    assert Inf.main(["--data_root", str(d / name), "--mode", "normal", "--model", "pointnet", "--model_path", ck, "--num_points", "54"]) == 0
    line = capsys.readouterr().out.strip().splitlines()[-1]
    acc = float(line.split("Overall accuracy:")[1].split(",")[0])
    assert "%.4f" % acc == "%.4f" % (sum(counts) / 6.0)
