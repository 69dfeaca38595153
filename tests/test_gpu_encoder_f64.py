"""The encoder half of the pipeline against float64: the point-net + scatter-mean (csrc/encoder.hip), the Winograd U-Net
(csrc/unet.hip) and the ONet point encoder (csrc/onet.hip), at the launch shapes production uses and at the edges where
their index arithmetic, tails and chunking could go wrong.

The float64 reference is the oracle with the weights cast to double.  Its discrete decisions are the reference's: the cell
of a point comes from the float32 coordinate arithmetic (``O.plane_index`` on the float32 points, injected through
``index=``), so float64 changes the features only.  tests/test_oracle_golden.py shows that this helper reproduces the
reference's fixtures within one float32 rounding floor.

Bars are stated against the float32 oracle's own floor, measured on the same input in the same test: for every compared
tensor (one image, or one cloud's features / latent code)
    err(x) = max|x - ref64| / max|ref64|,
    err(hip) <= 4 err(f32 oracle) + 1e-7        and        err(hip) <= 5e-6 (planes, point features), 2e-6 (ONet c).
Each test prints both errors; the ranges measured on the MI355X are in the docstrings.  Measured: the largest ratio
err(hip) / err(f32 oracle) anywhere is 2.1 (ONet c and two-point clouds, both near the 1e-7 floor); the Winograd U-Net is
closer to float64 than the float32 oracle's direct convolution (ratio <= 0.66 with random weights, <= 1.08 trained-like).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PL = ("xz", "xy", "yz")
CAP_PLANES, CAP_ONET = 5e-6, 2e-6


def _err(x, ref):
    """Per leading index: max|x - ref| / max|ref| over the rest."""
    x = np.asarray(x, np.float64).reshape(len(ref), -1)
    ref = np.asarray(ref, np.float64).reshape(len(ref), -1)
    return np.abs(x - ref).max(1) / np.abs(ref).max(1)


def _gate(tag, hip, f32, ref64, cap):
    """The section-2 bar on every leading index of hip / f32 / ref64; prints the measured ranges."""
    eh, eo = _err(hip, ref64), _err(f32, ref64)
    ratio = eh / (eo + 2.5e-8)
    print("%-44s n %4d  err(hip) %.2e .. %.2e  err(f32 oracle) %.2e .. %.2e  max ratio %.2f"
          % (tag, len(eh), eh.min(), eh.max(), eo.min(), eo.max(), ratio.max()))
    bad = np.nonzero((eh > 4 * eo + 1e-7) | (eh > cap))[0]
    assert bad.size == 0, (tag, bad[:8].tolist(), eh[bad[:8]].tolist(), eo[bad[:8]].tolist())
    return eh, eo


def _w64(w):
    return {k: v.double() if v.is_floating_point() else v for k, v in w.items()}


def _realistic_sel(clouds, T=600):
    """The encoder's input as the pipeline builds it: the first T points of each cloud, preprocessed like the reference
    (centred, largest extent 0.9; opt_defense.py:122-127)."""
    from oracle import convonet_oracle as O
    return np.stack([O.preprocess_pc(c[:T]) for c in clouds])


def _bench_clouds(n):
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench.synth_clouds(n)


# ------------------------------------------------------------------------------------------------
# weight sets: random seed 0 and the trained-like checkpoint, each with its own context
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wsets(np_weights):
    import ifdefense_amd as I
    from oracle import convonet_oracle as O
    z = np.load(os.path.join(HERE, "golden", "trained_like_f16.npz"))
    out = {}
    for name, w in (("random0", np_weights), ("trained", {k: z[k].astype(np.float32) for k in z.files})):
        w32 = O.to_torch(w)
        out[name] = (w32, _w64(w32), I.Restorer(I.weights.pack_state_dict(w), device="cuda:0"))
    yield out
    for _, _, r in out.values():
        r.close()


def _unet_refs(w32, w64, imgs):
    """float64 and float32 oracle U-Net of channel-last images [N,64,64,32] (CPU, in batches) -> two [N,64,64,32]."""
    from oracle import convonet_oracle as O
    r64, r32 = [], []
    with torch.no_grad():
        for i in range(0, len(imgs), 12):
            x = torch.as_tensor(imgs[i:i + 12]).permute(0, 3, 1, 2)
            r64.append(O.unet_forward(w64, x.double()).permute(0, 2, 3, 1).numpy())
            r32.append(O.unet_forward(w32, x.float()).permute(0, 2, 3, 1).numpy())
    return np.concatenate(r64), np.concatenate(r32)


def _pointnet_refs(w32, w64, sel, t):
    """One cloud's first t points: float64 and float32 features [t,32] and pre-U-Net planes [3,64,64,32] channel-last,
    and the occupied-cell map [3,64,64] of the float32 cells (the reference's)."""
    from oracle import convonet_oracle as O
    p = torch.as_tensor(sel[None, :t])
    index = O.plane_index(p)
    with torch.no_grad():
        c64, _ = O.pointnet_features(w64, p.double(), index=index)
        c32, _ = O.pointnet_features(w32, p)
        pre64 = np.stack([O.scatter_mean_plane(c64, index[pl])[0].permute(1, 2, 0).numpy() for pl in PL])
        pre32 = np.stack([O.scatter_mean_plane(c32, index[pl])[0].permute(1, 2, 0).numpy() for pl in PL])
    occ = np.zeros((3, 64 * 64), bool)
    for i, pl in enumerate(PL):
        occ[i, index[pl][0].numpy()] = True
    return c64[0].numpy(), c32[0].numpy(), pre64, pre32, occ.reshape(3, 64, 64)


# ------------------------------------------------------------------------------------------------
# 3. U-Net accuracy at small batches
# ------------------------------------------------------------------------------------------------
DELTA_AT = [(0, 0), (63, 63), (0, 63), (63, 0),                 # image corners
            (7, 8), (8, 7), (15, 16), (31, 32),                  # 8-pixel region edges (a Winograd tile group is 8 x 16 pixels)
            (4, 44), (44, 4), (60, 27), (27, 60)]                # pooled three times: top, left, bottom, right border of 8 x 8


def _unet_inputs(restorer, golden):
    """33 channel-last images [64,64,32], a different one on each plane of a cloud: realistic pre-U-Net planes (bench and
    golden clouds, ~600 occupied cells of 4096), dense Gaussian, the realistic ones x 1e3 and x 1e-3, the all-zero image
    (biases and zero padding only) and single-pixel deltas at corners, region edges and pixels that pooling takes to the
    8 x 8 level's border."""
    proc = golden["proc_pad"][0, :golden["proc_len"][0]]
    sel = np.concatenate([_realistic_sel(_bench_clouds(2)), proc[golden["sel_idx"][0]][None]])
    real = restorer.encode_points(torch.from_numpy(sel)).cpu().numpy().reshape(9, 64, 64, 32)
    g = np.random.default_rng(11)
    dense = g.standard_normal((5, 64, 64, 32)).astype(np.float32) * 0.3
    deltas = np.zeros((len(DELTA_AT), 64, 64, 32), np.float32)
    for k, (y, x) in enumerate(DELTA_AT):
        for j, (ch, amp) in enumerate(((k % 32, 1.0), ((7 * k + 3) % 32, -0.7), ((13 * k + 5) % 32, 0.4))):
            deltas[k, y, x, ch] = amp
    names = (["realistic"] * 9 + ["dense"] * 5 + ["x1e3"] * 3 + ["x1e-3"] * 3 + ["zero"]
             + ["delta %s" % (yx,) for yx in DELTA_AT])
    imgs = np.concatenate([real, dense, real[:3] * 1e3, real[3:6] * 1e-3, np.zeros((1, 64, 64, 32), np.float32), deltas])
    assert len(imgs) == len(names) == 33
    return imgs.astype(np.float32), names


@pytest.mark.parametrize("wname", ["random0", "trained"])
def test_unet_small_batches_against_float64(wsets, golden, wname):
    """ifd_unet on 11 clouds (33 different images, per = 1 everywhere) against the float64 U-Net, per image.
    Measured (MI355X), err(hip) / err(f32 oracle): random weights 2.6e-7 ... 4.1e-7 / 4.8e-7 ... 9.6e-7 (max ratio 0.60),
    trained-like 2.0e-7 ... 6.0e-7 / 3.3e-7 ... 6.3e-7 (max ratio 1.08); the zero image 2.9e-7 / 5.4e-7, the deltas
    2.5e-7 ... 3.2e-7 / 4.3e-7 ... 6.4e-7."""
    w32, w64, r = wsets[wname]
    imgs, names = _unet_inputs(r, golden)
    got = r.unet(torch.from_numpy(imgs).reshape(11, 3, 64, 64, 32)).cpu().numpy().reshape(33, 64, 64, 32)
    ref64, ref32 = _unet_refs(w32, w64, imgs)
    eh, eo = _gate("U-Net %s, 33 images" % wname, got, ref32, ref64, CAP_PLANES)
    for fam in dict.fromkeys(n.split(" ")[0] for n in names):
        sel = [i for i, n in enumerate(names) if n.split(" ")[0] == fam]
        print("    %-10s err(hip) %.2e .. %.2e   err(f32 oracle) %.2e .. %.2e"
              % (fam, eh[sel].min(), eh[sel].max(), eo[sel].min(), eo[sel].max()))


# ------------------------------------------------------------------------------------------------
# 4. U-Net launch-shape invariance, and the composite call
# ------------------------------------------------------------------------------------------------
def _tail_images(B):
    """Images that lie in the last two blocks of each level of a B-cloud launch, plus the first and the last image.
    launch_wino (csrc/unet.hip) gives a block per = max(1, min(16, n_items * gy / 6144)) (image, region) work items;
    per level (items per image, gy = output-channel groups): 64^2 (32, 1), 32^2 (8, 2), 16^2 (2, 4), 8^2 (1, 4).

        clouds | 64^2       | 32^2      | 16^2      | 8^2
        1-16   | 1          | 1         | 1         | 1
        164    | 2          | 1         | 1         | 1
        683    | 10, tail 8 | 5, tail 2 | 2         | 1
        1237   | 16         | 9, tail 6 | 4, tail 2 | 2, tail 1
        2304   | 16         | 16        | 9         | 4
        2468   | 16         | 16        | 9, tail 3 | 4

    The software-pipelined fetch of wino_kernel carries a block across region and image boundaries, and the last block of
    a level is partial where there is a tail.  (The formula only picks the images; the test asserts nothing about it.)"""
    n_img = 3 * B
    pick = {0, n_img - 1}
    for ipi, gy in ((32, 1), (8, 2), (2, 4), (1, 4)):
        n_items = n_img * ipi
        per = max(1, min(16, n_items * gy // 6144))
        n_blk = -(-n_items // per)
        if per > 1:
            first = max(0, (n_blk - 2) * per)
            pick.update(range(first // ipi, n_img))
    return sorted(pick)


def test_unet_launch_shapes_bitwise_and_tails_against_float64(np_weights, oracle_weights):
    """One ifd_unet call on B = 164, 683, 1237, 2304, 2468 clouds of realistic pre-U-Net planes (per > 1 and partial
    last blocks, see _tail_images): every image bitwise equal to the same cloud run in launches of 16 clouds (per = 1
    everywhere; the kernel's summation order does not depend on the batch), and the images of the last two blocks of
    every level, plus the first and the last, against float64.  ifd_encode_planes is bitwise ifd_unet(ifd_encode_points)
    at B = 1 and B = 2468.  Own context, closed at the end: the U-Net scratch is ~5 MB per image (~37 GB at 2468).
    Measured (MI355X): every image of all five launches bitwise equal; the 28 tail images 3.1e-7 ... 4.6e-7 from float64,
    the float32 oracle 5.5e-7 ... 9.2e-7 (max ratio 0.66)."""
    import ifdefense_amd as I
    r = I.Restorer(I.weights.pack_state_dict(np_weights), device="cuda:0")
    try:
        sel = torch.from_numpy(_realistic_sel(_bench_clouds(2468))).cuda()
        pre = r.encode_points(sel)
        small = torch.empty_like(pre)
        for b0 in range(0, 2468, 16):
            small[b0:b0 + 16] = r.unet(pre[b0:b0 + 16])
        picked_in, picked_out, tags = [], [], []
        full = None
        for B in (164, 683, 1237, 2304, 2468):
            full = r.unet(pre[:B])
            if not torch.equal(full, small[:B]):
                diff = (full != small[:B]).flatten(2).any(2).nonzero().cpu().tolist()
                raise AssertionError("B = %d: %d images differ from 16-cloud launches, first (cloud, plane) %s"
                                     % (B, len(diff), diff[:8]))
            imgs = _tail_images(B)
            tags += ["B%d/img%d" % (B, i) for i in imgs]
            idx = torch.tensor(imgs, device=pre.device)
            picked_in.append(pre[:B].reshape(3 * B, 64, 64, 32)[idx].cpu().numpy())
            picked_out.append(full.reshape(3 * B, 64, 64, 32)[idx].cpu().numpy())
            print("B = %4d: all %d images bitwise equal to 16-cloud launches; float64 check of images %s" % (B, 3 * B, imgs))
        planes = r.encode_inputs(sel)                                             # ifd_encode_planes, B = 2468
        assert torch.equal(planes, full)
        del planes
        assert torch.equal(r.encode_inputs(sel[:1]), r.unet(r.encode_points(sel[:1])))
    finally:
        r.close()
    imgs_in, got = np.concatenate(picked_in), np.concatenate(picked_out)
    ref64, ref32 = _unet_refs(oracle_weights, _w64(oracle_weights), imgs_in)
    _gate("U-Net tail blocks, %d images of 5 launches" % len(tags), got, ref32, ref64, CAP_PLANES)


# ------------------------------------------------------------------------------------------------
# 5. point encoder edges
# ------------------------------------------------------------------------------------------------
def _check_points(restorer, w32, w64, sel, tpc, tag):
    """encode_points of sel [B,Tmax,3] (t_per_cloud tpc or None) against float64 per cloud: features of the live points
    and the three pre-U-Net planes, and the occupied cells equal to the float32 reference's exactly."""
    B, Tmax = sel.shape[:2]
    t = [Tmax] * B if tpc is None else list(tpc)
    pre, c = restorer.encode_points(torch.from_numpy(sel), None if tpc is None else torch.tensor(tpc), want_c=True)
    pre, c = pre.cpu().numpy(), c.cpu().numpy()
    hc, oc, rc, hp, op, rp = [], [], [], [], [], []
    for b in range(B):
        c64, c32, pre64, pre32, occ = _pointnet_refs(w32, w64, sel[b], t[b])
        got_occ = (pre[b] != 0).any(-1)
        assert np.array_equal(got_occ, occ), (tag, b, int((got_occ != occ).sum()))
        hc.append(c[b, :t[b]]); oc.append(c32); rc.append(c64)
        hp.append(pre[b]); op.append(pre32); rp.append(pre64)
    eh, eo = [], []
    for b in range(B):                                         # features: one cloud at a time (ragged lengths)
        h, o = _err(hc[b][None], rc[b][None]), _err(oc[b][None], rc[b][None])
        eh.append(h[0]); eo.append(o[0])
    eh, eo = np.array(eh), np.array(eo)
    print("%-44s c: err(hip) %.2e .. %.2e  err(f32 oracle) %.2e .. %.2e" % (tag, eh.min(), eh.max(), eo.min(), eo.max()))
    bad = np.nonzero((eh > 4 * eo + 1e-7) | (eh > CAP_PLANES))[0]
    assert bad.size == 0, (tag, "c", bad.tolist(), eh[bad].tolist(), eo[bad].tolist())
    _gate(tag + " planes", np.concatenate(hp), np.concatenate(op), np.concatenate(rp), CAP_PLANES)
    return pre, c


@pytest.mark.parametrize("wname", ["random0", "trained"])
def test_point_encoder_sizes_and_ragged_against_float64(wsets, wname):
    """Tmax in {1, 2, 63, 64, 65, 600, 640, 641, 1000, 1024} (the <10> / <16>-wave kernel switch lies between 640 and
    641), and ragged batches mixing t = 1, Tmax - 1 and Tmax; each ragged cloud bitwise equal to the same cloud alone.
    Measured (MI355X), features and planes: random weights err(hip) 2.3e-7 ... 5.3e-7, err(f32 oracle) 2.2e-7 ... 5.3e-7
    (max ratio 1.48, Tmax 1); trained-like 1.3e-7 ... 3.6e-7 against 8.0e-8 ... 3.5e-7 (max ratio 2.09, Tmax 2: both
    within 1e-7 of each other).  Occupied cells equal everywhere."""
    w32, w64, r = wsets[wname]
    g = np.random.default_rng(21)
    for Tmax in (1, 2, 63, 64, 65, 600, 640, 641, 1000, 1024):
        sel = (g.uniform(-0.45, 0.45, (2, Tmax, 3))).astype(np.float32)
        _check_points(r, w32, w64, sel, None, "%s Tmax %d" % (wname, Tmax))
    for Tmax in (65, 640, 641, 1024):
        sel = _realistic_sel(_bench_clouds(3), 1024)[:, :Tmax].copy()
        tpc = [1, Tmax - 1, Tmax]
        for b, t in enumerate(tpc):
            sel[b, t:] = 7.0                                                    # padding is never read
        pre, c = _check_points(r, w32, w64, sel, tpc, "%s ragged Tmax %d" % (wname, Tmax))
        for b, t in enumerate(tpc):
            pa, ca = r.encode_points(torch.from_numpy(sel[b:b + 1, :t].copy()), want_c=True)
            assert np.array_equal(pa[0].cpu().numpy(), pre[b]), (Tmax, b)
            assert np.array_equal(ca[0].cpu().numpy(), c[b, :t]), (Tmax, b)


def _boundary_values(sdiv):
    """For each of the 65 grid lines k: p = float32((k / 64 - 0.5) sdiv) and its +-1, +-2 ulp neighbours (325 values)."""
    out = []
    for k in range(65):
        p = np.float32((k / 64 - 0.5) * float(sdiv))
        out += [p, np.nextafter(p, np.float32(1)), np.nextafter(p, np.float32(-1)),
                np.nextafter(np.nextafter(p, np.float32(1)), np.float32(1)),
                np.nextafter(np.nextafter(p, np.float32(-1)), np.float32(-1))]
    return np.array(out, np.float32)


def test_point_encoder_cell_boundaries_clamp_and_crowding(wsets):
    """The cell index int((p / sdiv + 0.5) * 64) at every grid line and 1 / 2 ulp off it, the clamp (|p| at and beyond
    0.5505, u = 1 - 10e-6), all 1024 points in one cell, and a cloud of 16 points repeated 64 times: cells equal to the
    float32 reference's exactly, features and planes against float64.  Also prints how torch-ROCm's own float32
    normalize_coordinate on the GPU places the boundary points (informational: the fixtures and the kernel use the CPU
    form).  Measured (MI355X): occupied cells equal in every case; features / planes 2.3e-7 ...
    4.1e-7 (boundaries, clamp) and 4.2e-7 ... 1.7e-6 (crowded; the float32 oracle 3.6e-7 ... 1.8e-6), max ratio 1.11;
    torch-ROCm's GPU form puts 330 of the 2925 boundary cells elsewhere - exactly the cells of x * float32(1 / sdiv)."""
    from oracle import convonet_oracle as O
    w32, w64, r = wsets["random0"]
    sdiv = np.float32(1 + 0.1 + 10e-6)
    v = _boundary_values(sdiv)
    n = len(v)
    sel = np.stack([np.stack([v, np.roll(v, 7 * j + 1), np.roll(v, -(11 * j + 3))], 1) for j in range(3)]).astype(np.float32)
    _check_points(r, w32, w64, sel, None, "cell boundaries (3 x %d points)" % n)
    cpu = O.plane_index(torch.from_numpy(sel))
    gpu = O.plane_index(torch.from_numpy(sel).cuda())
    n_diff = sum(int((cpu[pl] != gpu[pl].cpu()).sum()) for pl in PL)
    print("torch-ROCm normalize_coordinate on the GPU: %d of %d boundary cells differ from the CPU form" % (n_diff, 3 * 3 * n))
    # the points are close enough to the grid lines to tell the forms apart: a kernel that multiplied by the reciprocal
    # (the form above) would put cells elsewhere, and the exact occupancy check would fail
    recip = np.float32(1 / float(sdiv))
    n_recip = 0
    for pl, (a0, a1) in O.PLANE_AXES.items():
        u = np.stack([sel[..., a0], sel[..., a1]], -1) * recip + np.float32(0.5)
        u = np.where(u >= 1, np.float32(1 - 10e-6), np.where(u < 0, np.float32(0), u))
        ij = (u * np.float32(64)).astype(np.int64)
        n_recip += int((ij[..., 0] + 64 * ij[..., 1] != cpu[pl].numpy()).sum())
    print("x * float32(1 / sdiv): %d of %d boundary cells differ from the CPU form" % (n_recip, 3 * 3 * n))
    assert n_recip > 0
    # the clamp: at and beyond +-0.5505 (u >= 1 -> 1 - 10e-6, u < 0 -> 0), and points whose u is 1 - 10e-6 and its neighbours
    uc = np.float32(1 - 10e-6)
    pu = np.float32((float(uc) - 0.5) * float(sdiv))
    edge = [0.5505, 0.55050004, 0.55055, 0.5506, 0.56, 0.6, 1.0, 5.0, pu, np.nextafter(pu, np.float32(1)),
            np.nextafter(pu, np.float32(0)), np.nextafter(np.nextafter(pu, np.float32(1)), np.float32(1))]
    edge = np.array(edge + [-e for e in edge], np.float32)
    g = np.random.default_rng(31)
    clamp = g.uniform(-0.45, 0.45, (2, 3 * len(edge), 3)).astype(np.float32)
    for j in range(3):
        clamp[0, j * len(edge):(j + 1) * len(edge), j] = edge
        clamp[1, j * len(edge):(j + 1) * len(edge), j] = edge
        clamp[1, j * len(edge):(j + 1) * len(edge), (j + 1) % 3] = edge[::-1]
    _check_points(r, w32, w64, clamp, None, "clamp (2 x %d points)" % clamp.shape[1])
    # crowding: every point in one cell (cell (20, 33, 41) in x, y, z), and 16 distinct points, each 64 times
    cell = np.array([20, 33, 41])
    centre = ((cell + 0.5) / 64 - 0.5) * float(sdiv)
    one = (centre + g.uniform(-0.3, 0.3, (1024, 3)) * float(sdiv) / 64).astype(np.float32)
    dup = np.repeat(g.uniform(-0.45, 0.45, (16, 3)), 64, axis=0).astype(np.float32)[g.permutation(1024)]
    _check_points(r, w32, w64, np.stack([one, dup]), None, "1024 points in one cell / 16 points x 64")


# ------------------------------------------------------------------------------------------------
# 6. ONet encoder
# ------------------------------------------------------------------------------------------------
def test_onet_encoder_batches_chunks_and_row_tails_against_float64():
    """ifd_onet_encode at B in {1, 255, 256, 257, 600} (passes of 256 clouds), Tmax in {1, 300, 301, 1024} (M = B Tmax rows
    in GEMM tiles of 128: row tails), and ragged t_per_cloud that changes across the chunk boundaries (t_per_cloud + b0).
    The clouds around each chunk boundary and the last are held to float64 and are bitwise equal to the same cloud
    encoded alone.  Measured (MI355X): err(hip) 4.5e-7 ... 6.7e-7, err(f32 oracle) 2.3e-7 ... 4.2e-7 (max ratio 2.01: the
    GEMMs' MFMA accumulation order against the CPU's blocked sums; the bar is 4)."""
    import ifdefense_amd as I
    from oracle import onet_oracle as OO
    w_np = OO.make_random_weights(0)
    w32 = OO.to_torch(w_np)
    w64 = _w64(w32)
    clouds = _realistic_sel(_bench_clouds(600), 1024)
    r = I.OnetRestorer(I.weights.pack_state_dict(w_np, "onet"), device="cuda:0")
    try:
        g = np.random.default_rng(41)
        cases = [(1, 1, None), (255, 301, None), (256, 300, None), (257, 1024, None)]
        t600 = g.integers(1, 301, 600)
        t600[[0, 254, 255, 256, 257, 511, 512, 513, 599]] = [300, 1, 300, 1, 299, 7, 300, 2, 150]
        cases.append((600, 300, t600))
        for B, Tmax, tpc in cases:
            sel = clouds[:B, :Tmax].copy()
            if tpc is not None:
                for b in range(B):
                    sel[b, tpc[b]:] = 3.0                                      # padding is never read
            c = r.encode_inputs(torch.from_numpy(sel), None if tpc is None else torch.from_numpy(tpc)).cpu().numpy()
            check = sorted({b for b in (0, 254, 255, 256, 257, 511, 512, 513, B - 1) if b < B})
            ref64, ref32, got = [], [], []
            for b in check:
                t = Tmax if tpc is None else int(tpc[b])
                p = torch.from_numpy(sel[b:b + 1, :t].copy())
                alone = r.encode_inputs(p).cpu().numpy()
                assert np.array_equal(alone[0], c[b]), (B, Tmax, b)
                with torch.no_grad():
                    ref64.append(OO.encode_latent(w64, p.double())[0].numpy())
                    ref32.append(OO.encode_latent(w32, p)[0].numpy())
                got.append(c[b])
            _gate("ONet c, B %d Tmax %d%s, clouds %s" % (B, Tmax, " ragged" if tpc is not None else "", check),
                  np.stack(got), np.stack(ref32), np.stack(ref64), CAP_ONET)
    finally:
        r.close()
