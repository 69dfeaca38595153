"""The kernels of csrc/mesh.hip on caller-supplied arrays, through the validation seams ifd_mesh_from_grid / ifd_mise_from_field:
all 256 cube configurations, values on the iso-value, special values, cube counts around the scan chunk, a 129^3 grid with
triangles at both ends of the cube order, tiny triangle capacities, degenerate and empty meshes, MISE cascades and ties.

Every expected value comes from tests/mesh_plain.py (numpy, float64), which tests/test_mesh_cpu.py holds to the reference's own
libraries; nothing here needs oracle/_ref.  Bars:
  vertices   2^-24 absolute: the kernel forms a vertex in double and rounds it to float32; coordinates stay below 1, so half an
             ulp is at most 2^-25, and the bar is twice that.
  cum_area   n 2^-52 relative to the float64 running sum of the plain triangles' areas (n = triangles summed): the kernel's scan
             adds the same double areas in blocked order instead of sequentially.
  samples    4 * 2^-24 absolute against the float64 formula on the GPU's own float32 triangles (float32 evaluation with FMA
             contraction), on exactly the face the exact pick gives from the GPU's own cum_area and the regenerated uniforms.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mesh_plain as MP

pytestmark = pytest.mark.gpu

VERTEX_TOL = 2.0 ** -24
SAMPLE_TOL = 4 * 2.0 ** -24
T_FILL, A_FILL, P_FILL = -7.5, -3.0, 9.25          # what the output arrays hold before a call: untouched rows still do afterwards


@pytest.fixture(scope="module")
def onet():
    import ifdefense_amd as I
    r = I.OnetRestorer(I.weights.pack_state_dict(I.weights.onet_random_state_dict(0), "onet"), device="cuda:0")
    yield r
    r.close()


_PLAIN = {}


def plain_tris(grid, iso):
    """plain_mc, computed once per (grid, iso) and never modified"""
    key = (grid.shape, grid.tobytes(), float(iso))
    if key not in _PLAIN:
        t = MP.plain_mc(grid, iso)
        t.setflags(write=False)
        _PLAIN[key] = t
    return _PLAIN[key]


def run_mc(onet, grids, iso=0.0, cap=None, n_sample=1024, seed=3, base=0):
    """mesh_from_grid on a batch of equally sized grids, every output array pre-filled; numpy results."""
    g = torch.from_numpy(np.stack(grids))
    B = len(grids)
    if cap is None:
        cap = max(1, max(len(plain_tris(x, iso)) for x in grids))
    dev = onet.device
    out = onet.mesh_from_grid(g, iso=iso, max_triangles=cap, n_sample=n_sample, seed=seed, cloud_index_base=base,
                              points=torch.full((B, n_sample, 3), P_FILL, device=dev),
                              triangles=torch.full((B, cap, 9), T_FILL, device=dev),
                              cum_area=torch.full((B, cap), A_FILL, device=dev, dtype=torch.float64))
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_mc(out, b, grid, iso, cap, tag):
    """count, triangles in order and winding, cum_area, untouched rows - of cloud b against the plain reference"""
    ref = plain_tris(grid, iso)
    n = int(out["n_triangles"][b])
    assert n == len(ref), (tag, n, len(ref))                                   # the UNCAPPED total
    nv = min(n, cap)
    tris = out["triangles"][b].reshape(cap, 3, 3)
    cum = out["cum_area"][b]
    assert (tris[nv:] == T_FILL).all() and (cum[nv:] == A_FILL).all(), tag     # rows past the count are untouched
    if nv == 0:
        return
    dv = np.abs(tris[:nv].astype(np.float64) - ref[:nv]).max()
    ref_cum = np.cumsum(MP.triangle_areas(ref[:nv]))
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref_cum > 0, np.abs(cum[:nv] - ref_cum) / ref_cum, np.where(cum[:nv] == 0, 0.0, np.inf))
    print("%s: %d triangles (%d held), max vertex error %.3g (bar %.3g), max cum_area error %.3g (bar %.3g)"
          % (tag, n, nv, dv, VERTEX_TOL, rel.max(), nv * 2.0 ** -52))
    assert dv <= VERTEX_TOL, (tag, dv)
    assert rel.max() <= nv * 2.0 ** -52, (tag, rel.max(), int(rel.argmax()))


def check_samples(out, b, cap, n_sample, seed, base, tag):
    """every sample of cloud b is the float64 formula's point on exactly the face the exact pick gives"""
    nv = min(int(out["n_triangles"][b]), cap)
    pick, u, v = MP.sampler_uniforms(seed, base + b, n_sample)
    face = MP.exact_face_pick(out["cum_area"][b][:nv], pick)
    want = MP.face_points(out["triangles"][b][:nv], face, u, v)
    d = np.abs(out["points"][b].astype(np.float64) - want).max(axis=1)
    print("%s: %d samples, max distance to the exact pick's point %.3g (bar %.3g), %d off" % (tag, n_sample, d.max(), SAMPLE_TOL, (d > SAMPLE_TOL).sum()))
    assert (d <= SAMPLE_TOL).all(), (tag, int((d > SAMPLE_TOL).sum()), d.max())
    return face


# ------------------------------------------------------------------------------------------------
# marching cubes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise13", "noise5", "noise9", "quant13", "special7", "noise2", "noise3", "noise11", "noise12",
                                  "noise15", "noise16"])
def test_marching_cubes_on_hard_grids(onet, name):
    """noise13 holds all 256 configurations in interior cubes; quant13 has corners on the iso-value (inside: zero-area triangles);
    special7 -0.0, +-3e38 and padding-valued entries; P = 2, 3 the smallest grids; 11, 12, 15, 16 have 1728, 2197, 4096 and 4913
    cubes, around the 2048-cube scan chunk.  Each as a batch of the grid and its negation."""
    grid, iso = MP.mc_cases()[name]
    grids = [grid, -grid]
    cap = max(len(plain_tris(g, iso)) for g in grids) + 3
    out = run_mc(onet, grids, iso, cap)
    for b, g in enumerate(grids):
        check_mc(out, b, g, iso, cap, "%s[%d]" % (name, b))
        check_samples(out, b, cap, 1024, 3, 0, "%s[%d]" % (name, b))


def test_marching_cubes_129_with_triangles_at_both_ends(onet):
    """constant but for noisy slabs in the first two and the last two x-layers: a carry lost in either offset scan moves the
    triangles at the far end"""
    grid, iso = MP.mc_cases()["slab129"]
    cap = len(plain_tris(grid, iso)) + 1000
    out = run_mc(onet, [grid], iso, cap, seed=(7 << 32) | 11, base=5)
    check_mc(out, 0, grid, iso, cap, "slab129")
    face = check_samples(out, 0, cap, 1024, (7 << 32) | 11, 5, "slab129")
    n = int(out["n_triangles"][0])
    assert face.min() < n // 4 and face.max() > 3 * n // 4                     # samples at both ends of the cube order


def test_a_cloud_is_the_same_alone_in_a_batch_and_at_another_index(onet):
    mc = MP.mc_cases()
    grids = [mc["quant13"][0], -mc["noise13"][0], MP.noise_grid(13, 501), mc["noise13"][0], MP.noise_grid(13, 502)]
    cap = max(len(plain_tris(g, 0.0)) for g in grids) + 1
    batch = run_mc(onet, grids, 0.0, cap, seed=9, base=20)
    for b in (0, 3, 4):
        alone = run_mc(onet, [grids[b]], 0.0, cap, seed=9, base=20 + b)         # the same GLOBAL index: the samples too
        moved = run_mc(onet, [grids[b]], 0.0, cap, seed=9, base=1000)
        for k in ("n_triangles", "triangles", "cum_area"):
            assert np.array_equal(alone[k][0], batch[k][b]) and np.array_equal(moved[k][0], batch[k][b]), (b, k)
        assert np.array_equal(alone["points"][0].view(np.uint32), batch["points"][b].view(np.uint32)), b
        assert not np.array_equal(moved["points"][0], batch["points"][b]), b
    # (seed, global index) alone decide the draws: the same cloud at two places of two batches
    again = run_mc(onet, [grids[1], grids[3]], 0.0, cap, seed=9, base=22)
    assert np.array_equal(again["points"][1].view(np.uint32), batch["points"][3].view(np.uint32))


# ------------------------------------------------------------------------------------------------
# capacities
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cap", [("slab129", 536), ("slab129", 100), ("noise16", 1), ("noise13", None)])
def test_triangle_capacity_below_the_count(onet, name, cap):
    """536 for 129^3 (1073 chunks > 2 * 536) and 1 for 16^3 (3 chunks > 2) take the one-block offset scan; half the true count on
    13^3 truncates behind the chunked scan.  n_triangles stays the uncapped total, the triangles held are the reference's first,
    and every sample lies on one of those."""
    grid, iso = MP.mc_cases()[name]
    n = len(plain_tris(grid, iso))
    cap = n // 2 if cap is None else cap
    assert cap < n
    out = run_mc(onet, [grid], iso, cap, seed=4, base=2)
    check_mc(out, 0, grid, iso, cap, "%s cap %d" % (name, cap))
    face = check_samples(out, 0, cap, 1024, 4, 2, "%s cap %d" % (name, cap))
    assert face.max() < cap


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
def test_sampler_never_picks_a_zero_area_face(onet):
    grid, iso = MP.mc_cases()["quant13"]
    cap = len(plain_tris(grid, iso))
    out = run_mc(onet, [grid], iso, cap, n_sample=4096, seed=21)
    face = check_samples(out, 0, cap, 4096, 21, 0, "quant13")
    cum = out["cum_area"][0]
    step = np.diff(np.concatenate([[0.0], cum]))
    assert (step == 0).sum() > 1000 and (step[face] > 0).all()


def test_all_degenerate_mesh(onet):
    """one interior point exactly on the iso-value, everything else (the padding included) above: 8 triangles of zero area, and
    every sample is that grid point"""
    grid, iso = MP.mc_cases()["degenerate5"]
    out = run_mc(onet, [grid], iso, 16, n_sample=256)
    check_mc(out, 0, grid, iso, 16, "degenerate5")
    assert int(out["n_triangles"][0]) == 8 and (out["cum_area"][0][:8] == 0).all()
    point = MP.to_frame(np.array([2.0, 1.0, 3.0]) + 1.0, 5, 0.1)
    pts = out["points"][0]
    assert np.isfinite(pts).all() and np.abs(pts - point).max() <= VERTEX_TOL
    assert (pts == out["triangles"][0][0][:3]).all()


def test_empty_meshes_leave_their_rows_untouched(onet):
    """all below the iso-value, and all above it (the -1e6 padding too: an iso-value below it - at iso 0 an all-above grid has the
    box boundary for a surface)"""
    for name in ("below4", "above4"):
        grid, iso = MP.mc_cases()[name]
        out = run_mc(onet, [grid, grid], iso, 8)
        assert (out["n_triangles"] == 0).all() and (out["points"] == P_FILL).all() and (out["triangles"] == T_FILL).all(), name
    # an empty cloud beside a full one
    full = MP.noise_grid(4, 41)
    out = run_mc(onet, [MP.mc_cases()["below4"][0], full], 0.0, 600)
    assert int(out["n_triangles"][0]) == 0 and (out["points"][0] == P_FILL).all()
    check_mc(out, 1, full, 0.0, 600, "noise4 beside an empty cloud")
    check_samples(out, 1, 600, 1024, 3, 0, "noise4 beside an empty cloud")


# ------------------------------------------------------------------------------------------------
# MISE
# ------------------------------------------------------------------------------------------------
_MISE = {}


def plain_mise(res0, depth, name):
    if (res0, depth, name) not in _MISE:
        _MISE[(res0, depth, name)] = MP.plain_mise(MP.mise_field(name, res0, depth), res0, depth, 0.0)
    return _MISE[(res0, depth, name)]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("res0,depth", MP.MISE_CONFIGS)
def test_mise_on_hard_fields(onet, res0, depth):
    """sphere, a blob between the coarse points (missed in one round, like the reference), noise, quantised noise (ties), all on
    the threshold, a step whose zero plane lies on lattice points, a thin tilted sheet (cascades), all above: dense grid
    bit-identical to the plain reference, rounds and points of the call equal; all eight in one batch - its clouds finish in
    different rounds - give per cloud the same bits as each alone, which also runs every cloud after a larger call."""
    fields = [MP.mise_field(name, res0, depth) for name in MP.MISE_FIELDS]
    ref = [plain_mise(res0, depth, name) for name in MP.MISE_FIELDS]
    out = onet.mise_from_field(torch.from_numpy(np.stack(fields)), res0, depth, 0.0)
    grids = out["grid"].cpu().numpy()
    print("MISE (%d, %d): rounds per field %s, batch %d rounds %d points" % (res0, depth, [r[1] for r in ref], out["rounds"], out["points"]))
    for b, name in enumerate(MP.MISE_FIELDS):
        assert same_bits(grids[b], ref[b][0]), (name, int((grids[b] != ref[b][0]).sum()))
    assert out["rounds"] == max(r[1] for r in ref) and out["points"] == sum(r[2] for r in ref)
    for b, name in enumerate(MP.MISE_FIELDS):
        alone = onet.mise_from_field(torch.from_numpy(fields[b][None]), res0, depth, 0.0)
        assert same_bits(alone["grid"].cpu().numpy()[0], grids[b]), name
        assert (alone["rounds"], alone["points"]) == ref[b][1:], (name, alone["rounds"], alone["points"], ref[b][1:])


def test_mise_small_call_after_a_larger_one_reads_no_stale_workspace(onet):
    big = onet.mise_from_field(torch.from_numpy(np.stack([MP.mise_field("noise", 8, 2)] * 3)), 8, 2, 0.0)
    assert big["points"] == 3 * 33 ** 3
    for res0, depth in ((2, 2), (4, 1)):
        for name in ("sphere", "sheet", "above", "blob"):
            out = onet.mise_from_field(torch.from_numpy(MP.mise_field(name, res0, depth)[None]), res0, depth, 0.0)
            ref = plain_mise(res0, depth, name)
            assert same_bits(out["grid"].cpu().numpy()[0], ref[0]) and (out["rounds"], out["points"]) == ref[1:], (res0, depth, name)


def test_mise_then_marching_cubes_end_to_end(onet):
    field = MP.mise_field("sphere", 8, 2)
    grid = onet.mise_from_field(torch.from_numpy(field[None]), 8, 2, 0.0)["grid"]
    ref_grid = plain_mise(8, 2, "sphere")[0]
    assert same_bits(grid.cpu().numpy()[0], ref_grid)
    ref = plain_tris(ref_grid, 0.0)
    cap = len(ref) + 5
    dev = onet.device
    out = onet.mesh_from_grid(grid, iso=0.0, max_triangles=cap, seed=3, points=torch.full((1, 1024, 3), P_FILL, device=dev),
                              triangles=torch.full((1, cap, 9), T_FILL, device=dev),
                              cum_area=torch.full((1, cap), A_FILL, device=dev, dtype=torch.float64))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert len(ref) > 500
    check_mc(out, 0, ref_grid, 0.0, cap, "sphere (8, 2)")
    check_samples(out, 0, cap, 1024, 3, 0, "sphere (8, 2)")


# ------------------------------------------------------------------------------------------------
# arguments, and the driver's answer to a truncated mesh
# ------------------------------------------------------------------------------------------------
def test_seams_refuse_bad_arguments(onet):
    import ifdefense_amd as I
    lib, ctx, dev = onet.lib, onet.ctx, onet.device
    g = torch.zeros(1, 5, 5, 5, device=dev)
    pts = torch.full((1, 16, 3), P_FILL, device=dev)
    nt = torch.full((1,), -5, device=dev, dtype=torch.int32)
    out = torch.full((1, 5, 5, 5), P_FILL, device=dev)

    def mesh(ctx_=ctx, grid=g.data_ptr(), B=1, P=5, cap=8, n=16, points=pts.data_ptr(), ntri=nt.data_ptr()):
        return lib.ifd_mesh_from_grid(ctx_, grid, B, P, 0.0, 0.1, cap, n, 0, 0, points, ntri, None, None, None)

    def mise(ctx_=ctx, field=g.data_ptr(), B=1, P=5, res0=2, steps=1, grid=out.data_ptr()):
        return lib.ifd_mise_from_field(ctx_, field, B, P, res0, steps, 0.0, grid, None)

    assert mesh() == 0 and mise() == 0                                          # the good calls these are variations of
    torch.cuda.synchronize()
    pts.fill_(P_FILL), nt.fill_(-5), out.fill_(P_FILL)
    bad = [mesh(P=1), mesh(P=130), mesh(cap=0), mesh(cap=-1), mesh(grid=None), mesh(points=None), mesh(ntri=None), mesh(B=0), mesh(n=0),
           mesh(ctx_=None), mise(P=1), mise(P=6), mise(res0=4, steps=1), mise(res0=1, steps=2), mise(steps=3, res0=1, P=9), mise(steps=-1),
           mise(P=257, res0=64, steps=2), mise(field=None), mise(grid=None), mise(B=0), mise(ctx_=None)]
    assert bad == [-1] * len(bad), bad
    conv = I.Restorer(I.weights.pack_state_dict(I.weights.random_state_dict(0)), device="cuda:0")
    try:
        assert mesh(ctx_=conv.ctx) == -1 and b"not an ONet context" in lib.ifd_last_error(conv.ctx)
        assert mise(ctx_=conv.ctx) == -1 and b"not an ONet context" in lib.ifd_last_error(conv.ctx)
    finally:
        conv.close()
    torch.cuda.synchronize()
    assert (pts == P_FILL).all() and (nt == -5).all() and (out == P_FILL).all()   # no refused call wrote anything
    with pytest.raises(I.IfdError):
        onet.mesh_from_grid(torch.zeros(1, 130, 130, 130), max_triangles=8)


def test_driver_does_not_return_samples_of_a_truncated_mesh(onet):
    """remesh_point_cloud with a triangle capacity below the clouds' counts == the run whose capacity suffices, bit for bit: the
    clouds whose n_triangles exceeds the capacity are meshed again with room for every triangle."""
    import bench
    import ifdefense_amd as I
    clouds = bench.synth_clouds(2)
    calls = []
    real = onet.mesh_sample

    def spy(*a, **k):
        res = real(*a, **k)
        calls.append((k.get("max_triangles"), res["n_triangles"].cpu().tolist()))
        return res

    full = I.remesh_point_cloud(onet, clouds, I.DefenseArgs(input_npoint=300, seed=4), cloud_index_base=7)
    onet.mesh_sample = spy
    try:
        small = I.remesh_point_cloud(onet, clouds, I.DefenseArgs(input_npoint=300, seed=4, max_triangles=1000), cloud_index_base=7)
    finally:
        del onet.mesh_sample
    print("driver: mesh_sample calls (capacity, n_triangles):", calls)
    assert len(calls) == 3 and calls[0][0] == 1000 and min(calls[0][1]) > 1000         # both clouds were truncated and meshed again
    assert [c[0] for c in calls[1:]] == calls[0][1] and [c[1][0] for c in calls[1:]] == calls[0][1]
    assert np.array_equal(small.view(np.uint32), full.view(np.uint32))
