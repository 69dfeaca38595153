"""CPU checks of the plain mesh reference (tests/mesh_plain.py) that the GPU tests of tests/test_gpu_mesh_grid.py rest on: it
equals the reference's own compiled MISE / marching-cubes libraries - live where oracle/_ref is built, and always through the
numbers recorded from them in tests/golden/mesh_hard_ref.npz - and the hard cases are as hard as they claim."""
import importlib.util
import os

import numpy as np
import pytest

import mesh_plain as MP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def recorded():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "mesh_hard_ref.npz")))


@pytest.fixture(scope="module")
def plain_mc_results():
    return {name: MP.plain_mc(grid, iso) for name, (grid, iso) in MP.mc_cases().items()}


@pytest.fixture(scope="module")
def plain_mise_results():
    return {(res0, depth, name): MP.plain_mise(MP.mise_field(name, res0, depth), res0, depth, 0.0)
            for res0, depth in MP.MISE_CONFIGS for name in MP.MISE_FIELDS}


def test_plain_reference_equals_the_live_reference_libraries(plain_mc_results, plain_mise_results):
    """Grids, rounds and points bit-identical; triangle count and order identical, vertices within 1e-12."""
    d = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.isdir(d) or not any(f.startswith("mise") for f in os.listdir(d)):
        pytest.skip("oracle/_ref not built (python oracle/build_ref.py needs the reference sources)")
    spec = importlib.util.spec_from_file_location("make_golden_mesh_hard", os.path.join(ROOT, "tests", "golden", "make_golden_mesh_hard.py"))
    live = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(live)
    import mcubes
    import mise
    for (res0, depth, name), (grid, rounds, points) in plain_mise_results.items():
        ref_grid, ref_rounds, ref_points = live.live_mise(mise, MP.mise_field(name, res0, depth), res0, depth, 0.0)
        assert np.array_equal(grid.astype(np.float64), ref_grid), (res0, depth, name)
        assert (rounds, points) == (ref_rounds, ref_points), (res0, depth, name)
    for name, (grid, iso) in MP.mc_cases().items():
        ref = live.live_mc(mcubes, grid, iso)
        assert plain_mc_results[name].shape == ref.shape, name
        if len(ref):
            np.testing.assert_allclose(plain_mc_results[name], ref, rtol=0, atol=1e-12, err_msg=name)


def test_plain_reference_matches_the_recorded_reference_numbers(recorded, plain_mc_results, plain_mise_results):
    """Without the libraries: triangle count, total area (the sum of ~1e5 areas agrees to 1e-12 relative when every vertex agrees
    to 1e-12 absolute and no triangle is missing or swapped for another), rounds, points, and the digest of the dense grid."""
    assert len(recorded) == 2 * len(plain_mc_results) + 3 * len(plain_mise_results)
    for name, tris in plain_mc_results.items():
        assert len(tris) == int(recorded["mc_%s_ntri" % name]), name
        area = float(recorded["mc_%s_area" % name])
        assert abs(MP.triangle_areas(tris).sum() - area) <= 1e-12 * max(area, 1.0), name
    for (res0, depth, name), (grid, rounds, points) in plain_mise_results.items():
        key = "mise_%d_%d_%s" % (res0, depth, name)
        assert rounds == int(recorded[key + "_rounds"]) and points == int(recorded[key + "_points"]), key
        assert MP.grid_digest(grid) == str(recorded[key + "_digest"]), key


def test_hard_cases_are_as_hard_as_they_claim(plain_mc_results, plain_mise_results):
    mc = MP.mc_cases()
    # all 256 sign configurations in INTERIOR cubes of the noise grid (no corner is padding)
    interior = MP.cube_configs(mc["noise13"][0], 0.0)[1:-1, 1:-1, 1:-1]
    assert len(np.unique(interior)) == 256
    print("noise13: %d of 256 configurations in interior cubes, %d in the padded grid"
          % (len(np.unique(interior)), len(np.unique(MP.cube_configs(mc["noise13"][0], 0.0)))))
    # values exactly on the iso-value, and the zero-area triangles they make
    assert int((mc["quant13"][0] == 0.0).sum()) >= 100
    assert int((MP.triangle_areas(plain_mc_results["quant13"]) == 0).sum()) > 0
    assert len(plain_mc_results["degenerate5"]) == 8 and (MP.triangle_areas(plain_mc_results["degenerate5"]) == 0).all()
    assert len(plain_mc_results["above4"]) == 0 and len(plain_mc_results["below4"]) == 0
    g = mc["special7"][0]
    assert (np.signbit(g) & (g == 0)).any() and (g == np.float32(3e38)).any() and (g == np.float32(-3e38)).any() and (g == -1e6).any()
    # cube counts on both sides of the 2048-cube scan chunk
    assert [(P + 1) ** 3 for P in (11, 12, 15, 16)] == [1728, 2197, 4096, 4913]
    # the slab grid has triangles at both ends of the cube order, and a modest number of them
    slab = plain_mc_results["slab129"]
    assert 1000 < len(slab) < 400000 and slab[0, :, 0].max() < -0.5 and slab[-1, :, 0].min() > 0.5
    # MISE: cascades beyond depth + 1 rounds, one-round cases, and a batch whose clouds finish in rounds 1 ... 4
    rounds = {k: v[1] for k, v in plain_mise_results.items()}
    assert any(r > depth + 1 for (res0, depth, name), r in rounds.items())
    assert any(r == 1 for (res0, depth, name), r in rounds.items() if depth > 0)
    assert {rounds[(3, 2, name)] for name in MP.MISE_FIELDS} >= {1, 3, 4}
    for res0, depth in MP.MISE_CONFIGS:
        if depth > 0:
            # the blob between the coarse points is missed, as the reference misses it
            grid, r, n = plain_mise_results[(res0, depth, "blob")]
            assert r == 1 and n == (res0 + 1) ** 3 and (grid == -1).all() and (MP.mise_field("blob", res0, depth) == 1).sum() == 1
        P = (res0 << depth) + 1
        assert plain_mise_results[(res0, depth, "equal")][2] == P ** 3           # ties make every voxel mixed


def test_existing_onet_field_reaches_a_fraction_of_the_table():
    """What the older mesh tests can reach: the occupancy field of the random-weight ONet decoder (float32 oracle) on the dense
    33^3 lattice, cut at its own median like tests/test_gpu_parity.py::_cutting_threshold does.  Printed for the record; the bar is
    only that it stays far from the whole table, which is why the grid seams exist."""
    import torch
    from oracle import onet_oracle as OO
    w = OO.to_torch(OO.make_random_weights(0))
    c = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "onet_golden.npz"))["c"][:1])
    g = torch.Generator().manual_seed(9)
    p = (torch.rand(1, 4096, 3, generator=g) - 0.5) * 1.1
    i = torch.arange(33, dtype=torch.float32)
    lattice = torch.stack(torch.meshgrid(i, i, i, indexing="ij"), -1).reshape(1, -1, 3)
    lattice = 1.1 * (lattice / 32 - 0.5)
    with torch.no_grad():
        med = float(OO.decode_logits(w, p, c).median())
        field = OO.decode_logits(w, lattice, c)[0].reshape(33, 33, 33).numpy()
    cfg = MP.cube_configs(field, med)
    n_all, n_in = len(np.unique(cfg)), len(np.unique(cfg[1:-1, 1:-1, 1:-1]))
    print("ONet random-weight field, 33^3, median threshold: %d of 256 configurations in the padded grid, %d in interior cubes"
          % (n_all, n_in))
    assert n_in <= n_all < 128


def test_sampler_helpers():
    # Philox-4x32-10 known answer (Random123 kat_vectors: zero counter, zero key)
    r = MP._philox4x32_10(0, 0, np.zeros(1), 0, 0, 0)
    assert [int(x[0]) for x in r] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    pick, u, v = MP.sampler_uniforms(11, 5, 1024)
    assert pick.dtype == np.float64 and u.dtype == np.float32 and (pick >= 0).all() and (pick < 1).all() and (u <= 1).all()
    assert 0.4 < pick.mean() < 0.6 and 0.4 < u.mean() < 0.6 and 0.4 < v.mean() < 0.6
    assert not np.array_equal(pick, MP.sampler_uniforms(11, 6, 1024)[0])
    # the exact pick: first index whose cumulative area exceeds the target - zero-area faces are never picked
    cum = np.cumsum([0.0, 1.0, 0.0, 0.0, 2.0, 0.0])
    face = MP.exact_face_pick(cum, np.array([0.0, 0.3, 1.0 / 3.0, 0.5, 0.999999]))
    assert face.tolist() == [1, 1, 4, 4, 4]
    assert MP.exact_face_pick(np.zeros(8), np.array([0.0, 0.7])).tolist() == [7, 7]
    tri = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], float)
    pts = MP.face_points(tri, np.array([0, 0]), np.array([0.25, 0.75], np.float32), np.array([0.5, 0.75], np.float32))
    np.testing.assert_array_equal(pts, [[0.25, 0.5, 0], [0.25, 0.25, 0]])
