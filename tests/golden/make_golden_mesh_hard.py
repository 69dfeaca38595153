#!/usr/bin/env python
"""Writes tests/golden/mesh_hard_ref.npz: what the reference's own compiled MISE and marching-cubes libraries (oracle/_ref, built
by oracle/build_ref.py) give on the hard cases of tests/mesh_plain.py - per marching-cubes case the triangle count and the total
area, per MISE case the round count, the points evaluated and a digest of the dense grid.  Recorded numbers only (the triangles of
the noise cases alone would be half a megabyte).  The only file of the mesh tests that needs oracle/_ref.

    python tests/golden/make_golden_mesh_hard.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref"))

import mesh_plain as MP  # noqa: E402


def live_mise(mise, field, res0, depth, thr):
    """The query / update loop around the reference's MISE class, values looked up in `field`: (dense grid, rounds, points)."""
    m = mise.MISE(res0, depth, thr)
    pts = m.query()
    rounds = points = 0
    while pts.shape[0] != 0:
        m.update(pts, field[pts[:, 0], pts[:, 1], pts[:, 2]].astype(np.float64))
        rounds += 1
        points += len(pts)
        pts = m.query()
    return m.to_dense(), rounds, points


def live_mc(mcubes, grid, iso, padding=0.1):
    """The reference's marching cubes on the padded grid, its cell-centre shift undone, in the decoder's frame: [n,3,3]."""
    v, t = mcubes.marching_cubes(np.pad(np.asarray(grid, np.float64), 1, "constant", constant_values=MP.PAD_VALUE), iso)
    if len(t) == 0:
        return np.zeros((0, 3, 3))
    return MP.to_frame(v - 0.5, grid.shape[0], padding)[t.astype(np.int64)]


def main():
    import mcubes
    import mise
    out = {}
    for name, (grid, iso) in MP.mc_cases().items():
        tris = live_mc(mcubes, grid, iso)
        out["mc_%s_ntri" % name] = np.int64(len(tris))
        out["mc_%s_area" % name] = np.float64(MP.triangle_areas(tris).sum())
    for res0, depth in MP.MISE_CONFIGS:
        for name in MP.MISE_FIELDS:
            grid, rounds, points = live_mise(mise, MP.mise_field(name, res0, depth), res0, depth, 0.0)
            key = "mise_%d_%d_%s" % (res0, depth, name)
            out[key + "_rounds"], out[key + "_points"] = np.int64(rounds), np.int64(points)
            out[key + "_digest"] = np.array(MP.grid_digest(grid))
    np.savez(os.path.join(HERE, "mesh_hard_ref.npz"), **out)
    print("wrote mesh_hard_ref.npz: %d entries" % len(out))


if __name__ == "__main__":
    main()
