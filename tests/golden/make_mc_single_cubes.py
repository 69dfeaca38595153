#!/usr/bin/env python
"""Generate tests/golden/mc_single_cubes_ref.npz: the triangles the REFERENCE's own libmcubes (ONet/im2mesh/utils/libmcubes,
compiled into oracle/_ref by oracle/build_ref.py) makes of the single-cube cases of
tests/test_abi_cpu.py::test_marching_cubes_single_cubes_against_live_reference_library - every sign configuration x three
seeded draws of corner values.  The .npz is data: the corner values, the reference's triangle count per case and its triangles,
so the test holds the HIP path's table against the reference where the library cannot be built.

    python oracle/build_ref.py && python tests/golden/make_mc_single_cubes.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "_ref"))
import mcubes  # noqa: E402
import test_abi_cpu as T  # noqa: E402


def main():
    vals, counts, tris = [], [], []
    for _, val, grid in T._single_cube_cases():
        t = T._ref_single_cube_triangles(mcubes, grid)
        vals.append(val)
        counts.append(len(t))
        tris.append(t)
    out = os.path.join(HERE, "mc_single_cubes_ref.npz")
    np.savez_compressed(out, val=np.array(vals), ntri=np.array(counts, np.int32), tris=np.concatenate(tris).astype(np.float64))
    print("wrote %s: %d cases, %d triangles" % (out, len(counts), sum(counts)))


if __name__ == "__main__":
    main()
