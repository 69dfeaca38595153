"""A plain numpy / float64 statement of the ONet-Mesh path - TEST INFRASTRUCTURE for the kernels of csrc/mesh.hip.

Written from the algorithm as the header comments of csrc/mesh.hip and include/ifd.h describe it, not from any program text:

  plain_mise   multi-resolution iso-surface extraction on a caller's dense field (what ifd_mise_from_field computes)
  plain_mc     marching cubes of the -1e6-padded grid with the recorded polygonisation table (tests/golden/mc_table_ref.npz),
               in the decoder's frame (what ifd_mesh_from_grid emits)
  the sampler  Philox-4x32-10 draws keyed by (seed, global cloud index, sample index), the exact area-weighted face pick and
               the point of the face

and the hard input families the CPU and GPU tests share (mc_cases, mise_cases): the GPU tests take every expected value from
here, tests/test_mesh_cpu.py holds this module to the reference's own compiled libraries (live where oracle/_ref is built, and
always through the recorded numbers of tests/golden/mesh_hard_ref.npz).
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD_VALUE = -1e6

# corner / edge numbering of csrc/mesh.hip (= libmcubes = Bourke): corners 0..3 = (0,0,0) (1,0,0) (1,1,0) (0,1,0), 4..7 at z + 1
CORNER = np.array([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)], np.int64)
EDGE = np.array([(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)], np.int64)

_TABLE = None


def mc_table():
    """(tri [256,16] int8, ntri [256] uint8): the recorded polygonisation table."""
    global _TABLE
    if _TABLE is None:
        z = np.load(os.path.join(GOLDEN, "mc_table_ref.npz"))
        _TABLE = (z["tri"].copy(), z["ntri"].copy())
    return _TABLE


# ------------------------------------------------------------------------------------------------
# MISE
# ------------------------------------------------------------------------------------------------
def _closed_cube_any(a: np.ndarray, s: int, nv: int) -> np.ndarray:
    """any() of the boolean lattice array a [P,P,P] over the closed cube [v s, v s + s]^3 of every voxel v: [nv,nv,nv]."""
    for axis in range(3):
        span = (nv - 1) * s + 1
        out = None
        for o in range(s + 1):
            sl = [slice(None)] * 3
            sl[axis] = slice(o, o + span, s)
            part = a[tuple(sl)]
            out = part.copy() if out is None else (out | part)
        a = out
    return a


def plain_mise(field: np.ndarray, res0: int, depth: int, thr: float):
    """MISE on a dense field [P,P,P] (P = (res0 << depth) + 1) whose value at a lattice point is what an evaluation returns.
    -> (dense grid float32 [P,P,P], rounds, points evaluated).

    The coarse lattice is pending.  Each round evaluates the pending points; then, from the state at that moment, every level
    < depth marks its leaf voxels (not subdivided, parent subdivided) whose KNOWN points of the closed cube lie on both sides of
    the threshold (>= and <=, compared in float64, so one point exactly on it is both); the marked voxels are subdivided and the
    not-known, not-pending points of their 27-point half lattice become pending.  Ends when nothing is pending; unknown entries
    then take the value of their predecessor along x, then y, then z."""
    field = np.asarray(field, np.float32)
    P = (res0 << depth) + 1
    assert field.shape == (P, P, P)
    val = np.zeros((P, P, P), np.float32)
    known = np.zeros((P, P, P), bool)
    pend = np.zeros((P, P, P), bool)
    s0 = 1 << depth
    pend[::s0, ::s0, ::s0] = True
    sub = [np.zeros((res0 << l,) * 3, bool) for l in range(depth)]
    rounds = points = 0
    while pend.any():
        val[pend] = field[pend]
        known |= pend
        points += int(pend.sum())
        pend[:] = False
        rounds += 1
        f = val.astype(np.float64)
        pos, neg = known & (f >= thr), known & (f <= thr)
        marks = []
        for l in range(depth):
            nv, s = res0 << l, 1 << (depth - l)
            leaf = ~sub[l]
            if l > 0:
                leaf &= np.repeat(np.repeat(np.repeat(sub[l - 1], 2, 0), 2, 1), 2, 2)
            marks.append(leaf & _closed_cube_any(pos, s, nv) & _closed_cube_any(neg, s, nv))
        for l in range(depth):
            s = 1 << (depth - l)
            h = s >> 1
            sub[l] |= marks[l]
            vx, vy, vz = np.nonzero(marks[l])
            for a in range(3):
                for b in range(3):
                    for c in range(3):
                        ix, iy, iz = vx * s + a * h, vy * s + b * h, vz * s + c * h
                        new = ~known[ix, iy, iz]
                        pend[ix[new], iy[new], iz[new]] = True
    for axis in range(3):                                     # to_dense
        v, k = np.moveaxis(val, axis, 0), np.moveaxis(known, axis, 0)
        for i in range(1, P):
            take = ~k[i] & k[i - 1]
            v[i][take] = v[i - 1][take]
            k[i] |= take
    assert known.all()
    return val, rounds, points


# ------------------------------------------------------------------------------------------------
# marching cubes
# ------------------------------------------------------------------------------------------------
def box_size(padding: float) -> float:
    """include/ifd.h: the padding is a float32 and box_size = 1 + padding is formed in float32."""
    return float(np.float32(1.0) + np.float32(padding))


def to_frame(g: np.ndarray, P: int, padding: float) -> np.ndarray:
    """Padded-grid coordinates (cube index + corner offset + crossing) -> the decoder's frame: padding undone, normalised to the
    bounding box (include/ifd.h, ifd_onet_mesh_sample)."""
    return box_size(padding) * ((g - 1.0) / float(P - 1) - 0.5)


def cube_configs(grid: np.ndarray, iso: float) -> np.ndarray:
    """Sign configuration of every cube of the padded grid, [P+1,P+1,P+1] uint8 (bit m set: corner m <= iso, i.e. inside)."""
    pad = np.pad(np.asarray(grid, np.float64), 1, "constant", constant_values=PAD_VALUE)
    n = pad.shape[0] - 1
    inside = pad <= iso
    cfg = np.zeros((n, n, n), np.uint8)
    for m, (ox, oy, oz) in enumerate(CORNER):
        cfg |= inside[ox:ox + n, oy:oy + n, oz:oz + n].astype(np.uint8) << np.uint8(m)
    return cfg


def plain_mc(grid: np.ndarray, iso: float, padding: float = 0.1) -> np.ndarray:
    """Marching cubes of grid [P,P,P] padded with -1e6 -> triangles [n,3,3] float64 in the decoder's frame: cubes in x-major
    order, a corner inside when its value <= iso, the triangles of a cube in the table's order and winding, vertices at the linear
    crossings of the cube edges."""
    tri, ntri = mc_table()
    grid = np.asarray(grid, np.float64)
    P = grid.shape[0]
    pad = np.pad(grid, 1, "constant", constant_values=PAD_VALUE)
    cfg = cube_configs(grid, iso)
    n = P + 1
    flat = cfg.reshape(-1)
    keys, verts = [], []
    for c in np.unique(flat):
        if ntri[c] == 0:
            continue
        cube = np.nonzero(flat == c)[0]
        xyz = np.stack([cube // (n * n), (cube // n) % n, cube % n], 1)
        f = np.stack([pad[xyz[:, 0] + ox, xyz[:, 1] + oy, xyz[:, 2] + oz] for ox, oy, oz in CORNER], 1)      # [cubes, 8]
        for t in range(int(ntri[c])):
            tv = np.empty((len(cube), 3, 3))
            for k in range(3):
                a, b = EDGE[tri[c, 3 * t + k]]
                fa, fb = f[:, a], f[:, b]
                with np.errstate(divide="ignore", invalid="ignore"):
                    w = np.where(fb == fa, 0.5, (iso - fa) / (fb - fa))
                g = (xyz + CORNER[a])[:, :] + (CORNER[b] - CORNER[a])[None, :] * w[:, None]
                tv[:, k] = to_frame(g, P, padding)
            keys.append(cube * 8 + t)
            verts.append(tv)
    if not keys:
        return np.zeros((0, 3, 3))
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(verts)[order]


def triangle_areas(tris: np.ndarray) -> np.ndarray:
    """half the norm of the cross product of the two edge vectors at vertex 0, every operation rounded on its own"""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    u, v = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    cx = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
    cy = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
    cz = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
    return 0.5 * np.sqrt(cx * cx + cy * cy + cz * cz)


# ------------------------------------------------------------------------------------------------
# the sampler
# ------------------------------------------------------------------------------------------------
def _philox4x32_10(k0, k1, c0, c1, c2, c3):
    """Philox-4x32-10 (Salmon et al. 2011) on uint32 numpy arrays - the generator of prep.hip / mesh.hip."""
    k0, k1 = np.uint64(k0), np.uint64(k1)
    c = [np.asarray(x, np.uint64) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    M = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & M, p1 & M, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & M, p0 & M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return c


def sampler_uniforms(seed: int, cloud_index: int, n: int):
    """The three uniforms of samples 0 .. n-1 of the cloud with this GLOBAL index: (pick float64 in [0,1), u, v float32)."""
    r = _philox4x32_10(seed & 0xffffffff, (seed >> 32) & 0xffffffff, np.arange(n), 0x5a3f, cloud_index & 0xffffffff, 0)
    pick = (r[0].astype(np.float64) + r[1].astype(np.float64) * 4294967296.0) * (1.0 / 18446744073709551616.0)
    scale = np.float32(1.0 / 4294967296.0)
    return pick, r[2].astype(np.float32) * scale, r[3].astype(np.float32) * scale


def exact_face_pick(cum: np.ndarray, pick: np.ndarray) -> np.ndarray:
    """The first index whose cumulative area exceeds pick * cum[-1] (the last face if none does: an all-degenerate mesh)."""
    cum = np.asarray(cum, np.float64)
    face = np.searchsorted(cum, np.asarray(pick, np.float64) * cum[-1], side="right")
    return np.minimum(face, len(cum) - 1)


def face_points(tris: np.ndarray, face: np.ndarray, u: np.ndarray, v: np.ndarray) -> np.ndarray:
    """The point of triangle `face` at the two float32 uniforms, reflected into the triangle where their (float32) sum exceeds
    one; evaluated in float64 on the given triangles [n,3,3]."""
    u, v = np.asarray(u, np.float32).copy(), np.asarray(v, np.float32).copy()
    flip = (u + v) > np.float32(1.0)
    u[flip], v[flip] = np.float32(1.0) - u[flip], np.float32(1.0) - v[flip]
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)[face]
    return t[:, 0] + u.astype(np.float64)[:, None] * (t[:, 1] - t[:, 0]) + v.astype(np.float64)[:, None] * (t[:, 2] - t[:, 0])


# ------------------------------------------------------------------------------------------------
# the hard cases
# ------------------------------------------------------------------------------------------------
NOISE13_SEED = 0        # the first seed whose 13^3 grid shows all 256 configurations in interior cubes (test_mesh_cpu.py asserts it)


def noise_grid(P: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (P, P, P)).astype(np.float32)


def quantised(g: np.ndarray) -> np.ndarray:
    """values in {-1, -0.5, 0, 0.5, 1}"""
    return (np.round(g * 2.0) / 2.0).astype(np.float32)


def slab_grid(P: int = 129, seed: int = 5) -> np.ndarray:
    """constant (inside, like the padding: no surface of its own) except for noise in the first two and the last two x-layers"""
    g = np.full((P, P, P), -1.0, np.float32)
    rng = np.random.default_rng(seed)
    g[:2] = rng.uniform(-1.0, 1.0, (2, P, P)).astype(np.float32)
    g[-2:] = rng.uniform(-1.0, 1.0, (2, P, P)).astype(np.float32)
    return g


def special_grid() -> np.ndarray:
    """noise 7^3 sprinkled with -0.0 (on the iso-value 0: inside), +-3e38 and values equal to the padding"""
    g = noise_grid(7, 77)
    rng = np.random.default_rng(78)
    where = rng.permutation(7 ** 3)[:120]
    g.reshape(-1)[where] = np.resize(np.array([-0.0, 3e38, -3e38, -1e6], np.float32), 120)
    return g


DEGENERATE_ISO = -2e6


def degenerate_grid() -> np.ndarray:
    """above the iso-value everywhere - the -1e6 padding included, hence an iso-value below it - but for one interior point exactly
    on it: 8 triangles, all of zero area, all at that point"""
    g = np.zeros((5, 5, 5), np.float32)
    g[2, 1, 3] = DEGENERATE_ISO
    return g


def mc_cases():
    """name -> (grid [P,P,P] float32, iso): every marching-cubes input of the GPU tests."""
    out = {
        "noise13": (noise_grid(13, NOISE13_SEED), 0.0),
        "noise5": (noise_grid(5, 105), 0.0),
        "noise9": (noise_grid(9, 109), 0.0),
        "quant13": (quantised(noise_grid(13, 213)), 0.0),
        "special7": (special_grid(), 0.0),
        "degenerate5": (degenerate_grid(), DEGENERATE_ISO),
        # all above: the padding must be above too, or the box boundary is a surface
        "above4": (np.ones((4, 4, 4), np.float32), -2e6),
        "below4": (-np.ones((4, 4, 4), np.float32), 0.0),
        "slab129": (slab_grid(), 0.0),
    }
    for P in (2, 3, 11, 12, 15, 16):
        out["noise%d" % P] = (noise_grid(P, 300 + P), 0.0)
    return out


MISE_CONFIGS = ((2, 2), (3, 2), (4, 1), (4, 2), (8, 0), (8, 2))
MISE_FIELDS = ("sphere", "blob", "noise", "quant", "equal", "step", "sheet", "above")


def mise_field(name: str, res0: int, depth: int) -> np.ndarray:
    """The field `name` on the (res0 << depth) + 1 lattice, threshold 0."""
    P = (res0 << depth) + 1
    s = 1 << depth
    i = np.arange(P, dtype=np.float64)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    t = [a / (P - 1) for a in (x, y, z)]
    if name == "sphere":
        f = 0.31 - np.sqrt((t[0] - 0.47) ** 2 + (t[1] - 0.52) ** 2 + (t[2] - 0.45) ** 2)
    elif name == "blob":                    # smaller than a coarse cell, between the coarse points: missed, in one round
        f = -np.ones((P, P, P))
        if s > 1:
            f[s // 2, s + s // 2, s // 2] = 1.0
    elif name == "noise":
        f = noise_grid(P, 1000 + 10 * res0 + depth)
    elif name == "quant":
        f = quantised(noise_grid(P, 2000 + 10 * res0 + depth))
    elif name == "equal":
        f = np.zeros((P, P, P))
    elif name == "step":                    # the zero plane lies on lattice points
        f = np.sign(x - (P - 1) // 2)
    elif name == "sheet":                   # thin and tilted
        f = np.abs(t[0] + 0.37 * t[1] + 0.19 * t[2] - 0.8) - 0.02
    elif name == "above":
        f = np.ones((P, P, P))
    else:
        raise KeyError(name)
    return np.ascontiguousarray(f, np.float32)


def grid_digest(grid: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(grid, np.float32).tobytes()).hexdigest()
