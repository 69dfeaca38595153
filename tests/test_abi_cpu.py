"""CPU-only checks of the drop-in boundary: the C-ABI library loads, exports every symbol that
include/ifd.h declares, and the host-side weight packing follows the documented canonical order."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd.h")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    if not os.path.exists(I.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("ifd_build", os.path.join(ROOT, "if-defense_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build()
    return I.load_library()


def test_header_symbols_exported(lib):
    names = declared_symbols()
    assert len(names) >= 9
    for n in names:
        assert hasattr(lib, n), "libifd.so does not export %s declared in include/ifd.h" % n


def test_binding_covers_header():
    from ifdefense_amd import _lib
    assert sorted(_lib.SIGNATURES) == declared_symbols()


def test_exports_are_c_abi():
    import ifdefense_amd as I
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l and "ifd_" in l.split()[-1][:4]}
    assert set(declared_symbols()) <= exported


def test_abi_version_and_weight_count(lib):
    from ifdefense_amd import weights
    assert lib.ifd_abi_version() == 5
    n = sum(int(np.prod(s)) for _, s in weights.canonical_keys())
    assert n == 16001 + 27232 + 1934976 == lib.ifd_weight_count()


def test_pack_state_dict(np_weights):
    from ifdefense_amd import weights
    flat = weights.pack_state_dict(np_weights)
    assert flat.dtype == np.float32 and flat.size == 1978209
    np.testing.assert_array_equal(flat[:96], np_weights["decoder.fc_p.weight"].reshape(-1))
    np.testing.assert_array_equal(flat[-32:], np_weights["encoder.unet.conv_final.bias"])
    bad = dict(np_weights)
    del bad["decoder.fc_out.bias"]
    with pytest.raises(KeyError):
        weights.pack_state_dict(bad)
    bad = dict(np_weights)
    bad["decoder.fc_p.weight"] = np.zeros((3, 32), np.float32)
    with pytest.raises(ValueError):
        weights.pack_state_dict(bad)


def test_create_rejects_bad_arguments(lib):
    """Argument validation happens before any HIP call, so it is testable without a GPU."""
    from ifdefense_amd._lib import IfdConfig
    cfg = IfdConfig(ctypes.sizeof(IfdConfig), 64, 32, 32, 5, 4, 32, 0.1)
    w = np.zeros(10, np.float32)
    assert not lib.ifd_create(w.ctypes.data, w.size, ctypes.byref(cfg), 0)
    assert b"expected 1978209" in lib.ifd_last_error(None)
    w = np.zeros(1978209, np.float32)
    cfg.plane_resolution = 128
    assert not lib.ifd_create(w.ctypes.data, w.size, ctypes.byref(cfg), 0)
    assert b"only the shipped" in lib.ifd_last_error(None)
    assert lib.ifd_optimize(None, None, None, 1, 1024, None, None, None, None, None, None) == -1


def test_no_gpu_fails_loudly(np_weights):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import ifdefense_amd as I
    with pytest.raises(I.IfdError):
        I.Restorer(I.weights.pack_state_dict(np_weights))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "if-defense_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f


def _mc_table(lib=None):
    import ctypes as C
    import numpy as np
    from ifdefense_amd import _lib
    lib = C.CDLL(_lib.LIB_PATH)
    tri = np.zeros((256, 16), np.int8)
    ntri = np.zeros(256, np.uint8)
    assert lib.ifd_mc_table(tri.ctypes.data_as(C.c_void_p), ntri.ctypes.data_as(C.c_void_p)) == 0
    return tri, ntri


_EC = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7)]
_CORNER = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]


def test_marching_cubes_table_is_the_reference_polygonisation():
    """ifd_mc_table == the fixture recorded from the reference's compiled libmcubes (scripts/probe_mc_table.py ->
    tests/golden/mc_table_ref.npz): same triangles, same order, same winding, for all 256 sign configurations; plus the
    structural facts any polygonisation must satisfy (only crossed edges, every crossed edge, at most 5 triangles)."""
    import os
    import numpy as np
    tri, ntri = _mc_table()
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mc_table_ref.npz"))
    assert np.array_equal(tri, ref["tri"]) and np.array_equal(ntri, ref["ntri"])
    assert ntri.max() == 5 and ntri[0] == 0 and ntri[255] == 0 and int(ntri.sum()) == 820
    for cfg in range(256):
        crossed = {e for e, (a, b) in enumerate(_EC) if ((cfg >> a) & 1) != ((cfg >> b) & 1)}
        used = {int(x) for x in tri[cfg, :3 * ntri[cfg]]}
        assert used == crossed, cfg
        assert (tri[cfg, 3 * ntri[cfg]:] == -1).all()


def _single_cube_cases():
    """(cfg_eff, val, grid) of every single-cube case: each sign configuration x three seeded draws of corner values, the third
    with a corner exactly on the iso-value."""
    rng = np.random.default_rng(7)
    corner = np.array(_CORNER, float)
    for cfg in range(256):
        for rep in range(3):
            val = np.where([(cfg >> m) & 1 for m in range(8)], -1.0, 1.0) * rng.uniform(0.05, 1.0, 8)
            if rep == 2:
                val[rng.integers(0, 8)] = -0.0 if (cfg >> 0) & 1 else val[0]          # a corner exactly on the iso-value (inside: <=)
                cfg_eff = sum(1 << m for m in range(8) if val[m] <= 0.0)
            else:
                cfg_eff = cfg
            grid = np.empty((2, 2, 2))
            for m in range(8):
                grid[tuple(corner[m].astype(int))] = val[m]
            yield cfg_eff, val, grid


def _ref_single_cube_triangles(mcubes, grid):
    """The reference libmcubes' triangles [n, 3, 3] of one 2 x 2 x 2 grid at iso-value 0."""
    v, t = mcubes.marching_cubes(grid, 0.0)
    v = v - 0.5                                                          # mcubes.pyx's cell-centre shift
    return v[t.astype(int)] if len(t) else np.zeros((0, 3, 3))


def test_marching_cubes_single_cubes_against_live_reference_library():
    """Every sign configuration x random corner values through (ifd_mc_table + the iso-crossing interpolation) and through
    the reference's own libmcubes: identical vertex coordinates in identical triangle order - the surface is the reference's
    triangle for triangle, so triangle count, area and orientation (signed volume) agree exactly.  The reference's triangles
    for these inputs are stored in tests/golden/mc_single_cubes_ref.npz (tests/golden/make_mc_single_cubes.py); where
    oracle/_ref is built the live library is asked again and must reproduce them bit for bit."""
    import sys
    ref = dict(np.load(os.path.join(ROOT, "tests", "golden", "mc_single_cubes_ref.npz")))
    starts = np.concatenate([[0], np.cumsum(ref["ntri"])])
    mcubes = None
    d = os.path.join(ROOT, "oracle", "_ref")
    if os.path.isdir(d) and any(f.startswith("mcubes") for f in os.listdir(d)):
        sys.path.insert(0, d)
        import mcubes
    tri, ntri = _mc_table()
    corner = np.array(_CORNER, float)
    n_cases = 0
    for i, (cfg_eff, val, grid) in enumerate(_single_cube_cases()):
        np.testing.assert_array_equal(val, ref["val"][i])
        theirs = ref["tris"][starts[i]:starts[i + 1]]
        if mcubes is not None:
            np.testing.assert_array_equal(_ref_single_cube_triangles(mcubes, grid), theirs, err_msg=str(i))
        ours = []
        for k in range(ntri[cfg_eff]):
            for e in tri[cfg_eff, 3 * k:3 * k + 3]:
                a, b = _EC[e]
                w = 0.5 if val[b] == val[a] else (0.0 - val[a]) / (val[b] - val[a])     # marchingcubes.cpp:290-297
                ours.append(corner[a] + (corner[b] - corner[a]) * w)
        ours = np.array(ours).reshape(-1, 3, 3)
        assert ours.shape == theirs.shape, (i, cfg_eff)
        np.testing.assert_allclose(ours, theirs, rtol=0, atol=1e-12, err_msg=str((i, cfg_eff)))
        n_cases += 1
    assert n_cases == len(ref["ntri"]) == 768


def _gfx950_code_objects(path):
    """The gfx950 code objects embedded in a host object / shared library (clang offload bundles in .hip_fatbin)."""
    import struct
    d = open(path, "rb").read()
    out, i = [], 0
    while True:
        i = d.find(b"__CLANG_OFFLOAD_BUNDLE__", i)
        if i < 0:
            return out
        n = struct.unpack_from("<Q", d, i + 24)[0]
        off = i + 32
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", d, off)
            off += 24
            if b"gfx950" in d[off:off + tl]:
                out.append(d[i + o:i + o + sz])
            off += tl
        i += 24


def _disassemblies(lib_path, tmp_path):
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not in this image")
    for k, co in enumerate(_gfx950_code_objects(lib_path)):
        f = tmp_path / ("co%d.elf" % k)
        f.write_bytes(co)
        yield subprocess.run([objdump, "-d", "--no-show-raw-insn", str(f)], capture_output=True, text=True).stdout


def test_split_cloud_arrivals_are_preceded_by_a_vmcnt0_wait(lib, tmp_path):
    """Round-3 advisor finding: a member of a split cloud must drain its stores / atomics to the exchange block
    (`s_waitcnt vmcnt(0)`, knn_device.h coop_publish) before it bumps an arrival counter - the workgroup-scope release
    fence alone emits no vmcnt wait on gfx950.  Checked in the shipped ISA: in optimize_kernel<8, 2, P> and <8, 4, P> (P = 0: f32
    tiles, 1 / 2: the split-precision tiles) the nearest preceding memory-write-or-wait of every arrival atomic (a 32-bit
    global_atomic_add through an SGPR base) is the wait."""
    import ifdefense_amd as I
    found = {}
    for txt in _disassemblies(I.LIB_PATH, tmp_path):
        for sym in sorted(set(re.findall(r"<_ZN3ifd15(optimize_kernelILi8ELi[24]ELi[012]E)", txt))):
            body = txt[txt.index("<_ZN3ifd15" + sym):]
            body = body[:body.index("s_endpgm")]
            ins = [l.split("//")[0].strip() for l in body.splitlines()]
            ins = [l for l in ins if l and not l.endswith(":")]
            arrivals = [i for i, l in enumerate(ins) if re.match(r"global_atomic_add v\d+, v\d+, s\[", l)]
            assert len(arrivals) >= 2, "expected the bar_knn and bar_step arrivals in " + sym
            for a in arrivals:
                prev = next(l for l in reversed(ins[:a])
                            if l.startswith(("global_store", "global_atomic", "s_waitcnt vmcnt(0)")) or "vmcnt(0)" in l)
                assert "vmcnt(0)" in prev and prev.startswith("s_waitcnt"), (sym, ins[max(0, a - 12):a + 1])
            found[sym] = len(arrivals)
    assert len(found) == 6, "optimize_kernel<8, 2 | 4, 0 | 1 | 2> not all found in libifd.so: %s" % sorted(found)


def test_split_precision_kernels_contain_no_packed_f32_instruction(lib, tmp_path):
    """Round 5: on gfx950 a packed-f32 vector instruction (v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32) whose dependent consumer does
    not issue back to back occasionally delivers a wrong result while the OTHER wave of its SIMD streams bf16 MFMAs (0 wrong of 5e9
    with an idle or f32-MFMA partner, 48 - 288 with a bf16-MFMA partner: scripts/pk_mfma_coexec.hip, profiles/r05_pk_mfma_coexec.txt;
    it made ~1 % of the split-precision tile's sub-tiles wrong, run to run).  The split-precision optimiser kernels are the only ones
    that issue bf16 MFMAs, and they are built without packed f32 (build.py FILE_FLAGS: -fno-slp-vectorize, scalar sampling code in
    tile_bf.h): checked in the shipped ISA.  (An earlier hypothesis - a satisfied s_waitcnt counted as the pair's wait state - was
    disproved by scripts/pk_waitcnt_hazard.hip: 0 wrong in every form.)"""
    import ifdefense_amd as I
    found = {}
    for txt in _disassemblies(I.LIB_PATH, tmp_path):
        for sym in sorted(set(re.findall(r"<_ZN3ifd15(optimize_kernelILi8ELi[124]ELi[012]E)", txt))):
            body = txt[txt.index("<_ZN3ifd15" + sym):]
            body = body[:body.index("s_endpgm")]
            found[sym] = (len(re.findall(r"\bv_pk_(?:mul|fma|add)_f32\b", body)), len(re.findall(r"\bv_mfma_f32_16x16x32_bf16\b", body)))
    assert len(found) == 9, sorted(found)
    # the ONet-Opt optimiser likewise (onet.hip: <0>, onet_bf.hip: <1>, <2>)
    for txt in _disassemblies(I.LIB_PATH, tmp_path):
        for sym in sorted(set(re.findall(r"<_ZN3ifd20(onet_optimize_kernelILi[012]E)", txt))):
            body = txt[txt.index("<_ZN3ifd20" + sym):]
            body = body[:body.index("s_endpgm")]
            found[sym] = (len(re.findall(r"\bv_pk_(?:mul|fma|add)_f32\b", body)), len(re.findall(r"\bv_mfma_f32_16x16x32_bf16\b", body)))
    assert len(found) == 12, sorted(found)
    for sym, (n_pk, n_bf) in found.items():
        if sym.endswith("Li0E"):
            assert n_bf == 0 and (n_pk > 0 or sym.startswith("onet")), (sym, n_pk, n_bf)     # the f32 kernels: packed f32 is fine beside f32 MFMAs
        else:
            assert n_bf > 100 and n_pk == 0, (sym, n_pk, n_bf)


def test_kernels_with_bf16_mfmas_leave_no_room_for_a_foreign_wave(lib, tmp_path):
    """Round-5 advisor: the packed-f32 erratum (test above) needs a bf16-MFMA wave and a packed-f32 wave on ONE SIMD.  The kernels that
    issue bf16 MFMAs contain no packed f32 themselves; kernels of other translation units (and torch's) do, and pipeline.defend_stream
    runs pre-processing kernels on a second stream while a split-precision optimiser is resident.  They can never share a SIMD: every
    kernel with bf16 MFMAs is launched as 512-thread workgroups = two waves per SIMD, and its waves allocate 256 of the SIMD's 512
    vector registers each - checked in the shipped kernel metadata - so no wave of another kernel fits beside them."""
    import ifdefense_amd as I
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not os.path.exists(readelf):
        pytest.skip("llvm-readelf not in this image")
    bf_kernels = set()
    for txt in _disassemblies(I.LIB_PATH, tmp_path):
        for m in re.finditer(r"^[0-9a-f]+ <(_ZN3ifd\w+)>:$", txt, re.M):
            body = txt[m.end():]
            body = body[:body.index("s_endpgm")]
            if "v_mfma_f32_16x16x32_bf16" in body:
                bf_kernels.add(m.group(1))
                # ... and none of them, whichever translation unit it comes from, holds a packed-f32 instruction itself
                assert not re.search(r"\bv_pk_(?:mul|fma|add)_f32\b", body), m.group(1)
    # optimize_kernel<8, 1|2|4, 1|2>, large_occupancy3_kernel<1|2>, decode3_bf_kernel<1|2>, onet_optimize_kernel<1|2>,
    # onet_grid_eval_kernel<1|2>, onet_decode_bf_kernel<1|2>
    assert len(bf_kernels) >= 16, sorted(bf_kernels)
    seen = {}
    for k, co in enumerate(_gfx950_code_objects(I.LIB_PATH)):
        f = tmp_path / ("meta%d.elf" % k)
        f.write_bytes(co)
        notes = subprocess.run([readelf, "--notes", str(f)], capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if name in bf_kernels:
                agpr = int(blk.split()[0])
                vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1))
                wg = int(re.search(r"\.max_flat_workgroup_size:\s+(\d+)", blk).group(1))
                seen[name] = (vgpr + agpr, wg)
    assert set(seen) == bf_kernels, sorted(bf_kernels - set(seen))
    for name, (regs, wg) in seen.items():
        alloc = (regs + 7) // 8 * 8                             # allocation granule of the unified register file
        assert wg == 512 and (wg // 64 // 4) * alloc == 512, (name, regs, wg)
