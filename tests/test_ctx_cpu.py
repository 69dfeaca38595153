"""CPU checks of the host half of libifd (csrc/api.cpp): the failure path of the four create functions through the C ABI, and
the stand-alone program tests/host/ctx_selftest.cpp (workspace layouts and the kernels' LDS layouts against their recorded byte
formulas, the carve cursor, the same failed creates) built with the host sanitizers.  Neither needs a GPU: a device ordinal that no machine has makes
hipSetDevice return an error, which is the first thing the common create path can fail on."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_SUCH_DEVICE = 1 << 20


def _build_module():
    spec = importlib.util.spec_from_file_location("ifd_build", os.path.join(ROOT, "if-defense_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    if not os.path.exists(I.LIB_PATH):
        _build_module().build()
    return I.load_library()


def test_failed_creates_name_their_function_and_leave_nothing_behind(lib):
    from ifdefense_amd import _lib
    w = np.zeros(max(lib.ifd_weight_count(), lib.ifd_onet_weight_count(), lib.ifd_punet_weight_count(),
                     lib.ifd_cls_weight_count(_lib.CLS_POINTNET, 0)), np.float32)
    cfg = _lib.IfdConfig(C.sizeof(_lib.IfdConfig), 64, 32, 32, 5, 4, 32, 0.1)
    creates = {
        "ifd_create": lambda: lib.ifd_create(w.ctypes.data, lib.ifd_weight_count(), C.byref(cfg), NO_SUCH_DEVICE),
        "ifd_onet_create": lambda: lib.ifd_onet_create(w.ctypes.data, lib.ifd_onet_weight_count(), NO_SUCH_DEVICE),
        "ifd_dup_create": lambda: lib.ifd_dup_create(w.ctypes.data, lib.ifd_punet_weight_count(), NO_SUCH_DEVICE),
        "ifd_cls_create": lambda: lib.ifd_cls_create(w.ctypes.data, lib.ifd_cls_weight_count(_lib.CLS_POINTNET, 0),
                                                     _lib.CLS_POINTNET, 0, 40, NO_SUCH_DEVICE),
    }
    for name, create in creates.items():
        for rep in range(3):
            assert not create(), (name, rep)
            err = lib.ifd_last_error(None).decode()
            print(name, rep, repr(err))
            assert err.startswith(name + ": ") and len(err) > len(name) + 2, (name, rep, err)
            assert "NULL" not in err and "expected" not in err, (name, err)          # HIP's text, not an argument check's
    hip_text = lib.ifd_last_error(None).decode()
    assert not lib.ifd_create(None, 0, None, 0)                                       # a bad-argument call replaces the text
    assert lib.ifd_last_error(None).decode() == "ifd_create: NULL argument" != hip_text
    assert not lib.ifd_dup_create(None, 5, NO_SUCH_DEVICE)
    assert lib.ifd_last_error(None).decode().startswith("ifd_dup_create: expected ")
    lib.ifd_destroy(None)                                                             # returns


def test_host_selftest_under_the_sanitizers(tmp_path):
    """tests/host/ctx_selftest.cpp includes api.cpp, is compiled with -fsanitize=address,undefined on the host side and linked
    with the kernel objects of the library's own build; leak detection stays on."""
    build = _build_module()
    build.build()                                                                     # the objects (nothing to do after build())
    objs = [os.path.splitext(s)[0] + ".o" for s in build.sources() if os.path.basename(s) != "api.cpp"]
    exe = str(tmp_path / "ctx_selftest")
    cmd = [build.HIPCC, "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-O1", "-g", "-std=c++17", "-Wall",
           "-Wno-unused-function", "-I" + build.CSRC, "-I" + os.path.join(ROOT, "include"),
           "-x", "hip", os.path.join(ROOT, "tests", "host", "ctx_selftest.cpp"), "-x", "none"] + objs + ["-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    print(out[-3000:])
    assert r.returncode == 0, out[-6000:]
    assert "0 failed" in r.stdout and "runtime error" not in out and "AddressSanitizer" not in out and "LeakSanitizer" not in out, out[-6000:]
