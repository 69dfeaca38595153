"""CPU checks of the baseline defenses (include/ifd_dup.h): the C ABI and its binding, the PU-Net weight order, the oracle
pinned to the reference's recorded outputs, and the host logic of the defend_npz CLI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_dup.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dup_golden.npz")
GOLDEN_OUT = os.path.join(ROOT, "tests", "golden", "dup_golden_out.npz")


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
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


def test_dup_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.DUP_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported


def test_dup_abi_version_and_weight_count(lib):
    from ifdefense_amd import weights
    assert lib.ifd_dup_abi_version() == 1
    assert lib.ifd_punet_weight_count() == 814307
    assert sum(int(np.prod(s)) for _, s in weights.punet_canonical_keys()) == 814307


def test_pack_punet_follows_state_dict_order():
    import punet_oracle as PO
    from ifdefense_amd import weights
    sd = PO.load_weights()
    keys = weights.punet_canonical_keys()
    assert [k for k, _ in keys] == list(sd.keys())
    w = weights.pack_state_dict(sd, "punet")
    assert w.size == 814307 and w.dtype == np.float32
    first = sd["SA_modules.0.mlps.0.layer0.conv.weight"].reshape(-1)
    assert np.array_equal(w[:first.size], first)
    last = sd["pcd_layer.1.layer0.conv.bias"]
    assert np.array_equal(w[-3:], last)
    assert np.array_equal(w[-3 - 192:-3], sd["pcd_layer.1.layer0.conv.weight"].reshape(-1))
    bad = dict(sd)
    del bad["FC_Modules.2.layer1.conv.bias"]
    with pytest.raises(KeyError):
        weights.pack_state_dict(bad, "punet")
    bad = dict(sd)
    bad["FP_Modules.0.mlp.layer0.conv.weight"] = np.zeros((64, 127, 1, 1), np.float32)
    with pytest.raises(ValueError):
        weights.pack_state_dict(bad, "punet")


def test_load_checkpoint_punet_npz(tmp_path):
    import punet_oracle as PO
    from ifdefense_amd import weights
    sd = PO.load_weights()
    p = str(tmp_path / "pu.npz")
    np.savez(p, **sd)
    a = weights.load_checkpoint(p, "punet")
    q = str(tmp_path / "pu.pth")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, q)
    assert np.array_equal(a, weights.load_checkpoint(q, "punet"))


def test_dup_create_rejects_bad_arguments(lib):
    lib.ifd_dup_create.restype = ctypes.c_void_p
    w = np.zeros(10, np.float32)
    assert not lib.ifd_dup_create(w.ctypes.data, 10, 0)               # wrong count: fails before any HIP call
    assert b"814307" in lib.ifd_last_error(None)
    assert not lib.ifd_dup_create(None, 5, 0)


def test_oracle_reproduces_the_reference():
    """punet_oracle in float32 with the reference's distance form and draws == the recorded reference run."""
    import punet_oracle as PO
    g = dict(np.load(GOLDEN), out=np.load(GOLDEN_OUT)["out"])
    W = PO.to_torch(PO.load_weights())
    out, rec = PO.forward(W, torch.from_numpy(g["filled"]), torch.from_numpy(g["fps_start"]))
    assert np.array_equal(rec["fps_idx"].numpy(), g["fps_idx"])
    d = np.abs(out.numpy() - g["out"])
    print("oracle vs reference: max |diff| %.3e, exact %s" % (d.max(), bool((d == 0).all())))
    assert d.max() <= 1e-6


# ---------------------------------------------------------------------------------------------- CLI host logic
class FakeDefender:
    """Stands in for runtime.DupNet: SRS keeps the first K - drop rows, SOR drops every 3rd row of odd clouds."""

    def srs(self, pc, drop_num, cloud_index_base=0):
        return pc[:, :pc.shape[1] - drop_num]

    def sor(self, pc, k, alpha):
        return [pc[i] if i % 2 == 0 else pc[i][torch.arange(pc.shape[1]) % 3 != 0] for i in range(pc.shape[0])]

    def dup(self, pc, k, alpha, cloud_index_base=0):
        return pc.repeat(1, 4, 1)


def _write_npz(path, B=3, K=12):
    rng = np.random.default_rng(0)
    np.savez(path, test_pc=rng.standard_normal((B, K, 6)).astype(np.float32),
             test_label=np.arange(B, dtype=np.int64), target_label=np.arange(B, dtype=np.int64) + 1)


def test_cli_save_names_and_defense_list(tmp_path):
    from ifdefense_amd import defend_npz as D
    assert D.defense_list('') == ['srs', 'sor', 'dup']
    assert D.defense_list('sor') == ['sor']
    assert D.save_path('/a/b/adv.npz', 'srs') == '/a/b/srs/srs_adv.npz'
    d = tmp_path / "data"
    d.mkdir()
    _write_npz(str(d / "x.npz"))
    _write_npz(str(d / "y.npz"))
    (d / "sub").mkdir()
    assert sorted(os.path.basename(f) for f in D.input_files(str(d))) == ["x.npz", "y.npz"]


def test_cli_runs_all_defenses_with_fake_defender(tmp_path, monkeypatch):
    from ifdefense_amd import defend_npz as D, weights
    monkeypatch.setattr(weights, "load_checkpoint", lambda p, m: np.zeros(1, np.float32))
    d = tmp_path / "data"
    d.mkdir()
    _write_npz(str(d / "x.npz"))
    assert D.main(["--data_root", str(d), "--pu_weight", "w.pth", "--srs_drop_num", "4"],
                  make_defender=lambda w: FakeDefender()) == 0
    srs = np.load(str(d / "srs" / "srs_x.npz"))
    assert srs["test_pc"].shape == (3, 8, 3) and srs["test_pc"].dtype == np.float32
    assert srs["test_label"].dtype == np.uint8 and srs["target_label"].dtype == np.uint8
    sor = np.load(str(d / "sor" / "sor_x.npz"), allow_pickle=True)
    assert sor["test_pc"].dtype == object and [c.shape for c in sor["test_pc"]] == [(12, 3), (8, 3), (12, 3)]
    dup = np.load(str(d / "dup" / "dup_x.npz"))
    assert dup["test_pc"].shape == (3, 48, 3)
    assert list(dup["target_label"]) == [1, 2, 3]


def test_cli_dup_without_weights_fails_before_the_gpu(tmp_path, capsys):
    from ifdefense_amd import defend_npz as D

    def never(w):
        raise AssertionError("the defender must not be made")
    assert D.main(["--data_root", str(tmp_path / "x.npz")], make_defender=never) != 0
    assert "--pu_weight" in capsys.readouterr().err
    assert D.main(["--data_root", str(tmp_path / "x.npz"), "--defense", "dup"], make_defender=never) != 0


def test_assemble_test_pc_ragged_and_regular(tmp_path):
    from ifdefense_amd import defend_npz as D
    reg = D.assemble_test_pc([np.ones((5, 3)), np.zeros((5, 3))])
    assert reg.shape == (2, 5, 3) and reg.dtype == np.float32
    rag = D.assemble_test_pc([np.ones((5, 3)), np.zeros((4, 3))])
    assert rag.shape == (2,) and rag.dtype == object
    p = str(tmp_path / "r.npz")
    np.savez(p, test_pc=rag)
    back = np.load(p, allow_pickle=True)["test_pc"]
    assert back[0].shape == (5, 3) and back[1].shape == (4, 3) and back[1].dtype == np.float32
