"""CPU checks of the victim classifier (include/ifd_cls.h): the C ABI and its binding, the PointNet weight order and BatchNorm
folding, the oracle pinned to the reference's recorded outputs, and the host logic of the inference CLI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_cls.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cls_golden.npz")
N_PLAIN, N_FT = 1606193, 3459569


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


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def golden_clouds(g):
    return [g["pc_%d" % i] for i in range(int(g["n_clouds"]))]


def test_cls_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.CLS_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    for n in names:
        assert getattr(lib, n).argtypes is not None


def test_cls_abi_version_and_weight_count(lib):
    from ifdefense_amd import _lib, weights
    assert lib.ifd_cls_abi_version() == 1 == _lib.CLS_ABI_VERSION
    assert lib.ifd_abi_version() == 5                         # the main ABI did not move
    for ft, want in ((False, N_PLAIN), (True, N_FT)):
        assert lib.ifd_cls_weight_count(_lib.CLS_POINTNET, int(ft)) == want
        assert sum(int(np.prod(s)) for _, s in weights.pointnet_canonical_keys(ft)) == want
    for other in (_lib.CLS_POINTNET2, _lib.CLS_DGCNN, _lib.CLS_POINTCONV, 17, -1):
        assert lib.ifd_cls_weight_count(other, 0) == 0


@pytest.mark.parametrize("ft", [False, True])
def test_bn_folding_matches_unfolded_network_in_float64(g, ft):
    """The oracle on fold_pointnet's float64 tensors (BatchNorms left out) == the oracle with its BatchNorms, to 1e-12."""
    import pointnet_oracle as PO
    from ifdefense_amd import weights
    w = PO.make_weights(3, ft)
    pcs = golden_clouds(g)
    a = PO.forward(PO.to_torch(dict(weights.fold_pointnet(w, ft)), torch.float64), pcs, dtype=torch.float64)
    b = PO.forward(PO.to_torch(w, torch.float64), pcs, dtype=torch.float64)
    for x, y, name in zip(a, b, ("logits", "trans", "trans_feat", "global_feat")):
        assert (x is None) == (y is None)
        if x is not None:
            rel = float((x - y).abs().max() / y.abs().max())
            print("%s: folded vs unfolded, relative %.3e" % (name, rel))
            assert rel <= 1e-12
    # the statistics are not the init values: folding is not the identity
    f = dict(weights.fold_pointnet(w, ft))
    assert np.abs(f["feat.conv1.0.weight"] - w["feat.conv1.0.weight"][:, :, 0]).max() > 1e-3


@pytest.mark.parametrize("ft", [False, True])
def test_pack_pointnet_prefix_order_and_errors(tmp_path, ft):
    import pointnet_oracle as PO
    from ifdefense_amd import weights
    w = PO.make_weights(1, ft)
    bare = weights.pack_state_dict(w, "pointnet")
    assert bare.dtype == np.float32 and bare.size == (N_FT if ft else N_PLAIN)
    sd = PO.reference_state_dict(w)                           # module. prefix, num_batches_tracked, torch tensors
    assert all(k.startswith("module.") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    assert np.array_equal(bare, weights.pack_state_dict(sd, "pointnet"))
    assert np.array_equal(bare, weights.pack_state_dict(sd, "pointnet", feature_transform=ft))
    assert np.array_equal(bare, np.concatenate([a.astype(np.float32).reshape(-1) for _, a in weights.fold_pointnet(w, ft)]))
    assert [k for k, _ in weights.fold_pointnet(w, ft)] == [k for k, _ in weights.pointnet_canonical_keys(ft)]
    assert {k for k, _ in weights.pointnet_state_keys(ft)} == set(w)
    # fc3 layers have no BatchNorm: they pass through
    assert np.array_equal(bare[-40 * 256 - 40:-40], w["fc3.weight"].reshape(-1)) and np.array_equal(bare[-40:], w["fc3.bias"])
    # .pth and .npz load alike
    p, q = str(tmp_path / "pn.pth"), str(tmp_path / "pn.npz")
    torch.save(sd, p)
    np.savez(q, **w)
    assert np.array_equal(bare, weights.load_checkpoint(p, "pointnet")) and np.array_equal(bare, weights.load_checkpoint(q, "pointnet"))
    bad = dict(w)
    del bad["feat.stn.fc2.1.running_var"]
    with pytest.raises(KeyError):
        weights.pack_state_dict(bad, "pointnet")
    bad = dict(w)
    bad["feat.conv2.0.weight"] = np.zeros((128, 63, 1), np.float32)
    with pytest.raises(ValueError):
        weights.pack_state_dict(bad, "pointnet")
    if not ft:
        with pytest.raises(KeyError):
            weights.pack_state_dict(w, "pointnet", feature_transform=True)


def test_random_state_dict_is_the_oracle_recipe():
    import pointnet_oracle as PO
    from ifdefense_amd import weights
    for ft in (False, True):
        a, b = weights.pointnet_random_state_dict(5, ft), PO.make_weights(5, ft)
        assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
        v = a["feat.stn.conv1.1.running_var"]
        assert 0.5 <= v.min() and v.max() <= 1.25 and np.abs(a["feat.stn.conv1.1.running_mean"]).max() > 0


@pytest.mark.parametrize("ft", [False, True])
def test_oracle_reproduces_the_reference(g, ft):
    """pointnet_oracle in float32 against the recorded reference run (same torch CPU ops in the same order).  Measured where
    the fixture was made: 0.0 on logits, trans, trans_feat and the global feature, in float32 and float64 - bit for bit.
    4 x 0 is no usable bar on another CPU (the GEMM blocking may differ), so the bar is the reference's own float32 error:
    4 x e_32, e_32 = max |reference f32 logits - reference f64 logits| (4.1e-8 / 3.9e-8 on logits of 0.2)."""
    import pointnet_oracle as PO
    s = "_t" if ft else "_f"
    w = PO.make_weights(int(g["weight_seed"]), ft)
    lo, tr, tf, gf = PO.forward(PO.to_torch(w), golden_clouds(g))
    e32 = np.abs(g["logits" + s].astype(np.float64) - g["logits64" + s]).max()
    d = {"logits": np.abs(lo.numpy() - g["logits" + s]).max(), "trans": np.abs(tr.numpy() - g["trans" + s]).max(),
         "global_feat": np.abs(gf.numpy() - g["global_feat" + s]).max()}
    if ft:
        d["trans_feat"] = np.abs(tf.numpy() - g["trans_feat" + s]).max()
    lo64 = PO.forward(PO.to_torch(w, torch.float64), golden_clouds(g), dtype=torch.float64)[0]
    d["logits64"] = np.abs(lo64.numpy() - g["logits64" + s]).max()
    print("oracle vs reference:", {k: "%.3e" % v for k, v in d.items()}, "e_32 %.3e" % e32)
    assert e32 > 0
    # trans / global feature are O(1) where the logits are O(0.2): scale the bar by their magnitude
    assert d["logits"] <= 4 * e32 and d["logits64"] <= 4 * e32
    assert d["trans"] <= 4 * e32 * max(1.0, np.abs(g["trans" + s]).max() / np.abs(g["logits" + s]).max())
    assert d["global_feat"] <= 4 * e32 * max(1.0, np.abs(g["global_feat" + s]).max() / np.abs(g["logits" + s]).max())
    if ft:
        assert d["trans_feat"] <= 4 * e32 * max(1.0, np.abs(g["trans_feat" + s]).max() / np.abs(g["logits" + s]).max())
    assert np.array_equal(lo.numpy().argmax(1), g["logits" + s].argmax(1))


def test_normalize_points_matches_reference(g):
    from ifdefense_amd.inference import normalize_points_np
    for i in (3, 11):
        got = normalize_points_np(g["pc_%d" % i])
        assert got.dtype == g["normalized_%d" % i].dtype and np.array_equal(got, g["normalized_%d" % i])


def test_cls_create_rejects_bad_arguments_without_a_gpu(lib):
    from ifdefense_amd import _lib
    w = np.zeros(10, np.float32)
    assert not lib.ifd_cls_create(w.ctypes.data, 10, _lib.CLS_POINTNET, 0, 40, 0)          # wrong count
    assert str(N_PLAIN).encode() in lib.ifd_last_error(None)
    assert not lib.ifd_cls_create(w.ctypes.data, N_PLAIN, _lib.CLS_POINTNET, 1, 40, 0)     # the other variant's count
    assert str(N_FT).encode() in lib.ifd_last_error(None)
    assert not lib.ifd_cls_create(None, N_PLAIN, _lib.CLS_POINTNET, 0, 40, 0)
    for other in (_lib.CLS_POINTNET2, _lib.CLS_DGCNN, _lib.CLS_POINTCONV):
        assert not lib.ifd_cls_create(w.ctypes.data, 10, other, 0, 40, 0)
        assert b"not" in lib.ifd_last_error(None) and b"built" in lib.ifd_last_error(None)
    assert not lib.ifd_cls_create(w.ctypes.data, 10, 99, 0, 40, 0)
    assert b"unknown model" in lib.ifd_last_error(None)
    big = np.zeros(N_PLAIN, np.float32)
    assert not lib.ifd_cls_create(big.ctypes.data, N_PLAIN, _lib.CLS_POINTNET, 0, 10, 0)   # n_classes
    assert b"n_classes" in lib.ifd_last_error(None)
    assert lib.ifd_cls_forward(None, None, None, 1, 1024, None, None, None) == -1


def test_classifier_refuses_models_that_are_not_built(lib):
    import ifdefense_amd as I
    for m in ("dgcnn", "pointnet2", "pointconv"):
        with pytest.raises(I.IfdError, match="not built"):
            I.Classifier(np.zeros(4, np.float32), model=m)
    with pytest.raises(I.IfdError, match="expected %d" % N_PLAIN):
        I.Classifier(np.zeros(4, np.float32))


# ---------------------------------------------------------------------------------------------- CLI host logic
class StubClassifier:
    """Stands in for runtime.Classifier: the class of a cloud is its number of rows modulo 40."""

    def __init__(self):
        self.seen = None
        self.closed = False

    def predict(self, clouds):
        self.seen = [np.asarray(c) for c in clouds]
        return torch.tensor([len(c) % 40 for c in clouds])

    def close(self):
        self.closed = True


def _write(path, sizes, labels, targets=None, ragged=False, cols=3):
    rng = np.random.default_rng(0)
    if ragged:
        pc = np.empty(len(sizes), dtype=object)
        for i, n in enumerate(sizes):
            pc[i] = rng.standard_normal((n, cols)).astype(np.float32)
    else:
        pc = rng.standard_normal((len(sizes), sizes[0], cols)).astype(np.float32)
    kw = dict(test_pc=pc, test_label=np.asarray(labels, np.uint8))
    if targets is not None:
        kw["target_label"] = np.asarray(targets, np.uint8)
    np.savez(path, **kw)


def test_cli_model_from_path_order_and_num_points_rules():
    from ifdefense_amd import inference as Inf
    assert Inf.get_model_name("x/PointNet2-dgcnn.npz") == "dgcnn"
    assert Inf.get_model_name("x/pointconv_pointnet2.npz") == "pointconv"
    assert Inf.get_model_name("x/pointnet2_pointnet.npz") == "pointnet2"
    assert Inf.get_model_name("x/kNN-PointNet-0.npz") == "pointnet"
    assert Inf.get_model_name("x/unknown.npz") is None
    assert Inf.points_to_take("a/ADD-pointnet.npz", 1024) == 1536
    assert Inf.points_to_take("a/add_cluster-pointnet.npz", 1024) == 1536          # 'add' is tested first
    assert Inf.points_to_take("a/cluster-pointnet.npz", 1024) == 1120
    assert Inf.points_to_take("a/Object-pointnet.npz", 1024) == 1216
    assert Inf.points_to_take("a/add-pointnet.npz", 1536) == 1536
    assert Inf.points_to_take("a/perturb-pointnet.npz", 1024) == 1024
    assert Inf.points_to_take("a/perturb-pointnet.npz", 512) == 512
    assert Inf.default_weight_path("opt_mn40", "pointnet") == "pretrain/opt_mn40/pointnet.pth"


def test_cli_prints_the_reference_lines(tmp_path, capsys):
    from ifdefense_amd import inference as Inf
    made = []

    def make(model, ft, path):
        made.append((model, ft, path, StubClassifier()))
        return made[-1][3]
    # 7 clouds of 1536 rows in a file named 'add': all 1536 rows are taken -> class 1536 % 40 = 16
    p = str(tmp_path / "add-pointnet.npz")
    _write(p, [1536] * 7, [16, 16, 16, 0, 0, 0, 0], [0, 16, 0, 16, 1, 1, 1], cols=6)
    assert Inf.main(["--data_root", p, "--mode", "target", "--feature_transform", "true"], make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % (3 / 7, 2 / 7)
    model, ft, path, stub = made[-1]
    assert (model, ft, path) == ("pointnet", True, "pretrain/mn40/pointnet.pth") and stub.closed
    assert all(c.shape == (1536, 3) and c.dtype == np.float32 for c in stub.seen)
    # normal mode, explicit model / weights / num_points, ragged SOR file
    p = str(tmp_path / "sor_x.npz")
    _write(p, [50, 45, 41], [10, 5, 2], ragged=True)
    assert Inf.main(["--data_root", p, "--model", "pointnet", "--model_path", "w.npz", "--num_points", "45", "--dataset", "opt_mn40"],
                    make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f\n" % (1 / 3)      # rows taken: 45, 45, 41 -> classes 5, 5, 1
    assert made[-1][:3] == ("pointnet", False, "w.npz") and [len(c) for c in made[-1][3].seen] == [45, 45, 41]
    # --normalize_pc
    assert Inf.main(["--data_root", p, "--model", "pointnet", "--normalize_pc", "True"], make_classifier=make) == 0
    capsys.readouterr()
    c = made[-1][3].seen[0]
    assert abs(np.sqrt((c ** 2).sum(1)).max() - 1) < 1e-6 and np.abs(c.mean(0)).max() < 1e-6


def test_cli_target_mode_requires_target_label(tmp_path, capsys):
    from ifdefense_amd import inference as Inf
    p = str(tmp_path / "pointnet.npz")
    _write(p, [8] * 3, [0, 1, 2])
    assert Inf.main(["--data_root", p, "--mode", "target"], make_classifier=lambda *a: StubClassifier()) != 0
    assert "target_label" in capsys.readouterr().err
    with pytest.raises(KeyError):
        Inf.evaluate_npz(p, StubClassifier(), mode="target")
    import ifdefense_amd as I
    r = I.evaluate_npz(p, StubClassifier(), "normal", 1024, False)
    assert r["n"] == 3 and r["success_rate"] is None and list(r["pred"]) == [8, 8, 8] and r["accuracy"] == 0.0


def test_cli_refuses_other_victims(tmp_path, capsys):
    from ifdefense_amd import inference as Inf

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--data_root", "x.npz", "--model", "dgcnn"], ["--data_root", "a/kNN-pointnet2.npz"],
                 ["--data_root", "pointnet.npz", "--model", "pointconv"]):
        assert Inf.main(argv, make_classifier=never) != 0
        assert "not built" in capsys.readouterr().err
    assert Inf.main(["--data_root", "nothing.npz"], make_classifier=never) != 0
    assert "not recognized" in capsys.readouterr().err
