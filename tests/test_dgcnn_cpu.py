"""CPU checks of the DGCNN victim (include/ifd_dgcnn.h): the C ABI and its binding, the weight order and BatchNorm folding, the
oracle pinned to the reference's recorded run, the weight sets and the checker the GPU tests rest on, and the host logic of the
dgcnn_inference CLI."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_dgcnn.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dgcnn_golden.npz")
N_WEIGHTS = 1807016


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


def test_dgcnn_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.DGCNN_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    assert I.DgcnnClassifier is I.runtime.DgcnnClassifier


def test_dgcnn_abi_version_and_weight_count(lib):
    from ifdefense_amd import _lib, weights
    assert lib.ifd_dgcnn_abi_version() == 1 == _lib.DGCNN_ABI_VERSION
    assert lib.ifd_abi_version() == 5 and lib.ifd_cls_abi_version() == 1      # the other ABIs did not move
    assert lib.ifd_dgcnn_weight_count() == N_WEIGHTS
    assert sum(int(np.prod(s)) for _, s in weights.dgcnn_canonical_keys()) == N_WEIGHTS
    assert lib.ifd_cls_weight_count(_lib.CLS_DGCNN, 0) == 0                   # ... and DGCNN is not behind ifd_cls_*


def test_dgcnn_create_rejects_bad_arguments_without_a_gpu(lib):
    import ifdefense_amd as I
    w = np.zeros(N_WEIGHTS, np.float32)
    assert not lib.ifd_dgcnn_create(w.ctypes.data, 10, 20, 40, 0)             # wrong count
    assert str(N_WEIGHTS).encode() in lib.ifd_last_error(None)
    assert not lib.ifd_dgcnn_create(None, N_WEIGHTS, 20, 40, 0)
    for k in (0, 33, -1):
        assert not lib.ifd_dgcnn_create(w.ctypes.data, N_WEIGHTS, k, 40, 0)
        assert b"k must lie in [1, 32]" in lib.ifd_last_error(None)
    assert not lib.ifd_dgcnn_create(w.ctypes.data, N_WEIGHTS, 20, 10, 0)
    assert b"n_classes" in lib.ifd_last_error(None)
    assert lib.ifd_dgcnn_forward(None, None, None, 1, 1024, None, None, None) == -1
    with pytest.raises(I.IfdError, match="expected %d" % N_WEIGHTS):
        I.DgcnnClassifier(np.zeros(4, np.float32))
    with pytest.raises(I.IfdError, match="k must lie"):
        I.DgcnnClassifier(w, k=33)


def test_bn_folding_matches_unfolded_network_in_float64(g):
    """The oracle on fold_dgcnn's float64 tensors (BatchNorms left out) == the oracle with its BatchNorms, to 1e-12, the
    neighbour sets of the unfolded run forced into the folded one."""
    import dgcnn_oracle as DO
    from ifdefense_amd import weights
    w = DO.make_weights(3)
    pcs = golden_clouds(g)
    b = DO.forward(DO.to_torch(w, torch.float64), pcs, dtype=torch.float64)
    idx = [[t.numpy() for t in b["idx"][l]] for l in range(4)]
    a = DO.forward(DO.to_torch(dict(weights.fold_dgcnn(w)), torch.float64), pcs, dtype=torch.float64, idx=idx)
    for name in ("logits", "global_feat"):
        rel = float((a[name] - b[name]).abs().max() / b[name].abs().max())
        print("%s: folded vs unfolded, relative %.3e" % (name, rel))
        assert rel <= 1e-12
    for x, y in zip(a["feat"], b["feat"]):
        assert float((x - y).abs().max() / y.abs().max()) <= 1e-12
    f = dict(weights.fold_dgcnn(w))
    assert np.abs(f["conv1.0.weight"] - w["conv1.0.weight"][:, :, 0, 0]).max() > 1e-3       # folding is not the identity
    assert np.abs(f["conv1.0.bias"]).max() > 1e-3                                           # the shift became the bias


def test_pack_dgcnn_prefix_order_doubled_keys_and_errors(tmp_path):
    import dgcnn_oracle as DO
    from ifdefense_amd import weights
    w = DO.make_weights(1)
    bare = weights.pack_state_dict(w, "dgcnn")
    assert bare.dtype == np.float32 and bare.size == N_WEIGHTS
    sd = DO.reference_state_dict(w)                           # module. prefix, both BatchNorm keys, num_batches_tracked
    assert all(k.startswith("module.") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    assert "module.bn1.weight" in sd and "module.conv1.1.weight" in sd and "module.linear1.1.running_var" in sd
    assert np.array_equal(bare, weights.pack_state_dict(sd, "dgcnn")) and np.array_equal(bare, weights.pack_dgcnn(sd))
    assert [k for k, _ in weights.fold_dgcnn(w)] == [k for k, _ in weights.dgcnn_canonical_keys()]
    assert [(k, a.shape) for k, a in weights.fold_dgcnn(w)] == weights.dgcnn_canonical_keys()
    # only the Sequential's keys: read from there
    seq = {k: v for k, v in sd.items() if not re.match(r"module\.bn\d\.", k)}
    assert len(seq) < len(sd) and np.array_equal(bare, weights.pack_dgcnn(seq))
    # the two names of one BatchNorm disagree
    bad = dict(sd)
    bad["module.conv3.1.running_mean"] = sd["module.conv3.1.running_mean"] + 1
    with pytest.raises(ValueError, match="differ"):
        weights.pack_dgcnn(bad)
    # linear3 has no BatchNorm: it passes through; conv1's canonical bias is its BatchNorm's shift
    assert np.array_equal(bare[-40 * 256 - 40:-40], w["linear3.weight"].reshape(-1)) and np.array_equal(bare[-40:], w["linear3.bias"])
    sc = w["bn1.weight"].astype(np.float64) / np.sqrt(w["bn1.running_var"].astype(np.float64) + 1e-5)
    assert np.array_equal(bare[:384], (w["conv1.0.weight"].reshape(64, 6).astype(np.float64) * sc[:, None]).astype(np.float32).reshape(-1))
    assert np.array_equal(bare[384:448], (w["bn1.bias"] - w["bn1.running_mean"].astype(np.float64) * sc).astype(np.float32))
    # .pth and .npz load alike
    p, q = str(tmp_path / "dg.pth"), str(tmp_path / "dg.npz")
    torch.save(sd, p)
    np.savez(q, **w)
    assert np.array_equal(bare, weights.load_checkpoint(p, "dgcnn")) and np.array_equal(bare, weights.load_checkpoint(q, "dgcnn"))
    bad = dict(w)
    del bad["bn6.running_var"]
    with pytest.raises(KeyError):
        weights.pack_state_dict(bad, "dgcnn")
    bad = dict(w)
    bad["conv2.0.weight"] = np.zeros((64, 127, 1, 1), np.float32)
    with pytest.raises(ValueError):
        weights.pack_state_dict(bad, "dgcnn")


def test_random_state_dict_is_the_oracle_recipe():
    import dgcnn_oracle as DO
    from ifdefense_amd import weights
    a, b = weights.dgcnn_random_state_dict(5), DO.make_weights(5)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert "conv1.0.bias" not in a and "linear2.0.bias" in a and a["conv5.0.weight"].shape == (1024, 512, 1)
    v = a["bn4.running_var"]
    assert 0.5 <= v.min() and v.max() <= 1.25 and np.abs(a["bn4.running_mean"]).max() > 0


def test_oracle_reproduces_the_reference(g):
    """dgcnn_oracle against the recorded reference run (same torch CPU ops in the same order; 0.0 where the fixture was made).
    The bar is the reference's own float32 error: 4 x e_32, e_32 = max |reference f32 logits - reference f64 logits|."""
    import dgcnn_oracle as DO
    w = DO.make_weights(int(g["weight_seed"]))
    k = int(g["k"])
    pcs = golden_clouds(g)
    o = DO.forward(DO.to_torch(w), pcs, k=k)
    o64 = DO.forward(DO.to_torch(w, torch.float64), pcs, dtype=torch.float64, k=k)
    e32 = np.abs(g["logits"].astype(np.float64) - g["logits64"]).max()
    d = {"logits": np.abs(o["logits"].numpy() - g["logits"]).max(), "logits64": np.abs(o64["logits"].numpy() - g["logits64"]).max(),
         "global_feat": np.abs(o["global_feat"].numpy() - g["global_feat"]).max()}
    print("oracle vs reference:", {n: "%.3e" % v for n, v in d.items()}, "e_32 %.3e" % e32)
    assert e32 > 0
    assert d["logits"] <= 4 * e32 and d["logits64"] <= 4 * e32
    assert d["global_feat"] <= 4 * e32 * max(1.0, np.abs(g["global_feat"]).max() / np.abs(g["logits"]).max())
    for l in range(4):
        for i in range(len(pcs)):
            assert np.array_equal(np.sort(o["idx"][l][i].numpy(), axis=1), np.sort(g["idx%d_%d" % (l, i)], axis=1)), (l, i)
            assert np.array_equal(np.sort(o64["idx"][l][i].numpy(), axis=1), np.sort(g["idx64_%d_%d" % (l, i)], axis=1)), (l, i)


def test_forced_neighbours_are_honoured(g):
    import dgcnn_oracle as DO
    W = DO.to_torch(DO.make_weights(0))
    x = np.stack(golden_clouds(g)[:3])
    free = DO.forward(W, x)
    again = DO.forward(W, x, idx=[t.numpy() for t in free["idx"]])
    assert torch.equal(free["logits"], again["logits"]) and torch.equal(free["feat"], again["feat"])
    other = [t.numpy().copy() for t in free["idx"]]
    other[3][:, :, 0] = (other[3][:, :, 0] + 31) % 64
    assert not torch.equal(DO.forward(W, x, idx=other)["logits"], free["logits"])
    rag = DO.forward(W, [x[0], x[1][:40]], idx=[t.numpy()[:2] % 40 for t in free["idx"]])
    assert rag["feat"][1].shape == (40, 512) and rag["logits"].shape == (2, 40)


def test_calibrated_weights_give_varied_predictions():
    """The calibrated head alone (no GPU): on bench.synth_clouds(256, seed=23)[:, :128] the float64 oracle predicts at least 15
    classes, and at most 1 % of the clouds have a top-2 margin below 8 e_32 (e_32: the float32 oracle on the float64 oracle's
    neighbour sets against the float64 oracle)."""
    import bench
    import cls_checks
    import dgcnn_oracle as DO
    sd = DO.make_calibrated_weights(0)
    base = DO.make_weights(0)
    assert all(np.array_equal(sd[k], base[k]) for k in sd if not k.startswith("linear3."))
    x = np.ascontiguousarray(bench.synth_clouds(256, seed=23)[:, :128])
    lo32, lo64 = [], []
    for a in range(0, len(x), 32):
        o64 = DO.forward(DO.to_torch(sd, torch.float64), x[a:a + 32], dtype=torch.float64)
        lo64.append(o64["logits"])
        lo32.append(DO.forward(DO.to_torch(sd), x[a:a + 32], idx=[t.numpy() for t in o64["idx"]])["logits"])
    lo32, lo64 = torch.cat(lo32), torch.cat(lo64)
    e_32 = cls_checks.e32_of(lo32, lo64)
    excluded, classes = cls_checks.check_pred_against_f64(lo64.argmax(1).numpy(), lo64, e_32, "dgcnn calibrated head (oracle only)")
    share = np.bincount(lo64.argmax(1).numpy(), minlength=40).max() / len(x)
    print("e_32 %.3e, classes %d, largest class share %.3f, smallest margin %.1f e_32"
          % (e_32, classes, share, cls_checks.top2_margin(lo64).min() / e_32))
    assert e_32 > 0 and classes >= 15 and excluded <= 0.01 * len(x)
    tied = DO.make_tied_weights(sd)
    assert np.array_equal(tied["linear3.weight"][20:], tied["linear3.weight"][:20]) and np.array_equal(tied["linear3.bias"][20:], tied["linear3.bias"][:20])


def test_neighbour_checker_accepts_the_oracle_and_refuses_a_swap(g):
    import dgcnn_oracle as DO
    pcs = golden_clouds(g)
    o = DO.forward(DO.to_torch(DO.make_weights(0)), pcs)
    cols = ((0, 64), (64, 128), (128, 256))
    for i, c in enumerate(pcs):
        for l in range(4):
            x = c if l == 0 else o["feat"][i][:, cols[l - 1][0]:cols[l - 1][1]].numpy()
            idx = o["idx"][l][i].numpy()
            DO.check_neighbours(x, idx, 20, "oracle, cloud %d layer %d" % (i, l + 1))
            # one neighbour of one row replaced by the (k + 5)-th nearest
            s = DO.exact_scores(x)
            row = len(c) // 2
            order = np.argsort(-s[row], kind="stable")
            bad = idx.copy()
            bad[row, np.nonzero(bad[row] == order[3])[0][0]] = order[24]
            with pytest.raises(AssertionError):
                DO.check_neighbours(x, bad, 20, "swapped")
    dup = o["idx"][0][0].numpy().copy()
    dup[5, 1] = dup[5, 0]
    with pytest.raises(AssertionError):
        DO.check_neighbours(pcs[0], dup, 20, "repeated")
    out = o["idx"][0][0].numpy().copy()
    out[0, 0] = 64
    with pytest.raises(AssertionError):
        DO.check_neighbours(pcs[0], out, 20, "out of range")


# ---------------------------------------------------------------------------------------------- CLI host logic
class StubClassifier:
    """Stands in for runtime.DgcnnClassifier: the class of a cloud is its number of rows modulo 40."""

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


def test_cli_prints_the_reference_lines(tmp_path, capsys):
    from ifdefense_amd import dgcnn_inference as Inf
    made = []

    def make(model, k, path):
        made.append((model, k, path, StubClassifier()))
        return made[-1][3]
    # the model named by the path; a cluster file takes 1120 rows -> class 0
    p = str(tmp_path / "cluster-DGCNN-x.npz")
    _write(p, [1120] * 7, [0, 0, 0, 5, 5, 5, 5], [5, 0, 5, 0, 1, 1, 1], cols=6)
    assert Inf.main(["--data_root", p, "--mode", "target"], make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % (3 / 7, 2 / 7)
    model, k, path, stub = made[-1]
    assert (model, k, path) == ("dgcnn", 20, "pretrain/mn40/dgcnn.pth") and stub.closed
    assert all(c.shape == (1120, 3) and c.dtype == np.float32 for c in stub.seen)
    # normal mode, explicit model / weights / k / num_points, ragged SOR file
    p = str(tmp_path / "sor_x.npz")
    _write(p, [50, 45, 41], [10, 5, 2], ragged=True)
    assert Inf.main(["--data_root", p, "--model", "dgcnn", "--model_path", "w.npz", "--num_points", "45", "--dataset", "opt_mn40",
                     "--k", "7"], make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f\n" % (1 / 3)      # rows taken: 45, 45, 41 -> classes 5, 5, 1
    assert made[-1][:3] == ("dgcnn", 7, "w.npz") and [len(c) for c in made[-1][3].seen] == [45, 45, 41]
    assert Inf.main(["--data_root", p, "--model", "dgcnn", "--dataset", "conv_opt_mn40"], make_classifier=make) == 0
    assert made[-1][2] == "pretrain/conv_opt_mn40/dgcnn.pth"
    capsys.readouterr()


def test_cli_refusals(tmp_path, capsys):
    from ifdefense_amd import dgcnn_inference as Inf

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--data_root", "x.npz", "--model", "pointnet"], ["--data_root", "a/kNN-pointnet2.npz"],
                 ["--data_root", "dgcnn.npz", "--model", "pointconv"]):
        assert Inf.main(argv, make_classifier=never) == 2
        assert "ifdefense_amd.inference" in capsys.readouterr().err
    assert Inf.main(["--data_root", "nothing.npz"], make_classifier=never) == 2
    assert "not recognized" in capsys.readouterr().err
    assert Inf.main(["--data_root", "dgcnn.npz", "--emb_dims", "512"], make_classifier=never) == 2
    assert "emb_dims" in capsys.readouterr().err
    assert Inf.main(["--data_root", "dgcnn.npz", "--k", "33"], make_classifier=never) == 2
    assert "--k" in capsys.readouterr().err
    # a cloud of fewer than k points: refused with a message, the classifier closed, nothing run
    p = str(tmp_path / "sor-dgcnn.npz")
    _write(p, [50, 19, 41], [10, 5, 2], ragged=True)
    stub = StubClassifier()
    assert Inf.main(["--data_root", p], make_classifier=lambda *a: stub) == 2
    err = capsys.readouterr().err
    assert "cloud 1 has 19 points, fewer than k = 20" in err and stub.closed and stub.seen is None
    assert Inf.main(["--data_root", p, "--k", "19"], make_classifier=lambda *a: StubClassifier()) == 0
    capsys.readouterr()
    # target mode without target_label
    assert Inf.main(["--data_root", p, "--k", "5", "--mode", "target"], make_classifier=lambda *a: StubClassifier()) == 2
    assert "target_label" in capsys.readouterr().err
    # the PointNet CLI points here
    from ifdefense_amd import inference
    assert inference.main(["--data_root", "x.npz", "--model", "dgcnn"], make_classifier=never) == 2
    err = capsys.readouterr().err
    assert "not built" in err and "ifdefense_amd.dgcnn_inference" in err


# ---------------------------------------------------------------------------------------------- the header's choice, exactly
def _round_f32(v):
    """A Fraction rounded to the nearest float32, ties to even, denormals included (no overflow)."""
    from fractions import Fraction
    if v == 0:
        return np.float32(0.0)
    a, e = abs(v), 0
    while a >= 2 ** (e + 1):
        e += 1
    while a < Fraction(2) ** e:
        e -= 1
    quantum = Fraction(2) ** (max(e, -126) - 23)
    m = a / quantum
    n = m.numerator // m.denominator
    rest = m - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    r = float(n * quantum)                                   # exact: at most 24 bits
    return np.float32(-r if v < 0 else r)


def _exact_fma(a, b, c):
    from fractions import Fraction
    return np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_fma32_equals_rational_arithmetic_on_random_triples():
    import dgcnn_oracle as DO
    rng = np.random.default_rng(41)
    n = 24000

    def draw(lo=-5.0, hi=5.0):
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n) * rng.uniform(1, 2, n)).astype(np.float32)
    a, b, c = draw(), draw(), draw()
    c[:8000] = -(a[:8000] * b[:8000] * (1 + rng.normal(0, 1e-6, 8000))).astype(np.float32)        # heavy cancellation
    c[8000:12000] = (a[8000:12000] * b[8000:12000] * rng.choice([-1, 1], 4000) * 2.0 ** rng.integers(20, 28, 4000)).astype(np.float32)
    assert _same_bits(DO.fma32(a, b, c), _exact_fma(a, b, c))
    # results below 2^-126, where float32's last bit lies higher
    a, b, c = draw(-22, -19)[:4000], draw(-22, -19)[:4000], draw(-44, -38)[:4000]
    got = DO.fma32(a, b, c)
    assert (np.abs(got) < 2.0 ** -126).mean() > 0.3 and (got != 0).mean() > 0.9
    assert _same_bits(got, _exact_fma(a, b, c))
    assert DO.fma32(np.float32(3), np.float32(5), np.float32(-15)) == 0 and DO.fma32([1, 2], [3, 4], 1.0).dtype == np.float32


def test_fma32_in_the_double_rounding_case():
    """c with an odd (or even) last bit and a * b half an ulp of c, less or more than a term below 2^-53 relative: the float64
    sum lies exactly on a float32 tie and its own rounding error decides."""
    import dgcnn_oracle as DO
    u = 2.0 ** -23
    lo, hi = np.float32(1 - u), np.float32(1 + u)
    A, B, Cc = [], [], []
    for sc in (1.0, 2.0 ** -40, 2.0 ** 37):
        for sg in (1.0, -1.0):
            for c in (1 + u, 1 + 2 * u, 1 + 3 * u, 1.5 + u, 2 - u, 2 - 2 * u):
                for x, y in ((hi, lo), (hi, hi), (lo, lo)):               # a b = 2^-24 (1 - 2^-46), (1 + 2^-23)^2, (1 - 2^-23)^2
                    A.append(sg * sc * 2.0 ** -12 * x)
                    B.append(2.0 ** -12 * y)
                    Cc.append(sg * sc * c)
                    A.append(-sg * sc * 2.0 ** -12 * x)                     # ... and half an ulp below c
                    B.append(2.0 ** -12 * y)
                    Cc.append(sg * sc * c)
    a, b, c = (np.array(v, np.float32) for v in (A, B, Cc))
    assert np.array_equal(a.astype(np.float64), np.array(A)) and np.array_equal(c.astype(np.float64), np.array(Cc))
    want = _exact_fma(a, b, c)
    assert _same_bits(DO.fma32(a, b, c), want)
    naive = (a.astype(np.float64) * b + c).astype(np.float32)
    wrong = int((naive.view(np.uint32) != want.view(np.uint32)).sum())
    print("plain float32(float64(a) * b + c) is wrong on %d of %d crafted triples" % (wrong, len(a)))
    assert wrong >= 1
    one = DO.fma32(np.float32(2.0 ** -12) * hi, np.float32(2.0 ** -12) * lo, hi)      # the pair the contract names
    assert one == hi and np.float32(np.float64(np.float32(2.0 ** -12) * hi) * np.float64(np.float32(2.0 ** -12) * lo) + np.float64(hi)) != hi


def _lattice():
    rng = np.random.default_rng(5)                                                   # test_gpu_dgcnn's lattice
    return (rng.integers(0, 5, size=(257, 3)) * 0.25).astype(np.float32)


def test_header_neighbours_agree_with_the_oracle(g):
    import dgcnn_oracle as DO
    pcs = golden_clouds(g)
    o = DO.forward(DO.to_torch(DO.make_weights(0)), pcs)
    cols = ((0, 64), (64, 128), (128, 256))
    for i, c in enumerate(pcs):
        for l in range(4):
            x = c if l == 0 else o["feat"][i][:, cols[l - 1][0]:cols[l - 1][1]].numpy()
            idx = DO.header_neighbours(x, 20)
            DO.check_neighbours(x, idx, 20, "header, cloud %d layer %d" % (i, l + 1))
            assert DO.check_neighbours_exact(x, idx[:, ::-1], 20) >= 0
            s64 = DO.exact_scores(x)
            tau = DO.gamma(x.shape[1] + 2) * (np.sqrt((x.astype(np.float64) ** 2).sum(1))[:, None] + np.sqrt((x.astype(np.float64) ** 2).sum(1)).max()) ** 2
            assert (np.abs(DO.header_scores(x) - s64) <= tau).all()
    lat = _lattice()
    s = DO.exact_scores(lat)
    assert np.array_equal(DO.header_scores(lat).astype(np.float64), s)                # exact in float32 there
    got = DO.header_neighbours(lat, 20)
    for i in range(257):
        assert np.array_equal(got[i], np.sort(np.lexsort((np.arange(257), -s[i]))[:20])), i
    assert DO.check_neighbours_exact(lat, got, 20) > 100                              # ties everywhere on the lattice
    part = np.array([256, 0, 77])
    assert np.array_equal(DO.header_neighbours(lat, 20, part), got[part]) and np.array_equal(DO.header_scores(lat, part), DO.header_scores(lat)[part])


def test_exact_checker_refuses_planted_errors(g):
    import dgcnn_oracle as DO
    c = golden_clouds(g)[0]
    k, row = 20, 7
    S = DO.header_scores(c)
    good = DO.header_neighbours(c, k)
    assert DO.check_neighbours_exact(c, good, k) == int(DO.tied_rows(c, k).sum())
    order = np.lexsort((np.arange(len(c)), -S[row]))
    assert S[row, order[k - 1]] > S[row, order[k]]
    bad = good.copy()
    bad[row, np.nonzero(bad[row] == order[k - 1])[0][0]] = order[k]                    # the k-th swapped for the (k + 1)-th
    with pytest.raises(AssertionError, match="row %d" % row):
        DO.check_neighbours_exact(c, bad, k, what="swapped")
    DO.check_neighbours(c, good, k)
    dup = good.copy()
    dup[5, 1] = dup[5, 0]
    with pytest.raises(AssertionError, match="row 5"):
        DO.check_neighbours_exact(c, dup, k, what="repeated")
    with pytest.raises(AssertionError, match="row 2"):
        DO.check_neighbours_exact(c, good[[0, 1, 3]], k, rows=[0, 1, 2], what="another row's set")
    # a higher index among equal scores: the tolerance check cannot see it, the exact one does
    lat = _lattice()
    s = DO.exact_scores(lat)
    good = DO.header_neighbours(lat, k)
    tied = np.nonzero(DO.tied_rows(lat, k))[0]
    row = int(tied[0])
    order = np.lexsort((np.arange(257), -s[row]))
    assert s[row, order[k - 1]] == s[row, order[k]] and order[k - 1] < order[k]
    bad = good.copy()
    bad[row, np.nonzero(bad[row] == order[k - 1])[0][0]] = order[k]
    DO.check_neighbours(lat, bad, k)
    with pytest.raises(AssertionError, match="row %d: " % row):
        DO.check_neighbours_exact(lat, bad, k, what="higher index among equals")


def test_stress_inputs_meet_their_floors_and_the_trace_is_the_header():
    """The inputs of tests/test_gpu_dgcnn_exact.py section c, from the oracle alone: every query of the workgroup 448 .. 511
    meets the floor on layer 1, and the restated queue discipline ends with the header's sets."""
    import dgcnn_oracle as DO
    assert DO.CURVE_POINTS == 513 and list(DO.STRESS_GROUP[[0, -1]]) == [448, 511]
    for name, (k, L, counter, floor) in DO.STRESS.items():
        c, kk = DO.stress_cloud(name)
        assert kk == k and c.shape == (513, 3) and c.dtype == np.float32
        S = DO.header_scores(c, DO.STRESS_GROUP)
        tr = DO.wave_trace(S, k)
        print("%s: queued %d .. %d (%.2f .. %.2f of n - k), stale %d .. %d, applied %d .. %d, %d flushes"
              % (name, tr["queued"].min(), tr["queued"].max(), tr["queued"].min() / (513 - k), tr["queued"].max() / (513 - k),
                 tr["stale"].min(), tr["stale"].max(), tr["applied"].min(), tr["applied"].max(), tr["flushes"]))
        assert (tr[counter] >= floor).all(), (name, counter, int(tr[counter].min()), floor)
        assert np.array_equal(tr["queued"], tr["applied"] + tr["stale"])
        assert np.array_equal(tr["sets"], DO.header_neighbours(c, k, DO.STRESS_GROUP, scores=S)), name
        for rows in (np.arange(0, 64), np.arange(512, 513)):                         # the first workgroup, and the last (one query)
            S = DO.header_scores(c, rows)
            assert np.array_equal(DO.wave_trace(S, k)["sets"], DO.header_neighbours(c, k, rows, scores=S)), (name, rows[0])
    base = DO.curve_cloud()
    assert np.array_equal(DO.stress_cloud("approach, k = 20")[0], base)
    r8 = DO.stress_cloud("runs of 8, k = 5")[0]
    assert np.array_equal(r8[:5], base[:5]) and np.array_equal(r8[5:13], base[5:13][::-1]) and np.array_equal(r8[509:], base[509:][::-1])
    # the trace on other inputs: ties (the lattice), a cloud of exactly k points, pend = 1, random order for contrast
    lat = _lattice()
    for rows in (np.arange(64), np.arange(192, 256), np.arange(256, 257)):
        S = DO.header_scores(lat, rows)
        for pend in (1, 8):
            assert np.array_equal(DO.wave_trace(S, 20, pend)["sets"], DO.header_neighbours(lat, 20, rows, scores=S))
    S = DO.header_scores(base[:20])
    tr = DO.wave_trace(S, 20)
    assert np.array_equal(tr["sets"], np.tile(np.arange(20), (20, 1))) and tr["queued"].sum() == 0 and tr["flushes"] == 1
    rng = np.random.default_rng(1)
    sph = rng.normal(size=(513, 3))
    sph = (sph / np.linalg.norm(sph, axis=1)[:, None]).astype(np.float32)
    tr = DO.wave_trace(DO.header_scores(sph, DO.STRESS_GROUP), 20)
    print("random sphere, k = 20: queued %.2f of n - k, stale %.1f a query, %d flushes" % (tr["queued"].mean() / 493, tr["stale"].mean(), tr["flushes"]))


def test_translated_cloud_has_exact_ties_off_the_lattice():
    """The input of test_gpu_dgcnn_exact's tie test, from the oracle alone: far from the origin the scores cancel and exact ties
    at the k-th place occur on natural data."""
    import dgcnn_oracle as DO
    c = DO.translated_cloud()
    ties = int(DO.tied_rows(c, 20).sum())
    print("translated cloud: %d of %d rows tied at the 20th place in layer 1" % (ties, len(c)))
    assert ties >= 1


def test_tight_clouds_tell_the_header_from_its_near_misses():
    """The tight clouds of tests/test_gpu_dgcnn_exact.py, from the oracle alone (layer 1): a choice made with the channels summed
    in descending order, with |x_j|^2 as rounded products and sums, or with the highest index among equal scores differs from the
    header's, at 65 points for every k the GPU test runs and on its 96 rows at 2048 points.  On the natural clouds of the same
    sizes none of the three differs in a single row: there the exact check sees no more than the tolerance does."""
    import bench
    import dgcnn_oracle as DO
    s = bench.synth_clouds(24, seed=77)
    big = np.ascontiguousarray(np.concatenate([s[22], 0.7 * s[23] - 0.2]), dtype=np.float32)
    rows = np.concatenate([np.arange(32), np.arange(2016, 2048), np.sort(np.random.default_rng(2048).choice(np.arange(32, 2016), 32, replace=False))])

    def differing(x, k, rows):
        x = np.asarray(x, np.float32)
        S = DO.header_scores(x, rows)
        want = DO.header_neighbours(x, k, rows, scores=S)
        q = x if rows is None else x[rows]
        nrm = np.zeros(len(x), np.float32)
        d = np.zeros((len(q), len(x)), np.float32)
        for c in range(x.shape[1]):
            nrm = nrm + x[:, c] * x[:, c]
            d = DO.fma32(q[:, c:c + 1], x[None, :, c], d)
        unfused = np.float32(2) * d - nrm[None, :]
        highest = S.shape[1] - 1 - np.argsort(-S[:, ::-1], axis=1, kind="stable")        # score descending, index DEscending
        out = []
        for got in (DO.header_neighbours(x[:, ::-1].copy(), k, rows), DO.header_neighbours(x, k, rows, scores=unfused),
                    np.sort(highest[:, :k], axis=1)):
            out.append(int((got != want).any(1).sum()))
            if out[-1]:
                with pytest.raises(AssertionError):
                    DO.check_neighbours_exact(x, got, k, rows)
        return out
    total = np.zeros(3, int)
    for k in (1, 2, 3, 4, 5, 8, 9, 20, 31, 32):
        n = differing(DO.tight_cloud(s[9][:65]), k, None)
        print("tight 65 points, k = %2d: rows that differ (descending channels, unfused norm, highest index): %s" % (k, n))
        assert n[0] + n[1] >= 1, k
        total += n
        assert differing(s[9][:65], k, None) == [0, 0, 0]
    assert (total >= 10).all(), total
    n = differing(DO.tight_cloud(big), 20, rows)
    print("tight 2048 points, 96 rows: %s" % n)
    assert min(n) >= 32
    assert differing(big, 20, rows) == [0, 0, 0]
