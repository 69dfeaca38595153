"""CPU checks of the PointNet++ victim (include/ifd_pn2.h): the C ABI and its binding, the weight order and BatchNorm folding, the
oracle pinned to the reference's recorded run (selection tables equal, logits within the float32 error), the checker the GPU
tests rest on, and the host logic of the pointnet2_inference CLI."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_pn2.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointnet2_golden.npz")
N_WEIGHTS = 1469032
TABLES = ("fps1", "fps2", "ball1", "ball2")


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


def golden_tables(g):
    n = int(g["n_clouds"])
    return {k: np.stack([g["%s_%d" % (k, i)].astype(np.int32) for i in range(n)]) for k in TABLES}


# ---------------------------------------------------------------------------------------------- ABI
def test_pn2_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.PN2_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    assert I.PointNet2Classifier is I.runtime.PointNet2Classifier and I.PointNet2Classifier.MAX_POINTS == 2048


def test_pn2_abi_version_and_weight_count(lib):
    from ifdefense_amd import _lib, weights
    assert lib.ifd_pn2_abi_version() == 1 == _lib.PN2_ABI_VERSION
    assert lib.ifd_abi_version() == _lib.ABI_VERSION and lib.ifd_cls_abi_version() == _lib.CLS_ABI_VERSION
    assert lib.ifd_dgcnn_abi_version() == _lib.DGCNN_ABI_VERSION          # versioned on its own: the others are their own
    assert lib.ifd_pn2_weight_count() == N_WEIGHTS
    assert sum(int(np.prod(s)) for _, s in weights.pointnet2_canonical_keys()) == N_WEIGHTS
    assert "1,469,032" in open(HEADER).read()
    assert lib.ifd_cls_weight_count(_lib.CLS_POINTNET2, 0) == 0              # ... and PointNet++ is not behind ifd_cls_*


def test_pn2_create_rejects_bad_arguments_without_a_gpu(lib):
    """Every refusal comes before any HIP call: this test passes on a machine without a GPU."""
    import ifdefense_amd as I
    from ifdefense_amd import _lib
    w = np.zeros(N_WEIGHTS, np.float32)
    assert not lib.ifd_pn2_create(w.ctypes.data, 10, 40, 0)                  # wrong count
    assert str(N_WEIGHTS).encode() in lib.ifd_last_error(None) and b"got 10" in lib.ifd_last_error(None)
    assert not lib.ifd_pn2_create(None, N_WEIGHTS, 40, 0)
    assert b"NULL" in lib.ifd_last_error(None)
    assert not lib.ifd_pn2_create(w.ctypes.data, N_WEIGHTS, 10, 0)
    assert b"n_classes" in lib.ifd_last_error(None)
    assert lib.ifd_pn2_forward(None, None, None, None, 1, 1024, None, None, None) == -1
    with pytest.raises(I.IfdError, match="expected %d" % N_WEIGHTS):
        I.PointNet2Classifier(np.zeros(4, np.float32))
    # ifd_cls_create still refuses the model
    assert not lib.ifd_cls_create(w.ctypes.data, N_WEIGHTS, _lib.CLS_POINTNET2, 0, 40, 0)
    assert b"PointNet++" in lib.ifd_last_error(None) and b"are not" in lib.ifd_last_error(None)
    with pytest.raises(I.IfdError, match="not built"):
        I.Classifier(w, "pointnet2")


# ---------------------------------------------------------------------------------------------- fold and pack
def test_fold_against_a_hand_folded_layer_and_the_unfolded_network(g):
    import pointnet2_oracle as PO
    from ifdefense_amd import weights
    w = PO.make_weights(3)
    f = dict(weights.fold_pointnet2(w))
    assert [(k, a.shape) for k, a in weights.fold_pointnet2(w)] == weights.pointnet2_canonical_keys()
    # sa2's first layer by hand, in float64
    W = w["sa2.mlp_convs.0.weight"].reshape(128, 131).astype(np.float64)
    b = w["sa2.mlp_convs.0.bias"].astype(np.float64)
    ga, be = w["sa2.mlp_bns.0.weight"].astype(np.float64), w["sa2.mlp_bns.0.bias"].astype(np.float64)
    mu, var = w["sa2.mlp_bns.0.running_mean"].astype(np.float64), w["sa2.mlp_bns.0.running_var"].astype(np.float64)
    for o in (0, 77, 127):
        sc = ga[o] / np.sqrt(var[o] + 1e-5)
        assert np.array_equal(f["sa2.mlp_convs.0.weight"][o], W[o] * sc)
        assert f["sa2.mlp_convs.0.bias"][o] == (b[o] - mu[o]) * sc + be[o]
    assert np.abs(f["sa1.mlp_convs.0.weight"] - w["sa1.mlp_convs.0.weight"][:, :, 0, 0]).max() > 1e-3      # folding is not the identity
    assert np.array_equal(f["fc3.weight"], w["fc3.weight"]) and np.array_equal(f["fc3.bias"], w["fc3.bias"])
    # the folded network == the unfolded one in float64, the same tables forced
    pcs = golden_clouds(g)
    t = golden_tables(g)
    a = PO.forward(PO.to_torch(f, torch.float64), pcs, dtype=torch.float64, tables=t)
    b = PO.forward(PO.to_torch(w, torch.float64), pcs, dtype=torch.float64, tables=t)
    for name in ("logits", "global_feat", "l1_feat", "l2_feat"):
        rel = float((a[name] - b[name]).abs().max() / b[name].abs().max())
        print("%s: folded vs unfolded, relative %.3e" % (name, rel))
        assert rel <= 1e-12


def test_pack_prefix_order_round_trip_and_errors(tmp_path):
    import pointnet2_oracle as PO
    from ifdefense_amd import weights
    w = PO.make_weights(1)
    bare = weights.pack_state_dict(w, "pointnet2")
    assert bare.dtype == np.float32 and bare.size == N_WEIGHTS
    sd = PO.reference_state_dict(w)                           # module. prefix, [out, in, 1, 1] convolutions, num_batches_tracked
    assert all(k.startswith("module.") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    assert tuple(sd["module.sa1.mlp_convs.0.weight"].shape) == (64, 3, 1, 1) and "module.sa1.mlp_bns.0.running_mean" in sd
    assert np.array_equal(bare, weights.pack_state_dict(sd, "pointnet2")) and np.array_equal(bare, weights.pack_pointnet2(sd))
    # the canonical order: sa1's first layer in front, fc3 as it is at the end
    sc = w["sa1.mlp_bns.0.weight"].astype(np.float64) / np.sqrt(w["sa1.mlp_bns.0.running_var"].astype(np.float64) + 1e-5)
    assert np.array_equal(bare[:192], (w["sa1.mlp_convs.0.weight"].reshape(64, 3).astype(np.float64) * sc[:, None]).astype(np.float32).reshape(-1))
    assert np.array_equal(bare[192:256], ((w["sa1.mlp_convs.0.bias"].astype(np.float64) - w["sa1.mlp_bns.0.running_mean"]) * sc
                                          + w["sa1.mlp_bns.0.bias"]).astype(np.float32))
    assert np.array_equal(bare[-40 * 256 - 40:-40], w["fc3.weight"].reshape(-1)) and np.array_equal(bare[-40:], w["fc3.bias"])
    # .pth and .npz load alike
    p, q = str(tmp_path / "pn2.pth"), str(tmp_path / "pn2.npz")
    torch.save(sd, p)
    np.savez(q, **w)
    assert np.array_equal(bare, weights.load_checkpoint(p, "pointnet2")) and np.array_equal(bare, weights.load_checkpoint(q, "pointnet2"))
    # a key with and without the prefix, a missing key, a wrong shape
    bad = dict(sd)
    bad["fc1.weight"] = sd["module.fc1.weight"]
    with pytest.raises(ValueError, match="with and without"):
        weights.pack_pointnet2(bad)
    bad = dict(w)
    del bad["bn2.running_var"]
    with pytest.raises(KeyError):
        weights.pack_state_dict(bad, "pointnet2")
    bad = dict(w)
    bad["sa2.mlp_convs.0.weight"] = np.zeros((128, 128, 1, 1), np.float32)
    with pytest.raises(ValueError):
        weights.pack_state_dict(bad, "pointnet2")


def test_random_state_dict_is_the_oracle_recipe():
    import pointnet2_oracle as PO
    from ifdefense_amd import weights
    a, b = weights.pointnet2_random_state_dict(5), PO.make_weights(5)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["sa3.mlp_convs.0.weight"].shape == (256, 259, 1, 1) and "sa1.mlp_convs.0.bias" in a and "bn3.weight" not in a


# ---------------------------------------------------------------------------------------------- oracle against the fixture
def test_oracle_selection_equals_the_reference(g):
    """The header's definitions (difference-form distance, strict comparisons, lowest index) reproduce the reference's
    farthest_point_sample and query_ball_point on the six recorded clouds, index for index."""
    import pointnet2_oracle as PO
    pcs = golden_clouds(g)
    assert [len(c) for c in pcs] == [100, 100, 600, 600, 1024, 1024]
    t = PO.tables_of(pcs, fps_start=g["starts"])
    for k in TABLES:
        for i in range(len(pcs)):
            assert np.array_equal(t[k][i], g["%s_%d" % (k, i)].astype(np.int32)), (k, i)
    # both rules of the ball query are exercised: padded rows and truncated rows, at both levels
    for k, ns in (("ball1", 32), ("ball2", 64)):
        counts = np.concatenate([[len(set(r.tolist())) for r in t[k][i]] for i in range(len(pcs))])
        assert counts.min() < ns and counts.max() == ns
    assert len(set(t["fps1"][0].tolist())) == 100             # a cloud of 100 points: every point once, then repeats


def test_oracle_logits_against_the_reference(g):
    """The bar is the oracle's own float32 error: 4 x e_32, e_32 = max |float32 oracle - float64 oracle| on the same tables."""
    import pointnet2_oracle as PO
    w = PO.make_weights(int(g["weight_seed"]))
    pcs, t = golden_clouds(g), golden_tables(g)
    o = PO.forward(PO.to_torch(w), pcs, tables=t)
    o64 = PO.forward(PO.to_torch(w, torch.float64), pcs, dtype=torch.float64, tables=t)
    for name in ("logits", "global_feat"):
        e32 = float((o[name].double() - o64[name]).abs().max())
        d = float(np.abs(o[name].numpy() - g[name]).max())
        print("%s: oracle vs reference %.3e, e_32 %.3e" % (name, d, e32))
        assert e32 > 0 and d <= 4 * e32
    free = PO.forward(PO.to_torch(w), pcs, fps_start=g["starts"])            # ... and left to choose, it chooses the same
    assert torch.equal(free["logits"], o["logits"])


def test_table_checker_accepts_the_oracle_and_catches_planted_errors(g):
    import pointnet2_oracle as PO
    pcs, t = golden_clouds(g), golden_tables(g)
    for i, c in enumerate(pcs):
        PO.check_tables(c, {k: t[k][i] for k in TABLES}, g["starts"][i], "reference, cloud %d" % i)
    i, c = 4, pcs[4]                                          # 1024 points: full rows and padded rows at both levels
    good = {k: t[k][i].copy() for k in TABLES}

    def planted(change):
        bad = {k: v.copy() for k, v in good.items()}
        change(bad)
        with pytest.raises(AssertionError):
            PO.check_tables(c, bad, g["starts"][i], "planted")

    def swap_picks(b):
        b["fps1"][[7, 8]] = b["fps1"][[8, 7]]
    planted(swap_picks)

    def swap_level2_picks(b):
        b["fps2"][[100, 101]] = b["fps2"][[101, 100]]
    planted(swap_level2_picks)
    full = int(np.flatnonzero([len(set(r.tolist())) == 32 for r in good["ball1"]])[0])
    short = int(np.flatnonzero([1 < len(set(r.tolist())) < 32 for r in good["ball1"]])[0])

    def out_of_order(b):
        b["ball1"][full, [3, 4]] = b["ball1"][full, [4, 3]]
    planted(out_of_order)

    def wrong_pad(b):
        b["ball1"][short, -1] = b["ball1"][short, 1]          # a member, but not the first
    planted(wrong_pad)

    def wrong_pad_level2(b):
        rows = np.flatnonzero([1 < len(set(r.tolist())) < 64 for r in b["ball2"]])
        b["ball2"][rows[0], -1] = b["ball2"][rows[0], 1]
    planted(wrong_pad_level2)
    with pytest.raises(AssertionError):
        PO.check_tables(c, good, (int(g["starts"][i][0]) + 1, int(g["starts"][i][1])), "another start")


def test_distance_definition():
    """dist rounds every step to float32; a point and its bit-identical copy are at distance exactly 0; r2 is the float of the
    double product."""
    import pointnet2_oracle as PO
    rng = np.random.default_rng(0)
    x = rng.normal(size=(200, 3)).astype(np.float32)
    c = rng.normal(size=3).astype(np.float32)
    d = x - c
    want = np.float32(np.float32(d[:, 0] * d[:, 0]) + np.float32(d[:, 1] * d[:, 1])) + np.float32(d[:, 2] * d[:, 2])
    assert PO.dist(x, c).dtype == np.float32 and np.array_equal(PO.dist(x, c), want.astype(np.float32))
    assert (PO.dist(x, x[5])[5] == 0) and PO.dist(np.stack([x[5], x[5]]), x[5]).max() == 0
    assert PO.radius2(0.2) == np.float32(0.2 * 0.2) and PO.radius2(0.4) == np.float32(0.4 * 0.4)
    assert PO.radius2(0.2).dtype == np.float32


def test_wrong_distances_round_differently():
    """The four wrong distances are what their names say: each stays within a few float32 steps of dist (the matrix form within
    its cancellation error) and differs from it somewhere on a non-dyadic lattice, and each is 0 on a copy but for the matrix
    form's bound; the contracted chain is the correctly rounded fma chain."""
    import pointnet2_oracle as PO
    from dgcnn_oracle import fma32
    x = PO.lattice_cloud(3, 12, 400, 0.2 / 3, -0.4)
    c = x[17]
    d = PO.dist(x, c)
    exact = ((x.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1)
    ulp = np.spacing(np.maximum(d, np.float32(1e-30)))
    for name, f in PO.DIST_MUTANTS.items():
        got = f(x, c)
        assert got.dtype == np.float32 and got.shape == d.shape, name
        assert np.array_equal(f(x[None, :, :], x[:5, None, :])[3], f(x, x[3])), name      # the grouping's broadcast
        n_diff = int((got != d).sum())
        print("%s: %d of %d distances differ from the header's" % (name, n_diff, len(d)))
        assert n_diff > 0, name
        if name == "matrix":
            bound = 2.0 ** -21 * ((x.astype(np.float64) ** 2).sum(1) + float((c.astype(np.float64) ** 2).sum()))
            assert (np.abs(got - exact) <= bound).all()
        else:
            assert (np.abs(got.astype(np.float64) - d) <= 8 * ulp).all(), name        # a sanity bound, not a sharp one
            assert got[17] == 0
    dx, dy, dz = (x - c).T
    assert np.array_equal(PO.dist_contracted(x, c), fma32(dz, dz, fma32(dy, dy, (dx * dx).astype(np.float32))))
    assert np.array_equal(PO.dist_float64(x, c), exact.astype(np.float32))
    # the rule mutants on three points at equal distance from the first
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    assert PO.fps(t, 2, 0).tolist() == [0, 1] and PO.fps_highest(t, 2, 0).tolist() == [0, 3]
    edge = np.array([[0, 0, 0], [np.sqrt(PO.radius2(0.5)), 0, 0]], np.float32)               # 0.5 exactly: d == r2
    assert PO.ball(0.5, 2, edge, edge[:1]).tolist() == [[0, 1]] and PO.ball(0.5, 2, edge, edge[:1], open_edge=True).tolist() == [[0, 0]]


def test_lattice_family_refuses_every_wrong_definition():
    """The condition the GPU's selection tests rest on (test_gpu_pointnet2.py, section 1b).  With every earlier stage forced to the
    header's result, every wrong distance changes fps1, fps2, ball1 and ball2, and every rule mutant its own tables, on at least
    one cloud of LATTICE_FAMILY in each stride class: a GPU that equals the header oracle on the family computes the header's
    distance and rules, not one of these.  The tie lattice refuses the sampling's rule mutant too; it has no point at d == r2."""
    import pointnet2_oracle as PO
    fam = PO.LATTICE_FAMILY
    assert [f[2] for f in fam] == [20, 33, 100, 300, 512, 513, 1024, 1025, 2048]
    assert {0.04, 0.2 / 3} <= {f[3] for f in fam}
    for i, f in enumerate(fam):
        x = PO.family_cloud(i)[0]
        assert x.shape == (f[2], 3) and x.dtype == np.float32 and len(np.unique(x, axis=0)) == f[2]      # distinct places
    tables = ("fps1", "fps2", "ball1", "ball2")
    cells = PO.certify(range(len(fam)), PO.ball_refusals, tables)
    want = {(m, t) for m in PO.DIST_MUTANTS for t in tables} | {(PO.RULE_FPS, "fps1"), (PO.RULE_FPS, "fps2"),
                                                               (PO.RULE_BALL, "ball1"), (PO.RULE_BALL, "ball2")}
    assert set(cells) == want
    tie = PO.ball_refusals("dyadic")
    print("tie lattice:", tie)
    assert tie[PO.RULE_FPS]["fps1"] > 0 and tie[PO.RULE_FPS]["fps2"] > 0


def test_calibrated_weights_give_varied_predictions():
    """The calibrated head alone (no GPU): on bench.synth_clouds(64, seed=23)[:, :128] the float64 oracle predicts at least 10
    classes; fc3 alone differs from make_weights."""
    import bench
    import pointnet2_oracle as PO
    sd = PO.make_calibrated_weights(0)
    base = PO.make_weights(0)
    assert all(np.array_equal(sd[k], base[k]) for k in sd if not k.startswith("fc3."))
    x = np.ascontiguousarray(bench.synth_clouds(64, seed=23)[:, :128])
    lo64 = PO.forward(PO.to_torch(sd, torch.float64), x, dtype=torch.float64)["logits"]
    classes = len(set(lo64.argmax(1).tolist()))
    print("classes predicted on 64 clouds: %d" % classes)
    assert classes >= 10
    tied = PO.make_tied_weights(sd)
    assert np.array_equal(tied["fc3.weight"][20:], tied["fc3.weight"][:20]) and np.array_equal(tied["fc3.bias"][20:], tied["fc3.bias"][:20])


# ---------------------------------------------------------------------------------------------- CLI host logic
class StubClassifier:
    """Stands in for runtime.PointNet2Classifier: the class of a cloud is its number of rows modulo 40."""

    def __init__(self):
        self.seen = None
        self.starts = []
        self.closed = False

    def predict(self, clouds, fps_start=None):
        self.seen = [np.asarray(c) for c in clouds]
        self.starts.append(np.asarray(fps_start))
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
    from ifdefense_amd import pointnet2_inference as Inf
    made = []

    def make(model, path):
        made.append((model, path, StubClassifier()))
        return made[-1][2]
    # the model named by the path; a cluster file takes 1120 rows -> class 0
    p = str(tmp_path / "cluster-PointNet2-x.npz")
    _write(p, [1120] * 7, [0, 0, 0, 5, 5, 5, 5], [5, 0, 5, 0, 1, 1, 1], cols=6)
    assert Inf.main(["--data_root", p, "--mode", "target"], make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % (3 / 7, 2 / 7)
    model, path, stub = made[-1]
    assert (model, path) == ("pointnet2", "pretrain/mn40/pointnet2.pth") and stub.closed
    assert all(c.shape == (1120, 3) and c.dtype == np.float32 for c in stub.seen)
    assert np.array_equal(stub.starts[-1], Inf.fps_starts(1, [1120] * 7))     # the default seed is 1
    # normal mode, explicit model / weights / num_points / seed, ragged SOR file
    p = str(tmp_path / "sor_x.npz")
    _write(p, [50, 45, 41], [10, 5, 2], ragged=True)
    assert Inf.main(["--data_root", p, "--model", "pointnet2", "--model_path", "w.npz", "--num_points", "45", "--dataset", "opt_mn40",
                     "--fps_seed", "9"], make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f\n" % (1 / 3)      # rows taken: 45, 45, 41 -> classes 5, 5, 1
    assert made[-1][:2] == ("pointnet2", "w.npz") and [len(c) for c in made[-1][2].seen] == [45, 45, 41]
    assert np.array_equal(made[-1][2].starts[-1], Inf.fps_starts(9, [45, 45, 41]))
    assert not np.array_equal(Inf.fps_starts(9, [45, 45, 41]), Inf.fps_starts(1, [45, 45, 41]))
    assert Inf.main(["--data_root", p, "--model", "pointnet2", "--dataset", "conv_opt_mn40"], make_classifier=make) == 0
    assert made[-1][1] == "pretrain/conv_opt_mn40/pointnet2.pth"
    capsys.readouterr()


def test_fps_starts_depend_on_seed_position_and_count_only():
    from ifdefense_amd import pointnet2_inference as Inf
    sizes = [1024, 100, 1, 2048, 600, 100]
    s = Inf.fps_starts(1, sizes)
    assert s.shape == (6, 2) and s.dtype == np.int32
    assert (s[:, 0] >= 0).all() and (s[:, 0] < np.array(sizes)).all() and (s[:, 1] >= 0).all() and (s[:, 1] < 512).all()
    assert np.array_equal(s, Inf.fps_starts(1, sizes))
    # a cloud's starts do not depend on how many clouds follow it, nor on the other clouds' sizes: batching cannot matter
    assert np.array_equal(Inf.fps_starts(1, sizes[:3]), s[:3])
    other = Inf.fps_starts(1, [7, 100, 9, 2048, 5, 100])
    assert np.array_equal(other[[1, 3, 5]], s[[1, 3, 5]])
    many = Inf.fps_starts(1, [1024] * 400)
    assert len(set(many[:, 0].tolist())) > 100 and len(set(many[:, 1].tolist())) > 100


def test_cli_refusals(tmp_path, capsys):
    from ifdefense_amd import pointnet2_inference as Inf

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv, where in ((["--data_root", "x.npz", "--model", "pointnet"], "ifdefense_amd.inference"),
                        (["--data_root", "a/kNN-dgcnn.npz"], "ifdefense_amd.dgcnn_inference"),
                        (["--data_root", "pointnet2.npz", "--model", "pointconv"], "baselines/inference.py")):
        assert Inf.main(argv, make_classifier=never) == 2
        assert where in capsys.readouterr().err
    assert Inf.main(["--data_root", "nothing.npz"], make_classifier=never) == 2
    assert "not recognized" in capsys.readouterr().err
    # a cloud of more than 2048 points: refused with a message, the classifier closed, nothing run
    p = str(tmp_path / "sor-pointnet2.npz")
    _write(p, [50, 2049, 41], [10, 5, 2], ragged=True)
    stub = StubClassifier()
    assert Inf.main(["--data_root", p, "--num_points", "4096"], make_classifier=lambda *a: stub) == 2
    err = capsys.readouterr().err
    assert "cloud 1 has 2049 points, more than the 2048" in err and stub.closed and stub.seen is None
    assert Inf.main(["--data_root", p, "--num_points", "2048"], make_classifier=lambda *a: StubClassifier()) == 0
    capsys.readouterr()
    # target mode without target_label
    assert Inf.main(["--data_root", p, "--mode", "target"], make_classifier=lambda *a: StubClassifier()) == 2
    assert "target_label" in capsys.readouterr().err
    # the other CLIs point here, and keep their own words
    from ifdefense_amd import dgcnn_inference, inference
    assert inference.main(["--data_root", "x.npz", "--model", "pointnet2"], make_classifier=never) == 2
    err = capsys.readouterr().err
    assert "not built" in err and "ifdefense_amd.pointnet2_inference" in err
    assert inference.main(["--data_root", "x.npz", "--model", "pointconv"], make_classifier=never) == 2
    assert "not built" in capsys.readouterr().err
    assert dgcnn_inference.main(["--data_root", "x.npz", "--model", "pointnet2"], make_classifier=never) == 2
    err = capsys.readouterr().err
    assert "ifdefense_amd.inference" in err and "ifdefense_amd.pointnet2_inference" in err
