"""CPU checks of the PointConv victim (include/ifd_pc.h): the C ABI and its binding, the weight order and BatchNorm folding, the
oracle pinned to the reference's recorded run (sampling equal, neighbour rows equal as sets unless undecided, densities, global
feature and logits within the float32 error), the seeded weights keeping the network alive, the checker the GPU tests rest on,
and the host logic of the pointconv_inference CLI."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_pc.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointconv_golden.npz")
N_WEIGHTS = 19559411
TABLES = ("fps1", "fps2", "knn1", "knn2")


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


@pytest.fixture(scope="module")
def runs(g):
    """The float32 and the float64 oracle on the golden clouds with the reference's tables forced: computed once, shared."""
    import pointconv_oracle as PO
    w = PO.make_weights(int(g["weight_seed"]))
    pcs, t = golden_clouds(g), golden_tables(g)
    o32 = PO.forward(PO.to_torch(w), pcs, tables=t)
    o64 = PO.forward(PO.to_torch(w, torch.float64), pcs, dtype=torch.float64, tables=t)
    return w, o32, o64


# ---------------------------------------------------------------------------------------------- ABI
def test_pc_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.PC_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported
    assert I.PointConvClassifier is I.runtime.PointConvClassifier
    assert (I.PointConvClassifier.MAX_POINTS, I.PointConvClassifier.MIN_POINTS) == (2048, 32)
    head = open(HEADER).read()
    assert "#define IFD_PC_CHUNK %d" % _lib.PC_CHUNK in head and I.PointConvClassifier.CHUNK == _lib.PC_CHUNK
    assert "#define IFD_MODEL_PC 6" in head and "#define IFD_PC_MIN_POINTS 32" in head and "#define IFD_PC_MAX_POINTS 2048" in head


def test_pc_abi_version_and_weight_count(lib):
    from ifdefense_amd import _lib, weights
    assert lib.ifd_pc_abi_version() == 1 == _lib.PC_ABI_VERSION
    assert lib.ifd_pn2_abi_version() == _lib.PN2_ABI_VERSION and lib.ifd_cls_abi_version() == _lib.CLS_ABI_VERSION
    assert lib.ifd_pc_weight_count() == N_WEIGHTS == weights.pointconv_weight_count()
    assert sum(int(np.prod(s)) for _, s in weights.pointconv_canonical_keys()) == N_WEIGHTS
    head = open(HEADER).read()
    assert "19,559,411" in head
    per = {}
    for name, shape in weights.pointconv_canonical_keys():
        per[name.split(".")[0]] = per.get(name.split(".")[0], 0) + int(np.prod(shape))
    assert (per["sa1"], per["sa2"], per["sa3"], per["fc1"] + per["fc2"] + per["fc3"]) == (275353, 1115609, 17502041, 666408)
    assert all(format(v, ",") in head for v in (275353, 1115609, 17502041, 666408))
    dn = sum(int(np.prod(s)) for k, s in weights.pointconv_canonical_keys() if k.startswith("sa1.densitynet."))
    wn = sum(int(np.prod(s)) for k, s in weights.pointconv_canonical_keys() if k.startswith("sa3.weightnet."))
    assert (dn, wn) == (97, 248)
    assert lib.ifd_cls_weight_count(_lib.CLS_POINTCONV, 0) == 0               # ... and PointConv is not behind ifd_cls_*


def test_pc_create_rejects_bad_arguments_without_a_gpu(lib):
    """Every refusal comes before any HIP call: this test passes on a machine without a GPU."""
    import ifdefense_amd as I
    from ifdefense_amd import _lib
    w = np.zeros(N_WEIGHTS, np.float32)
    assert not lib.ifd_pc_create(w.ctypes.data, 10, 40, 0)                   # wrong count
    assert str(N_WEIGHTS).encode() in lib.ifd_last_error(None) and b"got 10" in lib.ifd_last_error(None)
    assert not lib.ifd_pc_create(None, N_WEIGHTS, 40, 0)
    assert b"NULL" in lib.ifd_last_error(None)
    assert not lib.ifd_pc_create(w.ctypes.data, N_WEIGHTS, 10, 0)
    assert b"n_classes" in lib.ifd_last_error(None)
    assert lib.ifd_pc_forward(None, None, None, None, 1, 1024, None, None, None) == -1
    with pytest.raises(I.IfdError, match="expected %d" % N_WEIGHTS):
        I.PointConvClassifier(np.zeros(4, np.float32))
    # ifd_cls_create still refuses the model, in its own words
    assert not lib.ifd_cls_create(w.ctypes.data, N_WEIGHTS, _lib.CLS_POINTCONV, 0, 40, 0)
    assert b"PointConv" in lib.ifd_last_error(None) and b"are not" in lib.ifd_last_error(None)
    with pytest.raises(I.IfdError, match="not built"):
        I.Classifier(w, "pointconv")


# ---------------------------------------------------------------------------------------------- fold and pack
def test_fold_against_a_hand_folded_layer_and_the_unfolded_network(g):
    import pointconv_oracle as PO
    from ifdefense_amd import weights
    w = PO.make_weights(3)
    f = dict(weights.fold_pointconv(w))
    assert [(k, a.shape) for k, a in weights.fold_pointconv(w)] == weights.pointconv_canonical_keys()
    # sa2's linear and its DensityNet's middle layer by hand, in float64
    for lin, bn, shape in (("sa2.linear", "sa2.bn_linear", (256, 4096)), ("sa2.densitynet.mlp_convs.1", "sa2.densitynet.mlp_bns.1", (8, 8))):
        W = w[lin + ".weight"].reshape(shape).astype(np.float64)
        b = w[lin + ".bias"].astype(np.float64)
        ga, be = w[bn + ".weight"].astype(np.float64), w[bn + ".bias"].astype(np.float64)
        mu, var = w[bn + ".running_mean"].astype(np.float64), w[bn + ".running_var"].astype(np.float64)
        for o in (0, 3, shape[0] - 1):
            sc = ga[o] / np.sqrt(var[o] + 1e-5)
            assert np.array_equal(f[lin + ".weight"][o], W[o] * sc)
            assert f[lin + ".bias"][o] == (b[o] - mu[o]) * sc + be[o]
    assert np.abs(f["sa1.mlp_convs.0.weight"] - w["sa1.mlp_convs.0.weight"][:, :, 0, 0]).max() > 1e-3      # folding is not the identity
    assert np.array_equal(f["fc3.weight"], w["fc3.weight"]) and np.array_equal(f["fc3.bias"], w["fc3.bias"])
    # the folded network == the unfolded one in float64, the same tables forced
    pcs = golden_clouds(g)[:4]
    t = {k: v[:4] for k, v in golden_tables(g).items()}
    a = PO.forward(PO.to_torch(f, torch.float64), pcs, dtype=torch.float64, tables=t)
    b = PO.forward(PO.to_torch(w, torch.float64), pcs, dtype=torch.float64, tables=t)
    for name in ("logits", "global_feat", "l1_feat", "l2_feat", "dens1", "dens2", "dens3"):
        rel = float((a[name] - b[name]).abs().max() / b[name].abs().max())
        print("%s: folded vs unfolded, relative %.3e" % (name, rel))
        assert rel <= 1e-12


def test_pack_prefix_order_round_trip_and_errors(tmp_path):
    import pointconv_oracle as PO
    from ifdefense_amd import weights
    w = PO.make_weights(1)
    bare = weights.pack_state_dict(w, "pointconv")
    assert bare.dtype == np.float32 and bare.size == N_WEIGHTS
    sd = PO.reference_state_dict(w)                           # module. prefix, Conv1d / Conv2d / Linear shapes, num_batches_tracked
    assert all(k.startswith("module.") for k in sd) and any(k.endswith("num_batches_tracked") for k in sd)
    assert tuple(sd["module.sa1.densitynet.mlp_convs.0.weight"].shape) == (8, 1, 1)
    assert tuple(sd["module.sa1.mlp_convs.0.weight"].shape) == (64, 3, 1, 1)
    assert tuple(sd["module.sa3.weightnet.mlp_convs.2.weight"].shape) == (16, 8, 1, 1)
    assert tuple(sd["module.sa3.linear.weight"].shape) == (1024, 16384) and "module.sa3.bn_linear.running_mean" in sd
    assert np.array_equal(bare, weights.pack_state_dict(sd, "pointconv")) and np.array_equal(bare, weights.pack_pointconv(sd))
    # the canonical order: per level densitynet, mlp, weightnet, linear; sa1's DensityNet in front, fc3 as it is at the end
    names = [k for k, _ in weights.pointconv_canonical_keys()][0:20:2]
    assert names == ["sa1.densitynet.mlp_convs.%d.weight" % i for i in range(3)] + ["sa1.mlp_convs.%d.weight" % i for i in range(3)] + \
        ["sa1.weightnet.mlp_convs.%d.weight" % i for i in range(3)] + ["sa1.linear.weight"]
    f = dict(weights.fold_pointconv(w))
    assert np.array_equal(bare[:8], f["sa1.densitynet.mlp_convs.0.weight"].astype(np.float32).reshape(-1))
    assert np.array_equal(bare[8:16], f["sa1.densitynet.mlp_convs.0.bias"].astype(np.float32))
    assert np.array_equal(bare[97:97 + 192], f["sa1.mlp_convs.0.weight"].astype(np.float32).reshape(-1))
    assert np.array_equal(bare[275353:275353 + 8], f["sa2.densitynet.mlp_convs.0.weight"].astype(np.float32).reshape(-1))
    assert np.array_equal(bare[-40 * 256 - 40:-40], w["fc3.weight"].reshape(-1)) and np.array_equal(bare[-40:], w["fc3.bias"])
    # .pth and .npz load alike
    p, q = str(tmp_path / "pc.pth"), str(tmp_path / "pc.npz")
    torch.save(sd, p)
    np.savez(q, **w)
    assert np.array_equal(bare, weights.load_checkpoint(p, "pointconv")) and np.array_equal(bare, weights.load_checkpoint(q, "pointconv"))
    # a key with and without the prefix, a missing key, a wrong shape
    bad = dict(sd)
    bad["fc1.weight"] = sd["module.fc1.weight"]
    with pytest.raises(ValueError, match="with and without"):
        weights.pack_pointconv(bad)
    bad = dict(w)
    del bad["sa2.bn_linear.running_var"]
    with pytest.raises(KeyError):
        weights.pack_state_dict(bad, "pointconv")
    bad = dict(w)
    bad["sa2.weightnet.mlp_convs.0.weight"] = np.zeros((8, 3, 1), np.float32)
    with pytest.raises(ValueError):
        weights.pack_state_dict(bad, "pointconv")


def test_random_state_dict_is_the_oracle_recipe():
    import pointconv_oracle as PO
    from ifdefense_amd import weights
    a, b = weights.pointconv_random_state_dict(5), PO.make_weights(5)
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert a["sa3.mlp_convs.0.weight"].shape == (256, 259, 1, 1) and "sa1.linear.bias" in a and "bn3.weight" not in a


# ---------------------------------------------------------------------------------------------- oracle against the fixture
def test_oracle_fps_equals_the_reference(g):
    import pointconv_oracle as PO
    pcs = golden_clouds(g)
    assert [len(c) for c in pcs] == [32, 100, 600, 600, 1024, 1024, 1024, 1024]
    for i, c in enumerate(pcs):
        f1 = PO.fps(c, 512, g["starts"][i][0])
        assert np.array_equal(f1, g["fps1_%d" % i].astype(np.int32)), i
        assert np.array_equal(PO.fps(c[f1], 128, g["starts"][i][1]), g["fps2_%d" % i].astype(np.int32)), i
    assert len(set(g["fps1_0"].tolist())) == 32                # a cloud of 32 points: every point once, then repeats


def undecided(x, centre, k):
    """The gap in oracle distance between the k-th and the next DISTINCT point (as coordinates) of a centre's list is at most
    2^-20 (|c|^2 + max_j |x_j|^2): 16 float32 epsilons of the matrix form's operands."""
    import pointconv_oracle as PO
    d = np.sort(PO.dist(x, centre).astype(np.float64))
    later = d[k:][d[k:] > d[k - 1]]
    if later.size == 0:
        return True
    return later[0] - d[k - 1] <= 2.0 ** -20 * (float((centre.astype(np.float64) ** 2).sum()) + float((x.astype(np.float64) ** 2).sum(1).max()))


def test_oracle_knn_rows_equal_the_reference(g):
    """As sorted lists of underlying cloud point ids (level 2 mapped through fps1: bit-identical copies are interchangeable); a
    row may differ only where it is undecided, and at most 1 % of a level's rows of a cloud."""
    import pointconv_oracle as PO
    for i, c in enumerate(golden_clouds(g)):
        t = PO.tables_of_cloud(c, g["starts"][i])
        f1 = t["fps1"]
        c1 = c[f1]
        for name, k, src, ids, centres in (("knn1", 32, c, np.arange(len(c)), c1), ("knn2", 64, c1, f1, c1[t["fps2"]])):
            mine = np.sort(ids[t[name]], axis=1)
            ref = np.sort(ids[g["%s_%d" % (name, i)].astype(np.int32)], axis=1)
            differ = np.flatnonzero((mine != ref).any(axis=1))
            n_und = sum(undecided(src, centres[r], k) for r in range(len(centres))) if len(c) == 1024 and i == 4 else None
            print("cloud %d (n = %d) %s: %d rows differ%s" % (i, len(c), name, len(differ), "" if n_und is None else ", %d undecided" % n_und))
            assert len(differ) <= len(centres) // 100, (i, name, len(differ))
            for r in differ:
                assert undecided(src, centres[r], k), (i, name, int(r))


def test_oracle_outputs_against_the_reference(g, runs):
    """The bar is the oracle's own float32 error: 4 x e_32, e_32 = max |float32 oracle - float64 oracle| on the same tables."""
    w, o, o64 = runs
    n = int(g["n_clouds"])
    sizes = [len(c) for c in golden_clouds(g)]
    ref = {"logits": g["logits"], "global_feat": g["global_feat"]}
    for lev, cols in ((1, None), (2, 512), (3, 128)):
        r = np.zeros((n, max(sizes) if cols is None else cols), np.float32)
        for i in range(n):
            v = g["dens%d_%d" % (lev, i)]
            r[i, :len(v)] = v
        ref["dens%d" % lev] = r
    for name in ("logits", "global_feat", "dens1", "dens2", "dens3"):
        e32 = float((o[name].double() - o64[name]).abs().max())
        d = float(np.abs(o[name].numpy() - ref[name]).max())
        print("%s: oracle vs reference %.3e, e_32 %.3e, ratio %.2f" % (name, d, e32, d / e32))
        assert e32 > 0 and d <= 4 * e32


def test_seeded_weights_keep_the_network_alive(g, runs):
    """DensityNet ends in a ReLU and its output multiplies every feature: on the golden clouds each level's s_j is positive on
    more than half of the points and not constant, and the global feature is not zero."""
    w, o, o64 = runs
    sizes = [len(c) for c in golden_clouds(g)]
    for b, n in enumerate(sizes):
        for name, m in (("dens1", n), ("dens2", 512), ("dens3", 128)):
            s = o64[name][b, :m]
            assert float((s > 0).double().mean()) > 0.5, (b, name)
            assert float(s.max() - s.min()) > 1e-3 * float(s.max()), (b, name)
        gf = o64["global_feat"][b]
        assert float(gf.abs().max()) > 0 and float((gf > 0).double().mean()) > 0.1, b
    for seed in (1, 2, 3):                                     # ... and under other seeds the DensityNets are alive by construction
        import pointconv_oracle as PO
        ws = PO.make_weights(seed)
        assert all((ws[k] >= 0).all() for k in ws if ".densitynet.mlp_convs." in k)


def test_table_checker_accepts_the_oracle_and_catches_planted_errors(g):
    import pointconv_oracle as PO
    pcs = golden_clouds(g)
    i, c = 4, pcs[4]
    good = PO.tables_of_cloud(c, g["starts"][i])
    PO.check_tables(c, good, g["starts"][i], "oracle, cloud %d" % i)

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

    def out_of_order(b):
        b["knn1"][5, [3, 4]] = b["knn1"][5, [4, 3]]
    planted(out_of_order)

    def wrong_member(b):
        row = set(b["knn1"][9].tolist())
        b["knn1"][9, -1] = next(j for j in range(len(c)) if j not in row)
    planted(wrong_member)

    def out_of_order_level2(b):
        b["knn2"][0, [62, 63]] = b["knn2"][0, [63, 62]]
    planted(out_of_order_level2)

    def not_itself_first(b):
        b["knn1"][3, 0] = b["knn1"][3, 1]
    planted(not_itself_first)
    with pytest.raises(AssertionError):
        PO.check_tables(c, good, (int(g["starts"][i][0]) + 1, int(g["starts"][i][1])), "another start")
    assert np.array_equal(good["knn1"][:, 0], good["fps1"])    # entry 0 of a row is the centroid itself (no copies in this cloud)
    # n = 32: every row is all 32 points; copies: the lower index first
    t = PO.tables_of_cloud(pcs[0], g["starts"][0])
    assert np.array_equal(np.sort(t["knn1"], axis=1), np.tile(np.arange(32), (512, 1)))
    twins = np.concatenate([pcs[1][:50], pcs[1][:50]])
    k = PO.knn(4, twins, twins[60:61])
    assert k[0, 0] == 10 and k[0, 1] == 60


def test_lattice_family_refuses_every_wrong_definition():
    """The condition the GPU's selection tests rest on (test_gpu_pointconv.py, section 1b), as in test_pointnet2_cpu.py with the kNN
    as the grouping: every wrong distance changes fps1, fps2, knn1 and knn2, and every rule mutant its own tables, on at least
    one cloud of the family (from 33 points on) in each stride class.  The tie lattice refuses both rule mutants too."""
    import pointconv_oracle as PO
    clouds = [i for i, f in enumerate(PO.LATTICE_FAMILY) if f[2] >= PO.K1]
    assert [PO.LATTICE_FAMILY[i][2] for i in clouds] == [33, 100, 300, 512, 513, 1024, 1025, 2048]
    cells = PO.certify(clouds, PO.knn_refusals, TABLES)
    assert set(cells) == {(m, t) for m in PO.DIST_MUTANTS for t in TABLES} | {(PO.RULE_FPS, "fps1"), (PO.RULE_FPS, "fps2"),
                                                                             (PO.RULE_KNN, "knn1"), (PO.RULE_KNN, "knn2")}
    tie = PO.knn_refusals("dyadic")
    print("tie lattice:", tie)
    assert all(tie[PO.RULE_FPS][t] > 0 for t in ("fps1", "fps2")) and all(tie[PO.RULE_KNN][t] > 0 for t in ("knn1", "knn2"))
    t = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    assert PO.knn(3, t, t[:1]).tolist() == [[0, 1, 2]] and PO.knn_higher_first(3, t, t[:1]).tolist() == [[0, 3, 2]]


def test_density_header_and_identity_density_weights(g, runs):
    """density_header is the header's density in numpy float32; make_identity_density_weights turns every DensityNet into the
    identity, in the packed image exactly, so that the GPU's dens outputs are rho itself (test_gpu_pointconv.py, section 3b)."""
    import pointconv_oracle as PO
    from ifdefense_amd import weights
    w, o32, o64 = runs
    ident = PO.make_identity_density_weights(w)
    assert all(np.array_equal(ident[k], w[k]) for k in w if ".densitynet." not in k) and ident.keys() == w.keys()
    # the packed image: 97 floats in front of every level, {[8][1], [8], [8][8], [8], [1][8], [1]}
    img = weights.pack_state_dict(ident, "pointconv")
    want = np.zeros(97, np.float32)
    want[[0, 16, 88]] = 1
    for at in (0, 275353, 275353 + 1115609):
        assert np.array_equal(img[at:at + 97], want), at
    other = np.ones(img.size, bool)
    for at in (0, 275353, 275353 + 1115609):
        other[at:at + 97] = False
    assert np.array_equal(img[other], weights.pack_state_dict(w, "pointconv")[other])
    # the torch oracle returns rho as s: in float32 bit for bit, in float64 up to running_var's rounding
    pcs, t = golden_clouds(g), golden_tables(g)
    W32, W64 = PO.to_torch(ident), PO.to_torch(ident, torch.float64)
    L = weights.pointconv_layers()
    for b in (0, 2, 4):
        for lv, (name, xyz, bw) in enumerate(PO.level_inputs(pcs[b], t["fps1"][b], t["fps2"][b])):
            rho, s = PO.density_scale(W32, L[10 * lv:10 * lv + 3], torch.from_numpy(xyz), bw)
            assert torch.equal(rho, s) and float(rho.min()) > 0, (b, name)
            rho, s = PO.density_scale(W64, L[10 * lv:10 * lv + 3], torch.from_numpy(xyz).double(), bw)
            assert float(((s - rho).abs() / rho).max()) <= 1e-7, (b, name)
            h = torch.from_numpy(PO.density_header(xyz, bw))
            assert torch.equal(PO.density_net(W32, lv, h), h), (b, name)
    # density_header against float64, per element and relative, beside the reference's matrix form in float32
    W = PO.to_torch(w)
    worst = 0.0
    for b in range(len(pcs)):
        for lv, (name, xyz, bw) in enumerate(PO.level_inputs(pcs[b], t["fps1"][b], t["fps2"][b])):
            r64 = PO.density_f64(xyz, bw)
            rel_h = np.abs(PO.density_header(xyz, bw) - r64) / r64
            e_h = float(rel_h.max())
            e_m = float((np.abs(PO.density_scale(W, L[0:3], torch.from_numpy(xyz), bw)[0].numpy() - r64) / r64).max())
            print("cloud %d (n = %d) %s: relative error of rho: header form %.2e, matrix form %.2e" % (b, len(pcs[b]), name, e_h, e_m))
            worst = max(worst, e_h)
            # To first order, in units of u = 2^-24: the argument carries 7 u (two differences 2 u, the product, two sums, the
            # division, c1), which moves rho_j by 7 u A_j with A_j the e-weighted mean of |arg| over i; expf 1 u; the sum of
            # positive terms ceil(n / 64) + 6 additions; the two divisions and c2 3 u.
            xd = xyz.astype(np.float64)
            arg = ((xd[None] - xd[:, None]) ** 2).sum(-1) / (2.0 * bw * bw)
            A = (arg * np.exp(-arg)).sum(-1) / np.exp(-arg).sum(-1)
            assert (rel_h <= (7 * A + -(-len(xyz) // 64) + 6 + 4) * 2.0 ** -24).all(), (b, name, e_h)
    print("worst relative error of density_header: %.2e" % worst)
    # ... and against the reference's recorded densities, at the bar of test_oracle_outputs_against_the_reference
    for lv in range(3):
        name = "dens%d" % (lv + 1)
        e32 = float((o32[name].double() - o64[name]).abs().max())
        d = 0.0
        for b in range(len(pcs)):
            xyz, bw = PO.level_inputs(pcs[b], t["fps1"][b], t["fps2"][b])[lv][1:]
            s = PO.density_net(W, lv, torch.from_numpy(PO.density_header(xyz, bw))).numpy()
            d = max(d, float(np.abs(s - g["%s_%d" % (name, b)]).max()))
        print("%s: density_header through DensityNet vs reference %.3e, e_32 %.3e, ratio %.2f" % (name, d, e32, d / e32))
        assert d <= 4 * e32


def test_calibrated_weights_give_varied_predictions():
    """The calibrated head alone (no GPU): on bench.synth_clouds(64, seed=23)[:, :128] the float64 oracle predicts at least 10
    classes; fc3 alone differs from make_weights."""
    import bench
    import pointconv_oracle as PO
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
    """Stands in for runtime.PointConvClassifier: the class of a cloud is its number of rows modulo 40."""

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
    from ifdefense_amd import pointconv_inference as Inf
    from ifdefense_amd import pointnet2_inference
    assert Inf.fps_starts is pointnet2_inference.fps_starts   # imported, not repeated
    made = []

    def make(model, path):
        made.append((model, path, StubClassifier()))
        return made[-1][2]
    # the model named by the path; a cluster file takes 1120 rows -> class 0
    p = str(tmp_path / "cluster-PointConv-x.npz")
    _write(p, [1120] * 7, [0, 0, 0, 5, 5, 5, 5], [5, 0, 5, 0, 1, 1, 1], cols=6)
    assert Inf.main(["--data_root", p, "--mode", "target"], make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % (3 / 7, 2 / 7)
    model, path, stub = made[-1]
    assert (model, path) == ("pointconv", "pretrain/mn40/pointconv.pth") and stub.closed
    assert all(c.shape == (1120, 3) and c.dtype == np.float32 for c in stub.seen)
    assert np.array_equal(stub.starts[-1], Inf.fps_starts(1, [1120] * 7))     # the default seed is 1
    # normal mode, explicit model / weights / num_points / seed, ragged SOR file
    p = str(tmp_path / "sor_x.npz")
    _write(p, [50, 45, 41], [10, 5, 2], ragged=True)
    assert Inf.main(["--data_root", p, "--model", "pointconv", "--model_path", "w.npz", "--num_points", "45", "--dataset", "opt_mn40",
                     "--fps_seed", "9"], make_classifier=make) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f\n" % (1 / 3)      # rows taken: 45, 45, 41 -> classes 5, 5, 1
    assert made[-1][:2] == ("pointconv", "w.npz") and [len(c) for c in made[-1][2].seen] == [45, 45, 41]
    assert np.array_equal(made[-1][2].starts[-1], Inf.fps_starts(9, [45, 45, 41]))
    assert Inf.main(["--data_root", p, "--model", "pointconv", "--dataset", "conv_opt_mn40"], make_classifier=make) == 0
    assert made[-1][1] == "pretrain/conv_opt_mn40/pointconv.pth"
    capsys.readouterr()


def test_cli_refusals(tmp_path, capsys):
    from ifdefense_amd import pointconv_inference as Inf

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv, where in ((["--data_root", "x.npz", "--model", "pointnet"], "ifdefense_amd.inference"),
                        (["--data_root", "a/kNN-dgcnn.npz"], "ifdefense_amd.dgcnn_inference"),
                        (["--data_root", "x.npz", "--model", "pointnet2"], "ifdefense_amd.pointnet2_inference")):
        assert Inf.main(argv, make_classifier=never) == 2
        err = capsys.readouterr().err
        assert where in err and "only the pointconv victim runs here" in err
    assert Inf.main(["--data_root", "nothing.npz"], make_classifier=never) == 2
    assert "not recognized" in capsys.readouterr().err
    # a cloud of more than 2048 points, a cloud of fewer than 32: refused with a message, the classifier closed, nothing run
    p = str(tmp_path / "sor-pointconv.npz")
    _write(p, [50, 2049, 41], [10, 5, 2], ragged=True)
    stub = StubClassifier()
    assert Inf.main(["--data_root", p, "--num_points", "4096"], make_classifier=lambda *a: stub) == 2
    err = capsys.readouterr().err
    assert "cloud 1 has 2049 points, more than the 2048" in err and stub.closed and stub.seen is None
    assert Inf.main(["--data_root", p, "--num_points", "2048"], make_classifier=lambda *a: StubClassifier()) == 0
    capsys.readouterr()
    q = str(tmp_path / "sor-pointconv-small.npz")
    _write(q, [50, 31, 41], [10, 5, 2], ragged=True)
    stub = StubClassifier()
    assert Inf.main(["--data_root", q], make_classifier=lambda *a: stub) == 2
    err = capsys.readouterr().err
    assert "cloud 1 has 31 points, fewer than the 32" in err and stub.closed and stub.seen is None
    # target mode without target_label
    assert Inf.main(["--data_root", p, "--mode", "target"], make_classifier=lambda *a: StubClassifier()) == 2
    assert "target_label" in capsys.readouterr().err
    # the other CLIs keep their own words for pointconv
    from ifdefense_amd import inference, pointnet2_inference
    assert inference.main(["--data_root", "x.npz", "--model", "pointconv"], make_classifier=never) == 2
    assert "not built" in capsys.readouterr().err
    assert pointnet2_inference.main(["--data_root", "x.npz", "--model", "pointconv"], make_classifier=never) == 2
    assert "baselines/inference.py" in capsys.readouterr().err
