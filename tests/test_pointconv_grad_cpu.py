"""CPU checks of the PointConv input gradient and its FGM family (include/ifd_pc_atk.h): the oracle
(tests/pointconv_grad_oracle.py) against gradients recorded from the reference's FGM.get_gradient on its own
PointConvDensityClsSsg (tests/golden/pointconv_grad_golden.npz), against pointconv_oracle.forward, against central differences,
and its two forms against each other; that each of the five paths of the coordinates moves the gradient by far more than the
parity bar; that the GPU parity cases meet their conditions from the oracle alone; the C ABI and its binding; the refusals that
need no GPU; and the host logic of the pointconv_fgm_attack CLI under a stub classifier."""
import ctypes
import functools
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import pointconv_grad_oracle as GO
import pointconv_oracle as PCO
from test_atk_cpu import _attack_file
from test_pointnet2_grad_cpu import Pn2Stub

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_pc_atk.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pointconv_grad_golden.npz")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")

# The GPU parity cases (tests/test_gpu_pointconv_grad.py imports them): name -> (points per cloud or a list of counts, clouds, loss,
# stride or None, non-zero starts?).  Every case leaves at most 10 % of its clouds out from the oracle alone
# (test_parity_cases_meet_their_conditions); with at most 5 clouds a case that is none at all.
CLOUD_SEED, WEIGHT_SEED = 77, 0
CASES = {"32": (32, 3, "logits", None, False), "33": (33, 3, "logits", None, False), "64": (64, 3, "logits", None, False),
         "65": (65, 3, "logits", None, False), "100": (100, 3, "logits", None, False), "511": (511, 3, "logits", None, False),
         "512": (512, 3, "logits", None, False), "513": (513, 3, "logits", None, False), "1024": (1024, 2, "logits", None, False),
         "2048": (2048, 1, "logits", None, False), "ragged": ([300, 32, 64, 513, 40], 5, "logits", 520, False),
         "100-ce": (100, 3, "cross_entropy", None, False), "600-starts": (600, 3, "logits", None, True)}
MAX_OUT = 0.1
# The degenerate clouds of the GPU tests: 32 identical points, every point twice (40 + 40), two far clusters
DEGENERATE = ("32 identical", "twins", "two clusters")
# The five paths of a coordinate into the loss (pointconv_grad_oracle.CUTS) and the cases on which each is held
TEETH_CASES = ("100", "1024")
TEETH = 100.0                                                              # in e_32 max |grad|; the GPU's bar is 4


def source_clouds():
    """24 clouds of 1024 points and two of 2048 (two shapes side by side), as tests/test_gpu_pointconv.py builds them."""
    import bench
    s = bench.synth_clouds(24, seed=CLOUD_SEED)
    big = [np.concatenate([s[20], 0.8 * s[21] + 0.1]), np.concatenate([s[22], 0.7 * s[23] - 0.2])]
    return s, [np.ascontiguousarray(b, dtype=np.float32) for b in big]


def _targets(sd, clouds, starts):
    W = PCO.to_torch(sd, torch.float64)
    lo = PCO.forward(W, clouds, dtype=torch.float64, tables=PCO.tables_of(clouds, None, starts))["logits"].numpy()
    return (lo.argmax(1) + 1) % 40


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (state dict, clouds list, targets, loss, stride, starts [B,2] or None): the target of a cloud is the float64 oracle's
    prediction + 1."""
    n, B, loss, stride, moved = CASES[name]
    sd = PCO.make_calibrated_weights(WEIGHT_SEED)
    counts = n if isinstance(n, list) else [n] * B
    s, big = source_clouds()
    clouds = [np.ascontiguousarray(s[i][:m] if m <= 1024 else big[i % 2][:m], dtype=np.float32) for i, m in enumerate(counts)]
    starts = np.array([[(7 * i + 3) % m, (131 * i + 17) % 512] for i, m in enumerate(counts)], np.int32) if moved else None
    return sd, clouds, _targets(sd, clouds, starts), loss, stride, starts


@functools.lru_cache(maxsize=None)
def degenerate_inputs(name):
    """-> (state dict, [cloud], targets) of a degenerate cloud."""
    sd = PCO.make_calibrated_weights(WEIGHT_SEED)
    s, _ = source_clouds()
    c = {"32 identical": np.repeat(s[6][3:4], 32, axis=0), "twins": np.concatenate([s[5][:40], s[5][:40]]),
         "two clusters": np.concatenate([0.05 * s[4][:40] - 0.9, 0.05 * s[4][40:80] + 0.9])}[name]
    clouds = [np.ascontiguousarray(c, dtype=np.float32)]
    return sd, clouds, _targets(sd, clouds, None)


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    """GO.oracle_case of a parity case (or a degenerate cloud), computed once."""
    if name in CASES:
        sd, clouds, targets, loss, _, starts = case_inputs(name)
    else:
        (sd, clouds, targets), loss, starts = degenerate_inputs(name), "logits", None
    return GO.oracle_case(sd, clouds, targets, loss, scale=1.0 / len(clouds), starts=starts)


@pytest.fixture(scope="module")
def sd():
    return PCO.make_weights(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def golden_clouds(g):
    import bench
    s = bench.synth_clouds(len(g["sizes"]), seed=int(g["cloud_seed"]))
    return [np.ascontiguousarray(s[i][:n], dtype=np.float32) for i, n in enumerate(g["sizes"])]


def golden_tables(g, i, p=""):
    return {k: g["%s%s_%d" % (k, p, i)].astype(np.int64) for k in GO.TABLES}


# ---------------------------------------------------------------------------------------------- the oracle
BAR64, BAR32_GRAD, BAR32_LOGITS = 1e-12, 5e-5, 1e-5


@pytest.mark.parametrize("loss,tag", [("logits", "logits"), ("cross_entropy", "ce")])
def test_reference_form_reproduces_the_recorded_gradients(sd, golden, loss, tag):
    """Bars, relative to the largest entry.  float64: PointNet++'s 1e-12 holds (measured on these three clouds, worst over both losses:
    gradient 3.3e-14, logits 8.6e-16).  float32 logits: PointNet++'s 1e-5 holds (measured 6.3e-7).  float32 gradient: PointConv needs
    more than 1e-5 - the oracle's linear layers on rows and the reference's convolutions on [B, C, K, S] tensors sum in other orders,
    and every one of the 25 thousand rows carries gradient.  Measured disagreement with the recorded float32 gradient: 1.7e-5 (cloud 0,
    logits loss; 6.1e-6 and 1.2e-6 on the others), while the recorded float32 gradient itself lies 2.5e-5 from the recorded float64 one
    on that cloud.  The bar is 5e-5, 3 times the measurement."""
    assert int(golden["weight_seed"]) == 0 and golden["sizes"].tolist() == [40, 64, 128]
    assert os.path.getsize(GOLDEN) <= 131072
    W32, W64 = PCO.to_torch(sd, torch.float32), PCO.to_torch(sd, torch.float64)
    for i, (c, t) in enumerate(zip(golden_clouds(golden), golden["targets"])):
        assert golden["fps1_%d" % i].dtype == np.int16 and golden["knn2_%d" % i].shape == (128, 64)
        assert int(golden["fps1_%d" % i][0]) == int(golden["starts"][i][0]) and int(golden["fps2_%d" % i][0]) == int(golden["starts"][i][1])
        r64 = GO.run_cloud(W64, c, t, golden_tables(golden, i, "64"), loss, dtype=torch.float64)
        want = golden["grad_%s64_%d" % (tag, i)]
        assert want.dtype == np.float64 and want.shape == (len(c), 3) and np.abs(want).max() > 0
        d64 = np.abs(r64["grad"] - want).max() / np.abs(want).max()
        l64 = np.abs(r64["logits"] - golden["lo_%s64_%d" % (tag, i)]).max() / np.abs(r64["logits"]).max()
        r32 = GO.run_cloud(W32, c, t, golden_tables(golden, i), loss, dtype=torch.float32)
        want32 = golden["grad_%s_%d" % (tag, i)]
        assert r32["grad"].dtype == np.float32 and want32.dtype == np.float32
        d32 = np.abs(r32["grad"] - want32).max() / np.abs(want32).max()
        l32 = np.abs(r32["logits"] - golden["lo_%s_%d" % (tag, i)]).max() / np.abs(r32["logits"]).max()
        print("cloud %d %s: float64 grad %.2e logits %.2e, float32 grad %.2e logits %.2e" % (i, loss, d64, l64, d32, l32))
        assert d64 <= BAR64 and l64 <= BAR64 and d32 <= BAR32_GRAD and l32 <= BAR32_LOGITS


def test_reference_form_is_the_forward_oracle(sd):
    """run_cloud restates pointconv_oracle._forward_cloud to keep the pre-activations: the same logits and features bit for bit."""
    import bench
    c = np.ascontiguousarray(bench.synth_clouds(2, seed=5)[1][:48], dtype=np.float32)
    t = PCO.tables_of_cloud(c, (5, 100))
    for dtype in (torch.float32, torch.float64):
        W = PCO.to_torch(sd, dtype)
        r = GO.run_cloud(W, c, 7, t, "cross_entropy", dtype=dtype)
        o = PCO.forward(W, [c], dtype=dtype, tables={k: v[None] for k, v in t.items()})
        assert np.array_equal(o["logits"][0].numpy(), r["logits"])
        for k in ("dens1", "dens2", "dens3", "l1_feat", "l2_feat", "global_feat"):
            assert np.array_equal(o[k][0].numpy(), r[k]), k


def test_reference_form_against_central_differences(sd):
    import bench
    c = bench.synth_clouds(1, seed=9)[0][:48].astype(np.float64)
    W = PCO.to_torch(sd, torch.float64)
    t = PCO.tables_of_cloud(c.astype(np.float32), (3, 9))
    for loss, kappa in (("logits", 0.5), ("cross_entropy", 0.)):
        r = GO.run_cloud(W, c, 3, t, loss, kappa, scale=0.5, dtype=torch.float64)
        assert r["loss"] > 0 and np.abs(r["grad"]).max() > 0
        rng, h = np.random.default_rng(1), 1e-6
        for _ in range(12):
            i, a = int(rng.integers(len(c))), int(rng.integers(3))
            up, dn = c.copy(), c.copy()
            up[i, a] += h
            dn[i, a] -= h
            f = [GO.run_cloud(W, p, 3, t, loss, kappa, dtype=torch.float64)["loss"] for p in (up, dn)]
            fd = 0.5 * (f[0] - f[1]) / (2 * h)
            assert abs(fd - r["grad"][i, a]) <= 1e-6 * np.abs(r["grad"]).max() + 1e-9, (loss, i, a, fd, r["grad"][i, a])


@pytest.mark.parametrize("loss", ["logits", "cross_entropy"])
def test_explicit_form_fed_the_reference_forms_choices_equals_it(sd, loss):
    """The explicit form runs the header's difference-form density, the reference form the reference's matrix form: in float64 the
    two lie within the matrix form's cancellation error, 1e-10 of the gradient at these scales."""
    import bench
    Wf, W = GO.folded(sd), PCO.to_torch(sd, torch.float64)
    src = bench.synth_clouds(3, seed=4)
    for c, st in ((src[2][:70], (0, 0)), (src[0][:33], (20, 400)), (src[1][:600], (599, 1))):
        c = np.ascontiguousarray(c, dtype=np.float32)
        r = GO.run_cloud(W, c, 11, PCO.tables_of_cloud(c, st), loss, 0.25, scale=0.125, dtype=torch.float64)
        x = GO.explicit_from(Wf, c, 11, r, loss=loss, kappa=0.25, scale=0.125)
        assert np.abs(r["grad"]).max() > 0
        assert np.abs(x["grad"] - r["grad"]).max() <= 1e-10 * np.abs(r["grad"]).max()
        assert np.abs(x["logits"] - r["logits"]).max() <= 1e-10 * np.abs(r["logits"]).max()
        # ... and it is a function of the choices: other gates give another gradient
        for k in ("dn1", "wn2", "mg3"):
            moved = dict(r, **{k: ~r[k]})
            assert np.abs(GO.explicit_from(Wf, c, 11, moved, loss=loss, kappa=0.25, scale=0.125)["grad"] - r["grad"]).max() > \
                1e-6 * np.abs(r["grad"]).max(), k


def test_validity_checks_refuse_wrong_choices(sd):
    import bench
    c = np.ascontiguousarray(bench.synth_clouds(1, seed=12)[0][:50], dtype=np.float32)
    r32, r64, e, _ = GO.oracle_case(sd, [c], [4])
    ch = {k: r32[0][k] for k in GO.CHOICES + ("tables",)}
    GO.choices_valid(ch, r64[0], e, "float32's own")
    p = r64[0]["pre"]
    far = np.abs(p["mlp2_1"]).argmax(-1)                                      # per row the channel furthest from zero
    bad = dict(ch, mg2=ch["mg2"].copy())
    np.put_along_axis(bad["mg2"], 128 + far[..., None], ~np.take_along_axis(bad["mg2"], 128 + far[..., None], -1), -1)
    with pytest.raises(AssertionError, match="mlp2_1: a gate"):
        GO.choices_valid(bad, r64[0], e)
    for k, key in (("dn1", "dn1_0"), ("wn3", "wn3_0")):
        flipped = dict(ch, **{k: ch[k].copy()})
        j = np.unravel_index(np.abs(p[key]).argmax(), p[key].shape)
        flipped[k][j] = ~flipped[k][j]
        with pytest.raises(AssertionError, match="%s: a gate" % key):
            GO.choices_valid(flipped, r64[0], e)
    with pytest.raises(AssertionError, match="lin1: a gate"):
        GO.choices_valid(dict(ch, pos1=np.abs(p["lin1"]) < 0), r64[0], e)
    swapped = {k: v.copy() for k, v in ch["tables"].items()}
    swapped["knn1"][[0, 1]] = swapped["knn1"][[1, 0]]
    with pytest.raises(AssertionError, match="table knn1"):
        GO.choices_valid(dict(ch, tables=swapped), r64[0], e)
    assert GO.unpack_bits(np.array([[5, -2 ** 31]], np.int32), 64)[0].nonzero()[0].tolist() == [0, 2, 63]


@pytest.mark.parametrize("name", TEETH_CASES)
def test_every_path_of_the_coordinates_has_teeth(name):
    """Cutting any one of the five paths - (a)'s WeightNet part, (a)'s MLP-xyz part, (b) the centroids, (c) sa3's mean, (d) the
    densities - changes the float64 explicit gradient by more than 100 e_32 max |grad| on every cloud of the case, so a kernel that
    leaves one out misses the GPU test's 4 e_32 by a wide margin.  Measured (smallest over the case's clouds, in e_32 max |grad|):
    case "100" (e_32 1.7e-5): wn 2.2e+04, mlp 4.1e+04, b 6.2e+04, c 1.8e+04, d 2.7e+03; case "1024" (e_32 4.7e-6): wn 2.0e+05,
    mlp 7.7e+04, b 1.8e+05, c 2.8e+04, d 8.7e+03.  make_calibrated_weights(0) holds all five; no further case is needed."""
    sd, clouds, targets, loss, _, starts = case_inputs(name)
    _, r64, _, _ = case_oracle(name)
    F32, F64 = GO.folded(sd, torch.float32), GO.folded(sd, torch.float64)
    kw = dict(loss=loss, scale=1.0 / len(clouds))
    full = [GO.explicit_from(F64, c, t, r, **kw)["grad"] for c, t, r in zip(clouds, targets, r64)]
    e32 = GO.grad_e32([GO.explicit_from(F32, c, t, r, dtype=torch.float32, **kw)["grad"] for c, t, r in zip(clouds, targets, r64)], full)
    for cut in GO.CUTS:
        moved = min(np.abs(GO.explicit_from(F64, c, t, r, cut=cut, **kw)["grad"] - g).max() / np.abs(g).max()
                    for c, t, r, g in zip(clouds, targets, r64, full))
        print("case %s, path %s: %.2e e_32 (e_32 = %.2e)" % (name, cut, moved / e32, e32))
        assert moved > TEETH * e32, (name, cut, moved, e32)


@pytest.mark.parametrize("name", list(CASES))
def test_parity_cases_meet_their_conditions(name):
    clouds = case_inputs(name)[1]
    _, r64, e, out = case_oracle(name)
    assert all(r["loss"] > 0 for r in r64)
    assert sum(1 for o in out if o) <= MAX_OUT * len(clouds), out


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_clouds_are_admitted(name):
    """The oracle alone admits all three degenerate clouds to the parity check of the GPU test."""
    _, r64, e, out = case_oracle(name)
    assert r64[0]["loss"] > 0 and not out[0], out


# ---------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    return I.load_library()


def declared_symbols(header=HEADER):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.PC_ATK_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    text = open(HEADER).read()
    version = int(re.search(r"#define IFD_PC_ATK_ABI_VERSION (\d+)", text).group(1))
    assert lib.ifd_pc_atk_abi_version() == version == _lib.PC_ATK_ABI_VERSION == 1
    assert lib.ifd_pc_abi_version() == 1 and lib.ifd_atk_abi_version() == 1 and lib.ifd_pn2_atk_abi_version() == 1   # the older headers stay
    fields = re.findall(r"^\s+(?:float|int32_t|uint32_t)\*\s+(\w+);", re.search(r"typedef struct ifd_pc_grad_out \{(.*?)\}", text, re.S).group(1),
                        re.M)
    assert fields == [f for f, _ in _lib.IfdPcGradOut._fields_] and ctypes.sizeof(_lib.IfdPcGradOut) == 22 * 8
    aux = [f for f, _ in _lib.IfdPcAux._fields_ if f != "pred"]              # every field of ifd_pc_aux is there
    assert set(aux) <= set(fields)
    decl = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in names:                                                      # the argument counts of the header's calls are the binding's
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.PC_ATK_SIGNATURES[name][1]), name


def test_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_pc_input_grad(None, None, None, None, 1, 32, None, 0, 0.0, 1.0, None, None, None) == -1
    assert lib.ifd_pc_fgm_update(None, 0, None, None, None, None, 0.0, 0.0, 0.0, None, 1, 32, None) == -1
    assert lib.ifd_pc_fgm_attack(None, None, None, None, None, None, 1, 32, None, None, None) == -1


def test_runtime_class_names_the_pointconv_calls():
    import inspect
    import ifdefense_amd as I
    assert I.PointConvClassifier.ATK_FNS == {"input_grad": "ifd_pc_input_grad", "fgm_update": "ifd_pc_fgm_update",
                                             "fgm_attack": "ifd_pc_fgm_attack"}
    assert I.PointNet2Classifier.ATK_FNS["input_grad"] == "ifd_pn2_input_grad" and I.Classifier.ATK_FNS["input_grad"] == "ifd_cls_input_grad"
    assert "not offered" not in I.PointConvClassifier.__doc__
    assert I.PointConvClassifier._starts is I.PointNet2Classifier._starts     # shared, not copied
    for name in ("input_grad", "fgm_update", "fgm_attack"):                 # Classifier's signatures plus fps_start=None
        base = list(inspect.signature(getattr(I.Classifier, name)).parameters.values())
        mine = list(inspect.signature(getattr(I.PointConvClassifier, name)).parameters.values())
        assert [(p.name, p.default) for p in mine] == [(p.name, p.default) for p in base] + [("fps_start", None)], name


# ---------------------------------------------------------------------------------------------- CLI host logic
def test_cli_file_name_and_starts_by_file_position(tmp_path, capsys):
    from ifdefense_amd import pointconv_fgm_attack as PA
    from ifdefense_amd.pointnet2_inference import fps_starts
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    want = fps_starts(5, [32] * 6)
    assert len({tuple(r) for r in want.tolist()}) > 1
    seen = {}
    for bs in (4, -1):
        stub, made = Pn2Stub(), []

        def make(model, path):
            made.append((model, path))
            return stub
        out_dir = tmp_path / ("bs%d" % bs)
        argv = ["--data_root", src, "--num_points", "32", "--attack_type", "IFGM", "--num_iter", "10", "--budget", "0.08", "--batch_size",
                str(bs), "--kappa", "0.5", "--local_rank", "2", "--out_dir", str(out_dir), "--dataset", "opt_mn40", "--fps_seed", "5"]
        assert PA.main(argv, make_classifier=make) == 0
        out = capsys.readouterr().out
        assert made == [("pointconv", "pretrain/opt_mn40/pointconv.pth")] and stub.closed
        assert "Loading weight pretrain/opt_mn40/pointconv.pth" in out
        d = out_dir / "attack" / "results" / "opt_mn40_32" / "FGM" / "pointconv"
        assert os.listdir(d) == ["ifgm-budget_0.08-iter_10-success_%.4f-rank_2.npz" % (4 / 6)]
        z = np.load(d / os.listdir(d)[0])
        assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 32, 3) and list(z["test_label"]) == list(range(6))
        # every call of a batch sees the starts of ITS clouds' places in the file
        batches = [(0, 4), (4, 6)] if bs == 4 else [(0, 6)]
        assert {c[3] for c in stub.calls if c[0] == "grad"} == {1 / 6}          # the loss is a mean over the file in every batch
        grads = [s for w, s in stub.starts if w == "grad"]
        assert len(grads) == 10 * len(batches)
        for j, (a, b) in enumerate(batches):
            for s in grads[10 * j:10 * j + 10]:
                assert np.array_equal(s, want[a:b])
        preds = [s for w, s in stub.starts if w == "predict"]
        assert len(preds) == len(batches) and all(np.array_equal(s, want[a:b]) for s, (a, b) in zip(preds, batches))
        seen[bs] = z["test_pc"]
    assert np.array_equal(seen[4], seen[-1])
    # plain FGM: one library call per batch, with the batch's starts
    stub = Pn2Stub()
    assert PA.main(["--data_root", src, "--num_points", "32", "--out_dir", str(tmp_path), "--adv_func", "cross_entropy", "--batch_size", "4"],
                   make_classifier=lambda model, path: stub) == 0
    assert "Successfully attack" in capsys.readouterr().out
    want1 = fps_starts(1, [32] * 6)
    assert [w for w, _ in stub.starts] == ["attack", "attack"]
    assert np.array_equal(stub.starts[0][1], want1[:4]) and np.array_equal(stub.starts[1][1], want1[4:])


@pytest.mark.parametrize("kind", ["ifgm", "pgd"])
def test_cli_start_noise_is_one_draw_of_the_file(tmp_path, capsys, kind):
    """33 points: 4 x 33 x 3 numbers are no multiple of torch's block of 16, so a draw per batch would give the clouds behind the
    first batch other noise than one draw of the file gives them."""
    from ifdefense_amd import pointconv_fgm_attack as PA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    seen = {}
    for bs in (4, -1):
        out_dir = tmp_path / ("bs%d" % bs)
        assert PA.main(["--data_root", src, "--num_points", "33", "--attack_type", kind, "--num_iter", "2", "--batch_size", str(bs),
                        "--out_dir", str(out_dir)], make_classifier=lambda model, path: Pn2Stub()) == 0
        d = out_dir / "attack" / "results" / "mn40_33" / "FGM" / "pointconv"
        seen[bs] = np.load(d / os.listdir(d)[0])["test_pc"]
    capsys.readouterr()
    assert np.array_equal(seen[4], seen[-1])


def test_cli_refusals_give_status_2_without_a_classifier(tmp_path, capsys):
    from ifdefense_amd import pointconv_fgm_attack as PA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src, k=40)
    big = str(tmp_path / "big.npz")
    np.savez(big, test_pc=np.zeros((2, 2049, 3), np.float32) + np.arange(2049)[None, :, None], test_label=np.zeros(2, np.uint8),
             target_label=np.ones(2, np.uint8))

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv, word in ((["--model", "pointnet"], "only the pointconv victim"), (["--model", "dgcnn"], "only the pointconv victim"),
                       (["--model", "pointnet2"], "only the pointconv victim"), (["--feature_transform", "true"], "pointnet"),
                       (["--attack_type", "cw"], "unknown --attack_type"),
                       (["--data_root", big, "--num_points", "4096"], "more than the 2048"),
                       (["--num_points", "31"], "fewer than the 32")):
        assert PA.main(["--data_root", src, "--out_dir", str(tmp_path)] + argv, make_classifier=never) == 2, argv
        assert word in capsys.readouterr().err, argv
    # the other attack CLIs keep turning pointconv away
    from ifdefense_amd import fgm_attack as FA, pointnet2_fgm_attack as P2
    assert FA.main(["--data_root", src, "--model", "pointconv"], make_classifier=never) == 2
    assert P2.main(["--data_root", src, "--model", "pointconv"], make_classifier=never) == 2
    capsys.readouterr()
