"""CPU checks of the PointNet++ input gradient and its FGM family (include/ifd_pn2_atk.h): the oracle
(tests/pointnet2_grad_oracle.py) against gradients recorded from the reference's FGM.get_gradient on its own PointNet2ClsSsg
(tests/golden/pointnet2_grad_golden.npz), against pointnet2_oracle._forward_batch, against central differences, and its two forms
against each other; that the GPU parity cases meet their conditions from the oracle alone; the C ABI and its binding; the
refusals that need no GPU; and the host logic of the pointnet2_fgm_attack CLI under a stub classifier."""
import ctypes
import functools
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import pointnet2_grad_oracle as GO
import pointnet2_oracle as PO
from test_atk_cpu import StubClassifier, _attack_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_pn2_atk.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")

# The GPU parity cases (tests/test_gpu_pointnet2_grad.py imports them): name -> (points per cloud or a list of counts, clouds, loss,
# stride or None, non-zero starts?).  Every case leaves at most 10 % of its clouds out from the oracle alone
# (test_parity_cases_meet_their_conditions); with at most 5 clouds a case that is none at all.
CLOUD_SEED, WEIGHT_SEED = 77, 0
CASES = {"2": (2, 3, "logits", None, False), "31": (31, 3, "logits", None, False), "32": (32, 3, "logits", None, False),
         "33": (33, 3, "logits", None, False), "100": (100, 3, "logits", None, False), "511": (511, 3, "logits", None, False),
         "512": (512, 3, "logits", None, False), "513": (513, 3, "logits", None, False), "600": (600, 3, "logits", None, False),
         "1024": (1024, 2, "logits", None, False), "2048": (2048, 1, "logits", None, False),
         "ragged": ([300, 1, 64, 513, 40], 5, "logits", 520, False), "100-ce": (100, 3, "cross_entropy", None, False),
         "600-starts": (600, 3, "logits", None, True)}
MAX_OUT = 0.1
# The degenerate clouds of the GPU tests: a 1-point cloud, 64 identical points, every point twice
DEGENERATE = ("one point", "64 identical", "twins")


def source_clouds():
    """24 clouds of 1024 points and two of 2048 (two shapes side by side), as tests/test_gpu_pointnet2.py builds them."""
    import bench
    s = bench.synth_clouds(24, seed=CLOUD_SEED)
    big = [np.concatenate([s[20], 0.8 * s[21] + 0.1]), np.concatenate([s[22], 0.7 * s[23] - 0.2])]
    return s, [np.ascontiguousarray(b, dtype=np.float32) for b in big]


def _targets(sd, clouds, starts):
    lo = PO.forward(PO.to_torch(sd, torch.float64), clouds, fps_start=starts, dtype=torch.float64)["logits"].numpy()
    return (lo.argmax(1) + 1) % 40


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (state dict, clouds list, targets, loss, stride, starts [B,2] or None): the target of a cloud is the float64 oracle's
    prediction + 1."""
    n, B, loss, stride, moved = CASES[name]
    sd = PO.make_calibrated_weights(WEIGHT_SEED)
    counts = n if isinstance(n, list) else [n] * B
    s, big = source_clouds()
    clouds = [np.ascontiguousarray(s[i][:m] if m <= 1024 else big[i % 2][:m], dtype=np.float32) for i, m in enumerate(counts)]
    starts = np.array([[(7 * i + 3) % m, (131 * i + 17) % 512] for i, m in enumerate(counts)], np.int32) if moved else None
    return sd, clouds, _targets(sd, clouds, starts), loss, stride, starts


@functools.lru_cache(maxsize=None)
def degenerate_inputs(name):
    """-> (state dict, [cloud], targets) of a degenerate cloud."""
    sd = PO.make_calibrated_weights(WEIGHT_SEED)
    s, _ = source_clouds()
    c = {"one point": s[6][3:4], "64 identical": np.repeat(s[6][3:4], 64, axis=0), "twins": np.concatenate([s[5][:40], s[5][:40]])}[name]
    clouds = [np.ascontiguousarray(c, dtype=np.float32)]
    return sd, clouds, _targets(sd, clouds, None)


@pytest.fixture(scope="module")
def sd():
    return PO.make_weights(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "pointnet2_grad_golden.npz"))


def golden_clouds(g):
    import bench
    s = bench.synth_clouds(len(g["sizes"]), seed=int(g["cloud_seed"]))
    return [np.ascontiguousarray(s[i][:n], dtype=np.float32) for i, n in enumerate(g["sizes"])]


def golden_tables(g, i, p=""):
    return {k: g["%s%s_%d" % (k, p, i)].astype(np.int64) for k in GO.TABLES}


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("loss,tag", [("logits", "logits"), ("cross_entropy", "ce")])
def test_reference_form_reproduces_the_recorded_gradients(sd, golden, loss, tag):
    assert int(golden["weight_seed"]) == 0 and golden["sizes"].tolist() == [40, 64, 128]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "pointnet2_grad_golden.npz")) <= 131072
    W32, W64 = PO.to_torch(sd, torch.float32), PO.to_torch(sd, torch.float64)
    for i, (c, t) in enumerate(zip(golden_clouds(golden), golden["targets"])):
        assert golden["fps1_%d" % i].dtype == np.int16 and golden["ball2_%d" % i].shape == (128, 64)
        assert int(golden["fps1_%d" % i][0]) == int(golden["starts"][i][0]) and int(golden["fps2_%d" % i][0]) == int(golden["starts"][i][1])
        r64 = GO.run_cloud(W64, c, t, golden_tables(golden, i, "64"), loss, dtype=torch.float64)
        want = golden["grad_%s64_%d" % (tag, i)]
        assert want.dtype == np.float64 and want.shape == (len(c), 3) and np.abs(want).max() > 0
        assert np.abs(r64["grad"] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(r64["logits"] - golden["lo_%s64_%d" % (tag, i)]).max() <= 1e-12 * np.abs(r64["logits"]).max()
        r32 = GO.run_cloud(W32, c, t, golden_tables(golden, i), loss, dtype=torch.float32)
        want32 = golden["grad_%s_%d" % (tag, i)]
        assert r32["grad"].dtype == np.float32 and want32.dtype == np.float32
        assert np.abs(r32["grad"] - want32).max() <= 1e-5 * np.abs(want32).max()
        assert np.abs(r32["logits"] - golden["lo_%s_%d" % (tag, i)]).max() <= 1e-5 * np.abs(r32["logits"]).max()


def test_reference_form_is_forward_batch(sd):
    """run_cloud restates pointnet2_oracle._forward_batch to keep the pre-activations: the same logits and features bit for bit."""
    import bench
    c = np.ascontiguousarray(bench.synth_clouds(2, seed=5)[1][:48], dtype=np.float32)
    t = PO.tables_of_cloud(c, (5, 100))
    for dtype in (torch.float32, torch.float64):
        W = PO.to_torch(sd, dtype)
        r = GO.run_cloud(W, c, 7, t, "cross_entropy", dtype=dtype)
        with torch.no_grad():
            o = PO._forward_batch(W, [c], {k: v[None] for k, v in t.items()}, dtype)
        assert np.array_equal(o["logits"][0].numpy(), r["logits"])
        for k in ("l1_feat", "l2_feat", "global_feat"):
            assert np.array_equal(o[k][0].numpy(), r[k]), k


def test_reference_form_against_central_differences(sd):
    import bench
    c = bench.synth_clouds(1, seed=9)[0][:40].astype(np.float64)
    W = PO.to_torch(sd, torch.float64)
    t = PO.tables_of_cloud(c.astype(np.float32), (3, 9))
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
    import bench
    Wf, W = GO.folded(sd), PO.to_torch(sd, torch.float64)
    src = bench.synth_clouds(3, seed=4)
    for c, st in ((src[2][:70], (0, 0)), (src[0][:33], (20, 400)), (src[1][:600], (599, 1))):
        c = np.ascontiguousarray(c, dtype=np.float32)
        r = GO.run_cloud(W, c, 11, PO.tables_of_cloud(c, st), loss, 0.25, scale=0.125, dtype=torch.float64)
        x = GO.explicit_from(Wf, c, 11, r, loss=loss, kappa=0.25, scale=0.125)
        assert np.abs(r["grad"]).max() > 0
        assert np.abs(x["grad"] - r["grad"]).max() <= 1e-12 * np.abs(r["grad"]).max()
        assert np.abs(x["logits"] - r["logits"]).max() <= 1e-12 * np.abs(r["logits"]).max()
        # ... and it is a function of the choices: another winner table gives another gradient
        for k in ("win1", "win2", "win3"):
            moved = dict(r, **{k: (r[k] + 1) % (128 if k == "win3" else {"win1": 32, "win2": 64}[k])})
            assert np.abs(GO.explicit_from(Wf, c, 11, moved, loss=loss, kappa=0.25, scale=0.125)["grad"] - r["grad"]).max() > \
                1e-6 * np.abs(r["grad"]).max(), k


def test_validity_checks_refuse_wrong_choices(sd):
    import bench
    c = np.ascontiguousarray(bench.synth_clouds(1, seed=12)[0][:50], dtype=np.float32)
    r32, r64, e, _ = GO.oracle_case(sd, [c], [4])
    ch = {k: r32[0][k] for k in GO.CHOICES}
    GO.choices_valid(ch, r64[0], e, "float32's own")
    p = r64[0]["pre"]
    far = np.abs(p["sa2_1"]).argmax(-1)                                       # per row the channel furthest from zero
    bad = dict(ch, act2=ch["act2"].copy())
    np.put_along_axis(bad["act2"], 128 + far[..., None], ~np.take_along_axis(bad["act2"], 128 + far[..., None], -1), -1)
    with pytest.raises(AssertionError, match="sa2 layer 2: a gate"):
        GO.choices_valid(bad, r64[0], e)
    with pytest.raises(AssertionError, match="sa1: winner"):
        GO.choices_valid(dict(ch, win1=p["sa1_2"].argmin(1)), r64[0], e)
    with pytest.raises(AssertionError, match="sa3: winner"):
        GO.choices_valid(dict(ch, win3=p["sa3_2"].argmin(0)), r64[0], e)
    with pytest.raises(AssertionError, match="outside its range"):
        GO.choices_valid(dict(ch, win2=ch["win2"] - 1), r64[0], e)
    assert GO.unpack_bits(np.array([[5, -2 ** 31]], np.int32), 64)[0].nonzero()[0].tolist() == [0, 2, 63]


@pytest.mark.parametrize("name", list(CASES))
def test_parity_cases_meet_their_conditions(name):
    sd, clouds, targets, loss, _, starts = case_inputs(name)
    _, r64, e, out = GO.oracle_case(sd, clouds, targets, loss, starts=starts)
    assert all(r["loss"] > 0 for r in r64)
    assert sum(1 for o in out if o) <= MAX_OUT * len(clouds), out


@pytest.mark.parametrize("name", DEGENERATE)
def test_degenerate_clouds_are_admitted(name):
    """Which of the degenerate clouds the oracle alone admits to the parity check of the GPU test (all three, as it turns out)."""
    sd, clouds, targets = degenerate_inputs(name)
    _, r64, e, out = GO.oracle_case(sd, clouds, targets)
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
    assert names == sorted(_lib.PN2_ATK_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    text = open(HEADER).read()
    version = int(re.search(r"#define IFD_PN2_ATK_ABI_VERSION (\d+)", text).group(1))
    assert lib.ifd_pn2_atk_abi_version() == version == _lib.PN2_ATK_ABI_VERSION == 1
    assert lib.ifd_pn2_abi_version() == 1 and lib.ifd_atk_abi_version() == 1 and lib.ifd_dgcnn_atk_abi_version() == 1   # the older headers stay
    fields = re.findall(r"^\s+(?:float|int32_t|uint32_t)\*\s+(\w+);", re.search(r"typedef struct ifd_pn2_grad_out \{(.*?)\}", text, re.S).group(1),
                        re.M)
    assert fields == [f for f, _ in _lib.IfdPn2GradOut._fields_] and ctypes.sizeof(_lib.IfdPn2GradOut) == 16 * 8
    # the argument counts of the header's calls are the binding's
    decl = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in names:
        args = re.search(r"\b%s\s*\(([^)]*)\)" % name, decl).group(1)
        n = 0 if args.strip() == "void" else len(args.split(","))
        assert n == len(_lib.PN2_ATK_SIGNATURES[name][1]), name


def test_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_pn2_input_grad(None, None, None, None, 1, 32, None, 0, 0.0, 1.0, None, None, None) == -1
    assert lib.ifd_pn2_fgm_update(None, 0, None, None, None, None, 0.0, 0.0, 0.0, None, 1, 32, None) == -1
    assert lib.ifd_pn2_fgm_attack(None, None, None, None, None, None, 1, 32, None, None, None) == -1


def test_runtime_class_names_the_pointnet2_calls():
    import inspect
    import ifdefense_amd as I
    assert I.PointNet2Classifier.ATK_FNS == {"input_grad": "ifd_pn2_input_grad", "fgm_update": "ifd_pn2_fgm_update",
                                             "fgm_attack": "ifd_pn2_fgm_attack"}
    assert I.Classifier.ATK_FNS["input_grad"] == "ifd_cls_input_grad" and I.DgcnnClassifier.ATK_FNS["input_grad"] == "ifd_dgcnn_input_grad"
    assert "not offered" not in I.PointNet2Classifier.__doc__
    for name in ("input_grad", "fgm_update", "fgm_attack"):                 # Classifier's signatures plus fps_start=None
        base = list(inspect.signature(getattr(I.Classifier, name)).parameters.values())
        mine = list(inspect.signature(getattr(I.PointNet2Classifier, name)).parameters.values())
        assert [(p.name, p.default) for p in mine] == [(p.name, p.default) for p in base] + [("fps_start", None)], name


# ---------------------------------------------------------------------------------------------- CLI host logic
class Pn2Stub(StubClassifier):
    """StubClassifier with PointNet2Classifier's fps_start arguments, which it records."""

    def __init__(self):
        super().__init__()
        self.starts = []

    def _see(self, what, fps_start):
        self.starts.append((what, np.array(fps_start)))

    def predict(self, pc, fps_start=None):
        if fps_start is not None:
            self._see("predict", fps_start)
        return super().predict(pc)

    def input_grad(self, pc, target, loss, kappa, scale, want_aux=False, fps_start=None):
        self._see("grad", fps_start)
        return super().input_grad(pc, target, loss, kappa, scale, want_aux)

    def fgm_attack(self, kind, pc, target, budget, step, num_iter, mu, loss, kappa, scale, fps_start=None):
        self._see("attack", fps_start)
        return super().fgm_attack(kind, pc, target, budget, step, num_iter, mu, loss, kappa, scale)


def test_cli_file_name_and_starts_by_file_position(tmp_path, capsys):
    from ifdefense_amd import pointnet2_fgm_attack as PA
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
        assert made == [("pointnet2", "pretrain/opt_mn40/pointnet2.pth")] and stub.closed
        assert "Loading weight pretrain/opt_mn40/pointnet2.pth" in out
        d = out_dir / "attack" / "results" / "opt_mn40_32" / "FGM" / "pointnet2"
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
    from ifdefense_amd import pointnet2_fgm_attack as PA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    seen = {}
    for bs in (4, -1):
        out_dir = tmp_path / ("bs%d" % bs)
        assert PA.main(["--data_root", src, "--num_points", "33", "--attack_type", kind, "--num_iter", "2", "--batch_size", str(bs),
                        "--out_dir", str(out_dir)], make_classifier=lambda model, path: Pn2Stub()) == 0
        d = out_dir / "attack" / "results" / "mn40_33" / "FGM" / "pointnet2"
        seen[bs] = np.load(d / os.listdir(d)[0])["test_pc"]
    capsys.readouterr()
    assert np.array_equal(seen[4], seen[-1])


def test_cli_refusals_give_status_2_without_a_classifier(tmp_path, capsys):
    from ifdefense_amd import pointnet2_fgm_attack as PA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src, k=40)
    big = str(tmp_path / "big.npz")
    np.savez(big, test_pc=np.zeros((2, 2049, 3), np.float32) + np.arange(2049)[None, :, None], test_label=np.zeros(2, np.uint8),
             target_label=np.ones(2, np.uint8))

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv, word in ((["--model", "pointnet"], "only the pointnet2 victim"), (["--model", "dgcnn"], "only the pointnet2 victim"),
                       (["--model", "pointconv"], "only the pointnet2 victim"), (["--feature_transform", "true"], "pointnet"),
                       (["--attack_type", "cw"], "unknown --attack_type"),
                       (["--data_root", big, "--num_points", "4096"], "more than the 2048")):
        assert PA.main(["--data_root", src, "--out_dir", str(tmp_path)] + argv, make_classifier=never) == 2, argv
        assert word in capsys.readouterr().err, argv
    # fgm_attack itself keeps turning pointnet2 away
    from ifdefense_amd import fgm_attack as FA
    assert FA.main(["--data_root", src, "--model", "pointnet2"], make_classifier=never) == 2
    # the adapter refuses a batch it has no starts for
    b = PA.BoundStarts(Pn2Stub(), np.zeros((6, 2), np.int32))
    b.at(0, 4)
    with pytest.raises(ValueError, match="does not match"):
        b.predict(np.zeros((3, 8, 3), np.float32))
