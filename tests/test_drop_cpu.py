"""CPU checks of the saliency Drop attack (include/ifd_drop.h): the test oracle (tests/drop_oracle.py) against a run of the
reference's own SaliencyDrop recorded in tests/golden/drop_golden.npz, the header's plain formula against torch's evaluation, the
lower median, the selection's total order, the stable compaction, the conditions of the GPU parity cases, the C ABI and its
binding, refusals that need no GPU, and the host logic of the drop_attack CLI and of attack.SaliencyDrop under a stub classifier."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import drop_oracle as DO
import pointnet_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_drop.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")


@pytest.fixture(scope="module")
def sd():
    return PO.make_calibrated_weights(0, False)


@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    return I.load_library()


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "drop_golden.npz"))


def sorted_rows(a):
    a = np.asarray(a)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


# ---------------------------------------------------------------------------------------------- the oracle
def test_oracle_reproduces_the_recorded_reference(sd, golden):
    """tests/golden/drop_golden.npz: the reference's SaliencyDrop(num_drop=23, alpha=1, k=5) on its own PointNetCls with the
    calibrated weights, 4 clouds x 64 points, 5 rounds of 5, 5, 5, 5, 3 (tests/golden/make_golden_drop.py).  On every cloud whose
    rounds are all clear on the float64 oracle's free run, the float32 oracle must leave the reference's SET of rows, bit for bit
    (rows compared sorted: the reference's order is topk's), and the success counts must agree."""
    g = golden
    W32, W64 = PO.to_torch(sd, torch.float32), PO.to_torch(sd, torch.float64)
    B, num_drop, k = len(g["data"]), int(g["num_drop"]), int(g["k"])
    runs64 = [DO.attack(W64, c, t, num_drop, k, float(g["alpha"]), 1. / B, torch.float64, W_other=W32) for c, t in zip(g["data"], g["label"])]
    clear = np.array([all(r["clear"] for r in run["rounds"]) for run in runs64])
    assert np.array_equal(clear, g["all_clear"]) and clear.sum() >= 3
    assert [r["k"] for r in runs64[0]["rounds"]] == [5, 5, 5, 5, 3]
    runs32 = [DO.attack(W32, c, t, num_drop, k, float(g["alpha"]), 1. / B, torch.float32) for c, t in zip(g["data"], g["label"])]
    assert g["adv"].shape == (B, g["data"].shape[1] - num_drop, 3)
    for b in np.nonzero(clear)[0]:
        assert np.array_equal(sorted_rows(runs32[b]["points"]), sorted_rows(g["adv"][b])), "cloud %d" % b
        assert np.array_equal(g["data"][b][runs32[b]["kept"]], runs32[b]["points"])
        assert np.array_equal(runs32[b]["kept"], runs64[b]["kept"])
    assert sum(r["correct"] for r in runs32) == int(g["success_num"])


def test_plain_restatement_against_torch(sd):
    """The header's formula in numpy float32 against Drop.py:78-88 evaluated by torch in float32, on a parity case's clouds with
    their own gradients and on dense random gradients: within 4 float32 ulps of max |s|; whether it is bit-equal is printed.  It
    is not everywhere: torch sums the three terms in the header's order, pow(x, 1) is x and pow(x, 0.5) is sqrt, but
    torch's vectorised CPU sqrt is not correctly rounded for every argument (1 of these 1024 saliencies differs, by 1 ulp), where
    numpy's and the header's are."""
    import atk_oracle as AO
    pts, labels, _ = DO.case_inputs(64, 8)
    W32 = PO.to_torch(sd, torch.float32)
    rng = np.random.default_rng(3)
    worst, equal = 0., True
    for c, t in zip(pts, labels):
        for grad in (AO.run_cloud(W32, c, t, "cross_entropy", 0., 1. / 8, dtype=torch.float32)["grad"],
                     rng.standard_normal(c.shape).astype(np.float32)):
            want, c_t = DO.saliency(c, grad, torch.float32, 1)
            got, c_p = DO.saliency_f32_plain(c, grad, 1.)
            assert got.dtype == np.float32 and np.array_equal(c_t, c_p)
            ulp = np.spacing(np.float32(np.abs(want).max()))
            worst = max(worst, float(np.abs(got.astype(np.float64) - want).max() / ulp))
            equal = equal and np.array_equal(got.view(np.int32), want.view(np.int32))
    print("plain float32 restatement against torch float32: worst %.2f ulp of max |s|, bit-equal everywhere: %s" % (worst, equal))
    assert worst <= 4
    # alpha != 1 goes through pow on both sides: the same bound
    got, _ = DO.saliency_f32_plain(pts[0], grad, 2.)
    want, _ = DO.saliency(pts[0], grad, torch.float32, 2)
    assert np.abs(got.astype(np.float64) - want).max() <= 4 * np.spacing(np.float32(np.abs(want).max()))


def test_lower_median_rule():
    """Rank (n - 1) // 2 ascending: torch.median's choice on the CPU, on odd and even n, duplicates and +-0."""
    for x in ([3., 1., 2.], [4., 1., 3., 2.], [5.], [2., 1.], [1., 1., 1., 0., 2., 2.], [0.5, 0.5, 0.5, 0.5],
              [-1., 0., -0., 1.], [-0., 0.], [0., -0., -0.], [7., -2., 7., -2., 7., -2., 0.]):
        a = np.array(x, np.float32)
        want = float(torch.median(torch.from_numpy(a)))
        got = DO.lower_median(a)
        assert float(got) == want == sorted(x)[(len(x) - 1) // 2], x          # as floats: -0 == +0
    rng = np.random.default_rng(0)
    for n in (2, 3, 64, 255, 256, 1000):
        p = rng.standard_normal((n, 3)).astype(np.float32)
        p[rng.integers(0, n, n // 4)] = p[0]                                   # duplicates
        _, c = DO.saliency_f32_plain(p, np.ones_like(p))
        assert np.array_equal(c, torch.median(torch.from_numpy(p).t()[None], dim=-1)[0][0].numpy())


def test_selection_takes_the_lowest_row_first_among_ties():
    """A gradient that is zero in all but two rows, k larger than the number of positive saliencies: the two go first, by
    saliency, then the zero saliencies by ascending row."""
    rng = np.random.default_rng(1)
    p = rng.standard_normal((20, 3)).astype(np.float32)
    g = np.zeros_like(p)
    s0, c = DO.saliency_f32_plain(p, g)
    assert not s0.any()
    g[13] = -(p[13] - c)                                                       # saliency r * |d|^2 > 0
    g[4] = -2 * (p[4] - c)
    s, _ = DO.saliency_f32_plain(p, g)
    assert s[13] > 0 and s[4] > 0 and np.count_nonzero(s) == 2
    first = [4, 13] if s[4] > s[13] else [13, 4]
    rest = [i for i in range(20) if i not in (4, 13)]
    for k in (1, 2, 3, 6, 19):
        assert list(DO.select(s, k)) == (first + rest)[:k]
    # -0 and +0 tie; a negative saliency goes last
    s = np.array([0., -0., -1., 0., 2.], np.float32)
    assert list(DO.select(s, 4)) == [4, 0, 1, 3]
    rank = [int(((s > s[i]) | ((s == s[i]) & (np.arange(5) < i))).sum()) for i in range(5)]   # the kernel's counting form
    assert list(np.argsort(rank)) == list(DO.select(s, 5))


def test_compaction_keeps_the_survivors_in_order():
    p = np.arange(30, dtype=np.float32).reshape(10, 3)
    s = np.array([0, 9, 1, 8, 2, 7, 3, 6, 4, 5], np.float32)
    st = DO.step(p, s, 4, index=np.arange(100, 110))
    assert list(st["dropped"]) == [1, 3, 5, 7] and list(st["keep"]) == [0, 2, 4, 6, 8, 9]
    assert np.array_equal(st["points"], p[[0, 2, 4, 6, 8, 9]]) and list(st["index"]) == [100, 102, 104, 106, 108, 109]
    st = DO.step(p, s, 9)
    assert list(st["keep"]) == [0] and st["index"] is None


@pytest.mark.parametrize("case", DO.CASES, ids=lambda c: "n%d_B%d_drop%d_k%d" % c)
def test_parity_cases_meet_their_conditions(case):
    """The GPU parity cases (tests/test_gpu_drop.py) from the float64 oracle's own free run: at most 10 % of the cloud-rounds are
    not clear (gap > 8 e_sal), and atk_oracle.row_exclusion takes the whole cloud out in at most 10 % of them."""
    n, B, num_drop, k = case
    _, _, _, runs = DO.case_run(case)
    rounds = [r for run in runs for r in run["rounds"]]
    assert len(rounds) == B * -(-num_drop // k) and all(run["points"].shape == (n - num_drop, 3) for run in runs)
    unclear = sum(not r["clear"] for r in rounds)
    whole = sum(r["whole_out"] for r in rounds)
    ratio = min((r["gap"] / r["e_sal"]) if r["e_sal"] > 0 else np.inf for r in rounds)
    print("case %s: %d cloud-rounds, %d not clear, %d wholly out, smallest gap / e_sal %.0f" % (case, len(rounds), unclear, whole, ratio))
    assert unclear <= 0.1 * len(rounds) and whole <= 0.1 * len(rounds)


# ---------------------------------------------------------------------------------------------- ABI
def declared_symbols(path):
    src = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_[a-z0-9_]+)\s*\(", src)))


def defined(path, name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, open(path).read()).group(1))


def test_drop_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols(HEADER)
    assert names == sorted(_lib.DROP_SIGNATURES) == ["ifd_drop_abi_version", "ifd_drop_attack", "ifd_drop_step"]
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert lib.ifd_drop_abi_version() == 1 == _lib.DROP_ABI_VERSION == defined(HEADER, "IFD_DROP_ABI_VERSION")
    assert _lib.DROP_MAX_POINTS == defined(HEADER, "IFD_DROP_MAX_POINTS") == 2048
    assert ctypes.sizeof(_lib.IfdDropParams) == 20 and ctypes.sizeof(_lib.IfdDropOut) == 24
    assert [f[0] for f in _lib.IfdDropParams._fields_] == ["struct_size", "num_drop", "k", "alpha", "scale"]
    # the header the new one builds on is as it was
    assert len(declared_symbols(os.path.join(ROOT, "include", "ifd_atk.h"))) == 4 and lib.ifd_atk_abi_version() == 1


def test_drop_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_drop_step(None, None, None, None, None, 1, 8, 2, 1.0, None, None) == -1
    assert lib.ifd_drop_attack(None, None, None, None, None, 1, 8, None, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------- host logic
class StubClassifier:
    """Stands in for runtime.Classifier on the CPU: the gradient is the cloud itself, a step drops the LAST k rows, every cloud but
    the last of a batch stays correctly classified."""
    device = "cpu"

    def __init__(self):
        self.calls, self.closed = [], False

    def drop_attack(self, pc, label, num_drop, k, alpha, scale):
        self.calls.append(("attack", tuple(pc.shape), np.asarray(label).tolist(), num_drop, k, alpha, scale))
        ok = torch.ones(len(pc), dtype=torch.bool)
        ok[-1] = False
        return pc[:, :pc.shape[1] - num_drop].clone(), ok

    def input_grad(self, pc, target, loss, kappa, scale, n_points=None, want_aux=False):
        self.calls.append(("grad", tuple(pc.shape), loss, kappa, scale, n_points.tolist()))
        pred = target.clone().int()
        pred[-1] += 1
        return pc.clone(), {"pred": pred}

    def drop_step(self, grad, pc, n_points, k, alpha):
        self.calls.append(("step", k, alpha, n_points.tolist()))
        for b in range(len(pc)):
            pc[b, int(n_points[b]) - k:int(n_points[b])] = 0
        n_points -= k

    def predict(self, pc):
        self.calls.append(("predict", tuple(pc.shape)))
        return torch.tensor([-1] * len(pc))

    def close(self):
        self.closed = True


def _attack_file(path, n=6, k=40):
    rng = np.random.default_rng(3)
    np.savez(path, test_pc=rng.standard_normal((n, k, 3)).astype(np.float32), test_label=np.array([7, 8, 9, 10, 11, 12][:n], np.uint8),
             target_label=np.array([3, 3, 3, 5, 5, 3][:n], np.uint8))


def test_cli_flags_batches_and_file(tmp_path, capsys):
    from ifdefense_amd import drop_attack as DA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    stub, made = StubClassifier(), []

    def make(model, ft, path):
        made.append((model, ft, path))
        return stub
    argv = ["--data_root", src, "--num_points", "32", "--num_drop", "10", "--batch_size", "4", "--out_dir", str(tmp_path), "--dataset", "opt_mn40"]
    assert DA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("pointnet", False, "pretrain/opt_mn40/pointnet.pth")] and stub.closed
    # print(args): the reference script's flags in its order, then the additions
    names = re.findall(r"(\w+)=", out.splitlines()[0])
    assert names == ["data_root", "model", "feature_transform", "dataset", "batch_size", "num_points", "emb_dims", "k", "num_drop",
                     "model_path", "device", "out_dir", "verbose"]
    assert out.count("Final success: 3/4, point num: 22/32") == 1 and out.count("Final success: 1/2, point num: 22/32") == 1
    assert "Iteration" not in out
    # two reference batches (4 + 2 clouds): one library call each against the TRUE labels, scale = 1 / batch, the script's k and alpha
    a, b = stub.calls
    assert a == ("attack", (4, 32, 3), [7, 8, 9, 10], 10, 5, 1.0, 0.25) and b == ("attack", (2, 32, 3), [11, 12], 10, 5, 1.0, 0.5)
    d = tmp_path / "attack" / "results" / "opt_mn40_32" / "Drop_10"
    name = "Drop-pointnet-acc_%.4f.npz" % (4 / 6)
    assert name == "Drop-pointnet-acc_0.6667.npz" and os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 22, 3)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8
    assert list(z["test_label"]) == [7, 8, 9, 10, 11, 12] and list(z["target_label"]) == [3, 3, 3, 5, 5, 3]
    # -1: one batch of the whole file; --verbose drives the rounds from the host
    stub.calls.clear()
    assert DA.main(argv + ["--batch_size", "-1", "--verbose", "true"], make_classifier=make) == 0
    out = capsys.readouterr().out
    assert [c[0] for c in stub.calls] == ["grad", "step"] * 2 + ["predict"] and stub.calls[0][4] == pytest.approx(1 / 6)
    assert "Iteration 0/2, success 5/6\nPoint num: 32/32" in out and "Iteration 1/2, success 5/6\nPoint num: 27/32" in out
    assert "Drop-pointnet-acc_0.0000.npz" in os.listdir(d)


def test_cli_and_class_refuse_what_is_not_built(capsys):
    from ifdefense_amd import drop_attack as DA

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv in (["--model", "dgcnn"], ["--model", "pointnet2"], ["--model", "pointconv"], ["--feature_transform", "true"]):
        assert DA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "not built" in capsys.readouterr().err
    for argv in (["--num_drop", "0"], ["--num_drop", "1024"], ["--num_points", "2049"], ["--num_drop", "64", "--num_points", "64"]):
        assert DA.main(["--data_root", "x.npz"] + argv, make_classifier=never) != 0
        assert "is needed" in capsys.readouterr().err
    for flag in ("--adv_func", "--kappa", "--local_rank", "--seed"):          # not flags of the reference's drop script
        with pytest.raises(SystemExit):
            DA.main([flag, "1"], make_classifier=never)
    capsys.readouterr()
    from ifdefense_amd import attack as A
    for kw in ({"num_drop": 0}, {"num_drop": 5, "k": 0}, {"num_drop": 5, "alpha": 0}):
        with pytest.raises(ValueError):
            A.SaliencyDrop(None, **kw)
    with pytest.raises(ValueError, match="more than num_drop"):
        A.SaliencyDrop(StubClassifier(), num_drop=8).attack(torch.zeros(2, 8, 3), [1, 2])


def test_existing_scripts_keep_their_flags():
    """parser_head / parser_tail's new switches default to what the four existing scripts had."""
    from ifdefense_amd import add_attack, fgm_attack, knn_attack, perturb_attack
    for mod in (add_attack, fgm_attack, knn_attack, perturb_attack):
        dests = [a.dest for a in mod.build_parser()._actions]
        for name in ("adv_func", "kappa", "local_rank", "model_path", "seed", "device", "out_dir"):
            assert name in dests, (mod.__name__, name)
        assert dests.index("k") < dests.index("adv_func") < dests.index("kappa") < dests.index("local_rank") < dests.index("model_path")


@pytest.mark.parametrize("num_drop,k,printed", [(23, 5, [0, 1, 2, 3, 4]), (50, 5, [0, 2, 4, 6, 8]), (7, 3, [0, 1, 2]), (4, 5, [0])])
def test_host_driven_loop_prints_the_reference_lines(capsys, num_drop, k, printed):
    """verbose=True: one input_grad on the current counts and one drop_step a round, the last round with what is left of num_drop;
    the reference's two lines every max(num_rounds // 5, 1) rounds - also below 5 rounds, where the reference divides by zero."""
    from ifdefense_amd import attack as A
    stub = StubClassifier()
    x = torch.arange(3 * 60 * 3, dtype=torch.float32).reshape(3, 60, 3)
    adv, n_ok = A.SaliencyDrop(stub, num_drop=num_drop, alpha=1, k=k, ref_batch=12).attack(x, [1, 2, 3])
    out = capsys.readouterr().out.splitlines()
    rounds = -(-num_drop // k)
    want = []
    for i in printed:
        want += ["Iteration %d/%d, success 2/3" % (i, rounds), "Point num: %d/60" % (60 - i * k)]
    assert out == want + ["Final success: 0/3, point num: %d/60" % (60 - num_drop)] and n_ok == 0
    steps = [c for c in stub.calls if c[0] == "step"]
    assert [c[1] for c in steps] == [k] * (rounds - 1) + [num_drop - (rounds - 1) * k] and all(c[2] == 1.0 for c in steps)
    grads = [c for c in stub.calls if c[0] == "grad"]
    assert len(grads) == rounds and all(c[1:5] == ((3, 60, 3), "cross_entropy", 0., pytest.approx(1 / 12)) for c in grads)
    assert [c[5] for c in grads] == [[60 - i * k] * 3 for i in range(rounds)]
    assert stub.calls[-1] == ("predict", (3, 60 - num_drop, 3))
    assert adv.shape == (3, 60 - num_drop, 3) and np.array_equal(adv, x.numpy()[:, :60 - num_drop])


def test_one_call_form_prints_the_last_line_only(capsys):
    from ifdefense_amd import attack as A
    stub = StubClassifier()
    adv, n_ok = A.SaliencyDrop(stub, num_drop=9, verbose=False).attack(np.zeros((4, 20, 3), np.float32), np.array([1, 2, 3, 4]))
    assert capsys.readouterr().out.splitlines() == ["Final success: 3/4, point num: 11/20"] and n_ok == 3
    assert stub.calls == [("attack", (4, 20, 3), [1, 2, 3, 4], 9, 5, 1.0, 0.25)] and adv.shape == (4, 11, 3)
