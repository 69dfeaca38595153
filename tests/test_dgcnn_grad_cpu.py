"""CPU checks of the DGCNN input gradient and its FGM family (include/ifd_dgcnn_atk.h): the oracle (tests/dgcnn_grad_oracle.py)
against gradients recorded from the reference's FGM.get_gradient on its own DGCNN (tests/golden/dgcnn_grad_golden.npz), against
dgcnn_oracle._forward_batch, against central differences, and its two forms against each other; that the GPU parity cases meet
their conditions from the oracle alone; the C ABI and its binding; the refusals that need no GPU; and the host logic of the
dgcnn_fgm_attack CLI under a stub classifier."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import atk_oracle as AO
import dgcnn_grad_oracle as GO
import dgcnn_oracle as DO
from test_atk_cpu import StubClassifier, _attack_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_dgcnn_atk.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")

# The GPU parity cases (tests/test_gpu_dgcnn_grad.py imports them): name -> (points per cloud or a list of counts, k, clouds, loss,
# stride or None).  Every case leaves at most 10 % of its clouds out from the oracle alone (test_parity_cases_meet_their_conditions).
CLOUD_SEED, WEIGHT_SEED = 77, 0
CASES = {"20": (20, 20, 5, "logits", None), "21": (21, 20, 5, "logits", None), "63": (63, 20, 3, "logits", None),
         "64": (64, 20, 3, "logits", None), "65": (65, 20, 3, "logits", None), "128-k1": (128, 1, 3, "logits", None),
         "129-k32": (129, 32, 2, "logits", None), "257": (257, 20, 2, "logits", None),
         "ragged": ([300, 64, 131, 20, 257], 20, 5, "logits", 320), "65-ce": (65, 20, 3, "cross_entropy", None)}
MAX_OUT = 0.1


def case_inputs(name):
    """-> (state dict, clouds list, targets, k, loss, stride): the target of a cloud is the float64 oracle's prediction + 1."""
    import bench
    n, k, B, loss, stride = CASES[name]
    sd = DO.make_calibrated_weights(WEIGHT_SEED, k)
    counts = n if isinstance(n, list) else [n] * B
    src = bench.synth_clouds(B, seed=CLOUD_SEED)
    clouds = [np.ascontiguousarray(src[i][:m], dtype=np.float32) for i, m in enumerate(counts)]
    lo = DO.forward(DO.to_torch(sd, torch.float64), clouds, dtype=torch.float64, k=k)["logits"].numpy()
    return sd, clouds, (lo.argmax(1) + 1) % 40, k, loss, stride


@pytest.fixture(scope="module")
def sd():
    return DO.make_weights(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "dgcnn_grad_golden.npz"))


def golden_clouds(g):
    import bench
    s = bench.synth_clouds(len(g["sizes"]), seed=int(g["cloud_seed"]))
    return [np.ascontiguousarray(s[i][:n], dtype=np.float32) for i, n in enumerate(g["sizes"])]


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("loss,tag", [("logits", "logits"), ("cross_entropy", "ce")])
def test_reference_form_reproduces_the_recorded_gradients(sd, golden, loss, tag):
    assert int(golden["weight_seed"]) == 0 and int(golden["k"]) == 20
    W32, W64 = DO.to_torch(sd, torch.float32), DO.to_torch(sd, torch.float64)
    for i, (c, t) in enumerate(zip(golden_clouds(golden), golden["targets"])):
        r64 = GO.run_cloud(W64, c, t, loss, dtype=torch.float64)
        want = golden["grad_%s64_%d" % (tag, i)]
        assert want.dtype == np.float64 and np.abs(want).max() > 0
        assert np.abs(r64["grad"] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.abs(r64["logits"] - golden["lo_%s64_%d" % (tag, i)]).max() <= 1e-12 * np.abs(r64["logits"]).max()
        # float32: the same operations in the same order; judged where the float32 run chose the float64 run's neighbours
        r32 = GO.run_cloud(W32, c, t, loss, dtype=torch.float32)
        want32 = golden["grad_%s_%d" % (tag, i)]
        assert r32["grad"].dtype == np.float32 and want32.dtype == np.float32
        if all(np.array_equal(np.sort(a, 1), np.sort(b, 1)) for a, b in zip(r32["idx"], r64["idx"])):
            assert np.abs(r32["grad"] - want32).max() <= 1e-5 * np.abs(want32).max()
        assert np.abs(want32 - want).max() <= 1e-3 * np.abs(want).max()


def test_reference_form_is_forward_batch(sd):
    """run_cloud restates dgcnn_oracle._forward_batch to keep the pre-activations: the same logits and features bit for bit, the same gradient."""
    import bench
    c = bench.synth_clouds(2, seed=5)[1][:48]
    for dtype in (torch.float32, torch.float64):
        W = DO.to_torch(sd, dtype)
        r = GO.run_cloud(W, c, 7, "cross_entropy", dtype=dtype)
        x = torch.as_tensor(c).to(dtype)[None].transpose(1, 2).contiguous().requires_grad_()
        o = DO._forward_batch(W, x, 20, None)
        (AO.adv_loss(o["logits"], torch.tensor([7]), "cross_entropy")[0].sum() * 1.).backward()
        assert np.array_equal(o["logits"][0].detach().numpy(), r["logits"])
        # the backward pass sums a point's neighbours' terms in an order torch does not fix: equal to rounding, not to the bit
        tol = 1e-5 if dtype == torch.float32 else 1e-13
        assert np.abs(x.grad[0].t().numpy() - r["grad"]).max() <= tol * np.abs(r["grad"]).max()
        assert np.array_equal(o["feat"][0].detach().numpy(), r["feat"])


def test_reference_form_against_central_differences(sd):
    import bench
    c = bench.synth_clouds(1, seed=9)[0][:40].astype(np.float64)
    W = DO.to_torch(sd, torch.float64)
    for loss, kappa in (("logits", 0.5), ("cross_entropy", 0.)):
        r = GO.run_cloud(W, c, 3, loss, kappa, scale=0.5, dtype=torch.float64)
        assert r["loss"] > 0
        rng, h = np.random.default_rng(1), 1e-6
        for _ in range(12):
            i, a = int(rng.integers(len(c))), int(rng.integers(3))
            up, dn = c.copy(), c.copy()
            up[i, a] += h
            dn[i, a] -= h
            f = [GO.run_cloud(W, p, 3, loss, kappa, dtype=torch.float64, idx=r["idx"])["loss"] for p in (up, dn)]
            fd = 0.5 * (f[0] - f[1]) / (2 * h)
            assert abs(fd - r["grad"][i, a]) <= 1e-6 * np.abs(r["grad"]).max() + 1e-9, (loss, i, a, fd, r["grad"][i, a])


@pytest.mark.parametrize("loss", ["logits", "cross_entropy"])
def test_explicit_form_fed_the_reference_forms_choices_equals_it(sd, loss):
    import bench
    Wf, W = GO.folded(sd), DO.to_torch(sd, torch.float64)
    for c, k in ((bench.synth_clouds(3, seed=4)[2][:70], 20), (bench.synth_clouds(3, seed=4)[0][:33], 5)):
        r = GO.run_cloud(W, c, 11, loss, 0.25, scale=0.125, k=k, dtype=torch.float64)
        x = GO.explicit_from(Wf, c, 11, r, loss=loss, kappa=0.25, scale=0.125)
        assert np.abs(r["grad"]).max() > 0
        assert np.abs(x["grad"] - r["grad"]).max() <= 1e-12 * np.abs(r["grad"]).max()
        assert np.abs(x["logits"] - r["logits"]).max() <= 1e-12 * np.abs(r["logits"]).max()
        # ... and it is a function of the choices: another winner table gives another gradient
        moved = dict(r, win_edge=[np.roll(w, 1, axis=0) for w in r["win_edge"]])
        assert np.abs(GO.explicit_from(Wf, c, 11, moved, loss=loss)["grad"] - r["grad"]).max() > 1e-6 * np.abs(r["grad"]).max()


def test_validity_checks_refuse_wrong_choices(sd):
    import bench
    c = bench.synth_clouds(1, seed=12)[0][:50]
    r32, r64, e, _ = GO.oracle_case(sd, [c], [4])
    ch = {k: r32[0][k] for k in ("idx", "win_edge", "feat_pos", "act5", "win_pool")}
    GO.choices_valid(ch, r64[0], e, "float32's own")
    far = np.abs(r64[0]["conv5"]).argmax(0)                              # per point the channel furthest from zero
    bad = dict(ch, act5=ch["act5"].copy())
    bad["act5"][np.arange(50), far] ^= True
    with pytest.raises(AssertionError, match="conv5: a sign"):
        GO.choices_valid(bad, r64[0], e)
    low = r64[0]["conv5"].argmin(1)
    with pytest.raises(AssertionError, match="below the maximum"):
        GO.choices_valid(dict(ch, win_pool=low), r64[0], e)
    E = r64[0]["edge"][3]
    worst = np.take_along_axis(r64[0]["idx"][3][:, None, :], E.argmin(-1).T[:, :, None], 2)[:, :, 0]
    with pytest.raises(AssertionError, match="edge 4: winner"):
        GO.choices_valid(dict(ch, win_edge=ch["win_edge"][:3] + [worst]), r64[0], e)
    assert GO.unpack_act5(np.array([[5] + [0] * 30 + [-2 ** 31]], np.int32), 1)[0].nonzero()[0].tolist() == [0, 2, 1023]


@pytest.mark.parametrize("name", list(CASES))
def test_parity_cases_meet_their_conditions(name):
    sd, clouds, targets, k, loss, _ = case_inputs(name)
    _, r64, e, out = GO.oracle_case(sd, clouds, targets, loss, k=k)
    assert all(r["loss"] > 0 for r in r64)
    assert sum(1 for o in out if o) <= MAX_OUT * len(clouds), out


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
    assert names == sorted(_lib.DGCNN_ATK_SIGNATURES) and len(names) == 4
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    assert set(names) <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    version = int(re.search(r"#define IFD_DGCNN_ATK_ABI_VERSION (\d+)", open(HEADER).read()).group(1))
    assert lib.ifd_dgcnn_atk_abi_version() == version == _lib.DGCNN_ATK_ABI_VERSION
    assert lib.ifd_dgcnn_abi_version() == 1 and lib.ifd_atk_abi_version() == 1              # the older headers stay as they were
    assert ctypes.sizeof(_lib.IfdDgcnnGradOut) == 15 * 8


def test_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_dgcnn_input_grad(None, None, None, 1, 32, None, 0, 0.0, 1.0, None, None, None) == -1
    assert lib.ifd_dgcnn_fgm_update(None, 0, None, None, None, None, 0.0, 0.0, 0.0, None, 1, 32, None) == -1
    assert lib.ifd_dgcnn_fgm_attack(None, None, None, None, None, 1, 32, None, None, None) == -1


def test_runtime_class_names_the_dgcnn_calls():
    import ifdefense_amd as I
    assert I.DgcnnClassifier.ATK_FNS == {"input_grad": "ifd_dgcnn_input_grad", "fgm_update": "ifd_dgcnn_fgm_update",
                                         "fgm_attack": "ifd_dgcnn_fgm_attack"}
    assert I.Classifier.ATK_FNS["input_grad"] == "ifd_cls_input_grad"
    assert "not offered" not in I.DgcnnClassifier.__doc__


# ---------------------------------------------------------------------------------------------- CLI host logic
def test_cli_arithmetic_path_and_file(tmp_path, capsys):
    from ifdefense_amd import dgcnn_fgm_attack as DA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src)
    stub, made = StubClassifier(), []

    def make(model, k, path):
        made.append((model, k, path))
        return stub
    argv = ["--data_root", src, "--num_points", "32", "--attack_type", "IFGM", "--num_iter", "10", "--budget", "0.08", "--batch_size", "4",
            "--kappa", "0.5", "--local_rank", "2", "--out_dir", str(tmp_path), "--dataset", "opt_mn40", "--k", "8"]
    assert DA.main(argv, make_classifier=make) == 0
    out = capsys.readouterr().out
    assert made == [("dgcnn", 8, "pretrain/opt_mn40/dgcnn.pth")] and stub.closed
    assert "Loading weight pretrain/opt_mn40/dgcnn.pth" in out
    assert [l for l in out.splitlines() if l.startswith("iter ")][:5] == ["iter %d/10, success: %d/4" % (i, 3 if i else 0) for i in (0, 2, 4, 6, 8)]
    assert out.count("Final success: 3/4") == 1 and out.count("Final success: 1/2") == 1
    budget = 0.08 * np.sqrt(32 * 3)
    grads = [c for c in stub.calls if c[0] == "grad"]
    assert len(grads) == 20 and grads[0] == ("grad", "logits", 0.5, 0.25) and grads[-1] == ("grad", "logits", 0.5, 0.5)
    ups = [c for c in stub.calls if c[0] == "update"]
    assert ups[0][1] == "ifgm" and ups[0][2] == pytest.approx(budget / 10) and ups[0][3] == pytest.approx(budget)
    d = tmp_path / "attack" / "results" / "opt_mn40_32" / "FGM" / "dgcnn"
    name = "ifgm-budget_0.08-iter_10-success_%.4f-rank_2.npz" % (4 / 6)
    assert os.listdir(d) == [name]
    z = np.load(d / name)
    assert sorted(z.files) == ["target_label", "test_label", "test_pc"]
    assert z["test_pc"].dtype == np.float32 and z["test_pc"].shape == (6, 32, 3)
    assert z["test_label"].dtype == np.uint8 and z["target_label"].dtype == np.uint8 and list(z["test_label"]) == list(range(6))
    stub.calls.clear()
    assert DA.main(["--data_root", src, "--num_points", "32", "--out_dir", str(tmp_path), "--adv_func", "cross_entropy"],
                   make_classifier=make) == 0
    assert "Successfully attack 4/6" in capsys.readouterr().out
    assert stub.calls == [("attack", "fgm", pytest.approx(budget), pytest.approx(budget), 1, 1.0, "cross_entropy", 0.0, pytest.approx(1 / 6))]
    assert made[-1] == ("dgcnn", 20, "pretrain/mn40/dgcnn.pth")


def test_cli_refusals_give_status_2_without_a_classifier(tmp_path, capsys):
    from ifdefense_amd import dgcnn_fgm_attack as DA
    src = str(tmp_path / "attack_data.npz")
    _attack_file(src, k=40)
    big = str(tmp_path / "big.npz")
    np.savez(big, test_pc=np.zeros((2, 2049, 3), np.float32) + np.arange(2049)[None, :, None], test_label=np.zeros(2, np.uint8),
             target_label=np.ones(2, np.uint8))

    def never(*a):
        raise AssertionError("the classifier must not be made")
    for argv, word in ((["--model", "pointnet"], "only the dgcnn victim"), (["--model", "pointnet2"], "only the dgcnn victim"),
                       (["--emb_dims", "512"], "--emb_dims 1024"), (["--k", "0"], "--k must lie"), (["--k", "33"], "--k must lie"),
                       (["--feature_transform", "true"], "pointnet"), (["--attack_type", "cw"], "unknown --attack_type"),
                       (["--num_points", "16"], "fewer than k = 20"),
                       (["--data_root", big, "--num_points", "4096"], "more than the 2048")):
        assert DA.main(["--data_root", src, "--out_dir", str(tmp_path)] + argv, make_classifier=never) == 2, argv
        assert word in capsys.readouterr().err, argv
    # fgm_attack itself keeps turning dgcnn away
    from ifdefense_amd import fgm_attack as FA
    assert FA.main(["--data_root", src, "--model", "dgcnn"], make_classifier=never) == 2
