"""CPU checks of the Perturb, kNN and Drop attacks on the DGCNN, PointNet++ and PointConv victims (include/ifd_victim_atk.h): the
C ABI and its binding, the refusals that need no GPU, the host logic of the three victim_*_attack CLIs under stub classifiers, the
start rule of Drop, the start-binding wrapper, input_grad's lean diagnostics, and the inputs of the GPU test of meaning
(tests/test_gpu_victim_atk.py imports them): a free-running float64 Perturb loop per victim, built from the gradient oracles and
cw_oracle.step, fixes the num_iter that test uses."""
import ctypes
import functools
import os
import re
import time
import warnings

import numpy as np
import pytest
import torch

import cw_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_victim_atk.h")
warnings.filterwarnings("ignore", message="Converting a tensor with requires_grad")

VICTIMS = ("dgcnn", "pointnet2", "pointconv")
DG_K = 8                                   # DGCNN's neighbour count in these tests
N_POINTS = 48                              # PointConv's minimum plus room to drop
SYMBOLS = ["ifd_victim_atk_abi_version", "ifd_victim_cw_adjust", "ifd_victim_cw_perturb_attack", "ifd_victim_cw_step",
           "ifd_victim_drop_attack", "ifd_victim_drop_step", "ifd_victim_knn_attack", "ifd_victim_knn_project_clip",
           "ifd_victim_knn_step"]


# ---------------------------------------------------------------------------------------------- the inputs of the test of meaning
# The Perturb run of tests/test_gpu_victim_atk.py::test_perturb_meaning: MEANING_CLOUDS clouds of 48 points per victim, targets the
# float64 oracle's runner-up class, non-zero starts, MEANING_STEPS search steps of NUM_ITER[victim] Adam iterations at lr 0.01.
MEANING_SEED, MEANING_STEPS, MEANING_LR = 11, 2, 1e-2
MEANING_CLOUDS = {"dgcnn": 4, "pointnet2": 4, "pointconv": 4}
ITER_LIST = (5, 10, 20, 40, 80)
# test_oracle_perturb_reaches_the_target: the smallest entry of ITER_LIST at which the float64 oracle alone reaches the target on at
# least half the clouds, and its count there - see that test's docstring
NUM_ITER = {"dgcnn": 5, "pointnet2": 5, "pointconv": 20}


def state_dict(victim):
    import dgcnn_oracle as DO
    import pointconv_oracle as PCO
    import pointnet2_oracle as PO
    return {"dgcnn": lambda: DO.make_calibrated_weights(0, DG_K), "pointnet2": lambda: PO.make_calibrated_weights(0),
            "pointconv": lambda: PCO.make_calibrated_weights(0)}[victim]()


def oracle_grad(victim, dtype=torch.float64):
    """-> f(cloud [n,3], target, start (2,), scale) = the reference-form oracle's run of one cloud (grad, logits, ...) on the
    tables its own float32 selection makes of the cloud."""
    sd = state_dict(victim)
    if victim == "dgcnn":
        import dgcnn_grad_oracle as GO
        import dgcnn_oracle as DO
        W = DO.to_torch(sd, dtype)
        return lambda x, t, start, scale: GO.run_cloud(W, x, t, "logits", 0., scale, k=DG_K, dtype=dtype)
    if victim == "pointnet2":
        import pointnet2_grad_oracle as GO
        import pointnet2_oracle as O
    else:
        import pointconv_grad_oracle as GO
        import pointconv_oracle as O
    W = O.to_torch(sd, dtype)
    return lambda x, t, start, scale: GO.run_cloud(W, x, t, O.tables_of_cloud(np.asarray(x, np.float32), tuple(int(s) for s in start)),
                                                   "logits", 0., scale, dtype)


@functools.lru_cache(maxsize=None)
def meaning_inputs(victim):
    """-> (clouds [B,48,3] float32 on the unit sphere, targets [B] int64, starts [B,2] int32 (zeros for DGCNN), noise
    [MEANING_STEPS,B,48,3] float32).  A cloud's target is the runner-up class of the float64 oracle on that cloud."""
    import bench
    from ifdefense_amd.inference import normalize_points_np
    B = MEANING_CLOUDS[victim]
    clouds = np.stack([normalize_points_np(c[:N_POINTS]) for c in bench.synth_clouds(B, seed=MEANING_SEED)]).astype(np.float32)
    starts = np.zeros((B, 2), np.int32)
    if victim != "dgcnn":
        starts = np.stack([(7 * np.arange(B) + 3) % N_POINTS, (11 * np.arange(B) + 5) % 512], axis=1).astype(np.int32)
    run = oracle_grad(victim)
    targets = np.array([int(np.argsort(run(c, 0, s, 1.0)["logits"])[-2]) for c, s in zip(clouds, starts)], np.int64)
    g = torch.Generator().manual_seed(MEANING_SEED)
    noise = torch.stack([torch.randn(clouds.shape, generator=g) * 1e-7 for _ in range(MEANING_STEPS)]).numpy()
    return clouds, targets, starts, noise


def oracle_perturb(victim, num_iter):
    """cw_oracle.attack's loop with the victim's gradient oracle in place of PointNet's -> success [B] bool (lower > 0)."""
    clouds, targets, starts, noise = meaning_inputs(victim)
    run = oracle_grad(victim)
    B = len(clouds)
    ok = np.zeros(B, bool)
    for b in range(B):
        ori, tg = clouds[b].astype(np.float64), int(targets[b])
        weight, lower, upper, rec = 10., 0., 80., CO.fresh_record(N_POINTS)
        for s in range(MEANING_STEPS):
            adv = ori + noise[s][b].astype(np.float64)
            m, v = np.zeros_like(ori), np.zeros_like(ori)
            for it in range(num_iter):
                r = run(adv, tg, starts[b], 1.0 / B)
                adv, m, v, rec, _, _ = CO.step(r["grad"], int(r["logits"].argmax()), tg, adv, ori, weight, m, v, it + 1, MEANING_LR, 1.0 / B, rec)
            weight, lower, upper, rec = CO.adjust(rec, tg, weight, lower, upper)
        ok[b] = lower > 0
    return ok


@pytest.mark.parametrize("victim", VICTIMS)
def test_oracle_perturb_reaches_the_target(victim):
    """A condition on the inputs of the GPU test of meaning, not a parity bar: the float32 trajectory of the GPU may leave the
    float64 one at the first gate the two precisions take differently.  NUM_ITER[victim] is the smallest entry of ITER_LIST at which
    the float64 oracle reaches the target (lower > 0 after MEANING_STEPS search steps) on at least half the clouds.  Found:
        dgcnn      5 iterations: 4 of 4 clouds
        pointnet2  5 iterations: 4 of 4 clouds
        pointconv  5 iterations: 1 of 4, 10 iterations: 1 of 4, 20 iterations: 2 of 4 clouds
    (the targets are the oracle's runner-up classes; on DGCNN and PointNet++ two Adam steps of 0.01 already reach most of them).
    The three runs of PointConv's oracle take about half a minute together."""
    n = NUM_ITER[victim]
    B = MEANING_CLOUDS[victim]
    for shorter in [i for i in ITER_LIST if i < n]:
        t0 = time.time()
        ok = oracle_perturb(victim, shorter)
        print("%s: %d iterations: %d of %d clouds (%.1f s)" % (victim, shorter, int(ok.sum()), B, time.time() - t0))
        assert 2 * int(ok.sum()) < B, "a shorter run already reaches the target on half the clouds: lower NUM_ITER"
    t0 = time.time()
    ok = oracle_perturb(victim, n)
    print("%s: %d iterations: %d of %d clouds (%.1f s)" % (victim, n, int(ok.sum()), B, time.time() - t0))
    assert 2 * int(ok.sum()) >= B


# ---------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def lib():
    import ifdefense_amd as I
    return I.load_library()


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ifd_victim_\w+)\s*\(", src)))


def test_header_binding_and_library_agree(lib):
    from ifdefense_amd import _lib
    assert declared_symbols() == SYMBOLS == sorted(_lib.VICTIM_ATK_SIGNATURES)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.ifd_victim_atk_abi_version() == _lib.VICTIM_ATK_ABI_VERSION == 1
    assert "#define IFD_VICTIM_ATK_ABI_VERSION 1" in open(HEADER).read()
    # the step calls have the signatures of the PointNet calls, the loops one pointer more (fps_start)
    for new, old, table in (("ifd_victim_cw_step", "ifd_cw_step", _lib.CW_SIGNATURES), ("ifd_victim_cw_adjust", "ifd_cw_adjust", _lib.CW_SIGNATURES),
                            ("ifd_victim_knn_step", "ifd_knn_step", _lib.KNN_SIGNATURES),
                            ("ifd_victim_knn_project_clip", "ifd_knn_project_clip", _lib.KNN_SIGNATURES),
                            ("ifd_victim_drop_step", "ifd_drop_step", _lib.DROP_SIGNATURES)):
        assert _lib.VICTIM_ATK_SIGNATURES[new] == table[old]
    for new, old, table in (("ifd_victim_cw_perturb_attack", "ifd_cw_perturb_attack", _lib.CW_SIGNATURES),
                            ("ifd_victim_knn_attack", "ifd_knn_attack", _lib.KNN_SIGNATURES),
                            ("ifd_victim_drop_attack", "ifd_drop_attack", _lib.DROP_SIGNATURES)):
        assert len(_lib.VICTIM_ATK_SIGNATURES[new][1]) == len(table[old][1]) + 1


def test_calls_refuse_a_null_context_before_any_hip_call(lib):
    assert lib.ifd_victim_cw_step(None, None, None, None, None, None, None, None, None, None, 1, 0.0, 1.0, None, 1, 48, None) == -1
    assert lib.ifd_victim_cw_adjust(None, None, None, None, 1, 48, None) == -1
    assert lib.ifd_victim_knn_step(None, None, None, None, None, None, None, None, None, 1, 0.0, 1.0, None, None, 1, 48, None) == -1
    assert lib.ifd_victim_knn_project_clip(None, None, None, None, 0.1, None, 1, 48, None) == -1
    assert lib.ifd_victim_drop_step(None, None, None, None, None, 1, 48, 1, 1.0, None, None) == -1
    assert lib.ifd_victim_cw_perturb_attack(None, None, None, None, None, None, None, 1, 48, None, None, None, None, None) == -1
    assert lib.ifd_victim_knn_attack(None, None, None, None, None, None, None, None, 1, 48, None, None, None, None) == -1
    assert lib.ifd_victim_drop_attack(None, None, None, None, None, None, 1, 48, None, None, None, None, None) == -1


def test_runtime_classes_name_the_calls():
    import ifdefense_amd as I
    for cls in (I.DgcnnClassifier, I.PointNet2Classifier, I.PointConvClassifier):
        assert cls.LOOP_FNS == {k: "ifd_victim_" + k for k in ("cw_step", "cw_adjust", "cw_perturb_attack", "knn_step", "knn_project_clip",
                                                               "knn_attack", "drop_step", "drop_attack")}
        assert "refuses them on a" not in cls.__doc__.split("point-adding")[0]
    assert I.Classifier.LOOP_FNS == {k: "ifd_" + k for k in I.DgcnnClassifier.LOOP_FNS}      # PointNet keeps its own entry points


# ---------------------------------------------------------------------------------------------- input_grad's lean diagnostics
@pytest.mark.parametrize("cls_name", ["Classifier", "DgcnnClassifier", "PointNet2Classifier", "PointConvClassifier"])
def test_want_aux_as_a_tuple_allocates_only_the_named(cls_name):
    import ifdefense_amd as I
    net = object.__new__(getattr(I, cls_name))             # no context: _grad_aux only allocates
    net.device, net.k, net.ctx = torch.device("cpu"), DG_K, None
    full, st_full = net._grad_aux(2, 40)
    assert {"logits", "loss", "pred", "global_feat"} <= set(full) and len(full) >= 6
    aux, st = net._grad_aux(2, 40, ("pred", "loss"))
    assert sorted(aux) == ["loss", "pred"] and aux["pred"].dtype == torch.int32 and tuple(aux["loss"].shape) == (2,)
    assert st.pred == aux["pred"].data_ptr() and st.loss == aux["loss"].data_ptr()
    for name, _ in st._fields_:
        if name not in ("pred", "loss"):
            v = getattr(st, name)
            assert not (list(v) if hasattr(v, "__len__") else [v])[0], name        # NULL: the library skips it
    for name, t in full.items():                           # the full table keeps its shapes and fills
        assert (list(getattr(st_full, name)) if isinstance(t, list) else [getattr(st_full, name)])[0]
    with pytest.raises(I.IfdError, match="unknown diagnostic 'nope'"):
        net._grad_aux(2, 40, ("pred", "nope"))
    if cls_name == "DgcnnClassifier":
        a, _ = net._grad_aux(1, 40, ("idx", "feat"))
        assert len(a["idx"]) == 4 and int(a["idx"][0].min()) == -1 and tuple(a["idx"][3].shape) == (1, 40, DG_K) and not a["feat"].any()
    if cls_name == "PointConvClassifier":
        a, _ = net._grad_aux(1, 40, ("dens1", "dgate1"))
        assert not a["dens1"].any() and not a["dgate1"].any() and a["dgate1"].dtype == torch.int32


# ---------------------------------------------------------------------------------------------- starts
def test_drop_starts_are_those_of_the_written_sizes():
    """Drop: fps_starts(seed, sizes - num_drop), the starts the victim's inference CLI takes for the file that is written; they
    name rows that every round still has, and they are not the starts of the clouds that go in."""
    from ifdefense_amd import victim_drop_attack as VD
    from ifdefense_amd.pointnet2_inference import fps_starts
    import tempfile
    for seed in range(1, 6):
        st = fps_starts(seed, [N_POINTS - 12] * 40)
        assert (st[:, 0] < N_POINTS - 12).all() and (st[:, 0] >= 0).all() and (st[:, 1] < 512).all() and (st[:, 1] >= 0).all()
        assert not np.array_equal(st, fps_starts(seed, [N_POINTS] * 40))
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "attack_data.npz")
        _file(src)
        for victim in ("pointnet2", "pointconv"):
            nets = []
            assert VD.main(["--data_root", src, "--model", victim, "--num_points", str(N_POINTS), "--num_drop", "12", "--fps_seed", "7",
                            "--out_dir", tmp, "--batch_size", "3"], make_classifier=_make(nets, victim)) == 0
            got = np.concatenate([c["starts"] for c in nets[0].calls])
            assert np.array_equal(got, fps_starts(7, [N_POINTS - 12] * 5)) and [len(c["pc"]) for c in nets[0].calls] == [3, 2]


def test_wrapper_binds_the_batch_and_raises_on_a_mismatch():
    from ifdefense_amd.victim_atk_cli import BoundLoopStarts
    net = StubNet()
    w = BoundLoopStarts(net, np.arange(12, dtype=np.int32).reshape(6, 2))
    pc = torch.zeros(2, 48, 3)
    with pytest.raises(ValueError, match="does not match"):
        w.predict(pc)                                                          # nothing bound yet
    w.at(2, 2)
    for call in (lambda: w.predict(pc), lambda: w.input_grad(pc, [1, 2], "logits", 0., 1., n_points=None, want_aux=("pred",)),
                 lambda: w.cw_perturb_attack(pc, [1, 2], None, "logits", 0., 1., 1e-2, 10., 80., 2, 3),
                 lambda: w.knn_attack(pc, [1, 2], None, None, "logits", 15., 1., 1e-3, 3),
                 lambda: w.drop_attack(pc, [1, 2], 5, 5, 1., 1.)):
        call()
        assert np.array_equal(net.last_starts, [[4, 5], [6, 7]])
        net.last_starts = None
    assert w.cw_state.__self__ is net and w.cw_step.__self__ is net and w.knn_step.__self__ is net and w.drop_step.__self__ is net
    with pytest.raises(AttributeError):
        w.add_attack
    w.at(0, 3)
    for call in (lambda: w.predict(pc), lambda: w.input_grad(pc, [1, 2]), lambda: w.knn_attack(pc, [1, 2]), lambda: w.drop_attack(pc, [1, 2], 5),
                 lambda: w.cw_perturb_attack(pc, [1, 2])):
        with pytest.raises(ValueError, match="the batch of 2 clouds does not match the 3 starts"):
            call()
    w.close()
    assert net.closed


# ---------------------------------------------------------------------------------------------- the CLIs' host logic
class StubNet:
    """A classifier of any victim: records what the CLIs hand to the whole-loop calls."""
    device = "cpu"

    def __init__(self):
        self.calls, self.closed, self.last_starts = [], False, None

    def _seen(self, what, pc, fps_start, **kw):
        self.last_starts = None if fps_start is None else np.asarray(fps_start).copy()
        self.calls.append(dict(what=what, pc=np.asarray(pc, np.float32).copy(), starts=self.last_starts, **kw))

    def predict(self, pc, n_points=None, fps_start=None):
        self._seen("predict", pc, fps_start)
        return torch.zeros(len(pc), dtype=torch.long)

    def input_grad(self, pc, target, loss="logits", kappa=0., scale=1., n_points=None, want_aux=False, fps_start=None):
        self._seen("grad", pc, fps_start, want_aux=want_aux)
        return torch.zeros_like(torch.as_tensor(pc)), {"pred": torch.zeros(len(pc), dtype=torch.int32), "loss": torch.zeros(len(pc))}

    def cw_perturb_attack(self, pc, target, noise=None, loss="logits", kappa=0., scale=1., lr=1e-2, init_weight=10., max_weight=80.,
                          binary_step=10, num_iter=500, fps_start=None):
        self._seen("perturb", pc, fps_start, noise=None if noise is None else noise.clone(), scale=scale, steps=(binary_step, num_iter))
        ok = torch.as_tensor(target) == 3
        return torch.as_tensor(pc) + 1.0, torch.where(ok, 0.5, 1e10).float(), ok

    def knn_attack(self, pc, target, normal=None, noise=None, loss="logits", kappa=15., scale=1., lr=1e-3, num_iter=2500, fps_start=None, **hyper):
        self._seen("knn", pc, fps_start, noise=None if noise is None else noise.clone(), scale=scale, normal=normal)
        ok = torch.as_tensor(target) == 3
        return torch.as_tensor(pc) + 2.0, torch.as_tensor(target), ok

    def drop_attack(self, pc, label, num_drop, k=5, alpha=1., scale=1., fps_start=None):
        self._seen("drop", pc, fps_start, scale=scale, num_drop=num_drop)
        return torch.as_tensor(pc)[:, :pc.shape[1] - num_drop], torch.as_tensor(label) == 3

    def cw_state(self, *a):
        return {}

    def cw_step(self, *a, **k):
        return None

    def knn_step(self, *a, **k):
        return {}

    def drop_step(self, *a, **k):
        return {}

    def close(self):
        self.closed = True


def _file(path, n=5, k=N_POINTS, cols=3):
    rng = np.random.default_rng(3)
    np.savez(path, test_pc=rng.standard_normal((n, k, cols)).astype(np.float32), test_label=np.array([3, 3, 1, 3, 2][:n], np.uint8),
             target_label=np.array([3, 5, 3, 5, 3][:n], np.uint8))


def _cli(kind):
    from ifdefense_amd import victim_drop_attack, victim_knn_attack, victim_perturb_attack
    return {"perturb": victim_perturb_attack, "knn": victim_knn_attack, "drop": victim_drop_attack}[kind]


def _make(nets, victim):
    def make(model, *a):
        assert model == victim and len(a) == (2 if victim == "dgcnn" else 1) and (victim != "dgcnn" or a[0] == DG_K)
        nets.append(StubNet())
        return nets[-1]
    return make


@pytest.mark.parametrize("victim", VICTIMS)
@pytest.mark.parametrize("kind", ["perturb", "knn", "drop"])
def test_cli_result_path_scale_noise_and_starts(tmp_path, capsys, kind, victim):
    """The file lands under the reference's path with the rate the stub returned; every batch sees scale 1 / N of the file, its
    rows of the file's noise, and (PointNet++, PointConv) its rows of fps_starts(fps_seed, sizes written); --batch_size 2 hands the
    library the same clouds, noise and starts as -1."""
    from ifdefense_amd.pointnet2_inference import fps_starts
    from ifdefense_amd.victim_atk_cli import file_noise
    src = str(tmp_path / "attack_data.npz")
    _file(src, cols=6 if kind == "knn" else 3)
    seen = {}
    for bs in (-1, 2):
        nets, out = [], tmp_path / ("bs%d" % bs)
        argv = ["--data_root", src, "--model", victim, "--num_points", str(N_POINTS), "--k", str(DG_K), "--fps_seed", "4", "--out_dir", str(out),
                "--batch_size", str(bs)]
        argv += {"perturb": ["--binary_step", "2", "--num_iter", "3", "--seed", "9"], "knn": ["--num_iter", "3", "--seed", "9"],
                 "drop": ["--num_drop", "12"]}[kind]
        assert _cli(kind).main(argv, make_classifier=_make(nets, victim)) == 0
        (net,) = nets
        assert net.closed and [c["what"] for c in net.calls] == [kind] * (1 if bs < 0 else 3)
        assert all(abs(c["scale"] - 0.2) < 1e-12 for c in net.calls)
        seen[bs] = net.calls
        sub = {"perturb": "Perturb", "knn": "kNN", "drop": "Drop_12"}[kind]
        d = out / "attack" / "results" / ("mn40_%d" % N_POINTS) / sub
        want = {"perturb": "Perturb-%s-logits_kappa=0.0-success_0.6000-rank_0.npz", "knn": "kNN-%s-logits_kappa=15.0-success_0.6000-rank_0.npz",
                "drop": "Drop-%s-acc_0.6000.npz"}[kind] % victim
        assert os.listdir(d) == [want]
        z = np.load(d / want)
        assert z["test_pc"].shape == (5, N_POINTS - (12 if kind == "drop" else 0), 3) and z["test_pc"].dtype == np.float32
        assert z["test_label"].tolist() == [3, 3, 1, 3, 2] and z["target_label"].tolist() == [3, 5, 3, 5, 3]
    whole = seen[-1][0]
    assert np.array_equal(np.concatenate([c["pc"] for c in seen[2]]), whole["pc"])
    if victim == "dgcnn":
        assert whole["starts"] is None and all(c["starts"] is None for c in seen[2])
    else:
        st = fps_starts(4, [N_POINTS - (12 if kind == "drop" else 0)] * 5)
        assert np.array_equal(whole["starts"], st) and np.array_equal(np.concatenate([c["starts"] for c in seen[2]]), st)
    if kind != "drop":
        steps = 2 if kind == "perturb" else 1
        noise = file_noise(9, (5, N_POINTS, 3), steps, 0, 5)
        noise = noise if kind == "perturb" else noise[0]
        axis = 1 if kind == "perturb" else 0
        assert torch.equal(whole["noise"], noise) and torch.equal(torch.cat([c["noise"] for c in seen[2]], dim=axis), noise)
        assert float(noise.abs().max()) < 1e-6 and float(noise.abs().max()) > 0
        assert torch.equal(file_noise(9, (5, N_POINTS, 3), steps, 2, 2), (noise[:, 2:4] if kind == "perturb" else noise[None, 2:4]))
    capsys.readouterr()


@pytest.mark.parametrize("kind", ["perturb", "knn", "drop"])
def test_cli_refusals_come_before_the_victim_is_made(tmp_path, capsys, kind):
    src = str(tmp_path / "attack_data.npz")
    _file(src, cols=6 if kind == "knn" else 3)
    cli = _cli(kind)
    tail = ["--num_drop", "12"] if kind == "drop" else []

    def made(*a):
        raise AssertionError("the victim was made")
    base = ["--data_root", src, "--num_points", str(N_POINTS), "--out_dir", str(tmp_path / "o")] + tail
    own = {"perturb": "ifdefense_amd.perturb_attack", "knn": "ifdefense_amd.knn_attack", "drop": "ifdefense_amd.drop_attack"}[kind]
    cases = [(["--model", "pointnet"], own), ([], own),                       # --model defaults to pointnet, as in the reference
             (["--model", "pointnet2", "--feature_transform", "true"], "--feature_transform belongs to pointnet"),
             (["--model", "dgcnn", "--k", "33"], r"--k must lie in \[1, 32\]"), (["--model", "dgcnn", "--emb_dims", "512"], "--emb_dims 1024"),
             (["--model", "dgcnn", "--k", "32", "--num_points", "40" if kind == "drop" else "20"], "fewer than the 32"),
             (["--model", "pointconv", "--num_points", "43" if kind == "drop" else "31"], "fewer than the 32")]
    if kind == "knn":
        cases.append((["--model", "pointnet2", "--num_points", "5"], "fewer than the 6"))
    if kind == "drop":
        cases += [(["--model", "pointnet2", "--num_drop", "48"], "--num_drop < --num_points"),
                  (["--model", "dgcnn", "--k", "8", "--num_drop", "41"], "fewer than the 8 points the DGCNN victim needs"),
                  (["--model", "pointconv", "--num_drop", "17"], "fewer than the 32 points the PointConv victim needs")]
    for extra, word in cases:
        assert cli.main(base + extra, make_classifier=made) == 2, extra
        err = capsys.readouterr().err
        assert re.search(word, err) and err.startswith("victim_%s_attack: " % kind), (extra, err)
    assert not (tmp_path / "o").exists()
    # a file whose clouds are larger than the victim takes
    big = str(tmp_path / "big.npz")
    _file(big, n=2, k=2050, cols=6 if kind == "knn" else 3)
    if kind != "drop":
        assert cli.main(["--data_root", big, "--num_points", "2050", "--model", "pointnet2"], make_classifier=made) == 2
        assert "more than the 2048 the PointNet++ victim takes" in capsys.readouterr().err


def test_existing_clis_keep_refusing_the_other_victims(capsys):
    from ifdefense_amd import drop_attack, knn_attack, perturb_attack
    for cli in (perturb_attack, knn_attack, drop_attack):
        for victim in VICTIMS:
            assert cli.main(["--model", victim]) == 2
            assert "not built here" in capsys.readouterr().err
