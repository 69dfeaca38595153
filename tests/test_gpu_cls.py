"""GPU parity of the victim classifier (include/ifd_cls.h) against tests/pointnet_oracle.py in float64 and against the recorded
reference run (tests/golden/cls_golden.npz), with the oracle's seeded weights.  Every bar is relative to
e_32 = max |float32 oracle - float64 oracle|, computed here."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cls_golden.npz")
NAMES = ("logits", "trans", "trans_feat", "global_feat")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "feature_transform"])
def ft(request):
    return request.param


@pytest.fixture(scope="module")
def sd(g, ft):
    import pointnet_oracle as PO
    return PO.make_weights(int(g["weight_seed"]), ft)


@pytest.fixture(scope="module")
def net(sd, ft):
    import ifdefense_amd as I
    from ifdefense_amd import weights
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), feature_transform=ft, device="cuda:0") as c:
        yield c


def clouds_of(g):
    return [g["pc_%d" % i] for i in range(int(g["n_clouds"]))]


def oracle_pair(sd, x, n_points=None, chunk=64):
    """(float32 oracle, float64 oracle) outputs of pointnet_oracle.forward, batched inputs in chunks."""
    import pointnet_oracle as PO
    out = []
    for dt in (torch.float32, torch.float64):
        W = PO.to_torch(sd, dt)
        if isinstance(x, list) or n_points is not None:
            out.append(PO.forward(W, x, n_points, dtype=dt))
        else:
            parts = [PO.forward(W, x[a:a + chunk], dtype=dt) for a in range(0, len(x), chunk)]
            out.append(tuple(None if parts[0][j] is None else torch.cat([p[j] for p in parts]) for j in range(4)))
    return out


def gpu_outputs(net, x, n_points=None):
    lo, aux = net.logits(x, n_points, want_aux=True)
    torch.cuda.synchronize()
    return (lo.cpu(), aux["trans"].cpu(), aux["trans_feat"].cpu() if "trans_feat" in aux else None, aux["global_feat"].cpu()), aux["pred"].cpu()


def check_against_f64(got, r32, r64, what):
    worst = 0.0
    for name, a, b32, b64 in zip(NAMES, got, r32, r64):
        if b64 is None:
            assert a is None
            continue
        e_gpu = float((a.double() - b64).abs().max())
        e_32 = float((b32.double() - b64).abs().max())
        print("%s %s: max |GPU - f64| %.3e, max |f32 oracle - f64| %.3e, ratio %.2f" % (what, name, e_gpu, e_32, e_gpu / e_32))
        worst = max(worst, e_gpu / e_32)
        assert torch.isfinite(a).all()
        assert e_gpu <= 4 * e_32, (what, name)
    return worst


def test_arithmetic_against_float64(net, sd, g):
    r32, r64 = oracle_pair(sd, clouds_of(g))
    got, _ = gpu_outputs(net, clouds_of(g))
    check_against_f64(got, r32, r64, "golden clouds")


def test_against_recorded_reference(net, sd, g, ft):
    s = "_t" if ft else "_f"
    r32, r64 = oracle_pair(sd, clouds_of(g))
    e_32 = float((r32[0].double() - r64[0]).abs().max())
    got, pred = gpu_outputs(net, clouds_of(g))
    d = float(np.abs(got[0].numpy() - g["logits" + s]).max())
    print("max |GPU - reference f32 logits| %.3e, e_32 %.3e" % (d, e_32))
    assert d <= 4 * e_32 + e_32
    assert np.array_equal(pred.numpy(), g["logits" + s].argmax(1))            # every golden cloud, no exclusions
    assert np.array_equal(net.predict(clouds_of(g)).cpu().numpy(), g["logits" + s].argmax(1))


def test_ragged_and_batch_invariance(net):
    import bench
    x = torch.from_numpy(bench.synth_clouds(300, seed=21))
    big = net.logits(x).cpu()
    alone = net.logits(x[123:124]).cpu()
    assert torch.equal(big[123:124], alone)
    moved = net.logits(torch.roll(x, 50, 0)).cpu()                             # cloud 123 at position 173
    assert torch.equal(moved[173:174], alone)
    padded = torch.full((5, 1500, 3), float("nan"))
    padded[:, :1024] = x[121:126]
    padded[0, 700:] = float("nan")
    n = torch.tensor([700, 1024, 1024, 1024, 1024], dtype=torch.int32)
    got = net.logits(padded, n).cpu()
    assert torch.isfinite(got).all() and torch.equal(got[2:3], alone) and torch.equal(got[1:], big[122:126])
    assert torch.equal(got[0:1], net.logits(x[121:122, :700]).cpu())
    assert torch.equal(net.logits([c.numpy() for c in x[121:124]] + [x[124, :600].numpy()]).cpu()[2:3], alone)   # ragged list
    f = torch.from_numpy(bench.synth_clouds(2468, seed=22))
    a, b = net.logits(f).cpu(), net.logits(f).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_large_file_argmax(net, sd):
    import bench
    f = bench.synth_clouds(2468, seed=23)
    r32, r64 = oracle_pair(sd, f)
    e_32 = float((r32[0].double() - r64[0]).abs().max())
    pred = net.predict(torch.from_numpy(f)).cpu().numpy()
    top = torch.sort(r64[0], dim=1).values
    margin = (top[:, -1] - top[:, -2]).numpy()
    close = margin < 100 * e_32
    lo = net.logits(torch.from_numpy(f)).cpu()
    print("2468 clouds: e_32 %.3e, max |GPU - f64| %.3e, clouds excluded for a top-2 margin below 100 e_32: %d, classes predicted: %d"
          % (e_32, float((lo.double() - r64[0]).abs().max()), int(close.sum()), len(set(pred.tolist()))))
    assert close.sum() <= 0.005 * len(f)
    want = r64[0].argmax(1).numpy()
    assert np.array_equal(pred[~close], want[~close])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 600, 824, 1024, 1536, 4096])
def test_point_counts(net, sd, n):
    import bench
    base = bench.synth_clouds(16, seed=24)
    x = np.concatenate([base[4 * j:4 * j + 3] + 0.003 * j for j in range(4)], 1)[:, :n].astype(np.float32)   # [3, n, 3], n <= 4096
    x = np.ascontiguousarray(x)
    r32, r64 = oracle_pair(sd, x)
    got, _ = gpu_outputs(net, torch.from_numpy(x))
    check_against_f64(got, r32, r64, "%d points" % n)


def test_bad_counts_are_errors_not_faults(net):
    import ifdefense_amd as I
    from ifdefense_amd import _lib
    x = torch.zeros(4, 64, 3)
    with pytest.raises(I.IfdError, match="n_points"):
        net.logits(x, torch.tensor([64, 0, 64, 64], dtype=torch.int32))
    with pytest.raises(I.IfdError, match="n_points"):
        net.logits(x, torch.tensor([64, 65, 64, 64], dtype=torch.int32))
    with pytest.raises(I.IfdError, match="stride"):
        net.logits(torch.zeros(1, _lib.CLS_MAX_POINTS + 1, 3))
    if not net.feature_transform:
        out = torch.empty(4, 40, device="cuda:0")
        tf = torch.empty(4, 64, 64, device="cuda:0")
        import ctypes as C
        rc = net.lib.ifd_cls_forward(net.ctx, x.cuda().data_ptr(), None, 4, 64, out.data_ptr(),
                                     C.byref(_lib.IfdClsAux(None, tf.data_ptr(), None, None)), None)
        assert rc == -1 and b"feature_transform" in net.lib.ifd_last_error(net.ctx)
    assert torch.isfinite(net.logits(x)).all()                                # the context still works


def test_cli_end_to_end(net, sd, ft, tmp_path, capsys):
    """Labels are built from the oracle's predictions so that accuracy and success rate are known fractions."""
    import bench
    import pointnet_oracle as PO
    from ifdefense_amd import inference as Inf
    wp = str(tmp_path / "pointnet.pth")
    torch.save(PO.reference_state_dict(sd), wp)                               # a DataParallel checkpoint, as the reference saves it
    x = bench.synth_clouds(10, seed=25)
    x = np.concatenate([x, x[:, :512] + 0.01], 1).astype(np.float32)          # 1536 rows: only the first 1024 count
    want = PO.forward(PO.to_torch(sd, torch.float64), x[:, :1024], dtype=torch.float64)[0].argmax(1).numpy()
    label = want.copy()
    label[[1, 4, 7]] = (label[[1, 4, 7]] + 1) % 40                            # 7 of 10 right
    target = (want + 3) % 40
    target[[0, 1, 2, 3]] = want[[0, 1, 2, 3]]                                 # 4 of 10 hit the target
    p = str(tmp_path / "kNN-pointnet-adv.npz")
    np.savez(p, test_pc=x, test_label=label.astype(np.uint8), target_label=target.astype(np.uint8))
    common = ["--data_root", p, "--model_path", wp, "--feature_transform", str(ft)]
    assert Inf.main(common) == 0
    assert capsys.readouterr().out == "Overall accuracy: 0.7000\n"
    assert Inf.main(common + ["--mode", "target", "--model", "pointnet"]) == 0
    assert capsys.readouterr().out == "Overall accuracy: 0.7000, attack success rate: 0.4000\n"
    # an object-array "sor" file of ragged clouds
    sizes = [1024, 1001, 987, 640, 1024, 999]
    rag = np.empty(6, dtype=object)
    for i, k in enumerate(sizes):
        rag[i] = x[i, :k].copy()
    want = PO.forward(PO.to_torch(sd, torch.float64), [rag[i] for i in range(6)], dtype=torch.float64)[0].argmax(1).numpy()
    label = want.copy()
    label[[0, 5]] = (label[[0, 5]] + 7) % 40                                  # 4 of 6 right
    target = (want + 1) % 40
    target[2] = want[2]                                                       # 1 of 6
    d = tmp_path / "sor"
    d.mkdir()
    p = str(d / "sor_kNN-pointnet-adv.npz")
    np.savez(p, test_pc=rag, test_label=label.astype(np.uint8), target_label=target.astype(np.uint8))
    assert Inf.main(["--data_root", p, "--model_path", wp, "--feature_transform", str(ft), "--mode", "target"]) == 0
    assert capsys.readouterr().out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % (4 / 6, 1 / 6)


def test_cli_evaluates_this_projects_dup_output(net, sd, ft, tmp_path, capsys):
    import bench
    import punet_oracle as PUO
    import pointnet_oracle as PO
    from ifdefense_amd import defend_npz as D, inference as Inf
    x = bench.synth_clouds(6, seed=26)
    data = tmp_path / "perturb-pointnet.npz"
    np.savez(str(data), test_pc=x, test_label=np.arange(6), target_label=np.arange(6) + 1)
    pu = tmp_path / "pu.npz"
    np.savez(str(pu), **PUO.load_weights())
    assert D.main(["--data_root", str(data), "--defense", "dup", "--pu_weight", str(pu)]) == 0
    capsys.readouterr()
    out = str(tmp_path / "dup" / "dup_perturb-pointnet.npz")
    restored = np.load(out)["test_pc"]
    assert restored.shape == (6, 4096, 3)
    wp = str(tmp_path / "pn.npz")
    np.savez(wp, **sd)
    import ifdefense_amd as I
    r = I.evaluate_npz(out, net, "target", 4096, False)
    want = PO.forward(PO.to_torch(sd, torch.float64), restored, dtype=torch.float64)[0].argmax(1).numpy()
    assert r["n"] == 6 and np.array_equal(r["pred"], want)
    assert Inf.main(["--data_root", out, "--model_path", wp, "--feature_transform", str(ft), "--mode", "target", "--num_points", "4096"]) == 0
    acc, suc = float((want == np.arange(6)).sum()) / 6, float((want == np.arange(6) + 1).sum()) / 6
    assert capsys.readouterr().out == "Overall accuracy: %.4f, attack success rate: %.4f\n" % (acc, suc)
