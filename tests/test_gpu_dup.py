"""GPU parity of the baseline defenses (include/ifd_dup.h) against the recorded reference run (tests/golden/dup_golden.npz,
the shipped PU-Net checkpoint) and against tests/punet_oracle.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dup_golden.npz")
GOLDEN_OUT = os.path.join(ROOT, "tests", "golden", "dup_golden_out.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN), out=np.load(GOLDEN_OUT)["out"])


@pytest.fixture(scope="module")
def net():
    import ifdefense_amd as I
    import punet_oracle as PO
    from ifdefense_amd import weights
    d = I.DupNet(weights.pack_state_dict(PO.load_weights(), "punet"), device="cuda:0", seed=3)
    yield d
    d.close()


@pytest.fixture(scope="module")
def gpu_golden(net, g):
    """The golden clouds through ifd_punet_forward with the reference's FPS starts, decisions recorded."""
    out, aux = net.pu_net(torch.from_numpy(g["filled"]), fps_start=torch.from_numpy(g["fps_start"]), want_aux=True)
    torch.cuda.synchronize()
    return out.cpu(), {k: v.cpu() for k, v in aux.items()}


def test_srs(net, g):
    for i in range(int(g["n_clouds"])):
        pc = torch.from_numpy(g["pc_%d" % i])[None]
        drop = int(g["srs_drop_%d" % i])
        got = net.srs(pc, drop, idx=torch.from_numpy(g["srs_idx_%d" % i])[None]).cpu().numpy()[0]
        assert np.array_equal(got, g["srs_out_%d" % i])
    pc = torch.from_numpy(np.stack([g["pc_%d" % i] for i in range(7)]))     # clouds without repeated rows
    a = net.srs(pc, 500).cpu()
    b = torch.cat([net.srs(pc[:3], 500).cpu(), net.srs(pc[3:], 500, cloud_index_base=3).cpu()])
    assert torch.equal(a, b) and torch.equal(a, net.srs(pc, 500).cpu())
    for i in range(7):
        rows = {tuple(r) for r in pc[i].numpy().tolist()}
        got = [tuple(r) for r in a[i].numpy().tolist()]
        assert len(got) == 524 and len(set(got)) == len(got) and set(got) <= rows


def test_dup_fill_matches_reference(net, g):
    paths = set()
    for i in range(int(g["n_clouds"])):
        pc = torch.from_numpy(g["pc_%d" % i])[None]
        keep = torch.from_numpy(g["sor_mask_%d" % i])[None]
        x, n = net.process_data(pc, keep, draws=torch.from_numpy(g["fill_draws"][i:i + 1]))
        assert int(n[0]) == int(g["n_kept"][i])
        assert np.array_equal(x.cpu().numpy()[0], g["filled"][i]), "cloud %d (N = %d)" % (i, int(n[0]))
        assert torch.equal(net.sor_mask(pc).cpu(), keep)            # ifd_sor gives the reference's SOR
        paths.add((int(n[0]) > 1024) - (int(n[0]) < 1024))
    assert paths == {-1, 0, 1}


def test_fps_indices_identical_to_reference(gpu_golden, g):
    _, aux = gpu_golden
    assert np.array_equal(aux["fps_idx"].numpy(), g["fps_idx"])


def test_ball_query_and_knn_match_oracle(gpu_golden, g):
    import punet_oracle as PO
    _, aux = gpu_golden
    W = PO.to_torch(PO.load_weights())
    _, rec = PO.forward(W, torch.from_numpy(g["filled"]), fps_idx=aux["fps_idx"])
    bd = (rec["ball_idx"] != aux["ball_idx"]).any(-1)
    kd = (rec["knn_idx"] != aux["knn_idx"]).any(-1)
    print("ball-query rows differing: %d of %d; 3-NN rows differing: %d of %d" % (int(bd.sum()), bd.numel(), int(kd.sum()), kd.numel()))
    assert int(bd.sum()) <= 0.01 * bd.numel() and int(kd.sum()) <= 0.01 * kd.numel()


def test_arithmetic_against_float64_with_gpu_decisions(gpu_golden, g):
    import punet_oracle as PO
    out, aux = gpu_golden
    sd = PO.load_weights()
    x = torch.from_numpy(g["filled"][:6])
    dec = {k: v[:6] for k, v in aux.items()}
    ref64, _ = PO.forward(PO.to_torch(sd, torch.float64), x, dtype=torch.float64, **dec)
    ref32, _ = PO.forward(PO.to_torch(sd), x, **dec)
    e_gpu = float((out[:6].double() - ref64).abs().max())
    e_32 = float((ref32.double() - ref64).abs().max())
    print("max |GPU - f64| %.3e, max |f32 oracle - f64| %.3e" % (e_gpu, e_32))
    assert e_gpu <= 4 * e_32


def test_end_to_end_against_reference(gpu_golden, g):
    out, _ = gpu_golden
    d = np.abs(out.numpy() - g["out"])
    print("|GPU - reference|: max %.3e, median %.3e" % (d.max(), np.median(d)))
    assert np.isfinite(out.numpy()).all()
    assert d.max() <= 1e-5


def test_cli_on_small_file(tmp_path, g, net):
    from ifdefense_amd import defend_npz as D
    import punet_oracle as PO
    pcs = np.stack([g["pc_%d" % i] for i in range(8)])
    data = tmp_path / "adv.npz"
    np.savez(str(data), test_pc=pcs, test_label=np.arange(8), target_label=np.arange(8) + 1)
    wp = tmp_path / "pu.npz"
    np.savez(str(wp), **PO.load_weights())
    assert D.main(["--data_root", str(data), "--pu_weight", str(wp)]) == 0
    srs = np.load(str(tmp_path / "srs" / "srs_adv.npz"))
    assert srs["test_pc"].shape == (8, 524, 3) and srs["test_label"].dtype == np.uint8
    sor = np.load(str(tmp_path / "sor" / "sor_adv.npz"), allow_pickle=True)["test_pc"]
    n = net.sor_mask(torch.from_numpy(pcs)).sum(1).cpu().numpy()
    assert [len(c) for c in sor] == list(n)
    dup = np.load(str(tmp_path / "dup" / "dup_adv.npz"))["test_pc"]
    assert dup.shape == (8, 4096, 3) and dup.dtype == np.float32 and np.isfinite(dup).all()


def test_batch_invariance_and_full_file(net):
    import bench
    x = torch.from_numpy(bench.synth_clouds(300, seed=11))
    big = net.pu_net(x, cloud_index_base=0).cpu()
    one = net.pu_net(x[123:124], cloud_index_base=123).cpu()
    assert torch.equal(big[123:124], one)
    f = torch.from_numpy(bench.synth_clouds(2468, seed=12))
    a = net.pu_net(f).cpu()
    b = net.pu_net(f).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)
