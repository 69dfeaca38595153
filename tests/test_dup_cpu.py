"""CPU checks of the baseline defenses (include/ifd_dup.h): the C ABI and its binding, the PU-Net weight order, the oracle
pinned to the reference's recorded outputs, and the host logic of the defend_npz CLI."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ifd_dup.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dup_golden.npz")
GOLDEN_OUT = os.path.join(ROOT, "tests", "golden", "dup_golden_out.npz")


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


def test_dup_header_symbols_exported_and_bound(lib):
    from ifdefense_amd import _lib
    import ifdefense_amd as I
    names = declared_symbols()
    assert names == sorted(_lib.DUP_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", I.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(names) <= exported


def test_dup_abi_version_and_weight_count(lib):
    from ifdefense_amd import weights
    assert lib.ifd_dup_abi_version() == 1
    assert lib.ifd_punet_weight_count() == 814307
    assert sum(int(np.prod(s)) for _, s in weights.punet_canonical_keys()) == 814307


def test_pack_punet_follows_state_dict_order():
    import punet_oracle as PO
    from ifdefense_amd import weights
    sd = PO.load_weights()
    keys = weights.punet_canonical_keys()
    assert [k for k, _ in keys] == list(sd.keys())
    w = weights.pack_state_dict(sd, "punet")
    assert w.size == 814307 and w.dtype == np.float32
    first = sd["SA_modules.0.mlps.0.layer0.conv.weight"].reshape(-1)
    assert np.array_equal(w[:first.size], first)
    last = sd["pcd_layer.1.layer0.conv.bias"]
    assert np.array_equal(w[-3:], last)
    assert np.array_equal(w[-3 - 192:-3], sd["pcd_layer.1.layer0.conv.weight"].reshape(-1))
    bad = dict(sd)
    del bad["FC_Modules.2.layer1.conv.bias"]
    with pytest.raises(KeyError):
        weights.pack_state_dict(bad, "punet")
    bad = dict(sd)
    bad["FP_Modules.0.mlp.layer0.conv.weight"] = np.zeros((64, 127, 1, 1), np.float32)
    with pytest.raises(ValueError):
        weights.pack_state_dict(bad, "punet")


def test_load_checkpoint_punet_npz(tmp_path):
    import punet_oracle as PO
    from ifdefense_amd import weights
    sd = PO.load_weights()
    p = str(tmp_path / "pu.npz")
    np.savez(p, **sd)
    a = weights.load_checkpoint(p, "punet")
    q = str(tmp_path / "pu.pth")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, q)
    assert np.array_equal(a, weights.load_checkpoint(q, "punet"))


def test_dup_create_rejects_bad_arguments(lib):
    lib.ifd_dup_create.restype = ctypes.c_void_p
    w = np.zeros(10, np.float32)
    assert not lib.ifd_dup_create(w.ctypes.data, 10, 0)               # wrong count: fails before any HIP call
    assert b"814307" in lib.ifd_last_error(None)
    assert not lib.ifd_dup_create(None, 5, 0)


def test_oracle_reproduces_the_reference():
    """punet_oracle in float32 with the reference's distance form and draws == the recorded reference run."""
    import punet_oracle as PO
    g = dict(np.load(GOLDEN), out=np.load(GOLDEN_OUT)["out"])
    W = PO.to_torch(PO.load_weights())
    out, rec = PO.forward(W, torch.from_numpy(g["filled"]), torch.from_numpy(g["fps_start"]))
    assert np.array_equal(rec["fps_idx"].numpy(), g["fps_idx"])
    d = np.abs(out.numpy() - g["out"])
    print("oracle vs reference: max |diff| %.3e, exact %s" % (d.max(), bool((d == 0).all())))
    assert d.max() <= 1e-6


# ---------------------------------------------------------------------------------------------- CLI host logic
class FakeDefender:
    """Stands in for runtime.DupNet: SRS keeps the first K - drop rows, SOR drops every 3rd row of odd clouds."""

    def srs(self, pc, drop_num, cloud_index_base=0):
        return pc[:, :pc.shape[1] - drop_num]

    def sor(self, pc, k, alpha):
        return [pc[i] if i % 2 == 0 else pc[i][torch.arange(pc.shape[1]) % 3 != 0] for i in range(pc.shape[0])]

    def dup(self, pc, k, alpha, cloud_index_base=0):
        return pc.repeat(1, 4, 1)


def _write_npz(path, B=3, K=12):
    rng = np.random.default_rng(0)
    np.savez(path, test_pc=rng.standard_normal((B, K, 6)).astype(np.float32),
             test_label=np.arange(B, dtype=np.int64), target_label=np.arange(B, dtype=np.int64) + 1)


def test_cli_save_names_and_defense_list(tmp_path):
    from ifdefense_amd import defend_npz as D
    assert D.defense_list('') == ['srs', 'sor', 'dup']
    assert D.defense_list('sor') == ['sor']
    assert D.save_path('/a/b/adv.npz', 'srs') == '/a/b/srs/srs_adv.npz'
    d = tmp_path / "data"
    d.mkdir()
    _write_npz(str(d / "x.npz"))
    _write_npz(str(d / "y.npz"))
    (d / "sub").mkdir()
    assert sorted(os.path.basename(f) for f in D.input_files(str(d))) == ["x.npz", "y.npz"]


def test_cli_runs_all_defenses_with_fake_defender(tmp_path, monkeypatch):
    from ifdefense_amd import defend_npz as D, weights
    monkeypatch.setattr(weights, "load_checkpoint", lambda p, m: np.zeros(1, np.float32))
    d = tmp_path / "data"
    d.mkdir()
    _write_npz(str(d / "x.npz"))
    assert D.main(["--data_root", str(d), "--pu_weight", "w.pth", "--srs_drop_num", "4"],
                  make_defender=lambda w: FakeDefender()) == 0
    srs = np.load(str(d / "srs" / "srs_x.npz"))
    assert srs["test_pc"].shape == (3, 8, 3) and srs["test_pc"].dtype == np.float32
    assert srs["test_label"].dtype == np.uint8 and srs["target_label"].dtype == np.uint8
    sor = np.load(str(d / "sor" / "sor_x.npz"), allow_pickle=True)
    assert sor["test_pc"].dtype == object and [c.shape for c in sor["test_pc"]] == [(12, 3), (8, 3), (12, 3)]
    dup = np.load(str(d / "dup" / "dup_x.npz"))
    assert dup["test_pc"].shape == (3, 48, 3)
    assert list(dup["target_label"]) == [1, 2, 3]


def test_cli_dup_without_weights_fails_before_the_gpu(tmp_path, capsys):
    from ifdefense_amd import defend_npz as D

    def never(w):
        raise AssertionError("the defender must not be made")
    assert D.main(["--data_root", str(tmp_path / "x.npz")], make_defender=never) != 0
    assert "--pu_weight" in capsys.readouterr().err
    assert D.main(["--data_root", str(tmp_path / "x.npz"), "--defense", "dup"], make_defender=never) != 0


def test_assemble_test_pc_ragged_and_regular(tmp_path):
    from ifdefense_amd import defend_npz as D
    reg = D.assemble_test_pc([np.ones((5, 3)), np.zeros((5, 3))])
    assert reg.shape == (2, 5, 3) and reg.dtype == np.float32
    rag = D.assemble_test_pc([np.ones((5, 3)), np.zeros((4, 3))])
    assert rag.shape == (2,) and rag.dtype == object
    p = str(tmp_path / "r.npz")
    np.savez(p, test_pc=rag)
    back = np.load(p, allow_pickle=True)["test_pc"]
    assert back[0].shape == (5, 3) and back[1].shape == (4, 3) and back[1].dtype == np.float32


# ---------------------------------------------------------------------------------------------- dense seeded weights
def _golden_cloud(i):
    g = np.load(GOLDEN)
    return torch.from_numpy(g["filled"][i:i + 1]), torch.from_numpy(g["fps_start"][i:i + 1])


def _input_activity(act, name):
    """Largest value of each input channel of layer `name` (reference column order) from forward()'s act_max: a channel
    that is 0 everywhere multiplies whatever column it meets by 0.  Coordinates count as live."""
    live = torch.ones(3, dtype=torch.float64)
    sa = re.match(r"SA_modules\.(\d)\.mlps\.0\.layer(\d)", name)
    fc = re.match(r"FC_Modules\.(\d)\.layer(\d)", name)
    if sa:
        v, j = int(sa.group(1)), int(sa.group(2))
        if j > 0:
            return act["SA_modules.%d.mlps.0.layer%d" % (v, j - 1)]
        return live if v == 0 else torch.cat([live, act["SA_modules.%d.mlps.0.layer2" % (v - 1)]])
    if name.startswith("FP_Modules"):
        return act["SA_modules.%d.mlps.0.layer2" % (int(name[11]) + 1)]
    if fc and fc.group(2) == "0":
        return torch.cat([live, act["SA_modules.0.mlps.0.layer2"]] + [act["FP_Modules.%d.mlp.layer0" % f] for f in range(3)])
    if fc:
        return act["FC_Modules.%s.layer0" % fc.group(1)]
    if name == "pcd_layer.0.layer0":
        return torch.stack([act["FC_Modules.%d.layer1" % k] for k in range(4)]).amax(0)
    return act["pcd_layer.0.layer0"]


def _first_two(candidates, live):
    """The first two of `candidates` (all indices if fewer than two are given) that are live."""
    cand = list(candidates) if len(candidates) >= 2 else list(range(len(live)))
    pick = [int(c) for c in cand if float(live[c]) > 0][:2]
    assert len(pick) == 2
    return pick


def test_make_weights_names_shapes_and_density():
    import punet_oracle as PO
    ship, a, b = PO.load_weights(), PO.make_weights(1), PO.make_weights(1)
    assert list(a) == list(ship) and all(a[k].shape == ship[k].shape and a[k].dtype == np.float32 for k in ship)
    assert all(np.array_equal(a[k], b[k]) for k in a) and not np.array_equal(a["pcd_layer.1.layer0.conv.weight"],
                                                                            PO.make_weights(2)["pcd_layer.1.layer0.conv.weight"])
    dead = {k[:-12]: tuple(len(d) for d in PO.dead_channels(w)) for k, w in ship.items() if k.endswith(".weight")}
    # the figures that motivate make_weights: (dead output rows, dead input columns) of the shipped checkpoint
    assert dead["SA_modules.3.mlps.0.layer2"][0] == 165 and dead["SA_modules.3.mlps.0.layer0"][1] == 151
    assert dead["FP_Modules.2.mlp.layer0"][1] == 187
    for k, w in a.items():
        if k.endswith(".weight"):
            rows, cols = PO.dead_channels(w)
            assert rows.size == 0 and cols.size == 0
            assert np.abs(w).max() <= np.sqrt(6.0 / w.shape[1])
        else:
            assert np.abs(w).max() <= 0.1


def test_decisions_equal_forwards_record():
    import punet_oracle as PO
    x, st = _golden_cloud(13)
    _, rec = PO.forward(PO.to_torch(PO.make_weights(1)), x, st)
    dec = PO.decisions(x, st)
    assert all(torch.equal(dec[k], rec[k]) for k in ("fps_idx", "ball_idx", "knn_idx"))
    _, rec = PO.forward(PO.to_torch(PO.make_weights(1)), x, st, dist_dtype=torch.float32)     # float32 in float32: no change
    assert all(torch.equal(dec[k], rec[k]) for k in ("fps_idx", "ball_idx", "knn_idx"))
    assert rec["knn_w"].shape == (1, 3, 1024, 3) and [tuple(f.shape) for f in rec["l_feats"]] == [
        (1, 64, 1024), (1, 128, 512), (1, 256, 256), (1, 512, 128)] and all(u.shape == (1, 64, 1024) for u in rec["up"])
    assert torch.allclose(rec["knn_w"].sum(-1), torch.ones(1, 3, 1024), atol=1e-5)


def test_dense_weights_see_every_swap_the_checkpoint_cannot():
    """Swap two input columns, and separately two output rows, of each of the 25 conv weights in the float64 oracle on
    golden cloud 0 with the decisions held fixed.  With make_weights(1) every swap moves the output by at least 1000 x the
    float32 oracle's own error on that cloud; with the shipped checkpoint 45 of the 50 swaps move it by exactly 0 (a recorded fact
    about that fixture: it is not a dense test).

    The pairs are the first two channels the shipped checkpoint leaves dead (|w| < 1e-6) where it has two, else the first
    two of all, skipping channels that cannot show in any implementation: a ReLU unit that never fires on this cloud with
    the dense weights (uniform weights on non-negative inputs leave about a third of the units silent), for a row its own
    unit, for a column the unit feeding it.  Which units fire is read from the unswapped forward, not from the swaps."""
    import punet_oracle as PO
    x, st = _golden_cloud(0)
    dec = PO.decisions(x, st)
    dec = {k: dec[k] for k in ("fps_idx", "ball_idx", "knn_idx")}
    ship, dense = PO.load_weights(), PO.make_weights(1)

    def run(sd, dt=torch.float64):
        return PO.forward(PO.to_torch(sd, dt), x, dtype=dt, dist_dtype=torch.float32, **dec)

    base, rec = run(dense)
    e_32 = float((run(dense, torch.float32)[0].double() - base).abs().max())
    base_ship = run(ship)[0]
    act = rec["act_max"]
    act["pcd_layer.1.layer0"] = torch.ones(3, dtype=torch.float64)              # no ReLU: every output shows
    unseen, worst = 0, np.inf
    for name, _, _ in PO.LAYERS:
        key = name + ".conv.weight"
        rows, cols = PO.dead_channels(ship[key])
        for axis, pair in ((1, _first_two(cols, _input_activity(act, name))), (0, _first_two(rows, act[name]))):
            moved = []
            for sd, ref in ((dense, base), (ship, base_ship)):
                w = sd[key].copy()
                sw = [slice(None)] * 4
                sw[axis] = pair
                rv = list(sw)
                rv[axis] = pair[::-1]
                w[tuple(sw)] = sd[key][tuple(rv)]
                moved.append(float((run(dict(sd, **{key: w}))[0] - ref).abs().max()))
            print("%-28s %s %3d <-> %3d: dense moves %.3e (%.0f x e_32), shipped %.3e" % (
                name, "rows" if axis == 0 else "cols", pair[0], pair[1], moved[0], moved[0] / e_32, moved[1]))
            assert moved[0] >= 1000 * e_32, (name, axis, pair, moved[0], e_32)
            worst = min(worst, moved[0] / e_32)
            unseen += moved[1] == 0.0
    print("e_32 %.3e; smallest dense move %.0f x e_32; swaps the shipped checkpoint does not see: %d of 50" % (e_32, worst, unseen))
    assert unseen == 45


def test_float32_distances_level_the_float64_bar():
    """e_32 = max |f32 oracle - f64 oracle| with the decisions fixed.  With float64 distances it is ten times larger on
    the duplicate-heavy golden clouds (the 3-NN weights at coinciding points see the expanded form's float32 noise in one run
    only); with dist_dtype=float32 on both sides clouds 7 and 13 come within 2 x of clouds 0-5."""
    import punet_oracle as PO
    sd = PO.load_weights()
    g = np.load(GOLDEN)

    def e32(sel, dd):
        x, st = torch.from_numpy(g["filled"][sel]), torch.from_numpy(g["fps_start"][sel])
        dec = PO.decisions(x, st)
        dec = {k: dec[k] for k in ("fps_idx", "ball_idx", "knn_idx")}
        r64, _ = PO.forward(PO.to_torch(sd, torch.float64), x, dtype=torch.float64, dist_dtype=dd, **dec)
        r32, _ = PO.forward(PO.to_torch(sd), x, dist_dtype=dd, **dec)
        return float((r32.double() - r64).abs().max())

    level = e32(list(range(6)), torch.float32)
    hard = {i: (e32([i], None), e32([i], torch.float32)) for i in (7, 13)}
    print("e_32 clouds 0-5 (f32 distances) %.3e; cloud 7 %.3e -> %.3e; cloud 13 %.3e -> %.3e" % (
        level, hard[7][0], hard[7][1], hard[13][0], hard[13][1]))
    assert hard[13][0] > 5 * level                       # the inflation the float64 distances cause
    for i in (7, 13):
        assert hard[i][1] <= 2 * level and hard[i][1] >= level / 2


def test_attribution_rules_accept_ties_and_reject_wrong_rows():
    import punet_oracle as PO
    d = np.full(100, 1.0)
    d[[3, 10, 40, 70]] = [0.1, 0.2499, 0.2501, 0.1]
    r2, band = 0.25, 1e-3
    pad = lambda m: m + [m[0]] * (32 - len(m))
    assert PO.ball_row_allowed(pad([3, 10, 40, 70]), d, r2, band)
    assert PO.ball_row_allowed(pad([3, 70]), d, r2, band)               # both near-radius points may fall out
    assert PO.ball_row_allowed(pad([3, 10, 70]), d, r2, band)
    assert not PO.ball_row_allowed(pad([3, 10, 40]), d, r2, band)       # 70 is surely inside
    assert not PO.ball_row_allowed(pad([3, 5, 70]), d, r2, band)        # 5 is surely outside
    assert not PO.ball_row_allowed([3, 70] + [70] * 30, d, r2, band)    # filled with the last member, not the first
    assert not PO.ball_row_allowed(pad([70, 3]), d, r2, band)           # not in index order
    assert not PO.ball_row_allowed(pad([3, 10, 40, 70]), d, r2, 1e-5)   # 40 is outside once the band excludes it
    full = np.zeros(100)
    assert PO.ball_row_allowed(list(range(32)), full, r2, band) and not PO.ball_row_allowed(list(range(1, 33)), full, r2, band)
    k = np.array([5.0, 1.0, 1.0 + 1e-4, 2.0, 3.0])
    assert PO.knn_row_allowed([1, 2, 3], k, 1e-3) and PO.knn_row_allowed([2, 1, 3], k, 1e-3)
    assert not PO.knn_row_allowed([2, 1, 3], k, 1e-5) and not PO.knn_row_allowed([1, 2, 4], k, 1e-3)
    assert not PO.knn_row_allowed([1, 1, 2], k, 1e-3) and not PO.knn_row_allowed([1, 3, 2], k, 1e-3)
