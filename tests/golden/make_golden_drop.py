#!/usr/bin/env python
"""Generate tests/golden/drop_golden.npz by running the REFERENCE's SaliencyDrop (baselines/attack/Saliency/Drop.py) on the CPU, on
the reference's PointNetCls (k=40, no feature_transform, eval mode) loaded with pointnet_oracle.make_calibrated_weights(0, False).

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its modules are imported where they lie (by file path), and inputs and outputs are saved as data.  Shims: a
no-op ``Tensor.cuda`` / ``Module.cuda``.

Run: SaliencyDrop(net, num_drop=23, alpha=1, k=5).attack - 5 rounds of 5, 5, 5, 5, 3; the reference cannot run fewer than 5 (it
divides by num_rounds // 5) - on 4 clouds of 64 points (bench.synth_clouds(4, seed=SEED_CLOUDS)[:, :64], normalised to the unit
sphere), labels = the float64 predictions.  The script asserts what the fixture's users rely on: at least 3 of the 4 clouds are
clear in every round (drop_oracle.round_margin on the float64 oracle's free run), so that their surviving row SETS do not hang on
float32 rounding or on torch.topk's order among equals.

    python tests/golden/make_golden_drop.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(os.environ.get("IFD_REFERENCE_ROOT", "/root/reference"), "baselines")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED_CLOUDS = int(os.environ.get("DROP_GOLDEN_SEED", "417"))
B, K, NUM_DROP, K_ROUND, ALPHA = 4, 64, 23, 5, 1


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(write=True):
    import bench
    import drop_oracle as DO
    import pointnet_oracle as PO
    from ifdefense_amd.inference import normalize_points_np
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    ref_net = by_path("ref_pointnet", os.path.join(REF, "model", "pointnet.py"))
    ref_drop = by_path("ref_drop", os.path.join(REF, "attack", "Saliency", "Drop.py"))

    sd = PO.make_calibrated_weights(0, False)
    model = torch.nn.DataParallel(ref_net.PointNetCls(k=40, feature_transform=False))
    model.load_state_dict(PO.reference_state_dict(sd))
    net = model.module.eval()
    data = np.stack([normalize_points_np(c[:K]) for c in bench.synth_clouds(B, seed=SEED_CLOUDS)]).astype(np.float32)
    W32, W64 = PO.to_torch(sd, torch.float32), PO.to_torch(sd, torch.float64)
    label = PO.forward(W64, data, dtype=torch.float64)[0].argmax(1).numpy().astype(np.int64)

    adv, success_num = ref_drop.SaliencyDrop(net, num_drop=NUM_DROP, alpha=ALPHA, k=K_ROUND).attack(torch.from_numpy(data),
                                                                                                    torch.from_numpy(label))
    assert adv.shape == (B, K - NUM_DROP, 3) and adv.dtype == np.float32

    runs = [DO.attack(W64, c, t, NUM_DROP, K_ROUND, ALPHA, 1. / B, torch.float64, W_other=W32) for c, t in zip(data, label)]
    clear = np.array([all(r["clear"] for r in run["rounds"]) for run in runs])
    for b, run in enumerate(runs):
        print("cloud %d: label %d, smallest gap / e_sal %.1f, all clear %s" % (
            b, label[b], min(r["gap"] / r["e_sal"] for r in run["rounds"]), clear[b]))
    assert [r["k"] for r in runs[0]["rounds"]] == [5, 5, 5, 5, 3]
    assert clear.sum() >= 3, "fewer than 3 of the 4 clouds are clear in every round: use another seed"
    rec = {"data": data, "label": label, "num_drop": np.int32(NUM_DROP), "k": np.int32(K_ROUND), "alpha": np.float64(ALPHA),
           "adv": adv, "success_num": np.int64(success_num), "all_clear": clear, "seed_clouds": np.int64(SEED_CLOUDS)}
    if write:
        path = os.path.join(HERE, "drop_golden.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")
    return rec


if __name__ == "__main__":
    main()
