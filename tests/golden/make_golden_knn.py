#!/usr/bin/env python
"""Generate tests/golden/knn_golden.npz by running the REFERENCE's CWKNN (baselines/attack/CW/kNN.py) with its
ChamferkNNDist('adv2ori', 5, 1.05, 5., 3.), ProjectInnerClipLinf(0.1) and LogitsAdvLoss(kappa) on the CPU, on the reference's
PointNetCls (k=40, no feature_transform, eval mode) loaded with pointnet_oracle.make_calibrated_weights(0, False).

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its modules are imported where they lie (by file path; the real util/set_distance.py too, as the ``util``
package dist_utils.py imports from) and inputs and outputs are saved as data.  Shims: a no-op ``Tensor.cuda`` / ``Module.cuda``, and
a wrapper around ``torch.randn`` that keeps the draw, which is how the start noise is captured (one [B,3,K] draw, recorded * 1e-7
and transposed to [B,K,3]).  The installed torch still accepts the reference's ``torch.cross(vng, normal)`` without ``dim`` (a
deprecation warning; with 4 clouds the first axis of size 3 is the coordinate axis), so that call is NOT shimmed.

Run: 4 clouds of 32 points with 6 channels - bench.synth_clouds(4, seed=SEED_CLOUDS)[:, :32] normalised to the unit sphere, and unit
normals made from the radial direction plus noise - 25 iterations, torch.manual_seed(SEED).  attack_lr is 0.01, not the script's
1e-3: 25 steps of 1e-3 cannot carry a point to the 0.1 budget, ten sign-like Adam steps of 0.01 can, so the run exercises the clip
as well as the projection.  Targets: (prediction + SHIFT[b]) % 40, kappa KAPPA, chosen so that at least one cloud reaches its target
and at least one does not.  The script asserts both, and - by replaying the float64 test oracle on the recorded inputs - that some
rows are projected during the run and some end on the budget.

    python tests/golden/make_golden_knn.py
"""
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(os.environ.get("IFD_REFERENCE_ROOT", "/root/reference"), "baselines")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = int(os.environ.get("KNN_GOLDEN_SEED", "7"))
SEED_CLOUDS = int(os.environ.get("KNN_GOLDEN_CLOUDS", "313"))
SHIFT = [int(x) for x in os.environ.get("KNN_GOLDEN_SHIFT", "1,1,1,1").split(",")]
KAPPA = float(os.environ.get("KNN_GOLDEN_KAPPA", "0"))
B, K, NUM_ITER, LR = 4, 32, 25, 1e-2


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def make_data():
    import bench
    pts = np.ascontiguousarray(bench.synth_clouds(B, seed=SEED_CLOUDS)[:, :K], dtype=np.float32)
    pts = pts - pts.mean(1, keepdims=True)
    pts = (pts / np.sqrt((pts ** 2).sum(-1)).max(1)[:, None, None]).astype(np.float32)
    rng = np.random.default_rng(SEED_CLOUDS)
    nrm = pts + 0.3 * rng.standard_normal(pts.shape)
    nrm = (nrm / np.sqrt((nrm ** 2).sum(-1, keepdims=True))).astype(np.float32)
    return np.concatenate([pts, nrm], axis=2)


def main(write=True):
    import pointnet_oracle as PO
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    util = types.ModuleType("util")
    util.__path__ = []
    sys.modules["util"] = util
    util.set_distance = by_path("util.set_distance", os.path.join(REF, "util", "set_distance.py"))
    ref_net = by_path("ref_pointnet", os.path.join(REF, "model", "pointnet.py"))
    ref_knn = by_path("ref_knn", os.path.join(REF, "attack", "CW", "kNN.py"))
    ref_adv = by_path("ref_adv_utils", os.path.join(REF, "attack", "util", "adv_utils.py"))
    ref_dist = by_path("ref_dist_utils", os.path.join(REF, "attack", "util", "dist_utils.py"))
    ref_clip = by_path("ref_clip_utils", os.path.join(REF, "attack", "util", "clip_utils.py"))

    sd = PO.make_calibrated_weights(0, False)
    model = torch.nn.DataParallel(ref_net.PointNetCls(k=40, feature_transform=False))
    model.load_state_dict(PO.reference_state_dict(sd))
    net = model.module.eval()
    data = make_data()
    with torch.no_grad():
        pred = net(torch.from_numpy(data[:, :, :3]).transpose(1, 2).contiguous())[0].argmax(1).numpy()
    target = (pred + np.array(SHIFT)) % 40

    draws, randn = [], torch.randn

    def keeping(*a, **k):
        r = randn(*a, **k)
        draws.append(r.clone())
        return r

    attacker = ref_knn.CWKNN(net, ref_adv.LogitsAdvLoss(kappa=KAPPA), ref_dist.ChamferkNNDist('adv2ori', 5, 1.05, 5., 3.),
                             ref_clip.ProjectInnerClipLinf(budget=0.1), attack_lr=LR, num_iter=NUM_ITER)
    torch.manual_seed(SEED)
    torch.randn = keeping
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            adv, success_num = attacker.attack(torch.from_numpy(data), torch.from_numpy(target))
    finally:
        torch.randn = randn
    assert len(draws) == 1 and tuple(draws[0].shape) == (B, 3, K)
    noise = (draws[0] * 1e-7).numpy().transpose(0, 2, 1).astype(np.float32)
    with torch.no_grad():
        final = net(torch.from_numpy(np.asarray(adv, np.float32)).transpose(1, 2).contiguous())[0].argmax(1).numpy()
    print("predictions %s, targets %s, final %s, success_num %d" % (pred.tolist(), target.tolist(), final.tolist(), success_num))
    assert 1 <= success_num <= B - 1, "every cloud or no cloud reaches its target: use another kappa or other targets"
    disp = np.sqrt(((np.asarray(adv, np.float64) - data[:, :, :3]) ** 2).sum(-1))
    on_budget = int((disp >= 0.1 * (1 - 1e-5)).sum())
    # which rows are projected: the float64 test oracle, free-running on the recorded inputs
    import atk_oracle as AO
    import knn_oracle as KO
    W64 = PO.to_torch(sd, torch.float64)
    projected = 0
    for b in range(B):
        ori, nrm = data[b, :, :3].astype(np.float64), data[b, :, 3:].astype(np.float64)
        a, m, v = ori + noise[b], np.zeros_like(ori), np.zeros_like(ori)
        for it in range(NUM_ITER):
            r = AO.run_cloud(W64, a, int(target[b]), "logits", KAPPA, 1.0 / B)
            s = KO.step(r["grad"], a, ori, nrm, m, v, it + 1, LR, 1.0 / B)
            a, m, v = s["adv"], s["m"], s["v"]
            projected += int((s["dn"] < 0).sum())
    print("rows on the budget at the end: %d of %d; rows projected over the run (float64 oracle): %d of %d"
          % (on_budget, B * K, projected, B * K * NUM_ITER))
    assert on_budget > 0 and projected > 0 and on_budget < B * K
    rec = {"data": data, "target": target.astype(np.int64), "noise": noise, "adv": np.asarray(adv, np.float64),
           "success_num": np.int64(success_num), "final_pred": final.astype(np.int64), "num_iter": np.int32(NUM_ITER),
           "attack_lr": np.float64(LR), "kappa": np.float64(KAPPA), "chamfer_weight": np.float64(5.), "knn_weight": np.float64(3.),
           "alpha": np.float64(1.05), "budget": np.float64(0.1), "seed": np.int64(SEED), "on_budget": np.int64(on_budget),
           "projected": np.int64(projected)}
    if write:
        path = os.path.join(HERE, "knn_golden.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")
    return rec


if __name__ == "__main__":
    main()
