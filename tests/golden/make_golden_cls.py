#!/usr/bin/env python
"""Generate tests/golden/cls_golden.npz by running the REFERENCE's PointNet victim (baselines/model/pointnet.py PointNetCls,
k=40, use_bn, eval mode) on CPU with the seeded weights of tests/pointnet_oracle.py (no victim checkpoint ships).

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its modules are imported where they lie (by file path), the oracle's weights go in through
load_state_dict in the checkpoint's own form (nn.DataParallel keys), and inputs and outputs are saved as data.

Clouds (16; every cloud is one reference batch, so ragged sizes need nothing special):
  0-2    baselines/data/airplane.npy, its first 1024 points: as it is, rotated 40 deg about z, rotated 75 deg about (1, 1, 0)
  3-6    bench.synth_clouds, 1024 points
  7      824 points (a drop attack's size)
  8      1120 points (add-cluster: 3 clusters of 32)
  9      1536 points (add: 512 more)
  10     4096 points (DUP-Net's output size)
  11-12  ragged SOR outputs: clouds 4 and 8 of tests/golden/dup_golden.npz under the reference's recorded SOR masks
  13     600 points
  14     65 points
  15     1 point
Recorded for feature_transform False (suffix _f) and True (suffix _t): float32 logits / trans / global feature (/ trans_feat),
float64 logits; and the reference's normalize_points_np of clouds 3 and 11.

    python tests/golden/make_golden_cls.py
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
SEED = 0


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a /= np.linalg.norm(a)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def clouds():
    import bench
    rng = np.random.default_rng(20261017)
    air = np.load(os.path.join(REF, "data", "airplane.npy"))[:1024, :3].astype(np.float64)
    out = [air, air @ rot((0, 0, 1), 40).T, air @ rot((1, 1, 0), 75).T]
    s = bench.synth_clouds(12, seed=501)
    out += [s[i] for i in range(4)]
    out.append(s[4][:824])
    centres = s[5][rng.choice(1024, 3)] * 1.2
    out.append(np.concatenate([s[5]] + [c + rng.normal(0, 0.02, (32, 3)) for c in centres]))
    out.append(np.concatenate([s[6], s[6][rng.choice(1024, 512)] + rng.normal(0, 0.03, (512, 3))]))
    out.append(np.concatenate([s[7] + rng.normal(0, 0.004 * k, (1024, 3)) for k in range(4)]))
    d = np.load(os.path.join(HERE, "dup_golden.npz"))
    out += [d["pc_4"][d["sor_mask_4"].astype(bool)], d["pc_8"][d["sor_mask_8"].astype(bool)]]
    out += [s[8][:600], s[9][:65], s[10][:1]]
    return [np.ascontiguousarray(c, dtype=np.float32) for c in out]


def main():
    import pointnet_oracle as PO
    ref = by_path("ref_pointnet", os.path.join(REF, "model", "pointnet.py"))
    ref_utils = by_path("ref_pointnet_utils", os.path.join(REF, "util", "pointnet_utils.py"))
    pcs = clouds()
    rec = {"n_clouds": np.int32(len(pcs)), "weight_seed": np.int32(SEED)}
    for i, c in enumerate(pcs):
        rec["pc_%d" % i] = c
    for i in (3, 11):
        rec["normalized_%d" % i] = ref_utils.normalize_points_np(pcs[i])
    for ft, sfx in ((False, "_f"), (True, "_t")):
        sd = PO.reference_state_dict(PO.make_weights(SEED, ft))
        model = torch.nn.DataParallel(ref.PointNetCls(k=40, feature_transform=ft))
        model.load_state_dict(sd)
        net = model.module.eval()
        net64 = torch.nn.DataParallel(ref.PointNetCls(k=40, feature_transform=ft))
        net64.load_state_dict(sd)
        net64 = net64.module.double().eval()
        lo, tr, tf, gf, lo64 = [], [], [], [], []
        with torch.no_grad():
            for c in pcs:
                x = torch.from_numpy(c)[None].transpose(1, 2).contiguous()
                l, t, f = net(x)
                lo.append(l[0].numpy()); tr.append(t[0].numpy()); gf.append(net.feat(x)[0][0].numpy())
                if ft:
                    tf.append(f[0].numpy())
                lo64.append(net64(x.double())[0][0].numpy())
        lo, lo64 = np.stack(lo), np.stack(lo64)
        e32 = np.abs(lo.astype(np.float64) - lo64).max()
        top = np.sort(lo64, axis=1)
        margin = (top[:, -1] - top[:, -2]).min()
        print("feature_transform=%s: e_32 %.3e, |logits| max %.3f, smallest top-1/top-2 margin %.3e" % (ft, e32, np.abs(lo).max(), margin))
        assert margin > 1000 * e32, "margin too small for a prediction test: use another SEED"
        rec["logits" + sfx], rec["trans" + sfx], rec["global_feat" + sfx], rec["logits64" + sfx] = lo, np.stack(tr), np.stack(gf), lo64
        if ft:
            rec["trans_feat" + sfx] = np.stack(tf)
    path = os.path.join(HERE, "cls_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
