#!/usr/bin/env python
"""Generate tests/golden/pointconv_golden.npz by running the REFERENCE's PointConv victim (baselines/model/pointconv.py
PointConvDensityClsSsg(num_classes=40), eval mode) on CPU with the seeded weights of tests/pointconv_oracle.py (no victim
checkpoint ships).

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its module is imported where it lies (by file path), the oracle's weights go in through load_state_dict in
the checkpoint's own form (nn.DataParallel keys), and inputs and outputs are saved as data.  The reference draws the first pick
of either farthest point sampling with torch.randint; for the duration of a run the imported module sees a ``torch`` whose
``randint`` hands out the recorded starts, nothing else changed.

Clouds (8): bench.synth_clouds(8, seed=611) cut to 32, 100, 600, 600, 1024, 1024, 1024 and 1024 points.  Recorded: the clouds,
the weight seed, the starts, both FPS index lists and both kNN tables (int16) as the reference's farthest_point_sample and
knn_point returned them (topk(sorted=False): a row's order is torch's), the three DensityNet outputs, the float32 logits and the
float32 global feature.

    python tests/golden/make_golden_pointconv.py
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
SIZES = (32, 100, 600, 600, 1024, 1024, 1024, 1024)
STARTS = ((31, 7), (99, 511), (17, 300), (599, 1), (1023, 128), (512, 77), (3, 400), (700, 255))


class _PinnedTorch:
    """``torch`` with ``randint`` handing out queued values; every other attribute is torch's own."""

    def __init__(self):
        self.queue = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def randint(self, low, high, size, **kw):
        v = self.queue.pop(0)
        assert low <= v < high and tuple(size) == (1,), (low, v, high, size)
        return torch.full(tuple(size), v, dtype=kw.get("dtype", torch.long))


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, sd, pcs):
    """-> (logits, global feature, [fps1, fps2], [knn1, knn2], [dens1, dens2, dens3]) of every cloud, each a batch of its own."""
    model = torch.nn.DataParallel(ref.PointConvDensityClsSsg(num_classes=40))
    model.load_state_dict(sd)
    net = model.module.eval()
    seen = {}
    net.fc1.register_forward_hook(lambda m, inp, out: seen.__setitem__("g", inp[0]))
    got_d = []
    for sa in (net.sa1, net.sa2, net.sa3):
        sa.densitynet.register_forward_hook(lambda m, inp, out: got_d.append(out[0, 0].numpy().copy()))
    fps, knn = ref.farthest_point_sample, ref.knn_point
    got_f, got_k = [], []

    def recording_fps(xyz, npoint):
        idx = fps(xyz, npoint)
        got_f.append(idx[0].numpy().astype(np.int16))
        return idx

    def recording_knn(nsample, xyz, new_xyz):
        idx = knn(nsample, xyz, new_xyz)
        got_k.append(idx[0].numpy().astype(np.int16))
        return idx

    ref.farthest_point_sample, ref.knn_point = recording_fps, recording_knn
    lo, gf, fi, ki, di = [], [], [], [], []
    try:
        with torch.no_grad():
            for c, st in zip(pcs, STARTS):
                del got_f[:], got_k[:], got_d[:]
                ref.torch.queue[:] = list(st)
                x = torch.from_numpy(c)[None].transpose(1, 2).contiguous()
                lo.append(net(x)[0].numpy())
                gf.append(seen["g"][0].numpy())
                assert len(got_f) == 2 and len(got_k) == 2 and len(got_d) == 3 and not ref.torch.queue
                fi.append(list(got_f))
                ki.append(list(got_k))
                di.append(list(got_d))
    finally:
        ref.farthest_point_sample, ref.knn_point = fps, knn
    return np.stack(lo), np.stack(gf), fi, ki, di


def main():
    import bench
    import pointconv_oracle as PO
    ref = by_path("ref_pointconv", os.path.join(REF, "model", "pointconv.py"))
    ref.torch = _PinnedTorch()
    s = bench.synth_clouds(8, seed=611)
    pcs = [np.ascontiguousarray(s[i][:n], dtype=np.float32) for i, n in enumerate(SIZES)]
    sd = PO.reference_state_dict(PO.make_weights(SEED))
    lo, gf, fi, ki, di = run(ref, sd, pcs)
    rec = {"n_clouds": np.int32(len(pcs)), "weight_seed": np.int32(SEED), "starts": np.asarray(STARTS, np.int32), "logits": lo,
           "global_feat": gf}
    for i, c in enumerate(pcs):
        rec["pc_%d" % i] = c
        rec["fps1_%d" % i], rec["fps2_%d" % i] = fi[i]
        rec["knn1_%d" % i], rec["knn2_%d" % i] = ki[i]
        rec["dens1_%d" % i], rec["dens2_%d" % i], rec["dens3_%d" % i] = di[i]
    print("|logits| max %.3f, |global_feat| max %.3f" % (np.abs(lo).max(), np.abs(gf).max()))
    path = os.path.join(HERE, "pointconv_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
