#!/usr/bin/env python
"""Throughput of the PointNet victim classifier (include/ifd_cls.h) on one MI355X: clouds/s of runtime.Classifier on a
2468 x 1024 bench.synth_clouds file (one call, as the inference CLI makes it) and at B = 512 (the reference's MAX_TEST_BATCH
for PointNet), each from warmed, synchronised, repeated runs (median of --reps); the fraction of the f32-MFMA roofline
(2 x 139,456 MAC per point and stack x 1024 points = 0.571 GFLOP per cloud without feature_transform, against 157.3
TFLOP/s: 275 k clouds/s); and, on the same GPU in the same process, the same clouds through tests/pointnet_oracle.py in
float32 on the GPU - torch ops in the reference's own structure, batch 512 - as the reference-style baseline.  The
per-kernel split comes from a rocprofv3 --kernel-trace --stats run of this script with --quick.

    python scripts/time_cls.py [--clouds 2468] [--reps 7] [--quick] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

PEAK_TFLOPS = 157.3
MAC_3D = 3 * 64 + 64 * 128 + 128 * 1024                      # STN3d and trunk, per point
MAC_KD = 64 * 64 + 64 * 128 + 128 * 1024                      # STNkd
REF_BATCH = 512                                                # baselines/config.py MAX_TEST_BATCH[1024]['pointnet']


def gflop_per_cloud(ft, n=1024):
    return 2.0 * n * (2 * MAC_3D + (MAC_KD + 64 * 64 if ft else 0)) * 1e-9


def timed(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=2468)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="one repetition, no torch baseline (for the rocprofv3 kernel split)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import bench
    import ifdefense_amd as I
    import pointnet_oracle as PO
    from ifdefense_amd import weights
    reps = 1 if a.quick else a.reps
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B = pc.shape[0]
    res = {"clouds": B, "points": int(pc.shape[1]), "reps": reps, "peak_tflops": PEAK_TFLOPS}
    for ft in (False, True):
        tag = "ft" if ft else "plain"
        sd = PO.make_weights(0, ft)
        with I.Classifier(weights.pack_state_dict(sd, "pointnet"), feature_transform=ft, device="cuda:0") as net:
            for name, x in (("file", pc), ("b%d" % REF_BATCH, pc[:REF_BATCH])):
                ms, ts = timed(lambda: net.logits(x), reps)
                cps = x.shape[0] / ms * 1e3
                frac = cps * gflop_per_cloud(ft) * 1e9 / (PEAK_TFLOPS * 1e12)
                res["%s_%s_ms" % (tag, name)], res["%s_%s_ms_all" % (tag, name)] = ms, ts
                res["%s_%s_clouds_per_s" % (tag, name)], res["%s_%s_roofline_fraction" % (tag, name)] = cps, frac
                print("%-5s %-5s %8.3f ms  %9.0f clouds/s  %5.1f %% of the f32-MFMA peak (%.3f GFLOP per cloud)"
                      % (tag, name, ms, cps, 100 * frac, gflop_per_cloud(ft)))
            if a.quick:
                continue
            W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}
            got = net.logits(pc[:REF_BATCH])
            ref = PO.forward(W, pc[:REF_BATCH])[0]
            res["%s_max_abs_diff_vs_torch" % tag] = float((got - ref).abs().max())
            for name, x in (("file", pc), ("b%d" % REF_BATCH, pc[:REF_BATCH])):
                def torch_run(x=x):
                    return [PO.forward(W, x[i:i + REF_BATCH])[0] for i in range(0, x.shape[0], REF_BATCH)]
                ms, ts = timed(torch_run, reps)
                cps = x.shape[0] / ms * 1e3
                res["%s_%s_torch_ms" % (tag, name)], res["%s_%s_torch_ms_all" % (tag, name)] = ms, ts
                res["%s_%s_torch_clouds_per_s" % (tag, name)] = cps
                res["%s_%s_speedup_vs_torch" % (tag, name)] = res["%s_%s_clouds_per_s" % (tag, name)] / cps
                print("%-5s %-5s torch oracle on the GPU (f32, batch %d): %8.3f ms  %9.0f clouds/s; the fused path is %.2fx"
                      % (tag, name, REF_BATCH, ms, cps, res["%s_%s_speedup_vs_torch" % (tag, name)]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
