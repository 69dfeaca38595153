#!/usr/bin/env python
"""Throughput of the baseline defenses (include/ifd_dup.h) on one MI355X: SRS, SOR and DUP-Net on a 2468 x 1024
bench.synth_clouds file, each from warmed, synchronised, repeated runs (median of --reps), plus the stage split of the
DUP path, the roofline fraction of the PU-Net's 4.98 GFLOP per cloud against the 157.3 TFLOP/s f32-MFMA peak, and the
same clouds through tests/punet_oracle.py in float32 on the GPU (torch ops, batch 128: the reference's own structure,
FPS as a Python loop) as the reference-style baseline.  The per-kernel split of the PU-Net forward (FPS, ball query,
SA1-SA4, 3-NN, head) comes from a rocprofv3 --kernel-trace --stats run of this script with --quick.

    python scripts/time_dup.py [--clouds 2468] [--reps 5] [--oracle-batches 4] [--quick] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

GFLOP_PER_CLOUD = 4.98
PEAK_TFLOPS = 157.3


def timed(fn, reps):
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--oracle-batches", type=int, default=4, help="batches of 128 clouds timed through the torch oracle")
    ap.add_argument("--quick", action="store_true", help="one repetition, no oracle (for the rocprofv3 kernel split)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import bench
    import ifdefense_amd as I
    import punet_oracle as PO
    from ifdefense_amd import weights
    reps = 1 if a.quick else a.reps
    net = I.DupNet(weights.pack_state_dict(PO.load_weights(), "punet"), device="cuda:0")
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B = pc.shape[0]
    res = {"clouds": B, "reps": reps}
    keep = net.sor_mask(pc)
    x, _ = net.process_data(pc, keep)
    stages = {"srs": lambda: net.srs(pc, 500), "sor": lambda: net.sor_mask(pc), "fill": lambda: net.process_data(pc, keep),
              "pu_net": lambda: net.pu_net(x), "dup": lambda: net.dup(pc)}
    for k, fn in stages.items():
        ms, ts = timed(fn, reps)
        res[k + "_ms"] = ms
        res[k + "_ms_all"] = ts
        print("%-7s %9.2f ms  %10.0f clouds/s" % (k, ms, B / ms * 1e3))
    res["srs_clouds_per_s"] = B / res["srs_ms"] * 1e3
    res["sor_clouds_per_s"] = B / res["sor_ms"] * 1e3
    res["dup_clouds_per_s"] = B / res["dup_ms"] * 1e3
    res["punet_roofline_fraction"] = GFLOP_PER_CLOUD * 1e9 * B / (res["pu_net_ms"] * 1e-3) / (PEAK_TFLOPS * 1e12)
    print("PU-Net: %.1f TFLOP/s = %.1f %% of the f32-MFMA peak" % (res["punet_roofline_fraction"] * PEAK_TFLOPS,
                                                                     100 * res["punet_roofline_fraction"]))
    if not a.quick and a.oracle_batches > 0:
        W = PO.to_torch(PO.load_weights())
        W = {k: v.cuda() for k, v in W.items()}
        nb = min(a.oracle_batches, (B + 127) // 128)
        # one start per level, below that level's input size (1024, 1024, 512, 256 points)
        starts = torch.stack([torch.randint(0, n, (128,)) for n in (1024, 1024, 512, 256)], 1)

        def oracle_run(nb=nb):
            for i in range(nb):
                xb = x[i * 128:(i + 1) * 128]
                PO.forward(W, xb, starts[:xb.shape[0]])
        oracle_run(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        oracle_run()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        n = min(B, nb * 128)
        res["oracle_pu_net_clouds_per_s"] = n / t
        # the reference's DUP path = SOR + process_data + PU-Net; charged here with the PU-Net alone (a lower bound on its time)
        res["dup_speedup_vs_oracle_pu_net"] = res["dup_clouds_per_s"] / res["oracle_pu_net_clouds_per_s"]
        print("torch oracle (f32, batch 128, %d clouds): %.1f clouds/s; dup path is %.1fx" %
              (n, res["oracle_pu_net_clouds_per_s"], res["dup_speedup_vs_oracle_pu_net"]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    net.close()


if __name__ == "__main__":
    main()
