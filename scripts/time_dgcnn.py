#!/usr/bin/env python
"""Throughput of the DGCNN victim classifier (include/ifd_dgcnn.h) on one MI355X: clouds/s of runtime.DgcnnClassifier at k = 20 on
a 2468 x 1024 bench.synth_clouds file (one call, as the dgcnn_inference CLI makes it) and at B = 96 (the reference's
MAX_TEST_BATCH for DGCNN), each from warmed, synchronised, repeated runs (median of --reps); the share of the f32-MFMA ceiling
of the FLOPs the split form really executes (Gram matrices 2 n^2 (3 + 64 + 64 + 128), P/Q layers, conv5, head: 1.81 GFLOP a cloud
of 1024 points, against 157.3 TFLOP/s: 87 k clouds/s); and, on the same GPU in the same process, the same clouds through
tests/dgcnn_oracle.py in float32 on the GPU - torch ops in the reference's own structure, batch 96 - as the reference-style
baseline.  The per-kernel split comes from a rocprofv3 --kernel-trace --stats run of this script with --quick.

    python scripts/time_dgcnn.py [--clouds 2468] [--reps 7] [--quick] [--json out.json]
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
REF_BATCH = 96                                                 # baselines/config.py MAX_TEST_BATCH[1024]['dgcnn']
K = 20


def gflop_per_cloud(n=1024):
    gram = n * n * (3 + 64 + 64 + 128)
    pq = n * (6 * 64 + 64 * 128 + 64 * 256 + 128 * 512)
    conv5 = n * 512 * 1024
    head = 2048 * 512 + 512 * 256 + 256 * 40
    return 2.0 * (gram + pq + conv5 + head) * 1e-9


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
    import dgcnn_oracle as DO
    import ifdefense_amd as I
    from ifdefense_amd import weights
    reps = 1 if a.quick else a.reps
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B = pc.shape[0]
    res = {"clouds": B, "points": int(pc.shape[1]), "k": K, "reps": reps, "peak_tflops": PEAK_TFLOPS,
           "gflop_per_cloud": gflop_per_cloud(int(pc.shape[1]))}
    sd = DO.make_weights(0)
    with I.DgcnnClassifier(weights.pack_state_dict(sd, "dgcnn"), k=K, device="cuda:0") as net:
        for name, x in (("file", pc), ("b%d" % REF_BATCH, pc[:REF_BATCH])):
            ms, ts = timed(lambda: net.logits(x), reps)
            cps = x.shape[0] / ms * 1e3
            frac = cps * res["gflop_per_cloud"] * 1e9 / (PEAK_TFLOPS * 1e12)
            res["%s_ms" % name], res["%s_ms_all" % name] = ms, ts
            res["%s_clouds_per_s" % name], res["%s_ceiling_fraction" % name] = cps, frac
            print("%-5s %9.3f ms  %9.0f clouds/s  %5.1f %% of the f32-MFMA ceiling (%.3f GFLOP per cloud)"
                  % (name, ms, cps, 100 * frac, res["gflop_per_cloud"]))
        if not a.quick:
            W = {k: v.cuda() for k, v in DO.to_torch(sd).items()}
            got, aux = net.logits(pc[:REF_BATCH], want_aux=True)
            ref = DO.forward(W, pc[:REF_BATCH], k=K, idx=[t.long() for t in aux["idx"]])["logits"]
            res["max_abs_diff_vs_torch_forced_idx"] = float((got - ref).abs().max())
            free = DO.forward(W, pc[:REF_BATCH], k=K)["logits"]
            res["pred_agreement_with_free_running_torch_f32"] = float((got.argmax(1) == free.argmax(1)).float().mean())
            for name, x in (("file", pc), ("b%d" % REF_BATCH, pc[:REF_BATCH])):
                def torch_run(x=x):
                    return [DO.forward(W, x[i:i + REF_BATCH], k=K)["logits"] for i in range(0, x.shape[0], REF_BATCH)]
                ms, ts = timed(torch_run, reps)
                cps = x.shape[0] / ms * 1e3
                res["%s_torch_ms" % name], res["%s_torch_ms_all" % name] = ms, ts
                res["%s_torch_clouds_per_s" % name] = cps
                res["%s_speedup_vs_torch" % name] = res["%s_clouds_per_s" % name] / cps
                print("%-5s torch oracle on the GPU (f32, batch %d): %9.3f ms  %9.0f clouds/s; the fused path is %.2fx"
                      % (name, REF_BATCH, ms, cps, res["%s_speedup_vs_torch" % name]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
