#!/usr/bin/env python
"""Throughput of the PointNet++ victim classifier (include/ifd_pn2.h) on one MI355X: clouds/s of runtime.PointNet2Classifier on a
2468 x 1024 bench.synth_clouds file (one call, as the pointnet2_inference CLI makes it, start indices given) and at B = 256, each
from warmed, synchronised, repeated runs (median of --reps); the share of the f32-MFMA ceiling of the FLOPs the kernels really
execute (sa1 204 M multiply-adds a cloud, sa2 8 M for U and 406 M on the grouped rows, sa3 92 M, head 0.7 M: 1.42 GFLOP a cloud
against 157.3 TFLOP/s; the reference's direct form of sa2's first layer would be 0.84 G multiply-adds = 1.68 GFLOP); and, as a
step of its own on the same GPU in the same process, the same clouds through a reference-style torch path in float32 - the
farthest-point loop of 512 + 128 dependent torch steps, the sort-based ball query on the matrix-form distances, gather, cat and
the conv2d -> batch_norm -> relu stacks, batch 256.  The per-kernel split comes from a rocprofv3 --kernel-trace --stats run of
this script with --quick.

    python scripts/time_pn2.py [--clouds 2468] [--reps 5] [--quick] [--json out.json]
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
import torch.nn.functional as F  # noqa: E402

PEAK_TFLOPS = 157.3
REF_BATCH = 256


def gflop_per_cloud():
    sa1 = 512 * 32 * (3 * 64 + 64 * 64 + 64 * 128)
    sa2 = 512 * 128 * 128 + 128 * 64 * (3 * 128 + 128 * 128 + 128 * 256)
    sa3 = 128 * (259 * 256 + 256 * 512 + 512 * 1024)
    head = 1024 * 512 + 512 * 256 + 256 * 40
    return 2.0 * (sa1 + sa2 + sa3 + head) * 1e-9


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


# ---- the reference-style torch path: the same work as baselines/model/pointnet2.py does it (a dependent torch step per FPS pick, a
# sort over all n candidates per centroid for the ball, the grouped tensor in memory under a conv2d stack), in this project's words
def t_pair_dist(a, b):
    """a [B,S,3], b [B,N,3] -> [B,S,N] squared distances in the matrix form |a|^2 + |b|^2 - 2 <a, b> (one batched GEMM)."""
    return a.square().sum(-1)[:, :, None] + b.square().sum(-1)[:, None, :] - 2.0 * torch.bmm(a, b.transpose(1, 2))


def t_index(points, idx):
    """points [B,N,C], idx [B,...] -> points[b, idx[b, ...]]."""
    B, C = points.shape[0], points.shape[2]
    flat = idx.reshape(B, -1, 1).expand(-1, -1, C)
    return torch.gather(points, 1, flat).reshape(*idx.shape, C)


def t_fps(xyz, npoint, start):
    B, N, _ = xyz.shape
    picks = torch.empty(B, npoint, dtype=torch.long, device=xyz.device)
    running = torch.full((B, N), 1e10, device=xyz.device)
    far = start.long()
    for i in range(npoint):                                       # npoint dependent steps of a few small kernels each
        picks[:, i] = far
        c = torch.gather(xyz, 1, far.view(B, 1, 1).expand(-1, -1, 3))
        running = torch.minimum(running, (xyz - c).square().sum(-1))
        far = running.argmax(-1)
    return picks


def t_ball(radius, nsample, xyz, new_xyz):
    N = xyz.shape[1]
    own = torch.arange(N, device=xyz.device)
    key = torch.where(t_pair_dist(new_xyz, xyz) > radius * radius, N, own)     # members keep their index, the others sort last
    kept = key.sort(dim=-1).values[:, :, :nsample]
    return torch.where(kept == N, kept[:, :, :1], kept)


def t_sa(W, layers, new_points):
    from ifdefense_amd.weights import BN_EPS
    h = new_points.permute(0, 3, 2, 1)
    for lin, bn, (co, ci), _ in layers:
        h = F.conv2d(h, W[lin + ".weight"].reshape(co, ci, 1, 1), W[lin + ".bias"])
        h = F.relu(F.batch_norm(h, W[bn + ".running_mean"], W[bn + ".running_var"], W[bn + ".weight"], W[bn + ".bias"], False, 0.0, BN_EPS))
    return torch.max(h, 2)[0].permute(0, 2, 1)


def t_forward(W, xyz, starts):
    from ifdefense_amd.weights import BN_EPS, pointnet2_layers
    L = pointnet2_layers()
    B = xyz.shape[0]
    with torch.no_grad():
        c1 = t_index(xyz, t_fps(xyz, 512, starts[:, 0]))
        b1 = t_ball(0.2, 32, xyz, c1)
        p1 = t_sa(W, L[0:3], t_index(xyz, b1) - c1.view(B, 512, 1, 3))
        c2 = t_index(c1, t_fps(c1, 128, starts[:, 1]))
        b2 = t_ball(0.4, 64, c1, c2)
        p2 = t_sa(W, L[3:6], torch.cat([t_index(c1, b2) - c2.view(B, 128, 1, 3), t_index(p1, b2)], dim=-1))
        g = t_sa(W, L[6:9], torch.cat([c2.view(B, 1, 128, 3), p2.view(B, 1, 128, -1)], dim=-1)).view(B, 1024)

        def bn(x, name):
            return F.batch_norm(x, W[name + ".running_mean"], W[name + ".running_var"], W[name + ".weight"], W[name + ".bias"], False, 0.0, BN_EPS)
        h = F.relu(bn(F.linear(g, W["fc1.weight"], W["fc1.bias"]), "bn1"))
        h = F.relu(bn(F.linear(h, W["fc2.weight"], W["fc2.bias"]), "bn2"))
        return F.linear(h, W["fc3.weight"], W["fc3.bias"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=2468)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="one repetition, no torch baseline (for the rocprofv3 kernel split)")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import bench
    import pointnet2_oracle as PO
    import ifdefense_amd as I
    from ifdefense_amd import pointnet2_inference, weights
    reps = 1 if a.quick else a.reps
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B, N = int(pc.shape[0]), int(pc.shape[1])
    starts = torch.from_numpy(pointnet2_inference.fps_starts(1, [N] * B)).cuda()
    res = {"clouds": B, "points": N, "reps": reps, "peak_tflops": PEAK_TFLOPS, "gflop_per_cloud": gflop_per_cloud(),
           "gflop_per_cloud_reference_form": 2 * 0.84, "device": torch.cuda.get_device_name(0)}
    sd = PO.make_weights(0)
    with I.PointNet2Classifier(weights.pack_state_dict(sd, "pointnet2"), device="cuda:0") as net:
        for name, n in (("file", B), ("b%d" % REF_BATCH, min(REF_BATCH, B))):
            ms, ts = timed(lambda: net.logits(pc[:n], fps_start=starts[:n]), reps)
            cps = n / ms * 1e3
            frac = cps * res["gflop_per_cloud"] * 1e9 / (PEAK_TFLOPS * 1e12)
            res["%s_ms" % name], res["%s_ms_all" % name] = ms, ts
            res["%s_clouds_per_s" % name], res["%s_ceiling_fraction" % name] = cps, frac
            print("%-5s %9.3f ms  %9.0f clouds/s  %5.1f %% of the f32-MFMA ceiling (%.3f GFLOP per cloud)"
                  % (name, ms, cps, 100 * frac, res["gflop_per_cloud"]))
        if not a.quick:
            W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}
            n = min(REF_BATCH, B)
            got = net.logits(pc[:n], fps_start=starts[:n])
            ref = t_forward(W, pc[:n], starts[:n])
            res["pred_agreement_with_torch_path"] = float((got.argmax(1) == ref.argmax(1)).float().mean())
            res["median_abs_diff_vs_torch_path"] = float((got - ref).abs().median())
            for name, n in (("file", B), ("b%d" % REF_BATCH, min(REF_BATCH, B))):
                def torch_run(n=n):
                    return [t_forward(W, pc[i:min(i + REF_BATCH, n)], starts[i:min(i + REF_BATCH, n)]) for i in range(0, n, REF_BATCH)]
                ms, ts = timed(torch_run, max(1, reps // 2))
                cps = n / ms * 1e3
                res["%s_torch_ms" % name], res["%s_torch_ms_all" % name] = ms, ts
                res["%s_torch_clouds_per_s" % name] = cps
                res["%s_speedup_vs_torch" % name] = res["%s_clouds_per_s" % name] / cps
                print("%-5s reference-style torch path on the GPU (f32, batch %d): %9.3f ms  %9.0f clouds/s; the HIP path is %.2fx"
                      % (name, REF_BATCH, ms, cps, res["%s_speedup_vs_torch" % name]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
