#!/usr/bin/env python
"""Time of one search step of the CW cluster-adding attack (include/ifd_cluster.h) on one MI355X, on a 2468 x 1024 bench.synth_clouds
file with 3 clusters of 32 points: ifd_cluster_attack with binary_step = 1 and --iters Adam iterations (default 500, the reference's
search step), against the same loop written the reference's way on the same GPU - torch autograd through tests/pointnet_oracle.py
in float32 on the concatenated clouds, LogitsAdvLoss + FarChamferDist in the reference's form (the expanded three-bmm Chamfer of
tests/add_oracle.py, the + 1e-7 delta matrix, torch.norm and two torch.max), torch.optim.Adam on the added points, batches of 512 -
over --torch_iters iterations.  The torch loop keeps its record in device tensors, without the reference's per-iteration copies to
the host, so it is the faster of the two ways to write it.  Warmed with a 5-iteration call, synchronised, median of --reps; ms per
iteration is what compares when --torch_iters differs from --iters.

The start clusters are attack.CWAddClusters' own (128 critical points, ifd_cluster_dbscan, the host draws); that initialisation is
timed once, on the whole file.

Also timed: ifd_cls_input_grad and ifd_cluster_step, each alone on the whole concatenated batch (median of 20 calls), whose ratio
is the step kernel's share of an iteration; and ifd_add_attack (Chamfer, num_add = 96: the same number of added rows) over the same
iterations on the same clouds, the iteration the cluster attack's is held against.

    python scripts/time_cluster.py [--clouds 2468] [--num_add 3] [--cl_num_p 32] [--iters 500] [--torch_iters 100] [--reps 2] [--json profiles/cluster_time.json]
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

import torch  # noqa: E402

REF_BATCH = 512
INIT_WEIGHT, MAX_WEIGHT = 5., 30.


def timed(fn, reps):
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
    ap.add_argument("--num_add", type=int, default=3)
    ap.add_argument("--cl_num_p", type=int, default=32)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--torch_iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import add_oracle as DO
    import atk_oracle as AO
    import bench
    import ifdefense_amd as I
    import pointnet_oracle as PO
    from ifdefense_amd import attack, weights
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    na, P = a.num_add, a.cl_num_p
    B, K, A = int(pc.shape[0]), int(pc.shape[1]), na * P
    sd = PO.make_calibrated_weights(0, False)
    noise = (torch.randn((1, B, A, 3), generator=torch.Generator().manual_seed(1)) * 1e-7).cuda()
    res = {"clouds": B, "points": K, "num_add": na, "cl_num_p": P, "reps": a.reps, "iters": a.iters, "torch_iters": a.torch_iters,
           "ref_batch": REF_BATCH}
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as net:
        tg = (net.predict(pc) + 1) % 40
        atk = attack.CWAddClusters(net, num_add=na, cl_num_p=P, ref_batch=REF_BATCH, verbose=False)
        atk._init_centers(pc[:64], tg[:64])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clusters = atk._init_centers(pc, tg).cuda()
        res["init_ms"] = 1e3 * (time.perf_counter() - t0)
        print("the start clusters of %d clouds (critical points, DBSCAN on the device, the host draws): %.1f ms" % (B, res["init_ms"]))
        run = lambda n: net.cluster_attack(pc, tg, clusters, na, P, noise, scale=1.0 / REF_BATCH, init_weight=INIT_WEIGHT,   # noqa: E731
                                           max_weight=MAX_WEIGHT, binary_step=1, num_iter=n)
        run(5)
        torch.cuda.synchronize()
        kept = []
        ms, ts = timed(lambda: kept.append(run(a.iters)[2]), a.reps)
        ok = kept[-1]
        res.update(cluster_step_ms=ms, cluster_step_ms_all=ts, cluster_ms_per_iteration=ms / a.iters, cluster_success=int(ok.sum()),
                   clouds_per_s=B / (ms / 1e3))
        print("ifd_cluster_attack, one search step of %d iterations: %9.1f ms = %.3f ms an iteration = %.0f clouds/s, %d/%d reach their target"
              % (a.iters, ms, ms / a.iters, B / (ms / 1e3), int(ok.sum()), B))
        # the two kernels of an iteration, each alone on the whole batch
        cat = torch.cat([pc, clusters + noise[0]], 1).contiguous()
        grad, aux = net.input_grad(cat, tg, scale=1.0 / REF_BATCH, want_aux=True)
        st = net.cw_state(B, A, INIT_WEIGHT, MAX_WEIGHT)
        t_grad = timed(lambda: net.input_grad(cat, tg, scale=1.0 / REF_BATCH), 20)[0]
        t_step = timed(lambda: net.cluster_step(st, grad, aux["pred"], tg, cat, na, P, 1, 1e-2, 1.0 / REF_BATCH, loss=aux["loss"]), 20)[0]
        res.update(input_grad_ms=t_grad, cluster_step_kernel_ms=t_step, step_share=t_step / (t_grad + t_step))
        print("  alone on %d x %d rows: ifd_cls_input_grad %.3f ms, ifd_cluster_step %.3f ms = %.1f %% of the two"
              % (B, K + A, t_grad, t_step, 100 * t_step / (t_grad + t_step)))
        # the CW Add attack with as many added rows, over the same iterations
        add = lambda n: net.add_attack("chamfer", pc, tg, A, noise, scale=1.0 / REF_BATCH, init_weight=5e3, max_weight=4e4,   # noqa: E731
                                       binary_step=1, num_iter=n)
        add(5)
        torch.cuda.synchronize()
        ms_a, ts_a = timed(lambda: add(a.iters), a.reps)
        res.update(add_step_ms=ms_a, add_step_ms_all=ts_a, add_ms_per_iteration=ms_a / a.iters, cluster_over_add=ms / ms_a)
        print("ifd_add_attack chamfer, num_add %d, the same %d iterations: %9.1f ms = %.3f ms an iteration; the cluster iteration is %.3f x"
              % (A, a.iters, ms_a, ms_a / a.iters, ms / ms_a))
    W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}

    def torch_step(iters):
        hit = 0
        for i in range(0, B, REF_BATCH):
            ori = pc[i:i + REF_BATCH]                                   # [n, K, 3]
            ori_t = ori.transpose(1, 2).contiguous()
            t = tg[i:i + REF_BATCH]
            n = ori.shape[0]
            adv = (clusters[i:i + REF_BATCH] + noise[0, i:i + REF_BATCH]).transpose(1, 2).contiguous().requires_grad_()      # [n, 3, A]
            w = torch.full((n,), INIT_WEIGHT, device="cuda")
            bestdist = torch.full((n,), 1e10, device="cuda")
            o_bestdist, o_best = bestdist.clone(), torch.zeros_like(adv)
            opt = torch.optim.Adam([adv], lr=1e-2, weight_decay=0.)
            for _ in range(iters):
                lo = PO._forward_batch(W, torch.cat([ori_t, adv], dim=-1))[0]
                rows = adv.transpose(1, 2).contiguous()                 # [n, A, 3]
                cd = torch.min(DO.pairwise(ori, rows), 1)[0].mean(1)
                c = rows.view(n, na, P, 3)
                norm = torch.norm(c[:, :, None, :, :] - c[:, :, :, None, :] + 1e-7, p=2, dim=-1)
                far = torch.max(torch.max(norm, dim=2)[0], dim=2)[0].sum(1)
                dist = far + cd * 0.1
                with torch.no_grad():
                    good = lo.argmax(1) == t
                    bestdist = torch.where(good & (dist < bestdist), dist, bestdist)
                    better = good & (dist < o_bestdist)
                    o_bestdist = torch.where(better, dist, o_bestdist)
                    o_best = torch.where(better[:, None, None], adv, o_best)
                loss = AO.adv_loss(lo, t)[0].mean() + (far * w + (cd * w) * 0.1).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
            hit += int((o_bestdist < 1e10).sum())
        return hit
    torch_step(5)
    torch.cuda.synchronize()
    hits = []
    ms_t, ts_t = timed(lambda: hits.append(torch_step(a.torch_iters)), a.reps)
    res.update(torch_step_ms=ms_t, torch_step_ms_all=ts_t, torch_ms_per_iteration=ms_t / a.torch_iters, torch_success=hits[-1],
               cluster_speedup_per_iteration=(ms_t / a.torch_iters) / res["cluster_ms_per_iteration"])
    print("torch autograd + torch.optim.Adam on the GPU (f32, batch %d), %d iterations: %9.1f ms = %.3f ms an iteration; "
          "ifd_cluster_attack is %.2fx an iteration" % (REF_BATCH, a.torch_iters, ms_t, ms_t / a.torch_iters, res["cluster_speedup_per_iteration"]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
