#!/usr/bin/env python
"""Time of one search step of the CW point-adding attack (include/ifd_add.h) on one MI355X, on a 2468 x 1024 bench.synth_clouds file
with 512 added points, for each set distance (chamfer, hausdorff): ifd_add_attack with binary_step = 1 and --iters Adam iterations
(default 500, the reference's search step; the selection of the critical points is inside the call), against the same loop written
the reference's way on the same GPU - torch autograd through tests/pointnet_oracle.py in float32 on the concatenated clouds,
LogitsAdvLoss + the expanded three-bmm set distance of tests/add_oracle.py, torch.optim.Adam on the added points, batches of 512 -
over --torch_iters iterations.  The torch loop keeps its record in device tensors, without the reference's per-iteration copies to
the host, so it is the faster of the two ways to write it.  Warmed with a 5-iteration call, synchronised, median of --reps; ms per
iteration is what compares when --torch_iters differs from --iters.

Also timed, each alone on the whole concatenated batch (median of 20 calls): ifd_cls_input_grad and ifd_add_step, whose ratio is
the step kernel's share of an iteration.

    python scripts/time_add.py [--clouds 2468] [--num_add 512] [--iters 500] [--torch_iters 100] [--reps 2] [--json profiles/add_time.json]
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

REF_BATCH = 512
WEIGHTS = {"chamfer": (5e3, 4e4), "hausdorff": (2e2, 9e2)}


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
    ap.add_argument("--num_add", type=int, default=512)
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
    from ifdefense_amd import weights
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B, K, A = int(pc.shape[0]), int(pc.shape[1]), a.num_add
    sd = PO.make_calibrated_weights(0, False)
    noise = (torch.randn((1, B, A, 3), generator=torch.Generator().manual_seed(1)) * 1e-7).cuda()
    res = {"clouds": B, "points": K, "num_add": A, "reps": a.reps, "iters": a.iters, "torch_iters": a.torch_iters, "ref_batch": REF_BATCH}
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as net:
        tg = (net.predict(pc) + 1) % 40
        cri = net.add_critical_points(pc, tg, A, 1.0 / REF_BATCH)
        for kind in DO.KINDS:
            w0, w1 = WEIGHTS[kind]
            run = lambda n: net.add_attack(kind, pc, tg, A, noise, scale=1.0 / REF_BATCH, init_weight=w0, max_weight=w1,   # noqa: E731
                                           binary_step=1, num_iter=n)
            run(5)
            torch.cuda.synchronize()
            kept = []
            ms, ts = timed(lambda: kept.append(run(a.iters)[2]), a.reps)
            ok = kept[-1]
            res[kind] = {"add_step_ms": ms, "add_step_ms_all": ts, "add_ms_per_iteration": ms / a.iters, "add_success": int(ok.sum())}
            print("ifd_add_attack %s, one search step of %d iterations: %9.1f ms = %.3f ms an iteration, %d/%d reach their target"
                  % (kind, a.iters, ms, ms / a.iters, int(ok.sum()), B))
            # the two kernels of an iteration, each alone on the whole batch
            cat = torch.cat([pc, cri + noise[0]], 1).contiguous()
            grad, aux = net.input_grad(cat, tg, scale=1.0 / REF_BATCH, want_aux=True)
            st = net.cw_state(B, A, w0, w1)
            t_grad = timed(lambda: net.input_grad(cat, tg, scale=1.0 / REF_BATCH), 20)[0]
            t_step = timed(lambda: net.add_step(kind, st, grad, aux["pred"], tg, cat, A, 1, 1e-2, 1.0 / REF_BATCH, loss=aux["loss"]), 20)[0]
            res[kind].update(input_grad_ms=t_grad, add_step_kernel_ms=t_step, step_share=t_step / (t_grad + t_step))
            print("  alone on %d x %d rows: ifd_cls_input_grad %.3f ms, ifd_add_step %.3f ms = %.1f %% of the two"
                  % (B, K + A, t_grad, t_step, 100 * t_step / (t_grad + t_step)))
    W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}

    def torch_step(kind, iters):
        hit = 0
        for i in range(0, B, REF_BATCH):
            ori = pc[i:i + REF_BATCH]                                   # [n, K, 3]
            ori_t = ori.transpose(1, 2).contiguous()
            t = tg[i:i + REF_BATCH]
            n = ori.shape[0]
            adv = (cri[i:i + REF_BATCH] + noise[0, i:i + REF_BATCH]).transpose(1, 2).contiguous().requires_grad_()      # [n, 3, A]
            w = torch.full((n,), WEIGHTS[kind][0], device="cuda")
            bestdist = torch.full((n,), 1e10, device="cuda")
            o_bestdist, o_best = bestdist.clone(), torch.zeros_like(adv)
            opt = torch.optim.Adam([adv], lr=1e-2, weight_decay=0.)
            for _ in range(iters):
                lo = PO._forward_batch(W, torch.cat([ori_t, adv], dim=-1))[0]
                mins = torch.min(DO.pairwise(ori, adv.transpose(1, 2).contiguous()), 1)[0]                              # [n, A]
                dist = mins.mean(1) if kind == "chamfer" else mins.max(1)[0]
                with torch.no_grad():
                    good = lo.argmax(1) == t
                    bestdist = torch.where(good & (dist < bestdist), dist, bestdist)
                    better = good & (dist < o_bestdist)
                    o_bestdist = torch.where(better, dist, o_bestdist)
                    o_best = torch.where(better[:, None, None], adv, o_best)
                loss = AO.adv_loss(lo, t)[0].mean() + (dist * w).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
            hit += int((o_bestdist < 1e10).sum())
        return hit
    for kind in DO.KINDS:
        torch_step(kind, 5)
        torch.cuda.synchronize()
        hits = []
        ms_t, ts_t = timed(lambda: hits.append(torch_step(kind, a.torch_iters)), a.reps)
        r = res[kind]
        r.update(torch_step_ms=ms_t, torch_step_ms_all=ts_t, torch_ms_per_iteration=ms_t / a.torch_iters, torch_success=hits[-1],
                 add_speedup_per_iteration=(ms_t / a.torch_iters) / r["add_ms_per_iteration"])
        print("torch autograd + torch.optim.Adam on the GPU, %s (f32, batch %d), %d iterations: %9.1f ms = %.3f ms an iteration; "
              "ifd_add_attack is %.2fx an iteration" % (kind, REF_BATCH, a.torch_iters, ms_t, ms_t / a.torch_iters, r["add_speedup_per_iteration"]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
