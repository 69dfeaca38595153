#!/usr/bin/env python
"""Time of one search step of the CW point-perturbation attack (include/ifd_cw.h) on one MI355X, on a 2468 x 1024
bench.synth_clouds file: ifd_cw_perturb_attack with binary_step = 1 and --iters Adam iterations (default 500, the reference's
search step), against the same loop written the reference's way on the same GPU - torch autograd through tests/pointnet_oracle.py in
float32, LogitsAdvLoss + L2Dist, torch.optim.Adam, batches of 512 - over --torch_iters iterations.  The torch loop keeps its record
(bestdist / o_bestdist / o_bestattack) in device tensors, without the reference's per-iteration copies to the host, so it is the
faster of the two ways to write it.  Warmed with a 5-iteration call, synchronised, median of --reps; ms per iteration is what
compares when --torch_iters differs from --iters.

    python scripts/time_cw.py [--clouds 2468] [--iters 500] [--torch_iters 500] [--reps 3] [--json profiles/cw_time.json]
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
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--torch_iters", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import atk_oracle as AO
    import bench
    import ifdefense_amd as I
    import pointnet_oracle as PO
    from ifdefense_amd import weights
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B = int(pc.shape[0])
    sd = PO.make_calibrated_weights(0, False)
    noise = (torch.randn((1,) + tuple(pc.shape), generator=torch.Generator().manual_seed(1)) * 1e-7).cuda()
    res = {"clouds": B, "points": int(pc.shape[1]), "reps": a.reps, "iters": a.iters, "torch_iters": a.torch_iters, "ref_batch": REF_BATCH}
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as net:
        tg = (net.predict(pc) + 1) % 40
        run = lambda n: net.cw_perturb_attack(pc, tg, noise, scale=1.0 / REF_BATCH, binary_step=1, num_iter=n)   # noqa: E731
        run(5)
        torch.cuda.synchronize()
        kept = []
        ms, ts = timed(lambda: kept.append(run(a.iters)[2]), a.reps)
        ok = kept[-1]
        res.update(cw_step_ms=ms, cw_step_ms_all=ts, cw_ms_per_iteration=ms / a.iters, cw_success=int(ok.sum()))
        print("ifd_cw_perturb_attack, one search step of %d iterations: %9.1f ms = %.3f ms an iteration, %d/%d reach their target"
              % (a.iters, ms, ms / a.iters, int(ok.sum()), B))
    W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}

    def torch_step(iters):
        hit = 0
        for i in range(0, B, REF_BATCH):
            ori = pc[i:i + REF_BATCH].transpose(1, 2).contiguous()
            t = tg[i:i + REF_BATCH]
            n = ori.shape[0]
            adv = (ori + noise[0, i:i + REF_BATCH].transpose(1, 2)).requires_grad_()
            w = torch.full((n,), 10., device="cuda")
            bestdist = torch.full((n,), 1e10, device="cuda")
            o_bestdist, o_best = bestdist.clone(), torch.zeros_like(ori)
            opt = torch.optim.Adam([adv], lr=1e-2, weight_decay=0.)
            for _ in range(iters):
                lo = PO._forward_batch(W, adv)[0]
                dist = torch.sqrt(torch.sum((adv - ori) ** 2, dim=[1, 2]))
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
    torch_step(5)
    torch.cuda.synchronize()
    hits = []
    ms_t, ts_t = timed(lambda: hits.append(torch_step(a.torch_iters)), a.reps)
    res.update(torch_step_ms=ms_t, torch_step_ms_all=ts_t, torch_ms_per_iteration=ms_t / a.torch_iters, torch_success=hits[-1],
               cw_speedup_per_iteration=(ms_t / a.torch_iters) / (ms / a.iters))
    print("torch autograd + torch.optim.Adam on the GPU (f32, batch %d), %d iterations: %9.1f ms = %.3f ms an iteration; "
          "ifd_cw_perturb_attack is %.2fx an iteration" % (REF_BATCH, a.torch_iters, ms_t, ms_t / a.torch_iters, res["cw_speedup_per_iteration"]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
