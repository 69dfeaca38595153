#!/usr/bin/env python
"""Time of the saliency Drop attack (include/ifd_drop.h) on one MI355X, on a 2468 x 1024 bench.synth_clouds file with num_drop = 200,
k = 5 (the reference script's settings: 40 rounds): ifd_drop_attack, one library call on the whole file, against the same attack
written the reference's way on the same GPU - torch autograd through tests/pointnet_oracle.py in float32 at batch 512, with
Drop.py's torch.median / topk and its per-cloud Python gathers every round.  Warmed (a 2-round call each), synchronised, median of
--reps.

Also timed, each alone on the whole batch (median of 20 calls): ifd_cls_input_grad and ifd_drop_step, whose ratio is the step
kernel's share of a round.

    python scripts/time_drop.py [--clouds 2468] [--num_drop 200] [--k 5] [--reps 3] [--json profiles/drop_time.json]
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
    ap.add_argument("--num_drop", type=int, default=200)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import bench
    import ifdefense_amd as I
    import pointnet_oracle as PO
    from ifdefense_amd import weights
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B, K = int(pc.shape[0]), int(pc.shape[1])
    rounds = -(-a.num_drop // a.k)
    sd = PO.make_calibrated_weights(0, False)
    res = {"clouds": B, "points": K, "num_drop": a.num_drop, "k": a.k, "rounds": rounds, "reps": a.reps, "ref_batch": REF_BATCH}
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as net:
        label = net.predict(pc)
        run = lambda num_drop: net.drop_attack(pc, label, num_drop, a.k, 1., 1.0 / REF_BATCH)       # noqa: E731
        run(2 * a.k)
        torch.cuda.synchronize()
        kept = []
        ms, ts = timed(lambda: kept.append(run(a.num_drop)[1]), a.reps)
        res.update(drop_ms=ms, drop_ms_all=ts, drop_clouds_per_s=B / ms * 1e3, drop_ms_per_round=ms / rounds, drop_correct=int(kept[-1].sum()))
        print("ifd_drop_attack, %d rounds on %d x %d: %9.1f ms = %.0f clouds/s, %.3f ms a round, %d/%d still classified correctly"
              % (rounds, B, K, ms, B / ms * 1e3, ms / rounds, int(kept[-1].sum()), B))
        # the two parts of a round, each alone on the whole batch; the step works in place, so it gets a fresh copy every call
        n = torch.full((B,), K, dtype=torch.int32, device="cuda")
        grad = net.input_grad(pc, label, "cross_entropy", 0., 1.0 / REF_BATCH, n_points=n)
        t_grad = timed(lambda: net.input_grad(pc, label, "cross_entropy", 0., 1.0 / REF_BATCH, n_points=n), 20)[0]
        steps = []
        for _ in range(21):
            cur, cnt = pc.clone(), n.clone()
            torch.cuda.synchronize()
            steps.append(timed(lambda: net.drop_step(grad, cur, cnt, a.k), 1)[0])
        t_step = statistics.median(steps[1:])
        res.update(input_grad_ms=t_grad, drop_step_ms=t_step, step_share=t_step / (t_grad + t_step))
        print("  alone on %d x %d rows: ifd_cls_input_grad %.3f ms, ifd_drop_step %.3f ms = %.1f %% of the two"
              % (B, K, t_grad, t_step, 100 * t_step / (t_grad + t_step)))
    W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}
    lab = label.long()

    def torch_attack(num_drop):
        correct = 0
        for i in range(0, B, REF_BATCH):
            data = pc[i:i + REF_BATCH].transpose(1, 2).contiguous()     # [n, 3, K]
            t = lab[i:i + REF_BATCH]
            nb = data.shape[0]
            for r in range(-(-num_drop // a.k)):
                Kc = data.shape[2]
                k = min(a.k, num_drop - r * a.k)
                x = data.clone().detach().requires_grad_()
                F.cross_entropy(PO._forward_batch(W, x)[0], t).backward()
                with torch.no_grad():
                    g = x.grad.detach()
                    center = torch.median(data, dim=-1)[0].clone().detach()
                    rr = torch.sum((data - center[:, :, None]) ** 2, dim=1) ** 0.5
                    sal = -1. * (rr ** 1) * torch.sum((data - center[:, :, None]) * g, dim=1)
                    _, idx = (-sal).topk(k=Kc - k, dim=-1)
                    data = torch.stack([data[j, :, idx[j]] for j in range(nb)], dim=0)
            with torch.no_grad():
                correct += int((PO._forward_batch(W, data)[0].argmax(1) == t).sum())
        return correct
    torch_attack(2 * a.k)
    torch.cuda.synchronize()
    hits = []
    ms_t, ts_t = timed(lambda: hits.append(torch_attack(a.num_drop)), a.reps)
    res.update(torch_ms=ms_t, torch_ms_all=ts_t, torch_clouds_per_s=B / ms_t * 1e3, torch_ms_per_round=ms_t / rounds, torch_correct=hits[-1],
               drop_speedup=ms_t / res["drop_ms"])
    print("torch autograd + median / topk / per-cloud gathers on the GPU (f32, batch %d), %d rounds: %9.1f ms = %.0f clouds/s; "
          "ifd_drop_attack is %.2fx" % (REF_BATCH, rounds, ms_t, B / ms_t * 1e3, res["drop_speedup"]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
