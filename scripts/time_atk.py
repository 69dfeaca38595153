#!/usr/bin/env python
"""Throughput of the attack primitives (include/ifd_atk.h) on one MI355X, on a 2468 x 1024 bench.synth_clouds file: clouds/s
of runtime.Classifier.input_grad against Classifier.logits (ifd_cls_forward) in the same process, a 50-iteration I-FGM
(ifd_fgm_attack, clouds/s and ms per iteration), and the reference-style path - torch autograd through tests/pointnet_oracle.py
in float32 on the GPU, batch 512, loss and gradient as FGM.get_gradient takes them.  Warmed, synchronised, median of --reps.

    python scripts/time_atk.py [--clouds 2468] [--reps 7] [--json profiles/atk_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

REF_BATCH = 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=2468)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import atk_oracle as AO
    import bench
    import ifdefense_amd as I
    import pointnet_oracle as PO
    from ifdefense_amd import weights
    from time_cls import timed
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    B = int(pc.shape[0])
    sd = PO.make_calibrated_weights(0, False)
    res = {"clouds": B, "points": int(pc.shape[1]), "reps": a.reps}
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as net:
        tg = (net.predict(pc) + 1) % 40
        ms_f, _ = timed(lambda: net.logits(pc), a.reps)
        ms_g, ts = timed(lambda: net.input_grad(pc, tg), a.reps)
        res.update(forward_ms=ms_f, forward_clouds_per_s=B / ms_f * 1e3, input_grad_ms=ms_g, input_grad_ms_all=ts,
                   input_grad_clouds_per_s=B / ms_g * 1e3, input_grad_over_forward=ms_g / ms_f)
        print("forward %8.3f ms %9.0f clouds/s | input_grad %8.3f ms %9.0f clouds/s = %.2f x the forward"
              % (ms_f, B / ms_f * 1e3, ms_g, B / ms_g * 1e3, ms_g / ms_f))
        budget = 0.08 * (3 * 1024) ** 0.5
        ms_a, _ = timed(lambda: net.fgm_attack("ifgm", pc, tg, budget, budget / 50, 50, scale=1.0 / REF_BATCH), a.reps)
        ok = net.fgm_attack("ifgm", pc, tg, budget, budget / 50, 50, scale=1.0 / REF_BATCH)[1]
        res.update(ifgm50_ms=ms_a, ifgm50_clouds_per_s=B / ms_a * 1e3, ifgm50_ms_per_iteration=ms_a / 50, ifgm50_success=int(ok.sum()))
        print("I-FGM, 50 iterations: %8.1f ms = %.3f ms an iteration, %7.0f clouds/s, %d/%d reach their target"
              % (ms_a, ms_a / 50, B / ms_a * 1e3, int(ok.sum()), B))
    W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}

    def torch_grad():
        out = []
        for i in range(0, B, REF_BATCH):
            x = pc[i:i + REF_BATCH].transpose(1, 2).contiguous().requires_grad_()
            lo = PO._forward_batch(W, x)[0]
            AO.adv_loss(lo, tg[i:i + REF_BATCH])[0].mean().backward()
            out.append(x.grad)
        return out
    ms_t, _ = timed(torch_grad, a.reps)
    res.update(torch_grad_ms=ms_t, torch_grad_clouds_per_s=B / ms_t * 1e3, input_grad_speedup_vs_torch=ms_t / res["input_grad_ms"])
    print("torch autograd through the oracle on the GPU (f32, batch %d): %8.3f ms %9.0f clouds/s; input_grad is %.2fx"
          % (REF_BATCH, ms_t, B / ms_t * 1e3, ms_t / res["input_grad_ms"]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
