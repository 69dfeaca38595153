#!/usr/bin/env python
"""Times of the DGCNN attack primitives (include/ifd_dgcnn_atk.h) on one MI355X, on 128 x 1024 bench.synth_clouds points, k = 20:
ifd_dgcnn_forward, ifd_dgcnn_input_grad, one I-FGM iteration (ifd_dgcnn_fgm_attack with num_iter 11 minus num_iter 1, over 10),
and the reference-style path - torch autograd through tests/dgcnn_oracle.py in float32 on the same GPU, batches of 32, loss and
gradient as FGM.get_gradient takes them.  Warmed, synchronised, median of --reps.  --kernels: the gradient call's time split by
kernel (torch.profiler's device activity, one call).

    python scripts/time_dgcnn_atk.py [--clouds 128] [--points 1024] [--k 20] [--reps 7] [--kernels] [--json profiles/dgcnn_atk_time.json]
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

REF_BATCH = 32


def kernel_split(fn):
    """-> [(kernel name, total device microseconds, calls)] of one fn(), longest first."""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = [(e.key, float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0)), int(e.count))
            for e in prof.key_averages() if "kernel" in e.key or "Memcpy" in e.key or "Memset" in e.key]
    return sorted([r for r in rows if r[1] > 0], key=lambda r: -r[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=128)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import atk_oracle as AO
    import bench
    import dgcnn_oracle as DO
    import ifdefense_amd as I
    from ifdefense_amd import weights
    from time_cls import timed
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)[:, :a.points].copy()).cuda()
    B = int(pc.shape[0])
    sd = DO.make_calibrated_weights(0, a.k)
    res = {"clouds": B, "points": int(pc.shape[1]), "k": a.k, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    with I.DgcnnClassifier(weights.pack_state_dict(sd, "dgcnn"), k=a.k, device="cuda:0") as net:
        tg = (net.predict(pc) + 1) % 40
        ms_f, _ = timed(lambda: net.logits(pc), a.reps)
        ms_g, ts = timed(lambda: net.input_grad(pc, tg), a.reps)
        budget = 0.08 * (3 * a.points) ** 0.5
        ms_1, _ = timed(lambda: net.fgm_attack("ifgm", pc, tg, budget, budget / 50, 1, scale=1.0 / B), a.reps)
        ms_11, _ = timed(lambda: net.fgm_attack("ifgm", pc, tg, budget, budget / 50, 11, scale=1.0 / B), a.reps)
        res.update(forward_ms=ms_f, input_grad_ms=ms_g, input_grad_ms_all=ts, input_grad_over_forward=ms_g / ms_f,
                   ifgm_iteration_ms=(ms_11 - ms_1) / 10)
        print("forward %8.3f ms | input_grad %8.3f ms = %.2f x the forward | one I-FGM iteration %8.3f ms"
              % (ms_f, ms_g, ms_g / ms_f, (ms_11 - ms_1) / 10))
        if a.kernels:
            split = kernel_split(lambda: net.input_grad(pc, tg))
            res["input_grad_kernels_us"] = split
            for name, us, calls in split:
                print("%10.1f us %3d x  %s" % (us, calls, name[:150]))
    W = {k: v.cuda() for k, v in DO.to_torch(sd).items()}

    def torch_grad():
        out = []
        for i in range(0, B, REF_BATCH):
            x = pc[i:i + REF_BATCH].transpose(1, 2).contiguous().requires_grad_()
            lo = DO._forward_batch(W, x, a.k, None)["logits"]
            AO.adv_loss(lo, tg[i:i + REF_BATCH])[0].mean().backward()
            out.append(x.grad)
        return out
    ms_t, _ = timed(torch_grad, a.reps)
    res.update(torch_grad_ms=ms_t, input_grad_speedup_vs_torch=ms_t / ms_g)
    print("torch forward + autograd through the oracle on the GPU (f32, batches of %d): %8.3f ms; input_grad is %.2fx" % (REF_BATCH, ms_t, ms_t / ms_g))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
