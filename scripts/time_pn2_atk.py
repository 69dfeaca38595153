#!/usr/bin/env python
"""Times of the PointNet++ attack primitives (include/ifd_pn2_atk.h) on one MI355X, on 128 x 1024 bench.synth_clouds points:
ifd_pn2_forward, ifd_pn2_input_grad, one I-FGM iteration (ifd_pn2_fgm_attack with num_iter 11 minus num_iter 1, over 10), and the
reference-style path - torch autograd through the layers of tests/pointnet2_oracle.py (_sa, _bn) in float32 on the same GPU,
batches of 32, loss and gradient as FGM.get_gradient takes them.  The torch path is handed the library's four index tables and
does not pay for the samplings or the ball queries.  Warmed, synchronised, median of --reps.  --kernels: the gradient call's time
split by kernel (torch.profiler's device activity, one call).

    python scripts/time_pn2_atk.py [--clouds 128] [--points 1024] [--reps 7] [--kernels] [--json profiles/pn2_atk_time.json]
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
import torch.nn.functional as F  # noqa: E402

REF_BATCH = 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=128)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import atk_oracle as AO
    import bench
    import pointnet2_oracle as PO
    import ifdefense_amd as I
    from ifdefense_amd import weights
    from time_cls import timed
    from time_dgcnn_atk import kernel_split
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)[:, :a.points].copy()).cuda()
    B = int(pc.shape[0])
    sd = PO.make_calibrated_weights(0)
    res = {"clouds": B, "points": int(pc.shape[1]), "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    with I.PointNet2Classifier(weights.pack_state_dict(sd, "pointnet2"), device="cuda:0") as net:
        _, aux = net.logits(pc, want_aux=True)
        tg = (aux["pred"].long() + 1) % 40
        tab = {k: aux[k].long() for k in ("fps1", "fps2", "ball1", "ball2")}
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
    W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}
    L = weights.pointnet2_layers()

    def torch_grad():
        out = []
        for i in range(0, B, REF_BATCH):
            x = pc[i:i + REF_BATCH].clone().requires_grad_()
            n = int(x.shape[0])
            ar = torch.arange(n, device=x.device)
            f1, f2, b1, b2 = (tab[k][i:i + n] for k in ("fps1", "fps2", "ball1", "ball2"))
            c1 = x[ar[:, None], f1]
            p1 = PO._sa(W, L[0:3], x[ar[:, None, None], b1] - c1.view(n, PO.NP1, 1, 3))
            c2 = c1[ar[:, None], f2]
            l2 = PO._sa(W, L[3:6], torch.cat([c1[ar[:, None, None], b2] - c2.view(n, PO.NP2, 1, 3), p1[ar[:, None, None], b2]], dim=-1))
            g = PO._sa(W, L[6:9], torch.cat([c2.view(n, 1, PO.NP2, 3), l2.view(n, 1, PO.NP2, -1)], dim=-1)).view(n, 1024)
            h1 = F.relu(PO._bn(W, F.linear(g, W["fc1.weight"], W["fc1.bias"]), "bn1"))
            h2 = F.relu(PO._bn(W, F.linear(h1, W["fc2.weight"], W["fc2.bias"]), "bn2"))
            lo = F.linear(h2, W["fc3.weight"], W["fc3.bias"])
            AO.adv_loss(lo, tg[i:i + n])[0].mean().backward()
            out.append(x.grad)
        return out
    ms_t, _ = timed(torch_grad, a.reps)
    res.update(torch_grad_ms=ms_t, input_grad_speedup_vs_torch=ms_t / ms_g)
    print("torch forward + autograd through the oracle's layers on the GPU (f32, batches of %d, tables given): %8.3f ms; input_grad is %.2fx"
          % (REF_BATCH, ms_t, ms_t / ms_g))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
