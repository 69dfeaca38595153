#!/usr/bin/env python
"""Times of the PointConv attack primitives (include/ifd_pc_atk.h) on one MI355X, on 128 x 1024 bench.synth_clouds points:
ifd_pc_forward, ifd_pc_input_grad, one I-FGM iteration (ifd_pc_fgm_attack with num_iter 11 minus num_iter 1, over 10), and the
reference-style path - torch autograd through the layers of tests/pointconv_oracle.py (_stack, _bn; the reference's matrix-form
density) in float32 on the same GPU, batches of 32, loss and gradient as FGM.get_gradient takes them.  The torch path is handed the
library's four index tables and does not pay for the samplings or the neighbour searches.  Warmed, synchronised, median of --reps.
--kernels: the gradient call's time split by kernel (torch.profiler's device activity, one call of its own).

    python scripts/time_pc_atk.py [--clouds 128] [--points 1024] [--reps 7] [--kernels] [--json profiles/pc_atk_time.json]
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
    ap.add_argument("--no_torch", action="store_true", help="skip the torch autograd path")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import atk_oracle as AO
    import bench
    import pointconv_oracle as PO
    import ifdefense_amd as I
    from ifdefense_amd import weights
    from time_cls import timed
    from time_dgcnn_atk import kernel_split
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)[:, :a.points].copy()).cuda()
    B = int(pc.shape[0])
    sd = PO.make_calibrated_weights(0)
    res = {"clouds": B, "points": int(pc.shape[1]), "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    with I.PointConvClassifier(weights.pack_state_dict(sd, "pointconv"), device="cuda:0") as net:
        _, aux = net.logits(pc, want_aux=True)
        tg = (aux["pred"].long() + 1) % 40
        tab = {k: aux[k].long() for k in PO.TABLES}
        ms_f, ts_f = timed(lambda: net.logits(pc), a.reps)
        ms_g, ts = timed(lambda: net.input_grad(pc, tg), a.reps)
        budget = 0.08 * (3 * a.points) ** 0.5
        ms_1, _ = timed(lambda: net.fgm_attack("ifgm", pc, tg, budget, budget / 50, 1, scale=1.0 / B), a.reps)
        ms_11, _ = timed(lambda: net.fgm_attack("ifgm", pc, tg, budget, budget / 50, 11, scale=1.0 / B), a.reps)
        res.update(forward_ms=ms_f, forward_ms_all=ts_f, input_grad_ms=ms_g, input_grad_ms_all=ts, input_grad_over_forward=ms_g / ms_f,
                   ifgm_iteration_ms=(ms_11 - ms_1) / 10)
        print("forward %8.3f ms (%.3f .. %.3f) | input_grad %8.3f ms = %.2f x the forward | one I-FGM iteration %8.3f ms"
              % (ms_f, min(ts_f), max(ts_f), ms_g, ms_g / ms_f, (ms_11 - ms_1) / 10))
        if a.kernels:
            split = kernel_split(lambda: net.input_grad(pc, tg))
            res["input_grad_kernels_us"] = split
            for name, us, calls in split:
                print("%10.1f us %3d x  %s" % (us, calls, name[:150]))
    if not a.no_torch:
        W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}
        L = weights.pointconv_layers()

        def scale_of(layers, xyz, bw):                                       # pointconv_oracle.density_scale on a batch [n,N,3]
            sq = (xyz * xyz).sum(-1)
            d = (sq[:, :, None] + sq[:, None, :]) - 2.0 * (xyz @ xyz.transpose(1, 2))
            rho = (torch.exp(-d / (2.0 * bw * bw)) / (2.5 * bw)).mean(-1)
            return PO._stack(W, layers, rho.reshape(-1, 1)).view(rho.shape)

        def level(Ls, grouped, feats, scale):                                # pointconv_oracle._level on a batch [n,S,K,.]
            n, S, K, _ = grouped.shape
            rows = grouped if feats is None else torch.cat([grouped, feats], dim=-1)
            h = PO._stack(W, Ls[3:6], rows.reshape(n * S * K, -1)).view(n, S, K, -1) * scale[..., None]
            wn = PO._stack(W, Ls[6:9], grouped.reshape(n * S * K, 3)).view(n, S, K, 16)
            return PO._stack(W, Ls[9:10], torch.matmul(h.transpose(-1, -2), wn).reshape(n * S, -1)).view(n, S, -1)

        def torch_grad():
            out = []
            for i in range(0, B, REF_BATCH):
                x = pc[i:i + REF_BATCH].clone().requires_grad_()
                n = int(x.shape[0])
                a1, a2 = torch.arange(n, device=x.device)[:, None], torch.arange(n, device=x.device)[:, None, None]
                f1, f2, k1, k2 = (tab[k][i:i + n] for k in PO.TABLES)
                s1 = scale_of(L[0:3], x, PO.BW1)
                c1 = x[a1, f1]
                p1 = level(L[0:10], x[a2, k1] - c1[:, :, None, :], None, s1[a2, k1])
                s2 = scale_of(L[10:13], c1, PO.BW2)
                c2 = c1[a1, f2]
                l2 = level(L[10:20], c1[a2, k2] - c2[:, :, None, :], p1[a2, k2], s2[a2, k2])
                s3 = scale_of(L[20:23], c2, PO.BW3)
                g = level(L[20:30], (c2 - c2.mean(dim=1, keepdim=True))[:, None], l2[:, None], s3[:, None]).view(n, 1024)
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
