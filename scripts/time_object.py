#!/usr/bin/env python
"""Time of one search step of the CW object-adding attack (include/ifd_object.h) on one MI355X, on a 2468 x 1024 bench.synth_clouds
file with 3 objects of 64 points (the object of tests/golden/objects_golden.npz): ifd_object_attack with binary_step = 1 and --iters
Adam iterations (default 500, the reference's search step), against
  - ifd_cluster_attack with as many added rows (6 clusters of 32 points) over the same iterations on the same clouds, the iteration
    the object attack's is held against, and
  - the same loop written the reference's way on the same GPU - torch autograd through tests/pointnet_oracle.py in float32 on the
    concatenated clouds, LogitsAdvLoss + L2ChamferDist in the reference's form (the stacked-matrix torch.bmm rotation, the expanded
    three-bmm Chamfer of tests/add_oracle.py, sqrt of the sum of squares), torch.optim.Adam over the three tensors, ``%`` on the
    angles, batches of 512 - over --torch_iters iterations.  The torch loop keeps its record in device tensors, without the
    reference's per-iteration copies to the host, so it is the faster of the two ways to write it.
Warmed with a 5-iteration call, synchronised, median of --reps; ms per iteration is what compares when --torch_iters differs from
--iters.  The centres are attack.CWAddObjects' own (128 critical points, ifd_cluster_dbscan, the host's selection); that
initialisation is timed once, on the whole file.  Also timed: ifd_cls_input_grad and ifd_object_step, each alone on the whole
concatenated batch (median of 20 calls), whose ratio is the step kernel's share of an iteration.

    python scripts/time_object.py [--clouds 2468] [--num_add 3] [--obj_num_p 64] [--iters 500] [--torch_iters 100] [--reps 2] [--json profiles/object_time.json]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

REF_BATCH = 512
INIT_WEIGHT, MAX_WEIGHT = 5., 40.
CLUSTER_P = 32


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
    ap.add_argument("--obj_num_p", type=int, default=64)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--torch_iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import add_oracle as DO
    import atk_oracle as AO
    import bench
    import ifdefense_amd as I
    import objects_oracle as OO
    import pointnet_oracle as PO
    from ifdefense_amd import attack, weights
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)).cuda()
    na, P = a.num_add, a.obj_num_p
    B, K, A = int(pc.shape[0]), int(pc.shape[1]), na * P
    if A % CLUSTER_P:
        raise SystemExit("num_add * obj_num_p must be a multiple of %d (the cluster attack it is held against)" % CLUSTER_P)
    sd = PO.make_calibrated_weights(0, False)
    airplane = np.load(os.path.join(ROOT, "tests", "golden", "objects_golden.npz"))["object_raw"]
    res = {"clouds": B, "points": K, "num_add": na, "obj_num_p": P, "reps": a.reps, "iters": a.iters, "torch_iters": a.torch_iters,
           "ref_batch": REF_BATCH}
    with I.Classifier(weights.pack_state_dict(sd, "pointnet"), device="cuda:0") as net:
        tg = (net.predict(pc) + 1) % 40
        atk = attack.CWAddObjects(net, airplane, num_add=na, obj_num_p=P, binary_step=1, ref_batch=REF_BATCH, verbose=False)
        objects = torch.from_numpy(atk.object_pc).float().cuda()
        atk._init_centers(pc[:64], tg[:64])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        centers = atk._init_centers(pc, tg).cuda()
        res["init_ms"] = 1e3 * (time.perf_counter() - t0)
        print("the centres of %d clouds (critical points, DBSCAN on the device, the host's selection): %.1f ms" % (B, res["init_ms"]))
        no, ns, an = [x.cuda() for x in atk.draws(pc)]
        run = lambda n: net.object_attack(pc, tg, objects, centers, an, no, ns, scale=1.0 / REF_BATCH, init_weight=INIT_WEIGHT,   # noqa: E731
                                          max_weight=MAX_WEIGHT, binary_step=1, num_iter=n)
        run(5)
        torch.cuda.synchronize()
        kept = []
        ms, ts = timed(lambda: kept.append(run(a.iters)[2]), a.reps)
        ok = kept[-1]
        res.update(object_step_ms=ms, object_step_ms_all=ts, object_ms_per_iteration=ms / a.iters, object_success=int(ok.sum()),
                   clouds_per_s=B / (ms / 1e3))
        print("ifd_object_attack, one search step of %d iterations: %9.1f ms = %.3f ms an iteration = %.0f clouds/s, %d/%d reach their target"
              % (a.iters, ms, ms / a.iters, B / (ms / 1e3), int(ok.sum()), B))
        # the two kernels of an iteration, each alone on the whole batch
        st = net.object_state(B, na, P, INIT_WEIGHT, MAX_WEIGHT)
        st["obj"].copy_(objects.reshape(1, A, 3) + no[0])
        st["shift"].copy_(centers + ns[0])
        st["angle"].copy_(an[0])
        cat = torch.cat([pc, torch.zeros(B, A, 3, device="cuda")], 1).contiguous()
        net.object_place(st["obj"], st["angle"], st["shift"], cat, na, P)
        grad, aux = net.input_grad(cat, tg, scale=1.0 / REF_BATCH, want_aux=True)
        t_grad = timed(lambda: net.input_grad(cat, tg, scale=1.0 / REF_BATCH), 20)[0]
        t_step = timed(lambda: net.object_step(st, objects, grad, aux["pred"], tg, cat, na, P, 1, 1e-2, 1.0 / REF_BATCH, loss=aux["loss"]),
                       20)[0]
        res.update(input_grad_ms=t_grad, object_step_kernel_ms=t_step, step_share=t_step / (t_grad + t_step))
        print("  alone on %d x %d rows: ifd_cls_input_grad %.3f ms, ifd_object_step %.3f ms = %.1f %% of the two"
              % (B, K + A, t_grad, t_step, 100 * t_step / (t_grad + t_step)))
        # the cluster attack with as many added rows, over the same iterations
        cna = A // CLUSTER_P
        catk = attack.CWAddClusters(net, num_add=cna, cl_num_p=CLUSTER_P, ref_batch=REF_BATCH, verbose=False)
        clusters = catk._init_centers(pc, tg).cuda()
        cl = lambda n: net.cluster_attack(pc, tg, clusters, cna, CLUSTER_P, no[:, :, :A], scale=1.0 / REF_BATCH, init_weight=5.,   # noqa: E731
                                          max_weight=30., binary_step=1, num_iter=n)
        cl(5)
        torch.cuda.synchronize()
        ms_c, ts_c = timed(lambda: cl(a.iters), a.reps)
        res.update(cluster_num_add=cna, cluster_cl_num_p=CLUSTER_P, cluster_step_ms=ms_c, cluster_step_ms_all=ts_c,
                   cluster_ms_per_iteration=ms_c / a.iters, object_over_cluster=ms / ms_c)
        print("ifd_cluster_attack, %d x %d, the same %d iterations: %9.1f ms = %.3f ms an iteration; the object iteration is %.3f x"
              % (cna, CLUSTER_P, a.iters, ms_c, ms_c / a.iters, ms / ms_c))
    W = {k: v.cuda() for k, v in PO.to_torch(sd).items()}

    def torch_step(iters):
        hit = 0
        for i in range(0, B, REF_BATCH):
            ori = pc[i:i + REF_BATCH]                                   # [n, K, 3]
            ori_t = ori.transpose(1, 2).contiguous()
            t = tg[i:i + REF_BATCH]
            n = ori.shape[0]
            tmpl = objects[None].expand(n, na, P, 3)
            obj = (tmpl + no[0, i:i + REF_BATCH].view(n, na, P, 3)).clone().requires_grad_()
            shift = (centers[i:i + REF_BATCH] + ns[0, i:i + REF_BATCH]).clone().requires_grad_()
            angle = an[0, i:i + REF_BATCH].clone().requires_grad_()
            w = torch.full((n,), INIT_WEIGHT, device="cuda")
            bestdist = torch.full((n,), 1e10, device="cuda")
            o_bestdist, o_best = bestdist.clone(), torch.zeros(n, A, 3, device="cuda")
            opt = torch.optim.Adam([obj, shift, angle], lr=1e-2, weight_decay=0.)
            for _ in range(iters):
                c, s = torch.cos(angle), torch.sin(angle)
                z, o = torch.zeros_like(c), torch.ones_like(c)
                rot = torch.stack([c, z, s, z, o, z, -s, z, c], dim=-1).view(n * na, 3, 3)
                rows = (torch.bmm(obj.view(n * na, P, 3), rot).view(n, na, P, 3) + shift[:, :, None, :]).view(n, A, 3)
                lo = PO._forward_batch(W, torch.cat([ori_t, rows.transpose(1, 2).contiguous()], dim=-1))[0]
                cd = torch.min(DO.pairwise(ori, rows), 1)[0].mean(1)
                l2 = torch.sqrt(torch.sum((obj.view(n, A, 3) - tmpl.reshape(n, A, 3)) ** 2, dim=[1, 2]))
                dist = l2 + OO.CHAMFER_WEIGHT * cd
                with torch.no_grad():
                    good = lo.argmax(1) == t
                    bestdist = torch.where(good & (dist < bestdist), dist, bestdist)
                    better = good & (dist < o_bestdist)
                    o_bestdist = torch.where(better, dist, o_bestdist)
                    o_best = torch.where(better[:, None, None], rows, o_best)
                loss = AO.adv_loss(lo, t)[0].mean() + (l2 * w + OO.CHAMFER_WEIGHT * (cd * w)).mean()
                opt.zero_grad()
                loss.backward()
                opt.step()
                with torch.no_grad():
                    angle.data = angle.data % (2. * np.pi)
            hit += int((o_bestdist < 1e10).sum())
        return hit
    torch_step(5)
    torch.cuda.synchronize()
    hits = []
    ms_t, ts_t = timed(lambda: hits.append(torch_step(a.torch_iters)), a.reps)
    res.update(torch_step_ms=ms_t, torch_step_ms_all=ts_t, torch_ms_per_iteration=ms_t / a.torch_iters, torch_success=hits[-1],
               object_speedup_per_iteration=(ms_t / a.torch_iters) / res["object_ms_per_iteration"])
    print("torch autograd + torch.optim.Adam on the GPU (f32, batch %d), %d iterations: %9.1f ms = %.3f ms an iteration; "
          "ifd_object_attack is %.2fx an iteration" % (REF_BATCH, a.torch_iters, ms_t, ms_t / a.torch_iters, res["object_speedup_per_iteration"]))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
