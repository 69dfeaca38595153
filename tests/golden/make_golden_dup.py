#!/usr/bin/env python
"""Generate tests/golden/dup_golden.npz (+ dup_golden_out.npz: the PU-Net outputs) and tests/golden/punet_weights_*.npz by running the REFERENCE's baseline defenses
(baselines/defense: SRSDefense, SORDefense, DUPNet with the shipped PU-Net checkpoint) on CPU.

Runs only where the reference tree lies; the fixtures are committed, this script is the provenance record.  Nothing
from the reference is copied: its modules are imported where they lie and their inputs, draws and outputs are saved as
data.  Shims: a no-op ``Tensor.cuda`` (DUPNet.process_data allocates with ``.cuda()``), and wrappers around
``np.random.choice`` and ``torch.randint`` that record every draw (SRS / process_data / the FPS start per level).

Clouds (16, in groups that share a point count, as one reference batch does):
  0-3    bench.synth_clouds at 1024 points (SOR drops a few: the duplicate path with a remainder draw)
  4-6    perturb-like: 1024 points of which 110 are scattered outliers
  7      1024 points with 300 exact duplicate rows
  8-10   add-like: 1216 points (SOR keeps > 1024: the trim path)
  11-12  400 points (kept < 512: two whole copies and a remainder draw)
  13     300 points (three copies)
  14     1024 points on a sphere
  15     a jittered 8 x 8 x 16 lattice + 8 far corners: SOR drops exactly the corners (N == 1024, the pass-through path)

    python tests/golden/make_golden_dup.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(os.environ.get("IFD_REFERENCE_ROOT", "/root/reference"), "baselines")
sys.path.insert(0, ROOT)


def clouds():
    import bench
    rng = np.random.default_rng(20261016)
    groups = [bench.synth_clouds(4, seed=77)]
    pert = []
    for i in range(3):
        p = bench.synth_clouds(1, seed=78 + i)[0]
        p[:110] = rng.uniform(-1, 1, (110, 3)).astype(np.float32)
        pert.append(p)
    dup = bench.synth_clouds(1, seed=90)[0]
    dup[724:] = dup[rng.choice(724, 300)]
    groups.append(np.stack(pert + [dup]))
    add = bench.synth_clouds(3, seed=91)
    extra = add[:, rng.choice(1024, 192)] + rng.normal(0, 0.01, (3, 192, 3)).astype(np.float32)
    groups.append(np.concatenate([add, extra], 1).astype(np.float32))
    groups.append(bench.synth_clouds(2, seed=92)[:, :400])
    groups.append(bench.synth_clouds(1, seed=93)[:, :300])
    s = rng.standard_normal((1, 1024, 3))
    groups.append((s / np.linalg.norm(s, axis=-1, keepdims=True)).astype(np.float32))
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(16), indexing="ij"), -1).reshape(-1, 3)
    lat = (g - [3.5, 3.5, 7.5]) * 0.125 + rng.uniform(-1e-3, 1e-3, (1024, 3))
    corners = np.array([[x, y, z] for x in (-1.5, 1.5) for y in (-1.5, 1.5) for z in (-1.5, 1.5)])
    groups.append(np.concatenate([lat, corners])[None].astype(np.float32))
    return [np.ascontiguousarray(g, dtype=np.float32) for g in groups]


def main():
    sys.path.insert(0, REF)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from defense import DUPNet, SORDefense, SRSDefense

    log = []
    np_choice, t_randint = np.random.choice, torch.randint

    def choice(*a, **k):
        r = np_choice(*a, **k)
        log.append(("np", np.asarray(r)))
        return r

    def randint(*a, **k):
        r = t_randint(*a, **k)
        log.append(("t", r.clone()))
        return r

    np.random.choice, torch.randint = choice, randint
    np.random.seed(5)
    torch.manual_seed(5)

    ck = os.path.join(REF, "defense", "DUP_Net", "pu-in_1024-up_4.pth")
    sd = torch.load(ck, map_location="cpu", weights_only=True)
    # the checkpoint as plain float32 arrays, in shards below the repository's 1 MiB file limit (tests/punet_oracle.py
    # load_weights joins them)
    shard, size, n = {}, 0, 0
    for k, v in sd.items():
        if size + v.numel() * 4 > 900_000 and shard:
            np.savez(os.path.join(HERE, "punet_weights_%d.npz" % n), **shard)
            shard, size, n = {}, 0, n + 1
        shard[k] = v.numpy().astype(np.float32)
        size += v.numel() * 4
    np.savez(os.path.join(HERE, "punet_weights_%d.npz" % n), **shard)
    net = DUPNet(sor_k=2, sor_alpha=1.1, npoint=1024, up_ratio=4)
    net.pu_net.load_state_dict(sd)
    net.eval()

    out = {}
    filled, fps_start, outs, fill_draws, n_kept, cloud_k = [], [], [], [], [], []
    ci = 0
    for g in clouds():
        B, K = g.shape[:2]
        pc = torch.from_numpy(g)
        for b in range(B):
            out["pc_%d" % (ci + b)] = g[b]
        with torch.no_grad():
            kept = SORDefense(k=2, alpha=1.1)(pc)
            sor_mask = []
            for b in range(B):
                # the kept rows are a subsequence of the input: recover the mask
                m = np.zeros(K, np.uint8)
                kp, j = kept[b].numpy(), 0
                for i in range(K):
                    if j < len(kp) and np.array_equal(g[b, i], kp[j]):
                        m[i] = 1
                        j += 1
                assert j == len(kp)
                sor_mask.append(m)
                out["sor_mask_%d" % (ci + b)] = m
            del log[:]
            x = net.process_data(kept)
            draws = [r for kind, r in log if kind == "np"]
            di = 0
            for b in range(B):
                N = len(kept[b])
                d = np.zeros(1024, np.int32)
                if N != 1024:
                    d[:len(draws[di])] = draws[di]
                    di += 1
                fill_draws.append(d)
                n_kept.append(N)
                cloud_k.append(K)
            assert di == len(draws)
            del log[:]
            y = net.pu_net(x)
            starts = [r.numpy() for kind, r in log if kind == "t"]
            assert len(starts) == 4
            fps_start.append(np.stack(starts, 1).astype(np.int32))
            # FPS indices of every level: the reference's farthest_point_sample re-run with the recorded starts
            filled.append(x.numpy())
            outs.append(y.numpy())
            # SRS (drop 500 of 1024 as the CLI default; half of the smaller clouds)
            del log[:]
            drop = 500 if K >= 1024 else K // 2
            s = SRSDefense(drop_num=drop)(pc)
            sd_draws = [r for kind, r in log if kind == "np"]
            for b in range(B):
                out["srs_idx_%d" % (ci + b)] = sd_draws[b].astype(np.int32)
                out["srs_out_%d" % (ci + b)] = s[b].numpy()
                out["srs_drop_%d" % (ci + b)] = np.int32(drop)
        ci += B

    # FPS indices per level, from the reference's own function on the recorded starts
    from defense.DUP_Net.pu_utils import farthest_point_sample, index_points
    X = torch.from_numpy(np.concatenate(filled))
    S = np.concatenate(fps_start)
    fidx = []
    it = iter([])

    def replay(*a, **k):
        return next(it)

    torch.randint = replay
    lx = X
    for v, npt in enumerate((1024, 512, 256, 128)):
        it = iter([torch.from_numpy(S[:, v]).long()])
        idx = farthest_point_sample(lx, npt)
        fidx.append(idx.numpy().astype(np.int32))
        lx = index_points(lx, idx)
    torch.randint = t_randint
    np.random.choice = np_choice

    out.update(n_clouds=np.int32(ci), cloud_k=np.array(cloud_k, np.int32), n_kept=np.array(n_kept, np.int32),
               fill_draws=np.stack(fill_draws), filled=np.concatenate(filled).astype(np.float32), fps_start=S,
               fps_idx=np.concatenate(fidx, 1))
    np.savez_compressed(os.path.join(HERE, "dup_golden.npz"), **out)
    # the PU-Net outputs in a file of their own (the repository's 1 MiB file limit)
    np.savez_compressed(os.path.join(HERE, "dup_golden_out.npz"), out=np.concatenate(outs).astype(np.float32))
    print("clouds", ci, "n_kept", n_kept)


if __name__ == "__main__":
    main()
