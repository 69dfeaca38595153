#!/usr/bin/env python
"""Generate tests/golden/dgcnn_golden.npz by running the REFERENCE's DGCNN victim (baselines/model/dgcnn.py DGCNN, emb_dims 1024,
k 20, use_bn, eval mode) on CPU with the seeded weights of tests/dgcnn_oracle.py (no victim checkpoint ships).

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its module is imported where it lies (by file path), the oracle's weights go in through load_state_dict in
the checkpoint's own form (nn.DataParallel keys, every BatchNorm under both of its names), and inputs and outputs are saved as
data.  The reference's get_graph_feature asks for torch.device('cuda'); for the duration of the run the imported module sees a
``torch`` whose ``device`` answers with the CPU, nothing else changed.

Clouds (6): bench.synth_clouds(6, seed=611); clouds 0-2 cut to 64 points, 3-5 to 128.  Recorded: the clouds, the weight seed,
k, float32 and float64 logits, the float32 global feature (max | mean of conv5) and, per edge convolution, the float32 and the
float64 run's neighbour indices.

    python tests/golden/make_golden_dgcnn.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(os.environ.get("IFD_REFERENCE_ROOT", "/root/reference"), "baselines")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED, K = 0, 20


class _CpuTorch:
    """``torch`` with ``device(...)`` pinned to the CPU; every other attribute is torch's own."""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def device(*_args, **_kw):
        return torch.device("cpu")


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(ref, sd, pcs, double):
    """-> (logits, global feature, idx per layer) of every cloud, each cloud a batch of its own."""
    model = torch.nn.DataParallel(ref.DGCNN(emb_dims=1024, k=K, output_channels=40))
    model.load_state_dict(sd)
    net = model.module.double().eval() if double else model.module.eval()
    seen = {}
    net.linear1.register_forward_hook(lambda m, inp, out: seen.__setitem__("g", inp[0]))
    knn = ref.knn
    chosen = []

    def recording_knn(x, k):
        idx = knn(x, k)
        chosen.append(idx[0].numpy().astype(np.int32))
        return idx

    ref.knn = recording_knn
    lo, gf, idx = [], [], []
    try:
        with torch.no_grad():
            for c in pcs:
                del chosen[:]
                x = torch.from_numpy(c)[None].transpose(1, 2).contiguous()
                lo.append(net(x.double() if double else x)[0].numpy())
                gf.append(seen["g"][0].numpy())
                idx.append(list(chosen))
    finally:
        ref.knn = knn
    return np.stack(lo), np.stack(gf), idx


def main():
    import bench
    import dgcnn_oracle as DO
    ref = by_path("ref_dgcnn", os.path.join(REF, "model", "dgcnn.py"))
    ref.torch = _CpuTorch()
    s = bench.synth_clouds(6, seed=611)
    pcs = [np.ascontiguousarray(s[i][:64 if i < 3 else 128], dtype=np.float32) for i in range(6)]
    sd = DO.reference_state_dict(DO.make_weights(SEED))
    lo, gf, idx = run(ref, sd, pcs, False)
    lo64, _, idx64 = run(ref, sd, pcs, True)
    rec = {"n_clouds": np.int32(len(pcs)), "weight_seed": np.int32(SEED), "k": np.int32(K), "logits": lo, "logits64": lo64,
           "global_feat": gf}
    for i, c in enumerate(pcs):
        rec["pc_%d" % i] = c
        for l in range(4):
            rec["idx%d_%d" % (l, i)] = idx[i][l]
            rec["idx64_%d_%d" % (l, i)] = idx64[i][l]
    print("e_32 %.3e, |logits| max %.3f" % (np.abs(lo.astype(np.float64) - lo64).max(), np.abs(lo).max()))
    path = os.path.join(HERE, "dgcnn_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
