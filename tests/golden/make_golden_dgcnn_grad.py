#!/usr/bin/env python
"""Generate tests/golden/dgcnn_grad_golden.npz by running the REFERENCE's FGM.get_gradient (baselines/attack/FGM/FGM.py:42-68,
normalize=False) on its own DGCNN victim (baselines/model/dgcnn.py, emb_dims 1024, k 20, eval mode) and its own adversarial
losses (baselines/attack/util/adv_utils.py) on the CPU, with the seeded weights of tests/dgcnn_oracle.py.

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its modules are imported where they lie (by file path) and only inputs' recipe and outputs are saved, as
data.  The reference asks for the GPU in three ways, each answered with the CPU for the duration of the run and nothing else
changed: get_graph_feature's torch.device('cuda') (the shim of make_golden_dgcnn.py), ``.cuda()`` on tensors (answered with the
tensor itself) and, in the float64 run alone, get_gradient's ``data.float()`` (answered with the tensor itself, so that the
gradient is float64's).  get_gradient is called on a bare object that carries ``model`` and ``adv_func``: FGM.__init__ moves the
model to the GPU.

Clouds (3): bench.synth_clouds(3, seed=612); clouds 0 and 1 cut to 64 points, cloud 2 to 128, each a batch of its own (the
reference's .mean() over one cloud is the cloud's loss).  Targets 5, 11, 23.  Recorded: the recipe's numbers, and per cloud and
loss (LogitsAdvLoss(kappa = 0), CrossEntropyAdvLoss) the float32 and the float64 gradient [n,3] and logits.

    python tests/golden/make_golden_dgcnn_grad.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from make_golden_dgcnn import REF, _CpuTorch, by_path           # noqa: E402

SEED, K, CLOUD_SEED, SIZES, TARGETS = 0, 20, 612, (64, 64, 128), (5, 11, 23)


def run(ref, fgm, adv, sd, pcs, double):
    model = torch.nn.DataParallel(ref.DGCNN(emb_dims=1024, k=K, output_channels=40))
    model.load_state_dict(sd)
    net = model.module.double().eval() if double else model.module.eval()
    out = {}
    for name, fn in (("logits", adv.LogitsAdvLoss(kappa=0.)), ("ce", adv.CrossEntropyAdvLoss())):
        me = types.SimpleNamespace(model=net, adv_func=fn)
        grads, los = [], []
        for c, t in zip(pcs, TARGETS):
            x = torch.from_numpy(c)[None].transpose(1, 2).contiguous()
            g, _ = fgm.FGM.get_gradient(me, x.double() if double else x, torch.tensor([t]), normalize=False)
            grads.append(g[0].t().contiguous().numpy())
            with torch.no_grad():
                los.append(net(x.double() if double else x)[0].numpy())
        out[name] = (grads, los)
    return out


def main():
    import bench
    import dgcnn_oracle as DO
    ref = by_path("ref_dgcnn", os.path.join(REF, "model", "dgcnn.py"))
    ref.torch = _CpuTorch()
    fgm = by_path("ref_fgm", os.path.join(REF, "attack", "FGM", "FGM.py"))
    adv = by_path("ref_adv", os.path.join(REF, "attack", "util", "adv_utils.py"))
    s = bench.synth_clouds(len(SIZES), seed=CLOUD_SEED)
    pcs = [np.ascontiguousarray(s[i][:n], dtype=np.float32) for i, n in enumerate(SIZES)]
    sd = DO.reference_state_dict(DO.make_weights(SEED))
    cuda, to_float = torch.Tensor.cuda, torch.Tensor.float
    rec = {"weight_seed": np.int32(SEED), "k": np.int32(K), "cloud_seed": np.int32(CLOUD_SEED), "sizes": np.int32(SIZES),
           "targets": np.int32(TARGETS)}
    try:
        torch.Tensor.cuda = lambda self, *a, **kw: self
        for double in (False, True):
            if double:
                torch.Tensor.float = lambda self, *a, **kw: self
            for loss, (grads, los) in run(ref, fgm, adv, sd, pcs, double).items():
                for i, (g, lo) in enumerate(zip(grads, los)):
                    tag = "%s%s_%d" % (loss, "64" if double else "", i)
                    rec["grad_" + tag], rec["lo_" + tag] = g, lo
                    print(tag, g.dtype, "max |grad| %.3e" % np.abs(g).max(), "pred", int(lo.argmax()))
    finally:
        torch.Tensor.cuda, torch.Tensor.float = cuda, to_float
    path = os.path.join(HERE, "dgcnn_grad_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
