#!/usr/bin/env python
"""Generate tests/golden/pointconv_grad_golden.npz by running the REFERENCE's FGM.get_gradient (baselines/attack/FGM/FGM.py:42-68,
normalize=False) on its own PointConv victim (baselines/model/pointconv.py PointConvDensityClsSsg(num_classes=40), eval mode) and
its own adversarial losses (baselines/attack/util/adv_utils.py) on the CPU, with the seeded weights of tests/pointconv_oracle.py.

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its modules are imported where they lie (by file path) and only inputs' recipe and outputs are saved, as
data.  For the duration of the run, and nothing else changed: the model's module sees a ``torch`` whose ``randint`` hands out the
recorded starts (make_golden_pointconv.py's shim); ``.cuda()`` on tensors is answered with the tensor itself; and in the float64
run alone get_gradient's ``data.float()`` is answered with the tensor itself and torch's default dtype is float64, so that the
model's own buffers and the gradient are float64's.  get_gradient is called on a bare object that carries ``model`` and
``adv_func``: FGM.__init__ moves the model to the GPU.

Clouds (3): bench.synth_clouds(3, seed=613) cut to 40, 64 and 128 points, each a batch of its own (the reference's .mean() over one
cloud is the cloud's loss).  Targets 5, 11, 23.  Recorded: the recipe's numbers, and per cloud, precision and loss
(LogitsAdvLoss(kappa = 0), CrossEntropyAdvLoss) the gradient [n,3] and the logits, and per cloud and precision the four index
tables (int16) as the reference's farthest_point_sample and knn_point returned them in that run (topk(sorted=False): a row's
order is torch's).

    python tests/golden/make_golden_pointconv_grad.py
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
from make_golden_pointconv import REF, _PinnedTorch, by_path           # noqa: E402

SEED, CLOUD_SEED, SIZES, TARGETS = 0, 613, (40, 64, 128), (5, 11, 23)
STARTS = ((0, 0), (63, 300), (100, 17))
TABLES = ("fps1", "fps2", "knn1", "knn2")


def run(ref, fgm, adv, sd, pcs, double):
    """-> {loss: (gradients, logits)}, tables: per cloud [fps1, fps2, knn1, knn2] as the run's get_gradient forward made them."""
    model = torch.nn.DataParallel(ref.PointConvDensityClsSsg(num_classes=40))
    model.load_state_dict(sd)
    net = model.module.double().eval() if double else model.module.eval()
    fps, knn = ref.farthest_point_sample, ref.knn_point
    got_f, got_k = [], []

    def recording_fps(xyz, npoint):
        idx = fps(xyz, npoint)
        got_f.append(idx[0].numpy().astype(np.int16))
        return idx

    def recording_knn(nsample, xyz, new_xyz):
        idx = knn(nsample, xyz, new_xyz)
        got_k.append(idx[0].numpy().astype(np.int16))
        return idx

    ref.farthest_point_sample, ref.knn_point = recording_fps, recording_knn
    out, tables = {}, [None] * len(pcs)
    try:
        for name, fn in (("logits", adv.LogitsAdvLoss(kappa=0.)), ("ce", adv.CrossEntropyAdvLoss())):
            me = types.SimpleNamespace(model=net, adv_func=fn)
            grads, los = [], []
            for i, (c, t, st) in enumerate(zip(pcs, TARGETS, STARTS)):
                x = torch.from_numpy(c)[None].transpose(1, 2).contiguous()
                x = x.double() if double else x
                del got_f[:], got_k[:]
                ref.torch.queue[:] = list(st)
                g, _ = fgm.FGM.get_gradient(me, x, torch.tensor([t]), normalize=False)
                assert len(got_f) == 2 and len(got_k) == 2 and not ref.torch.queue
                tab = got_f + got_k
                assert tables[i] is None or all(np.array_equal(a, b) for a, b in zip(tables[i], tab))
                tables[i] = tab
                grads.append(g[0].t().contiguous().numpy())
                ref.torch.queue[:] = list(st)
                with torch.no_grad():
                    lo = net(x)
                    los.append((lo[0] if isinstance(lo, (tuple, list)) else lo)[0].numpy())
            out[name] = (grads, los)
    finally:
        ref.farthest_point_sample, ref.knn_point = fps, knn
    return out, tables


def main():
    import bench
    import pointconv_oracle as PO
    ref = by_path("ref_pointconv", os.path.join(REF, "model", "pointconv.py"))
    ref.torch = _PinnedTorch()
    fgm = by_path("ref_fgm", os.path.join(REF, "attack", "FGM", "FGM.py"))
    adv = by_path("ref_adv", os.path.join(REF, "attack", "util", "adv_utils.py"))
    s = bench.synth_clouds(len(SIZES), seed=CLOUD_SEED)
    pcs = [np.ascontiguousarray(s[i][:n], dtype=np.float32) for i, n in enumerate(SIZES)]
    sd = PO.reference_state_dict(PO.make_weights(SEED))
    cuda, to_float = torch.Tensor.cuda, torch.Tensor.float
    rec = {"weight_seed": np.int32(SEED), "cloud_seed": np.int32(CLOUD_SEED), "sizes": np.int32(SIZES), "targets": np.int32(TARGETS),
           "starts": np.asarray(STARTS, np.int32)}
    try:
        torch.Tensor.cuda = lambda self, *a, **kw: self
        for double in (False, True):
            if double:
                torch.Tensor.float = lambda self, *a, **kw: self
                torch.set_default_dtype(torch.float64)
            res, tables = run(ref, fgm, adv, sd, pcs, double)
            p = "64" if double else ""
            for i, tab in enumerate(tables):
                for name, t in zip(TABLES, tab):
                    rec["%s%s_%d" % (name, p, i)] = t
            for loss, (grads, los) in res.items():
                for i, (g, lo) in enumerate(zip(grads, los)):
                    tag = "%s%s_%d" % (loss, p, i)
                    rec["grad_" + tag], rec["lo_" + tag] = g, lo
                    print(tag, g.dtype, "max |grad| %.3e" % np.abs(g).max(), "pred", int(lo.argmax()))
    finally:
        torch.Tensor.cuda, torch.Tensor.float = cuda, to_float
        torch.set_default_dtype(torch.float32)
    path = os.path.join(HERE, "pointconv_grad_golden.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
