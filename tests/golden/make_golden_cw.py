#!/usr/bin/env python
"""Generate tests/golden/cw_golden.npz by running the REFERENCE's CWPerturb (baselines/attack/CW/Perturb.py) with its L2Dist and
LogitsAdvLoss(kappa=0) on the CPU, on the reference's PointNetCls (k=40, no feature_transform, eval mode) loaded with
pointnet_oracle.make_calibrated_weights(0, False).

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its modules are imported where they lie (by file path) and inputs and outputs are saved as data.  Shims: a
no-op ``Tensor.cuda`` / ``Module.cuda``; an empty stand-in for ``util.set_distance`` (dist_utils.py imports the chamfer kernels,
which L2Dist does not use); and a wrapper around ``torch.randn`` that keeps every draw, which is how the start noise of each search
step is captured ([B,3,K] draws, recorded * 1e-7 and transposed to [B,K,3]).

Run: 4 clouds of 32 points (bench.synth_clouds(4, seed=SEED_CLOUDS)[:, :32]), binary_step 3, num_iter 20, attack_lr 0.01, weights
10 / 80, torch.manual_seed(SEED).  Targets: (prediction + SHIFT[b]) % 40.  Printed by this script and held by
tests/test_cw_cpu.py; which cloud is which is recorded in the fixture as `roles` and listed by the script when it runs:
  "up_down"   succeeds in some search steps and fails in others (its weight goes up and down)
  "success"   succeeds in every search step (lower > 0, weight only rises)
  "never"     never reaches its target (lower == 0: the last_input fallback), if the run has one

    python tests/golden/make_golden_cw.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.path.join(os.environ.get("IFD_REFERENCE_ROOT", "/root/reference"), "baselines")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SEED = int(os.environ.get("CW_GOLDEN_SEED", "7"))
SEED_CLOUDS = 313
SHIFT = [int(x) for x in os.environ.get("CW_GOLDEN_SHIFT", "34,22,34,1").split(",")]
B, K, BINARY_STEP, NUM_ITER, LR = 4, 32, 3, 20, 1e-2


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(write=True):
    import bench
    import pointnet_oracle as PO
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    util = types.ModuleType("util")
    util.set_distance = types.ModuleType("util.set_distance")
    util.set_distance.chamfer = util.set_distance.hausdorff = None
    sys.modules.setdefault("util", util)
    sys.modules.setdefault("util.set_distance", util.set_distance)
    ref_net = by_path("ref_pointnet", os.path.join(REF, "model", "pointnet.py"))
    ref_cw = by_path("ref_perturb", os.path.join(REF, "attack", "CW", "Perturb.py"))
    ref_adv = by_path("ref_adv_utils", os.path.join(REF, "attack", "util", "adv_utils.py"))
    ref_dist = by_path("ref_dist_utils", os.path.join(REF, "attack", "util", "dist_utils.py"))

    sd = PO.make_calibrated_weights(0, False)
    model = torch.nn.DataParallel(ref_net.PointNetCls(k=40, feature_transform=False))
    model.load_state_dict(PO.reference_state_dict(sd))
    net = model.module.eval()
    data = np.ascontiguousarray(bench.synth_clouds(B, seed=SEED_CLOUDS)[:, :K], dtype=np.float32)
    with torch.no_grad():
        pred = net(torch.from_numpy(data).transpose(1, 2).contiguous())[0].argmax(1).numpy()
    target = (pred + np.array(SHIFT)) % 40

    draws, randn = [], torch.randn

    def keeping(*a, **k):
        r = randn(*a, **k)
        draws.append(r.clone())
        return r

    # the reference keeps its weights in local arrays: read them from the frame of attack() at every adjustment
    history = []

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "attack":
            return None

        def local(frame, event, arg):
            if event == "line" and frame.f_lineno == 164:              # torch.cuda.empty_cache() behind the adjustment loop
                f = frame.f_locals
                history.append(np.stack([f["current_weight"], f["lower_bound"], f["upper_bound"]], 1).copy())
            return local
        return local

    attacker = ref_cw.CWPerturb(net, ref_adv.LogitsAdvLoss(kappa=0.), ref_dist.L2Dist(), attack_lr=LR, init_weight=10., max_weight=80.,
                                binary_step=BINARY_STEP, num_iter=NUM_ITER)
    torch.manual_seed(SEED)
    torch.randn = keeping
    sys.settrace(tracer)
    try:
        o_bestdist, o_bestattack, success_num = attacker.attack(torch.from_numpy(data), torch.from_numpy(target))
    finally:
        sys.settrace(None)
        torch.randn = randn
    assert len(draws) == BINARY_STEP and len(history) == BINARY_STEP and all(tuple(d.shape) == (B, 3, K) for d in draws)
    noise = np.stack([(d * 1e-7).numpy().transpose(0, 2, 1) for d in draws]).astype(np.float32)
    history = np.stack(history)                                        # [binary_step, B, 3]
    lower = history[-1, :, 1]
    roles = []
    for b in range(B):
        ups = sum(history[s, b, 1] > (history[s - 1, b, 1] if s else 0.) for s in range(BINARY_STEP))
        roles.append("never" if lower[b] == 0 else "success" if ups == BINARY_STEP else "up_down")
        print("cloud %d: prediction %d, target %d, role %s, o_bestdist %.6g, weights %s" % (b, pred[b], target[b], roles[-1], o_bestdist[b],
                                                                                         history[:, b, 0].tolist()))
    print("success_num", success_num)
    assert "success" in roles or "up_down" in roles, "no cloud succeeds: use another seed"
    assert "up_down" in roles, "no cloud's weight goes both ways: use another seed"
    rec = {"data": data, "target": target.astype(np.int64), "noise": noise, "o_bestdist": np.asarray(o_bestdist, np.float64),
           "o_bestattack": np.asarray(o_bestattack, np.float64), "success_num": np.int64(success_num), "history": history,
           "roles": np.array(roles), "binary_step": np.int32(BINARY_STEP), "num_iter": np.int32(NUM_ITER), "attack_lr": np.float64(LR),
           "init_weight": np.float64(10.), "max_weight": np.float64(80.), "seed": np.int64(SEED)}
    if write:
        path = os.path.join(HERE, "cw_golden.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")
    return rec


if __name__ == "__main__":
    main()
