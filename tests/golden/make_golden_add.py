#!/usr/bin/env python
"""Generate tests/golden/add_golden.npz by running the REFERENCE's CWAdd (baselines/attack/CW/Add.py) with its ChamferDist('adv2ori')
and its HausdorffDist('adv2ori') and LogitsAdvLoss(kappa=0) on the CPU, on the reference's PointNetCls (k=40, no
feature_transform, eval mode) loaded with pointnet_oracle.make_calibrated_weights(0, False).

Runs only where the reference tree lies; the fixture is committed, this script is the provenance record.  Nothing from the
reference is copied: its modules are imported where they lie (by file path) - the real baselines/util/set_distance.py among them,
registered as ``util.set_distance`` for dist_utils.py - and inputs and outputs are saved as data.  Shims: a no-op ``Tensor.cuda`` /
``Module.cuda``; a wrapper around ``torch.randn`` that keeps every draw, which is how the start noise of each search step is
captured ([B,3,num_add] draws, recorded * 1e-7 and transposed to [B,num_add,3]); a frame tracer that reads the weights and the
critical points from attack()'s locals behind every adjustment.

Run, once per distance: 4 clouds of 32 points (bench.synth_clouds(4, seed=SEED_CLOUDS)[:, :32]), num_add 8, binary_step 3, num_iter
20, attack_lr 0.01, the reference script's weights (chamfer 5e3 / 4e4, hausdorff 2e2 / 9e2), torch.manual_seed(SEED).  Targets:
(prediction + SHIFT[b]) % 40.  The script asserts what the fixture's users rely on: in every cloud the scores of the 8 selected rows
are pairwise distinct and non-zero and the 8th exceeds the 9th (so the fixture does not depend on torch.topk's order among
equals); for each distance at least one cloud succeeds and one cloud's weight moves both ways.

    python tests/golden/make_golden_add.py
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
SEED = int(os.environ.get("ADD_GOLDEN_SEED", "7"))
SEED_CLOUDS = 313
SHIFT = [int(x) for x in os.environ.get("ADD_GOLDEN_SHIFT", "34,5,34,7").split(",")]
B, K, NUM_ADD, BINARY_STEP, NUM_ITER, LR = 4, 32, 8, 3, 20, 1e-2
WEIGHTS = {"chamfer": (5e3, 4e4), "hausdorff": (2e2, 9e2)}
ADJUSTED_LINE = 205                                                    # Add.py: torch.cuda.empty_cache() behind the adjustment loop


def by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(write=True):
    import bench
    import pointnet_oracle as PO
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.nn.Module.cuda = lambda self, *a, **k: self
    sys.modules.setdefault("util", types.ModuleType("util"))
    sys.modules["util"].set_distance = by_path("util.set_distance", os.path.join(REF, "util", "set_distance.py"))
    ref_net = by_path("ref_pointnet", os.path.join(REF, "model", "pointnet.py"))
    ref_add = by_path("ref_add", os.path.join(REF, "attack", "CW", "Add.py"))
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

    # the selection must not hang on torch.topk's order among equals
    x = torch.from_numpy(data).transpose(1, 2).contiguous().requires_grad_()
    torch.nn.functional.cross_entropy(net(x)[0], torch.from_numpy(target).long()).backward()
    score = torch.sum(x.grad ** 2, dim=1).numpy()                      # [B, K]
    for b in range(B):
        s = np.sort(score[b])[::-1]
        gaps = (s[:NUM_ADD] - s[1:NUM_ADD + 1]) / s[:NUM_ADD]
        print("cloud %d: selected scores %.3e .. %.3e, smallest relative gap %.1e" % (b, s[0], s[NUM_ADD - 1], gaps.min()))
        assert s[NUM_ADD - 1] > 0 and len(set(s[:NUM_ADD].tolist())) == NUM_ADD and s[NUM_ADD - 1] > s[NUM_ADD], "ties in the selection"

    rec = {"data": data, "target": target.astype(np.int64), "num_add": np.int32(NUM_ADD), "binary_step": np.int32(BINARY_STEP),
           "num_iter": np.int32(NUM_ITER), "attack_lr": np.float64(LR), "seed": np.int64(SEED)}
    for kind in ("chamfer", "hausdorff"):
        draws, randn = [], torch.randn

        def keeping(*a, **k):
            r = randn(*a, **k)
            draws.append(r.clone())
            return r

        # the reference keeps its weights in local arrays: read them from the frame of attack() at every adjustment
        history, cri = [], []

        def tracer(frame, event, arg):
            if frame.f_code.co_name != "attack":
                return None

            def local(frame, event, arg):
                if event == "line" and frame.f_lineno == ADJUSTED_LINE:
                    f = frame.f_locals
                    history.append(np.stack([f["current_weight"], f["lower_bound"], f["upper_bound"]], 1).copy())
                    cri.append(f["cri_data"].detach().numpy().transpose(0, 2, 1).copy())
                return local
            return local

        dist = ref_dist.ChamferDist(method="adv2ori") if kind == "chamfer" else ref_dist.HausdorffDist(method="adv2ori")
        init_w, max_w = WEIGHTS[kind]
        attacker = ref_add.CWAdd(net, ref_adv.LogitsAdvLoss(kappa=0.), dist, attack_lr=LR, init_weight=init_w, max_weight=max_w,
                                 binary_step=BINARY_STEP, num_iter=NUM_ITER, num_add=NUM_ADD)
        torch.manual_seed(SEED)
        torch.randn = keeping
        sys.settrace(tracer)
        try:
            o_bestdist, o_bestattack, success_num = attacker.attack(torch.from_numpy(data), torch.from_numpy(target))
        finally:
            sys.settrace(None)
            torch.randn = randn
        assert len(draws) == BINARY_STEP and len(history) == BINARY_STEP and all(tuple(d.shape) == (B, 3, NUM_ADD) for d in draws)
        noise = np.stack([(d * 1e-7).numpy().transpose(0, 2, 1) for d in draws]).astype(np.float32)
        history = np.stack(history)                                    # [binary_step, B, 3]
        lower = history[-1, :, 1]
        roles = []
        for b in range(B):
            ups = sum(history[s, b, 1] > (history[s - 1, b, 1] if s else 0.) for s in range(BINARY_STEP))
            roles.append("never" if lower[b] == 0 else "success" if ups == BINARY_STEP else "up_down")
            print("%s cloud %d: prediction %d, target %d, role %s, o_bestdist %.6g, weights %s" % (
                kind, b, pred[b], target[b], roles[-1], o_bestdist[b], history[:, b, 0].tolist()))
        print(kind, "success_num", success_num)
        assert success_num >= 1, "no cloud succeeds: use another seed"
        assert "up_down" in roles, "no cloud's weight goes both ways: use another seed"
        assert o_bestattack.shape == (B, K + NUM_ADD, 3) and np.array_equal(o_bestattack[:, :K].astype(np.float32), data)
        rec.update({kind + "_noise": noise, kind + "_cri_data": cri[0].astype(np.float32), kind + "_history": history,
                    kind + "_o_bestdist": np.asarray(o_bestdist, np.float64), kind + "_o_bestattack": np.asarray(o_bestattack, np.float64),
                    kind + "_success_num": np.int64(success_num), kind + "_roles": np.array(roles),
                    kind + "_init_weight": np.float64(init_w), kind + "_max_weight": np.float64(max_w)})
    if write:
        path = os.path.join(HERE, "add_golden.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")
    return rec


if __name__ == "__main__":
    main()
