#!/usr/bin/env python
"""Generate tests/golden/objects_golden.npz by running the REFERENCE's CWAddObjects (baselines/attack/CW/Add_Objects.py) with its
L2ChamferDist(3, 'adv2ori', 0.2) and LogitsAdvLoss(kappa=0) on the CPU, on the reference's PointNetCls (k=40, no feature_transform,
eval mode) loaded with pointnet_oracle.make_calibrated_weights(0, False), with the reference's own object, baselines/data/airplane.npy.

Runs only where the reference tree and sklearn are; the fixture is committed, this script is the provenance record.  Nothing from
the reference is copied: its modules are imported where they lie (by file path) - the real baselines/util/set_distance.py and
baselines/util/pointnet_utils.py among them, registered as ``util.set_distance`` and ``util.pointnet_utils`` - and inputs and outputs
are saved as data; the object file is data the reference's programs read, kept as the array ``object_raw``.  Shims: a no-op
``Tensor.cuda`` / ``Module.cuda``; wrappers around ``torch.randn`` and ``torch.rand_like`` that keep every draw (per search step: the
objects' noise [B,num_add,P,3] and the shifts' noise [B,num_add,3], recorded * 1e-7, and the angles' draw [B,num_add,3], recorded * pi,
component 0 - the only one that enters the rotation); wrappers around the module's get_critical_points, DBSCAN and np.random.choice
and around the attacker's _init_centers that keep what they return; a frame tracer that reads the weights from attack()'s locals
behind every adjustment.

Run: 4 clouds of 192 points (bench.synth_clouds(6, seed=SEED_CLOUDS)[CLOUDS, :192]), num_add 3, obj_num_p 64, binary_step 3, num_iter
20, attack_lr 0.01, init_weight 5, max_weight 40, scaling 0.3, np.random.seed(SEED) before the attacker is made (its constructor
shuffles the object) and torch.manual_seed(SEED).  Targets: (prediction + SHIFT[b]) % 40.  The script asserts what the fixture's users
rely on: in every cloud the scores of the 128 selected rows are pairwise distinct and non-zero and the 128th exceeds the 129th
(torch.topk's order among equals plays no part); no pair of critical points lies within 4 * 2^-24 of eps^2 in float64 (the labels do
not hang on float32 rounding); in every cloud the num_add largest cluster counts are pairwise distinct and exceed the next, or the
cloud has fewer than num_add clusters (argsort's order among equals plays no part); in every chosen cluster the point nearest to the
mean is nearest by more than float32 rounding; among the clouds there is at least one fallback draw; at least one cloud succeeds, one
never does and one cloud's weight moves both ways.

    python tests/golden/make_golden_objects.py
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
SEED = int(os.environ.get("OBJECTS_GOLDEN_SEED", "7"))
SEED_CLOUDS, CLOUDS = 313, [1, 2, 3, 5]
SHIFT = [int(x) for x in os.environ.get("OBJECTS_GOLDEN_SHIFT", "1,13,12,5").split(",")]
B, K, NUM_ADD, OBJ_NUM_P, BINARY_STEP, NUM_ITER, LR = 4, 192, 3, 64, 3, 20, 1e-2
INIT_WEIGHT, MAX_WEIGHT, SCALING, NUM_CRI, EPS = 5., 40., 0.3, 128, 0.2
ADJUSTED_LINE = 353                                                    # Add_Objects.py: torch.cuda.empty_cache() behind the adjustment loop


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
    sys.modules["util"].pointnet_utils = by_path("util.pointnet_utils", os.path.join(REF, "util", "pointnet_utils.py"))
    ref_net = by_path("ref_pointnet", os.path.join(REF, "model", "pointnet.py"))
    ref_obj = by_path("ref_add_objects", os.path.join(REF, "attack", "CW", "Add_Objects.py"))
    ref_adv = by_path("ref_adv_utils", os.path.join(REF, "attack", "util", "adv_utils.py"))
    ref_dist = by_path("ref_dist_utils", os.path.join(REF, "attack", "util", "dist_utils.py"))
    object_raw = np.load(os.path.join(REF, "data", "airplane.npy"))
    assert object_raw.shape == (1024, 3) and object_raw.dtype == np.float32

    sd = PO.make_calibrated_weights(0, False)
    model = torch.nn.DataParallel(ref_net.PointNetCls(k=40, feature_transform=False))
    model.load_state_dict(PO.reference_state_dict(sd))
    net = model.module.eval()
    data = np.ascontiguousarray(bench.synth_clouds(6, seed=SEED_CLOUDS)[CLOUDS, :K], dtype=np.float32)
    with torch.no_grad():
        pred = net(torch.from_numpy(data).transpose(1, 2).contiguous())[0].argmax(1).numpy()
    target = (pred + np.array(SHIFT)) % 40

    # the selection must not hang on torch.topk's order among equals
    x = torch.from_numpy(data).transpose(1, 2).contiguous().requires_grad_()
    torch.nn.functional.cross_entropy(net(x)[0], torch.from_numpy(target).long()).backward()
    score = torch.sum(x.grad ** 2, dim=1).numpy()                      # [B, K]
    for b in range(B):
        s = np.sort(score[b])[::-1]
        print("cloud %d: %d non-zero scores, selected %.3e .. %.3e" % (b, int((s > 0).sum()), s[0], s[NUM_CRI - 1]))
        assert s[NUM_CRI - 1] > 0 and len(set(s[:NUM_CRI].tolist())) == NUM_CRI and s[NUM_CRI - 1] > s[NUM_CRI], "ties in the selection"

    kept = {"cri": [], "labels": [], "choice": [], "centers": [], "randn": [], "rand": [], "history": []}
    randn, rand_like, choice = torch.randn, torch.rand_like, np.random.choice
    get_cri, dbscan_cls = ref_obj.get_critical_points, ref_obj.DBSCAN

    def keeping_randn(*a, **k):
        r = randn(*a, **k)
        kept["randn"].append(r.clone())
        return r

    def keeping_rand_like(*a, **k):
        r = rand_like(*a, **k)
        kept["rand"].append(r.clone())
        return r

    def keeping_choice(a, size=None, replace=True, p=None):
        kept["choice"].append((int(a), int(size), bool(replace)))
        return choice(a, size, replace=replace, p=p)

    def keeping_cri(*a, **k):
        r = get_cri(*a, **k)
        kept["cri"].append(r.detach().numpy().transpose(0, 2, 1).copy())
        return r

    class KeepingDBSCAN(dbscan_cls):
        def fit_predict(self, X, *a, **k):
            r = super().fit_predict(X, *a, **k)
            kept["labels"].append(np.asarray(r).copy())
            return r

    def tracer(frame, event, arg):
        if frame.f_code.co_name != "attack":
            return None

        def local(frame, event, arg):
            if event == "line" and frame.f_lineno == ADJUSTED_LINE:
                f = frame.f_locals
                kept["history"].append(np.stack([f["current_weight"], f["lower_bound"], f["upper_bound"]], 1).copy())
            return local
        return local

    np.random.seed(SEED)                                               # the script's set_seed, before the constructor's shuffles
    torch.manual_seed(SEED)
    attacker = ref_obj.CWAddObjects(net, ref_adv.LogitsAdvLoss(kappa=0.), ref_dist.L2ChamferDist(NUM_ADD, 'adv2ori', 0.2),
                                    object_pc=object_raw.copy(), attack_lr=LR, init_weight=INIT_WEIGHT, max_weight=MAX_WEIGHT,
                                    binary_step=BINARY_STEP, num_iter=NUM_ITER, num_add=NUM_ADD, obj_num_p=OBJ_NUM_P, scaling=SCALING)
    objects = np.asarray(attacker.object_pc).copy()
    assert objects.shape == (NUM_ADD, OBJ_NUM_P, 3) and objects.dtype == np.float64
    init = attacker._init_centers

    def keeping_init(*a, **k):
        r = init(*a, **k)
        kept["centers"].append(np.asarray(r).copy())
        return r

    attacker._init_centers = keeping_init
    torch.randn, torch.rand_like, np.random.choice = keeping_randn, keeping_rand_like, keeping_choice
    ref_obj.get_critical_points, ref_obj.DBSCAN = keeping_cri, KeepingDBSCAN
    sys.settrace(tracer)
    try:
        o_bestdist, o_bestattack, success_num = attacker.attack(torch.from_numpy(data), torch.from_numpy(target))
    finally:
        sys.settrace(None)
        torch.randn, torch.rand_like, np.random.choice = randn, rand_like, choice
        ref_obj.get_critical_points, ref_obj.DBSCAN = get_cri, dbscan_cls
    A = NUM_ADD * OBJ_NUM_P
    assert len(kept["randn"]) == 2 * BINARY_STEP and len(kept["rand"]) == BINARY_STEP and len(kept["history"]) == BINARY_STEP
    assert all(tuple(d.shape) == (B, NUM_ADD, OBJ_NUM_P, 3) for d in kept["randn"][0::2])
    assert all(tuple(d.shape) == (B, NUM_ADD, 3) for d in kept["randn"][1::2] + kept["rand"])
    assert len(kept["cri"]) == 1 and len(kept["labels"]) == B and len(kept["centers"]) == 1
    cri, labels, centers = kept["cri"][0].astype(np.float32), np.stack(kept["labels"]).astype(np.int32), kept["centers"][0]
    assert cri.shape == (B, NUM_CRI, 3) and labels.shape == (B, NUM_CRI) and centers.shape == (B, NUM_ADD, 3)
    assert centers.dtype == np.float32

    for b in range(B):
        p = cri[b].astype(np.float64)
        d2 = ((p[:, None] - p[None]) ** 2).sum(2)
        margin = np.abs(d2 - EPS * EPS).min()
        ids, cnt = np.unique(labels[b][labels[b] >= 0], return_counts=True)
        counts = np.sort(cnt)[::-1]
        print("cloud %d: cluster counts %s, %d outliers, nearest pair to eps: |d2 - eps2| = %.2e" % (b, counts.tolist(), int((labels[b] < 0).sum()),
                                                                                                    margin))
        assert margin > 4 * 2.0 ** -24, "a pair of critical points within float32 rounding of eps"
        top = counts[:NUM_ADD + 1]
        assert len(counts) < NUM_ADD or (len(set(top[:NUM_ADD].tolist())) == NUM_ADD and (len(top) == NUM_ADD or top[NUM_ADD - 1] > top[NUM_ADD])), \
            "tied cluster counts at the boundary"
        for one in ids[np.argsort(cnt, kind="stable")[-NUM_ADD:]]:
            q = p[labels[b] == one]
            dm = np.sort(((q - q.mean(0)) ** 2).sum(1))
            assert len(dm) == 1 or dm[1] - dm[0] > 1e-6, "two cluster points equally near the mean"
    print("draws:", kept["choice"])
    assert len(kept["choice"]) >= 1 and all(size == 1 for _, size, _ in kept["choice"]), "the clouds must show a fallback draw"

    noise_obj = np.stack([(d * 1e-7).numpy().reshape(B, A, 3) for d in kept["randn"][0::2]]).astype(np.float32)
    noise_shift = np.stack([(d * 1e-7).numpy() for d in kept["randn"][1::2]]).astype(np.float32)
    angles0 = np.stack([(d.float() * np.pi).numpy()[..., 0] for d in kept["rand"]]).astype(np.float32)
    history = np.stack(kept["history"])                                # [binary_step, B, 3]
    lower = history[-1, :, 1]
    roles = []
    for b in range(B):
        ups = sum(history[s, b, 1] > (history[s - 1, b, 1] if s else 0.) for s in range(BINARY_STEP))
        roles.append("never" if lower[b] == 0 else "success" if ups == BINARY_STEP else "up_down")
        print("cloud %d: prediction %d, target %d, role %s, o_bestdist %.6g, weights %s" % (b, pred[b], target[b], roles[-1], o_bestdist[b],
                                                                                         history[:, b, 0].tolist()))
    print("success_num", success_num)
    assert success_num >= 1, "no cloud succeeds: use another seed or shift"
    assert "never" in roles, "every cloud succeeds: use another seed or shift"
    assert "up_down" in roles, "no cloud's weight goes both ways: use another seed or shift"
    assert o_bestattack.shape == (B, K + A, 3) and np.array_equal(o_bestattack[:, :K].astype(np.float32), data)
    rec = {"data": data, "target": target.astype(np.int64), "num_add": np.int32(NUM_ADD), "obj_num_p": np.int32(OBJ_NUM_P),
           "binary_step": np.int32(BINARY_STEP), "num_iter": np.int32(NUM_ITER), "attack_lr": np.float64(LR), "seed": np.int64(SEED),
           "init_weight": np.float64(INIT_WEIGHT), "max_weight": np.float64(MAX_WEIGHT), "scaling": np.float64(SCALING),
           "object_raw": object_raw, "objects": objects, "cri": cri, "labels": labels, "centers": centers, "noise_obj": noise_obj,
           "noise_shift": noise_shift, "angles0": angles0, "history": history, "o_bestdist": np.asarray(o_bestdist, np.float64),
           "o_bestattack": np.asarray(o_bestattack, np.float64), "success_num": np.int64(success_num), "roles": np.array(roles)}
    if write:
        path = os.path.join(HERE, "objects_golden.npz")
        np.savez_compressed(path, **rec)
        print("wrote", path, os.path.getsize(path), "bytes")
    return rec


if __name__ == "__main__":
    main()
