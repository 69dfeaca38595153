#!/usr/bin/env python
"""Times of the Perturb, kNN and Drop loops on the DGCNN, PointNet++ and PointConv victims (include/ifd_victim_atk.h) on one
MI355X, on 128 x 1024 bench.synth_clouds points.  Per victim:
  input_grad            the victim's gradient call alone
  perturb / knn / drop  one iteration (round) of the fused loop: the call with 11 iterations minus the call with 1, over 10
  *_step                the step kernel's call alone (cw_step, knn_step, drop_step), and its share of the fused iteration
  *_host                one iteration driven from the host as attack.py drives it: input_grad(want_aux=("pred", "loss")) + the step
Warmed, synchronised, median of --reps (scripts/time_cls.py timed).

--parent_lib PATH: a libifd.so built from the parent commit.  Each victim's gradient (PointNet's too) is then timed through the
raw C call on both libraries in one process, the same inputs, alternating this / parent --rounds times, each timing the median of
--reps calls.  The kernels are untouched, so the two must agree within the run-to-run spread, which is recorded: per library the
rounds' medians, their minimum and maximum.

    python scripts/time_victim_atk.py [--clouds 128] [--points 1024] [--reps 7] [--parent_lib P] [--json profiles/victim_atk_time.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DG_K = 20


def victims():
    import dgcnn_oracle as DO
    import pointconv_oracle as PCO
    import pointnet2_oracle as PO
    import pointnet_oracle as PNO
    import ifdefense_amd as I
    W = I.weights
    return {"pointnet": (lambda: I.Classifier(W.pack_state_dict(PNO.make_calibrated_weights(0), "pointnet"), device="cuda:0")),
            "dgcnn": (lambda: I.DgcnnClassifier(W.pack_state_dict(DO.make_calibrated_weights(0, DG_K), "dgcnn"), k=DG_K, device="cuda:0")),
            "pointnet2": (lambda: I.PointNet2Classifier(W.pack_state_dict(PO.make_calibrated_weights(0), "pointnet2"), device="cuda:0")),
            "pointconv": (lambda: I.PointConvClassifier(W.pack_state_dict(PCO.make_calibrated_weights(0), "pointconv"), device="cuda:0"))}


def loops(net, pc, tg, label, reps):
    """The figures of one victim (module docstring) -> dict of milliseconds and shares."""
    from time_cls import timed
    B, K = int(pc.shape[0]), int(pc.shape[1])
    scale = 1.0 / B
    noise = torch.randn(1, B, K, 3, generator=torch.Generator().manual_seed(1)).cuda() * 1e-7
    r = {}
    r["input_grad_ms"], _ = timed(lambda: net.input_grad(pc, tg, scale=scale), reps)

    def per_iteration(call):
        one, _ = timed(lambda: call(1), reps)
        eleven, _ = timed(lambda: call(11), reps)
        return (eleven - one) / 10

    r["perturb_iteration_ms"] = per_iteration(lambda n: net.cw_perturb_attack(pc, tg, noise, scale=scale, binary_step=1, num_iter=n))
    r["knn_iteration_ms"] = per_iteration(lambda n: net.knn_attack(pc, tg, None, noise[0], scale=scale, num_iter=n))
    r["drop_round_ms"] = per_iteration(lambda n: net.drop_attack(pc, label, 5 * n, 5, 1., scale))
    # the step calls alone, on state that a first iteration left
    adv = (pc + noise[0]).contiguous()
    grad, aux = net.input_grad(adv, tg, scale=scale, want_aux=("pred", "loss"))
    st = net.cw_state(B, K)
    r["cw_step_ms"], _ = timed(lambda: net.cw_step(st, grad, aux["pred"], tg, adv, pc, 1, 1e-2, scale, loss=aux["loss"]), reps)
    m, v = torch.zeros_like(pc), torch.zeros_like(pc)
    r["knn_step_ms"], _ = timed(lambda: net.knn_step(grad, adv, pc, m, v, 1, 1e-3, scale, loss=aux["loss"]), reps)
    full = torch.full((B,), K, dtype=torch.int32, device=pc.device)

    def drop_step():
        cur, n = pc.clone(), full.clone()
        net.drop_step(grad, cur, n, 5)
    def copies():
        pc.clone(), full.clone()
    both, _ = timed(drop_step, reps)
    clone, _ = timed(copies, reps)
    r["drop_step_ms"] = both - clone

    def host_perturb():
        g, a = net.input_grad(adv, tg, "logits", 0., scale, want_aux=("pred", "loss"))
        net.cw_step(st, g, a["pred"], tg, adv, pc, 1, 1e-2, scale, loss=a["loss"])

    def host_knn():
        g, a = net.input_grad(adv, tg, "logits", 15., scale, want_aux=("pred", "loss"))
        net.knn_step(g, adv, pc, m, v, 1, 1e-3, scale, loss=a["loss"])

    def host_drop():
        cur, n = pc.clone(), full.clone()
        g, a = net.input_grad(cur, label, "cross_entropy", 0., scale, n_points=n, want_aux=("pred",))
        net.drop_step(g, cur, n, 5)
    r["perturb_host_iteration_ms"], _ = timed(host_perturb, reps)
    r["knn_host_iteration_ms"], _ = timed(host_knn, reps)
    hd, _ = timed(host_drop, reps)
    r["drop_host_round_ms"] = hd - clone
    for kind, step, it in (("perturb", "cw_step_ms", "perturb_iteration_ms"), ("knn", "knn_step_ms", "knn_iteration_ms"),
                           ("drop", "drop_step_ms", "drop_round_ms")):
        r[kind + "_step_share"] = r[step] / r[it]
    return r


# ---- this commit's gradient against the parent's, through the raw C calls of two libraries in one process
def raw_grad_calls(lib_path, pc, tg):
    """{victim: a function that enqueues one gradient call of the library at lib_path}, and the contexts to destroy."""
    from ifdefense_amd import _lib, weights as W
    import dgcnn_oracle as DO
    import pointconv_oracle as PCO
    import pointnet2_oracle as PO
    import pointnet_oracle as PNO
    # RTLD_DEEPBIND: a second libifd.so must find its own launchers and kernels, not the like-named ones of the first
    lib = C.CDLL(lib_path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)
    tables = {**_lib.SIGNATURES, **_lib.CLS_SIGNATURES, **_lib.ATK_SIGNATURES, **_lib.DGCNN_SIGNATURES, **_lib.DGCNN_ATK_SIGNATURES,
              **_lib.PN2_SIGNATURES, **_lib.PN2_ATK_SIGNATURES, **_lib.PC_SIGNATURES, **_lib.PC_ATK_SIGNATURES}
    for name in ("ifd_destroy", "ifd_cls_create", "ifd_cls_input_grad", "ifd_dgcnn_create", "ifd_dgcnn_input_grad", "ifd_pn2_create",
                 "ifd_pn2_input_grad", "ifd_pc_create", "ifd_pc_input_grad"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = tables[name]
    B, K = int(pc.shape[0]), int(pc.shape[1])
    grad = torch.empty_like(pc)
    t32 = tg.to(torch.int32).contiguous()
    packs = {"pointnet": W.pack_state_dict(PNO.make_calibrated_weights(0), "pointnet"),
             "dgcnn": W.pack_state_dict(DO.make_calibrated_weights(0, DG_K), "dgcnn"),
             "pointnet2": W.pack_state_dict(PO.make_calibrated_weights(0), "pointnet2"),
             "pointconv": W.pack_state_dict(PCO.make_calibrated_weights(0), "pointconv")}
    packs = {k: np.ascontiguousarray(v, np.float32) for k, v in packs.items()}
    ctx = {"pointnet": lib.ifd_cls_create(packs["pointnet"].ctypes.data, packs["pointnet"].size, 0, 0, 40, 0),
           "dgcnn": lib.ifd_dgcnn_create(packs["dgcnn"].ctypes.data, packs["dgcnn"].size, DG_K, 40, 0),
           "pointnet2": lib.ifd_pn2_create(packs["pointnet2"].ctypes.data, packs["pointnet2"].size, 40, 0),
           "pointconv": lib.ifd_pc_create(packs["pointconv"].ctypes.data, packs["pointconv"].size, 40, 0)}
    assert all(ctx.values()), "a context of %s could not be made" % lib_path
    common = (B, K, t32.data_ptr(), 0, 0.0, 1.0 / B, grad.data_ptr(), None, None)

    def call(name, fn, *front):
        def run():
            rc = fn(ctx[name], pc.data_ptr(), None, *front, *common)
            assert rc == 0, (name, rc)
        return run
    calls = {"pointnet": call("pointnet", lib.ifd_cls_input_grad), "dgcnn": call("dgcnn", lib.ifd_dgcnn_input_grad),
             "pointnet2": call("pointnet2", lib.ifd_pn2_input_grad, None), "pointconv": call("pointconv", lib.ifd_pc_input_grad, None)}
    return calls, grad, (t32, lib, ctx)


def against_parent(this_lib, parent_lib, pc, tg, reps, rounds):
    from time_cls import timed
    a_calls, a_grad, a_keep = raw_grad_calls(this_lib, pc, tg)
    b_calls, b_grad, b_keep = raw_grad_calls(parent_lib, pc, tg)
    assert a_keep[1]._handle != b_keep[1]._handle, "--parent_lib is the library of this commit"
    out = {}
    for name in a_calls:
        a_calls[name]()
        b_calls[name]()
        torch.cuda.synchronize()
        same = bool(torch.equal(a_grad, b_grad))
        ts = {"this": [], "parent": []}
        for _ in range(rounds):
            ts["this"].append(timed(a_calls[name], reps)[0])
            ts["parent"].append(timed(b_calls[name], reps)[0])
        out[name] = {"same_bits": same}
        for who, v in ts.items():
            out[name][who] = {"rounds_ms": v, "median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}
        out[name]["this_over_parent"] = out[name]["this"]["median_ms"] / out[name]["parent"]["median_ms"]
        out[name]["spread"] = max((max(v) - min(v)) / statistics.median(v) for v in ts.values())
        print("%-10s gradient: this %8.3f ms [%.3f, %.3f] | parent %8.3f ms [%.3f, %.3f] | ratio %.4f, spread %.4f, same bits: %s"
              % (name, out[name]["this"]["median_ms"], min(ts["this"]), max(ts["this"]), out[name]["parent"]["median_ms"],
                 min(ts["parent"]), max(ts["parent"]), out[name]["this_over_parent"], out[name]["spread"], same))
    for keep in (a_keep, b_keep):
        for c in keep[2].values():
            keep[1].ifd_destroy(c)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=128)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent_lib", default="")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    import bench
    from ifdefense_amd import _lib
    pc = torch.from_numpy(bench.synth_clouds(a.clouds)[:, :a.points].copy()).cuda()
    B = int(pc.shape[0])
    res = {"clouds": B, "points": int(pc.shape[1]), "reps": a.reps, "dgcnn_k": DG_K, "device": torch.cuda.get_device_name(0), "victims": {}}
    tg = None
    for name, make in victims().items():
        if name == "pointnet":
            continue
        with make() as net:
            label = net.predict(pc)
            tg = (label + 1) % 40
            res["victims"][name] = r = loops(net, pc, tg, label, a.reps)
        print("%-10s grad %8.3f ms | Perturb it. %8.3f (step %.3f = %.1f %%, host-driven %8.3f) | kNN it. %8.3f (step %.3f = %.1f %%, host-driven "
              "%8.3f) | Drop round %8.3f (step %.3f = %.1f %%, host-driven %8.3f)"
              % (name, r["input_grad_ms"], r["perturb_iteration_ms"], r["cw_step_ms"], 100 * r["perturb_step_share"],
                 r["perturb_host_iteration_ms"], r["knn_iteration_ms"], r["knn_step_ms"], 100 * r["knn_step_share"], r["knn_host_iteration_ms"],
                 r["drop_round_ms"], r["drop_step_ms"], 100 * r["drop_step_share"], r["drop_host_round_ms"]))
    if a.parent_lib:
        res["rounds"] = a.rounds
        res["gradient_this_commit_vs_parent"] = against_parent(_lib.LIB_PATH, a.parent_lib, pc, tg, a.reps, a.rounds)
    else:
        res["gradient_this_commit_vs_parent"] = "not measured (no --parent_lib)"
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
