"""Test oracle of the saliency Drop attack (include/ifd_drop.h): one round of baselines/attack/Saliency/Drop.py:76-95 restated op
for op in torch (float32: the reference's rounding; float64: the yardstick), the header's formula in plain numpy float32, the
header's selection (a total order) with its stable compaction, the free-running attack on atk_oracle.run_cloud's gradients, and the
margin rule by which a round's discrete outcome is judged: the k-th and the (k + 1)-th saliency must be further apart than the two
oracles' rounding can move them."""
import numpy as np
import torch

import atk_oracle as AO

# the GPU parity cases (n, B, num_drop, k): clouds bench.synth_clouds(B, seed=SEED)[:, :n] normalised, calibrated weights (0, False),
# labels = the float64 predictions, scale = 1 / B
SEED = 91
CASES = [(64, 8, 12, 5), (33, 8, 7, 3), (300, 4, 10, 5), (6, 8, 5, 5), (2, 8, 1, 1), (1024, 3, 200, 5)]


def saliency(points, grad, dtype=torch.float32, alpha=1):
    """Drop.py:78-88 on one cloud: points, grad [n,3] -> (saliency [n], centre [3]) as numpy arrays of ``dtype``."""
    data = torch.as_tensor(np.asarray(points)).to(dtype).t()[None].contiguous()            # [1,3,n]
    g = torch.as_tensor(np.asarray(grad)).to(dtype).t()[None].contiguous()
    center = torch.median(data, dim=-1)[0].clone().detach()
    r = torch.sum((data - center[:, :, None]) ** 2, dim=1) ** 0.5
    s = -1. * (r ** alpha) * torch.sum((data - center[:, :, None]) * g, dim=1)
    return s[0].numpy(), center[0].numpy()


def lower_median(x):
    """The element of rank (n - 1) // 2 in ascending order; among equal values the lower row first (decides a zero's sign only)."""
    x = np.asarray(x)
    return np.sort(x, kind="stable")[(len(x) - 1) // 2]


def saliency_f32_plain(points, grad, alpha=1.):
    """The header's SALIENCY in numpy float32, term by term -> (saliency [n], centre [3])."""
    f = np.float32
    x, g = np.asarray(points, f), np.asarray(grad, f)
    c = np.array([lower_median(x[:, j]) for j in range(3)], f)
    d = (x - c[None]).astype(f)
    sq = (d * d).astype(f)
    r = np.sqrt(((sq[:, 0] + sq[:, 1]).astype(f) + sq[:, 2]).astype(f)).astype(f)
    p = (d * g).astype(f)
    dot = ((p[:, 0] + p[:, 1]).astype(f) + p[:, 2]).astype(f)
    ra = r if float(alpha) == 1. else np.power(r, f(alpha)).astype(f)
    return (-(ra * dot)).astype(f), c


def select(s, k):
    """The k rows in drop order: saliency descending, the lowest row first among equal values."""
    s = np.asarray(s)
    order = sorted(range(len(s)), key=lambda i: (-float(s[i]), i))
    return np.array(order[:k], np.int64)


def step(points, s, k, index=None):
    """Selection by the header's total order on the saliencies ``s`` plus stable compaction -> dict: points [n - k,3], index
    [n - k] (None without one), dropped [k] in drop order, keep: the surviving rows, ascending."""
    points = np.asarray(points)
    dropped = select(s, k)
    keep = np.setdiff1d(np.arange(len(points)), dropped)                # ascending: the survivors keep their order
    return {"points": points[keep], "index": None if index is None else np.asarray(index)[keep], "dropped": dropped, "keep": keep}


def round_margin(s32, s64, k):
    """(gap, e_sal) of one cloud state: gap = the float64 saliency of rank k minus that of rank k + 1 (1-based, descending); e_sal =
    max |float32 oracle - float64 oracle| of the saliencies, gradients included."""
    top = np.sort(np.asarray(s64, np.float64))[::-1]
    return float(top[k - 1] - top[k]), float(np.abs(np.asarray(s32, np.float64) - s64).max())


def is_clear(gap, e_sal):
    """The project's usual rule: each side may move a value by 4 e."""
    return gap > 8 * e_sal


def attack(W, pts, label, num_drop, k, alpha=1., scale=1., dtype=torch.float64, W_other=None, e_act=None):
    """The free-running loop on one cloud [n,3] in ``dtype``: Drop.py:56-107 with the header's selection.  -> dict: points (the
    result), kept (rows of pts), correct, logits, rounds: per round {n, k, dropped (rows of the state), saliency, center, grad}
    and, where W_other (the weights in the other precision) is given, gap / e_sal / clear of the state; with e_act (atk_oracle
    layer errors) also whole_out: atk_oracle.row_exclusion takes the whole cloud out."""
    other = torch.float32 if dtype == torch.float64 else torch.float64
    cur = np.asarray(pts, np.float32)
    kept = np.arange(len(cur))
    rounds = []
    done = 0
    while done < num_drop:
        kk = min(k, num_drop - done)
        r = AO.run_cloud(W, cur, label, "cross_entropy", 0., scale, dtype=dtype)
        s, c = saliency(cur, r["grad"], dtype, alpha)
        rec = {"n": len(cur), "k": kk, "saliency": s, "center": c, "grad": r["grad"], "points": cur}
        if W_other is not None:
            ro = AO.run_cloud(W_other, cur, label, "cross_entropy", 0., scale, dtype=other)
            so, _ = saliency(cur, ro["grad"], other, alpha)
            s32, s64 = (so, s) if dtype == torch.float64 else (s, so)
            rec["gap"], rec["e_sal"] = round_margin(s32, s64, kk)
            rec["clear"] = is_clear(rec["gap"], rec["e_sal"])
        if e_act is not None:
            rec["whole_out"] = bool(AO.row_exclusion(r, e_act, "cross_entropy")[0])
        st = step(cur, s, kk, kept)
        rec["dropped"] = st["dropped"]
        rounds.append(rec)
        cur, kept = st["points"], st["index"]
        done += kk
    import pointnet_oracle as PO
    logits = PO.forward(W, [cur], dtype=dtype)[0][0].numpy()
    return {"points": cur, "kept": kept, "logits": logits, "pred": int(logits.argmax()), "correct": int(logits.argmax()) == int(label),
            "rounds": rounds}


def case_inputs(n, B, seed=SEED):
    """-> (clouds [B,n,3] float32, labels [B] = the float64 predictions, the weight dict) of a parity case."""
    import bench
    import pointnet_oracle as PO
    from ifdefense_amd.inference import normalize_points_np
    sd = PO.make_calibrated_weights(0, False)
    pts = np.stack([normalize_points_np(c[:n]) for c in bench.synth_clouds(B, seed=seed)]).astype(np.float32)
    labels = PO.forward(PO.to_torch(sd, torch.float64), pts, dtype=torch.float64)[0].argmax(1).numpy().astype(np.int64)
    return pts, labels, sd


_CASE_RUNS = {}


def case_run(case):
    """The float64 oracle's free run of a parity case with every round's margin, computed once and shared: -> (pts, labels, sd, [one
    attack() dict per cloud])."""
    if case not in _CASE_RUNS:
        import pointnet_oracle as PO
        n, B, num_drop, k = case
        pts, labels, sd = case_inputs(n, B)
        W32, W64 = PO.to_torch(sd, torch.float32), PO.to_torch(sd, torch.float64)
        r32 = [AO.run_cloud(W32, c, t, "cross_entropy", 0., 1. / B, dtype=torch.float32) for c, t in zip(pts, labels)]
        r64 = [AO.run_cloud(W64, c, t, "cross_entropy", 0., 1. / B, dtype=torch.float64) for c, t in zip(pts, labels)]
        e_act = AO.layer_errors(r32, r64)
        runs = [attack(W64, c, t, num_drop, k, 1., 1. / B, torch.float64, W_other=W32, e_act=e_act) for c, t in zip(pts, labels)]
        _CASE_RUNS[case] = (pts, labels, sd, runs)
    return _CASE_RUNS[case]
