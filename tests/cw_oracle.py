"""Test oracle of the CW point-perturbation attack (include/ifd_cw.h): CWPerturb.attack (baselines/attack/CW/Perturb.py:43-175) with
L2Dist (baselines/attack/util/dist_utils.py:16-36) restated one cloud at a time.  The adversarial loss, its gradient and the
prediction come from atk_oracle.run_cloud; the distance term's gradient from autograd on sqrt(sum (adv - ori)^2) * weight.float();
the update from the real torch.optim.Adam on the CPU, its state (step, exp_avg, exp_avg_sq) put in from outside so that one
iteration can be taken from any state.  Runs in float32 (the reference's rounding) and float64 (the yardstick).

The reference's .mean() over its batch is ``scale`` = 1 / B_ref on both loss terms.  Where dist == 0 the distance term is left
out, as the header says (autograd gives NaN there; the reference's start noise keeps it away)."""
import numpy as np
import torch

import atk_oracle as AO


def fresh_record(K=None, dtype=np.float64):
    return {"bestdist": 1e10, "bestscore": -1, "o_bestdist": 1e10, "o_bestscore": -1,
            "o_bestattack": None if K is None else np.zeros((K, 3), dtype)}


def _rows(a, dtype):
    """[n,3] -> the reference's [1,3,n]."""
    return torch.as_tensor(np.asarray(a)).to(dtype).t()[None].contiguous()


def _back(a):
    return a.detach()[0].t().contiguous().numpy()


def step(grad_adv, pred, target, adv, ori, weight, m, v, t, lr, scale, record, dtype=torch.float64):
    """One iteration (Perturb.py:107-136 behind the forward pass) on one cloud, arrays [n,3].  grad_adv: scale * d adv_loss / d adv;
    t: the 1-based Adam step.  -> (adv', m', v', record', dist, dist * weight)."""
    p = _rows(adv, dtype).requires_grad_()
    o = _rows(ori, dtype)
    dist = torch.sqrt(torch.sum((p - o) ** 2, dim=[1, 2]))             # [1]
    d = dist.detach().numpy()[0]
    rec = dict(record)
    if d < rec["bestdist"] and pred == target:                          # Perturb.py:117-123
        rec["bestdist"], rec["bestscore"] = d, int(pred)
    if d < rec["o_bestdist"] and pred == target:
        rec["o_bestdist"], rec["o_bestscore"] = d, int(pred)
        rec["o_bestattack"] = np.array(np.asarray(adv), copy=True)
    w = torch.as_tensor([float(weight)]).float().to(dtype)             # L2Dist: weights.float()
    dl = dist * w
    g = _rows(grad_adv, dtype)
    if d > 0:
        (dl.sum() * scale).backward()
        g = g + p.grad
    p.grad = None
    opt = torch.optim.Adam([p], lr=lr, weight_decay=0.)                # Perturb.py:76
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": _rows(m, dtype), "exp_avg_sq": _rows(v, dtype)}
    p.grad = g.detach()
    opt.step()
    st = opt.state[p]
    return _back(p), _back(st["exp_avg"]), _back(st["exp_avg_sq"]), rec, d, dl.detach().numpy()[0]


def adjust(record, target, weight, lower, upper):
    """Perturb.py:154-162 and the reset of :74-75 -> (weight, lower, upper, record')."""
    if record["bestscore"] == target and record["bestscore"] != -1 and record["bestdist"] <= record["o_bestdist"]:
        lower = max(lower, weight)
    else:
        upper = min(upper, weight)
    rec = dict(record)
    rec["bestdist"], rec["bestscore"] = 1e10, -1
    return (lower + upper) / 2., lower, upper, rec


def attack(W, data, target, noise, dtype=torch.float64, binary_step=10, num_iter=500, lr=1e-2, init_weight=10., max_weight=80.,
           loss="logits", kappa=0., scale=None):
    """Free-running, cloud by cloud.  W: pointnet_oracle.to_torch(weights, dtype); data [B,K,3]; noise [binary_step,B,K,3] or None.
    -> dict: o_bestdist [B], o_bestattack [B,K,3], success [B] bool (lower > 0), success_num, history [binary_step,B,3] (weight,
    lower, upper behind every search step), first [B] (distance of the first state of search step 0 that reached the target,
    1e10 if none)."""
    B, K = np.asarray(data).shape[:2]
    npdt = np.float32 if dtype == torch.float32 else np.float64
    scale = 1.0 / B if scale is None else scale
    out = {"o_bestdist": np.full(B, 1e10), "o_bestattack": np.zeros((B, K, 3), npdt), "success": np.zeros(B, bool),
           "history": np.zeros((binary_step, B, 3)), "first": np.full(B, 1e10)}
    for b in range(B):
        ori = np.asarray(data[b]).astype(npdt)
        tg = int(target[b])
        weight, lower, upper = float(init_weight), 0., float(max_weight)
        rec = fresh_record(K, npdt)
        for s in range(binary_step):
            adv = ori if noise is None else ori + np.asarray(noise[s][b]).astype(npdt)
            m, v = np.zeros_like(ori), np.zeros_like(ori)
            for it in range(num_iter):
                r = AO.run_cloud(W, adv, tg, loss, kappa, scale, dtype=dtype)
                pred = int(r["logits"].argmax())
                last = adv
                adv, m, v, rec, d, _ = step(r["grad"], pred, tg, adv, ori, weight, m, v, it + 1, lr, scale, rec, dtype)
                if s == 0 and pred == tg and out["first"][b] == 1e10:
                    out["first"][b] = d
            weight, lower, upper, rec = adjust(rec, tg, weight, lower, upper)
            out["history"][s, b] = weight, lower, upper
        out["success"][b] = lower > 0
        out["o_bestdist"][b] = rec["o_bestdist"]
        out["o_bestattack"][b] = rec["o_bestattack"] if lower > 0 else last        # Perturb.py:169-170
    out["success_num"] = int(out["success"].sum())
    return out
