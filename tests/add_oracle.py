"""Test oracle of the CW point-adding attack (include/ifd_add.h): CWAdd.attack and get_critical_points (baselines/attack/CW/Add.py)
with ChamferDist('adv2ori') / HausdorffDist('adv2ori') (baselines/attack/util/dist_utils.py over baselines/util/set_distance.py)
restated one cloud at a time, in the reference's own form: the pairwise distances expanded from three bmm's, torch.min over the
originals, torch.mean / torch.max over the added points, autograd for the distance term's gradient, the real torch.optim.Adam on
the CPU with its state put in from outside, the record and the adjustment of cw_oracle.  The adversarial loss, its gradient and the
prediction come from atk_oracle.run_cloud on the concatenated cloud.  Runs in float32 (the reference's rounding) and float64 (the
yardstick).

The reference's .mean() over its batch is ``scale`` = 1 / B_ref on both loss terms and on the selection's cross-entropy.

Discrete decisions (which original is nearest, which added point is farthest) cannot be judged where float32 rounding may turn
them: ``exclusions`` marks those rows and clouds from the float64 oracle and the float32 oracle's measured error e alone."""
import numpy as np
import torch

import atk_oracle as AO
import cw_oracle as CO

KINDS = ("chamfer", "hausdorff")
fresh_record = CO.fresh_record
adjust = CO.adjust


def _b(a, dtype):
    """[n,3] -> [1,n,3], what the set distances take; a copy (Adam steps in place)."""
    return torch.as_tensor(np.asarray(a)).to(dtype)[None].clone()


def pairwise(x, y):
    """The reference's expanded form of the squared distances (set_distance.py batch_pairwise_dist): x [1,nx,3], y [1,ny,3] ->
    P [1,nx,ny] = (|x|^2 + |y|^2) - 2 x.y, the norms read off the diagonals of x x^T and y y^T: three bmm's."""
    nx = torch.diagonal(torch.bmm(x, x.transpose(1, 2)), dim1=1, dim2=2)
    ny = torch.diagonal(torch.bmm(y, y.transpose(1, 2)), dim1=1, dim2=2)
    return nx[:, :, None] + ny[:, None, :] - 2 * torch.bmm(x, y.transpose(1, 2))


def set_distance(adv, ori, kind):
    """adv [1,A,3], ori [1,n,3] tensors -> (dist [1], min_p [A], j(p) [A], arg-max p or -1): 'adv2ori' of ChamferDistance /
    HausdorffDistance.forward(preds=adv, gts=ori)."""
    P = pairwise(ori, adv)                                             # [1, n, A]
    mins, nn = torch.min(P, 1)                                         # [1, A]
    if kind == "chamfer":
        return torch.mean(mins, dim=1), mins[0], nn[0], -1
    if kind != "hausdorff":
        raise ValueError(kind)
    d, far = torch.max(mins, dim=1)
    return d, mins[0], nn[0], int(far[0])


def closed_form_grad(adv, ori, kind, weight, scale, nn, far):
    """The header's step 4: scale * (float)weight * (2 / A) (adv_p - ori_j(p)) for Chamfer, scale * (float)weight * 2 (adv_p -
    ori_j(p)) on the arg-max point alone for Hausdorff; float64, arrays [A,3]."""
    adv, ori = np.asarray(adv, np.float64), np.asarray(ori, np.float64)
    d = adv - ori[np.asarray(nn)]
    w = float(np.float32(weight))
    if kind == "chamfer":
        return scale * w * (2.0 / len(adv)) * d
    g = np.zeros_like(d)
    g[far] = scale * w * 2.0 * d[far]
    return g


def step(kind, grad_adv, pred, target, adv, ori, weight, m, v, t, lr, scale, record, dtype=torch.float64):
    """One iteration (Add.py:146-177 behind the forward pass) on one cloud.  adv, grad_adv, m, v: [A,3] (grad_adv: the added rows of
    scale * d adv_loss / d cat); ori [n,3]; t: the 1-based Adam step.
    -> (adv', m', v', record', dist, dist * weight, diag {min_p, nn, far, dist_grad})."""
    p = _b(adv, dtype).requires_grad_()
    o = _b(ori, dtype)
    dist, mins, nn, far = set_distance(p, o, kind)
    d = dist.detach().numpy()[0]
    rec = dict(record)
    if d < rec["bestdist"] and pred == target:                          # Add.py:157-163
        rec["bestdist"], rec["bestscore"] = d, int(pred)
    if d < rec["o_bestdist"] and pred == target:
        rec["o_bestdist"], rec["o_bestscore"] = d, int(pred)
        rec["o_bestattack"] = np.array(np.asarray(adv), copy=True)
    w = torch.as_tensor([float(weight)]).float().to(dtype)             # ChamferDist / HausdorffDist: weights.float()
    dl = dist * w
    (dl.sum() * scale).backward()
    dg = p.grad.detach().clone()
    g = _b(grad_adv, dtype) + dg
    p.grad = None
    opt = torch.optim.Adam([p], lr=lr, weight_decay=0.)                # Add.py:113
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": _b(m, dtype), "exp_avg_sq": _b(v, dtype)}
    p.grad = g.detach()
    opt.step()
    st = opt.state[p]
    diag = {"min_p": mins.detach().numpy(), "nn": nn.numpy(), "far": far, "dist_grad": dg[0].numpy()}
    return p.detach()[0].numpy(), st["exp_avg"][0].numpy(), st["exp_avg_sq"][0].numpy(), rec, d, dl.detach().numpy()[0], diag


def exclusions(adv, ori, e, kind):
    """From float64 alone and e, the float32 oracle's measured error of a distance: (rows_out [A] bool - the two nearest originals
    within 8 e of each other; cloud_out - for Hausdorff, the two largest min_p within 8 e of each other)."""
    a, o = np.asarray(adv, np.float64), np.asarray(ori, np.float64)
    P = ((a[:, None, :] - o[None, :, :]) ** 2).sum(2)                  # [A, n]
    part = np.partition(P, 1, axis=1) if P.shape[1] > 1 else np.concatenate([P, np.full_like(P, np.inf)], 1)
    rows_out = part[:, 1] - part[:, 0] <= 8 * e
    cloud_out = False
    if kind == "hausdorff" and len(a) > 1:
        top = np.sort(P.min(1))
        cloud_out = bool(top[-1] - top[-2] <= 8 * e)
    return rows_out, cloud_out


def scores(grad, dtype=np.float32):
    """(gx*gx + gy*gy) + gz*gz in `dtype`, [n,3] -> [n]: torch.sum(grad ** 2, dim=1) of the reference, in the header's order."""
    g = np.asarray(grad).astype(dtype)
    return ((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(dtype)


def select(grad, num_add, dtype=np.float32):
    """The header's total order: descending score, the lowest index first among equal scores - numpy's stable sort -> idx [num_add]."""
    return np.argsort(-scores(grad, dtype), kind="stable")[:num_add]


def critical_points(W, pts, target, num_add, scale, dtype=torch.float64):
    """get_critical_points (Add.py:14-42) on one cloud -> (cri [num_add,3], idx, scores [n])."""
    npdt = np.float32 if dtype == torch.float32 else np.float64
    r = AO.run_cloud(W, pts, int(target), "cross_entropy", 0., scale, dtype=dtype)
    idx = select(r["grad"], num_add, npdt)
    return np.asarray(pts).astype(npdt)[idx], idx, scores(r["grad"], npdt)


def attack(W, data, target, noise, kind, num_add, dtype=torch.float64, binary_step=10, num_iter=500, lr=1e-2, init_weight=5e3,
           max_weight=4e4, loss="logits", kappa=0., scale=None):
    """Free-running, cloud by cloud.  W: pointnet_oracle.to_torch(weights, dtype); data [B,K,3]; noise [binary_step,B,num_add,3] or
    None.  -> dict: cri [B,A,3], o_bestdist [B], o_bestattack [B,K+A,3] (the originals, then the best or the last forwarded added
    rows), success [B] bool (lower > 0), success_num, history [binary_step,B,3] (weight, lower, upper behind every search step)."""
    B, K = np.asarray(data).shape[:2]
    A = int(num_add)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    scale = 1.0 / B if scale is None else scale
    out = {"cri": np.zeros((B, A, 3), npdt), "o_bestdist": np.full(B, 1e10), "o_bestattack": np.zeros((B, K + A, 3), npdt),
           "success": np.zeros(B, bool), "history": np.zeros((binary_step, B, 3))}
    for b in range(B):
        ori = np.asarray(data[b]).astype(npdt)
        tg = int(target[b])
        cri = critical_points(W, ori, tg, A, scale, dtype)[0]
        out["cri"][b] = cri
        weight, lower, upper = float(init_weight), 0., float(max_weight)
        rec = fresh_record(A, npdt)
        for s in range(binary_step):
            adv = cri if noise is None else cri + np.asarray(noise[s][b]).astype(npdt)
            m, v = np.zeros_like(cri), np.zeros_like(cri)
            for it in range(num_iter):
                r = AO.run_cloud(W, np.concatenate([ori, adv]), tg, loss, kappa, scale, dtype=dtype)
                pred = int(r["logits"].argmax())
                last = adv
                adv, m, v, rec, _, _, _ = step(kind, r["grad"][K:], pred, tg, adv, ori, weight, m, v, it + 1, lr, scale, rec, dtype)
            weight, lower, upper, rec = adjust(rec, tg, weight, lower, upper)
            out["history"][s, b] = weight, lower, upper
        out["success"][b] = lower > 0
        out["o_bestdist"][b] = rec["o_bestdist"]
        out["o_bestattack"][b] = np.concatenate([ori, rec["o_bestattack"] if lower > 0 else last])       # Add.py:210-219
    out["success_num"] = int(out["success"].sum())
    return out


# ---------------------------------------------------------------------------------------------- teacher-forced step cases
# (name, B, largest n_ori, num_add): the shapes of the one-step parity test; "ragged" has clouds of different sizes in a wider stride
STEP_CASES = (("ragged", 5, 300, 77), ("small", 17, 64, 16), ("mid", 2, 1024, 512), ("max", 1, 2048, 1024))
STEP_LR, STEP_SCALE = 1e-2, 0.25


def make_step_case(name, kind, t, seed=0):
    """Inputs of one teacher-forced step, float32 as the library takes them: the network plays no part (grad, m and positive v are
    random).  Every cloud starts from adv = ori[idx] + 0.02 randn, idx a draw without repeats - never from the reference's 1e-7
    start, where the distances are rounding noise.  Rows beyond a cloud are NaN: reading them poisons the result."""
    _, B, n_max, A = next(c for c in STEP_CASES if c[0] == name)
    rng = np.random.default_rng([seed, t, KINDS.index(kind), sum(map(ord, name))])
    n_ori = np.full(B, n_max, np.int32)
    stride = n_max + A
    if name == "ragged":
        n_ori = np.array([n_max, A, 150, n_max - 1, 256], np.int32)
        stride = n_max + A + 3
    cat = np.full((B, stride, 3), np.nan, np.float32)
    grad = np.full((B, stride, 3), np.nan, np.float32)
    for b in range(B):
        n = int(n_ori[b])
        ori = rng.standard_normal((n, 3))
        ori = (ori / np.linalg.norm(ori, axis=1, keepdims=True) * rng.random((n, 1)) ** (1 / 3)).astype(np.float32)
        idx = rng.permutation(n)[:A]
        cat[b, :n] = ori
        cat[b, n:n + A] = ori[idx] + (0.02 * rng.standard_normal((A, 3))).astype(np.float32)
        grad[b, :n + A] = (rng.standard_normal((n + A, 3)) * 10 ** rng.uniform(-4, -1, (n + A, 1))).astype(np.float32)
    m = (rng.standard_normal((B, A, 3)) * 1e-2).astype(np.float32) if t > 1 else np.zeros((B, A, 3), np.float32)
    v = (rng.random((B, A, 3)) * 1e-3 + 1e-8).astype(np.float32) if t > 1 else np.zeros((B, A, 3), np.float32)
    lo, hi = (5e3, 4e4) if kind == "chamfer" else (2e2, 9e2)
    weight = rng.uniform(lo / 8, hi, B)
    target = rng.integers(0, 40, B).astype(np.int32)
    pred = np.where(rng.random(B) < 0.5, target, (target + 1) % 40).astype(np.int32)
    return {"name": name, "kind": kind, "t": t, "B": B, "A": A, "stride": stride, "n_ori": n_ori, "cat": cat, "grad": grad, "m": m, "v": v,
            "weight": weight, "target": target, "pred": pred}


def run_step_case(case, dtype):
    """The oracle on every cloud of a case -> list of dicts {adv, m, v, dist, dist_grad, min_p, nn, far, record}."""
    out = []
    npdt = np.float32 if dtype == torch.float32 else np.float64
    for b in range(case["B"]):
        n, A = int(case["n_ori"][b]), case["A"]
        ori, adv = case["cat"][b, :n].astype(npdt), case["cat"][b, n:n + A].astype(npdt)
        a, m, v, rec, d, _, diag = step(case["kind"], case["grad"][b, n:n + A].astype(npdt), int(case["pred"][b]), int(case["target"][b]),
                                        adv, ori, case["weight"][b], case["m"][b].astype(npdt), case["v"][b].astype(npdt), case["t"],
                                        STEP_LR, STEP_SCALE, fresh_record(A, npdt), dtype)
        out.append(dict(diag, adv=a, m=m, v=v, dist=d, record=rec))
    return out


def judge_step_case(case, r32, r64):
    """From the two oracles alone -> (e, rows_out list of bool [A], clouds_out list, e32 {quantity: the float32 oracle's largest
    error over the rows that are judged}).  Asserts the conditions a parity case must meet: at most 5 % of its rows are out, no
    Hausdorff cloud is out, and on the judged rows the two oracles agree on every discrete decision."""
    e = max(float(np.abs(a["min_p"].astype(np.float64) - b["min_p"]).max()) for a, b in zip(r32, r64))
    rows_out, clouds_out = [], []
    for b in range(case["B"]):
        n, A = int(case["n_ori"][b]), case["A"]
        ro, co = exclusions(case["cat"][b, n:n + A], case["cat"][b, :n], e, case["kind"])
        rows_out.append(ro)
        clouds_out.append(co)
    share = sum(int(r.sum()) for r in rows_out) / float(case["B"] * case["A"])
    assert share <= 0.05, "%s: %.1f %% of the rows are excluded" % (case["name"], 100 * share)
    assert not any(clouds_out), "%s: a Hausdorff cloud is excluded" % case["name"]
    e32 = {k: 0.0 for k in ("adv", "m", "v", "dist", "dist_grad")}
    for a, b, ro in zip(r32, r64, rows_out):
        assert np.array_equal(a["nn"][~ro], b["nn"][~ro]) and a["far"] == b["far"], "%s: the oracles disagree on a judged decision" % case["name"]
        for k in ("adv", "m", "v", "dist_grad"):
            e32[k] = max(e32[k], float(np.abs(a[k].astype(np.float64) - b[k])[~ro].max()))
        e32["dist"] = max(e32["dist"], abs(float(a["dist"]) - float(b["dist"])))
    return e, rows_out, clouds_out, e32, share
