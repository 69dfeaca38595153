"""Test oracle of the kNN attack (include/ifd_knn.h): one iteration of CWKNN.attack (baselines/attack/CW/kNN.py:97-116) behind the
forward pass, restated one cloud at a time in torch on the CPU, in the REFERENCE's form: ChamferDistance's expanded pairwise matrix
(baselines/util/set_distance.py:15-50), KNNDist's expanded matrix, topk(k + 1) with column 0 dropped, the no_grad threshold
(attack/util/dist_utils.py:131-166), ChamferkNNDist's weighted sum, autograd for the gradient; the real torch.optim.Adam with its
state put in from outside (as cw_oracle.step does); ProjectInnerPoints and ClipPointsLinf (attack/util/clip_utils.py:53-59, 79-113)
with both cross products along the coordinate axis.  The adversarial loss, its gradient and the prediction come from
atk_oracle.run_cloud.  Runs in float32 (the reference's rounding) and float64 (the yardstick).

The reference's .mean() over its batch is ``scale`` = 1 / B_ref on both loss terms; its `* K` is the cloud's own count.

The exclusion rule at the end says, from the float64 run and the measured float32 errors ALONE, on which rows a discrete decision
(the Chamfer nearest, the mask, the fifth neighbour, the side of the tangent plane) is too close to call at float32; it never looks
at the code under test."""
import numpy as np
import torch

import atk_oracle as AO

K_NN = 5


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)


def pairwise_expanded(x, y):
    """set_distance.py batch_pairwise_dist(x, y) on [1,Nx,3], [1,Ny,3] -> P [1,Nx,Ny] = |x_i|^2 + |y_j|^2 - 2 x_i.y_j."""
    xx, yy, zz = torch.bmm(x, x.transpose(2, 1)), torch.bmm(y, y.transpose(2, 1)), torch.bmm(x, y.transpose(2, 1))
    ix, iy = torch.arange(x.shape[1]), torch.arange(y.shape[1])
    rx = xx[:, ix, ix].unsqueeze(1).expand_as(zz.transpose(2, 1))
    ry = yy[:, iy, iy].unsqueeze(1).expand_as(zz)
    return rx.transpose(2, 1) + ry - 2 * zz


def knn_expanded(pc):
    """dist_utils.py KNNDist's matrix on [1,K,3] -> [1,K,K]."""
    p = pc.transpose(2, 1)
    inner = -2. * torch.matmul(p.transpose(2, 1), p)
    xx = torch.sum(p ** 2, dim=1, keepdim=True)
    return xx + inner + xx.transpose(2, 1)


def dist_terms(adv, ori, alpha=1.05):
    """adv (may require grad), ori [1,K,3] -> dict of tensors: cd [1], knn [1], P [1,K_ori,K_adv], D [1,K,K], value [1,K], thr [1],
    mask [1,K] bool, nn_ori [1,K], top6 [1,K,6] (indices, column 0 the reference's "self")."""
    P = pairwise_expanded(ori, adv)
    mins, nn_ori = torch.min(P, 1)                                      # every adversarial point's nearest original
    cd = torch.mean(mins, dim=1)
    D = knn_expanded(adv)
    neg, top6 = (-D).topk(k=K_NN + 1, dim=-1)
    value = torch.mean(-(neg[..., 1:]), dim=-1)
    with torch.no_grad():
        thr = torch.mean(value, dim=-1) + alpha * torch.std(value, dim=-1)
        mask = value > thr[:, None]
    knn = torch.mean(value * mask.to(value.dtype), dim=1)
    return {"cd": cd, "knn": knn, "P": P, "D": D, "value": value, "thr": thr, "mask": mask, "nn_ori": nn_ori, "top6": top6}


def project_clip(pc, ori, normal, budget=0.1):
    """ProjectInnerClipLinf(budget).forward on [B,3,K] tensors; normal None: the clip alone.  -> (pc', d.n [B,K] or None)."""
    diff = pc - ori
    dn = None
    if normal is not None:
        dn = torch.sum(diff * normal, dim=1)
        inner = dn < 0.
        vng = torch.cross(normal, diff, dim=1)
        vng_norm = torch.sum(vng ** 2, dim=1) ** 0.5
        vref = torch.cross(vng, normal, dim=1)
        vref_norm = torch.sum(vref ** 2, dim=1) ** 0.5
        proj = diff * vref / (vref_norm[:, None, :] + 1e-9)
        opposite = inner & (vng_norm < 1e-6)
        proj = torch.where(opposite.unsqueeze(1).expand_as(proj), torch.zeros_like(proj), proj)
        diff = torch.where(inner.unsqueeze(1).expand_as(diff), proj, diff)
    norm = torch.sum(diff ** 2, dim=1) ** 0.5
    sf = torch.clamp(budget / (norm + 1e-9), max=1.)
    return ori + diff * sf[:, None, :], dn


def project_clip_rows(adv, ori, normal, budget=0.1, dtype=torch.float64):
    """Arrays [n,3] -> (adv' [n,3], d.n [n] or None)."""
    rows = lambda a: None if a is None else _t(a, dtype).t()[None].contiguous()      # noqa: E731
    out, dn = project_clip(rows(adv), rows(ori), rows(normal), budget)
    return out[0].t().contiguous().numpy(), None if dn is None else dn[0].numpy()


def unit_sphere(x):
    """[B,n,3] -> float32, every cloud centred and scaled so that its farthest point has norm 1 (what the CLI does to a file)."""
    x = np.asarray(x, np.float64)
    x = x - x.mean(1, keepdims=True)
    return (x / np.sqrt((x ** 2).sum(-1)).max(1)[:, None, None]).astype(np.float32)


def synth_normals(pts, seed):
    """Unit normals for synthetic clouds [B,n,3]: the radial direction plus noise (tests/golden/make_golden_knn.py's recipe)."""
    nrm = np.asarray(pts, np.float64) + 0.3 * np.random.default_rng(seed).standard_normal(np.shape(pts))
    return (nrm / np.sqrt((nrm ** 2).sum(-1, keepdims=True))).astype(np.float32)


CRAFTED = ("inward", "outward", "anti-parallel", "zero", "on the budget", "far over", "inward and far over")


def crafted_rows():
    """Seven rows that between them take every branch of project / clip -> (adv, ori, normal) float32 [7,3], in CRAFTED's order.
    The normal is (1, 2, 2) / 3 on every row."""
    n = np.array([1., 2., 2.]) / 3.
    t1, t2 = np.array([2., -1., 0.]) / np.sqrt(5.), np.array([2., 4., -5.]) / np.sqrt(45.)       # two tangents
    d = np.stack([0.03 * t1 + 0.01 * t2 - 0.02 * n, 0.03 * t1 + 0.01 * t2 + 0.02 * n, -0.05 * n, 0 * n, 0.06 * t1 + 0.08 * n,
                  0.3 * t1 - 0.4 * t2 + 0.5 * n, 0.3 * t1 + 0.4 * t2 - 0.5 * n])
    ori = np.linspace(-0.5, 0.5, 21).reshape(7, 3).astype(np.float32)
    ori[3] = 0.25                                                       # 0.25 + 0 is exact: the zero row stays a zero row
    adv = (ori + d).astype(np.float32)
    adv[3] = ori[3]
    return adv, ori, np.tile(n.astype(np.float32), (7, 1))


def step(grad_adv, adv, ori, normal, m, v, t, lr, scale, dtype=torch.float64, w1=5., w2=3., alpha=1.05, budget=0.1):
    """One iteration on one cloud, arrays [n,3] (normal may be None).  grad_adv: scale * d adv_loss / d adv; t: the 1-based Adam
    step.  -> dict of numpy: adv, m, v (the new state), g_dist [n,3], cd, knn, dist_loss (= n (w1 cd + w2 knn)), value [n], thr,
    mask [n], nn_ori [n], nn5 [n,5], self_ok (column 0 of the top 6 is the point itself on every row), P [n,n] (adv x ori), D [n,n],
    dn [n] (d.n of the updated point, before the projection; None without normals)."""
    n = len(np.asarray(adv))
    p = _t(adv, dtype)[None].contiguous().requires_grad_()             # [1,n,3], the layout dist_func is called with
    o = _t(ori, dtype)[None].contiguous()
    T = dist_terms(p, o, alpha)
    dl = (T["cd"] * w1 + T["knn"] * w2) * n                             # kNN.py:102-104 for a batch of one
    (dl.sum() * scale).backward()
    g_dist = p.grad[0].detach().clone()
    q = p.detach()[0].t()[None].contiguous().requires_grad_()          # [1,3,n], the layout the optimiser sees
    opt = torch.optim.Adam([q], lr=lr, weight_decay=0.)                # kNN.py:65
    rows = lambda a: _t(a, dtype).t()[None].contiguous()               # noqa: E731
    opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": rows(m), "exp_avg_sq": rows(v)}
    q.grad = rows(grad_adv) + g_dist.t()[None]
    opt.step()
    st = opt.state[q]
    with torch.no_grad():
        new, dn = project_clip(q.detach(), o.transpose(1, 2).contiguous(), None if normal is None else rows(normal), budget)
    back = lambda a: a.detach()[0].t().contiguous().numpy()             # noqa: E731
    top6 = T["top6"][0].numpy()
    return {"adv": back(new), "m": back(st["exp_avg"]), "v": back(st["exp_avg_sq"]), "g_dist": g_dist.numpy(),
            "cd": float(T["cd"][0].detach()), "knn": float(T["knn"][0].detach()), "dist_loss": float(dl[0].detach()),
            "value": T["value"][0].detach().numpy(), "thr": float(T["thr"][0]), "mask": T["mask"][0].numpy(),
            "nn_ori": T["nn_ori"][0].numpy(), "nn5": top6[:, 1:], "self_ok": bool((top6[:, 0] == np.arange(n)).all()),
            "P": T["P"][0].detach().numpy().T, "D": T["D"][0].detach().numpy(), "dn": None if dn is None else dn[0].numpy()}


def g_dist_closed(adv, ori, scale, w1=5., w2=3., alpha=1.05):
    """The header's formula in float64, difference form, self excluded by index -> g_dist [n,3]."""
    a, o = np.asarray(adv, np.float64), np.asarray(ori, np.float64)
    n = len(a)
    D = ((a[:, None] - a[None]) ** 2).sum(-1)
    np.fill_diagonal(D, np.inf)
    nn5 = np.argsort(D, 1, kind="stable")[:, :K_NN]
    value = np.take_along_axis(D, nn5, 1).mean(1)
    mask = value > value.mean() + alpha * value.std(ddof=1)
    nn_ori = ((a[:, None] - o[None]) ** 2).sum(-1).argmin(1)
    g = 2 * w1 * (a - o[nn_ori])
    for p in np.nonzero(mask)[0]:
        for q in nn5[p]:
            g[p] += (2 * w2 / K_NN) * (a[p] - a[q])
            g[q] -= (2 * w2 / K_NN) * (a[p] - a[q])
    return scale * g


def attack(W, data, normal, target, noise, dtype=torch.float64, num_iter=2500, lr=1e-3, loss="logits", kappa=15., scale=None):
    """Free-running, cloud by cloud.  W: pointnet_oracle.to_torch(weights, dtype); data [B,K,3]; normal [B,K,3] or None; noise
    [B,K,3] or None.  -> dict: adv [B,K,3], pred [B], success [B] bool, success_num."""
    B, K = np.asarray(data).shape[:2]
    npdt = np.float32 if dtype == torch.float32 else np.float64
    scale = 1.0 / B if scale is None else scale
    out = {"adv": np.zeros((B, K, 3), npdt), "pred": np.zeros(B, np.int64)}
    for b in range(B):
        ori = np.asarray(data[b]).astype(npdt)
        nrm = None if normal is None else np.asarray(normal[b]).astype(npdt)
        adv = ori if noise is None else ori + np.asarray(noise[b]).astype(npdt)
        m, v = np.zeros_like(ori), np.zeros_like(ori)
        for it in range(num_iter):
            r = AO.run_cloud(W, adv, int(target[b]), loss, kappa, scale, dtype=dtype)
            s = step(r["grad"], adv, ori, nrm, m, v, it + 1, lr, scale, dtype)
            adv, m, v = s["adv"], s["m"], s["v"]
        out["adv"][b] = adv
        out["pred"][b] = int(AO.run_cloud(W, adv, int(target[b]), loss, kappa, scale, dtype=dtype)["logits"].argmax())
    out["success"] = out["pred"] == np.asarray(target)
    out["success_num"] = int(out["success"].sum())
    return out


# ---------------------------------------------------------------------------------------------- the exclusion rule
def errors(r32, r64):
    """max |float32 oracle - float64 oracle| over lists of step() results of one case: e_d (adversarial pair distances), e_c
    (adv-to-ori distances), e_val, e_thr, e_dn (0 without normals)."""
    f = lambda k: max(float(np.abs(np.asarray(a[k], np.float64) - b[k]).max()) for a, b in zip(r32, r64))      # noqa: E731
    return {"e_d": f("D"), "e_c": f("P"), "e_val": f("value"), "e_thr": f("thr"), "e_dn": 0.0 if r64[0]["dn"] is None else f("dn")}


def rows_out(r64, adv, ori, E):
    """The rows of one cloud left out, from the float64 oracle and the errors E alone -> (out [n] bool: decisions, gradient, m, v;
    out_clip [n] bool: additionally the projected point).  adv, ori: the step's inputs, for the float64 difference-form distances.
    The project's 8 e convention: each side may move a quantity by 4 e.  Row j is out when
      its two nearest originals differ by less than 8 e_c;
      it is a point p, or one of p's six nearest, with |value_p - thr| < 8 (e_val + e_thr);
      it is a point p, or one of p's six nearest, with p masked and its 5th and 6th neighbour distances closer than 8 e_d;
      (out_clip only) |d_j.n_j| < 8 e_dn."""
    a, o = np.asarray(adv, np.float64), np.asarray(ori, np.float64)
    sq = lambda x, y: sum((x[:, None, c] - y[None, :, c]) ** 2 for c in range(3))      # noqa: E731  ([n,n], no [n,n,3] temporary)
    C = np.partition(sq(a, o), 1, axis=1)[:, :2]
    out = np.abs(C[:, 1] - C[:, 0]) < 8 * E["e_c"]
    D = sq(a, a)
    np.fill_diagonal(D, np.inf)
    order = np.argsort(D, 1, kind="stable")[:, :K_NN + 1]
    d6 = np.take_along_axis(D, order, 1)
    src = np.abs(r64["value"] - r64["thr"]) < 8 * (E["e_val"] + E["e_thr"])
    src |= r64["mask"] & ((d6[:, 5] - d6[:, 4]) < 8 * E["e_d"])
    for p in np.nonzero(src)[0]:
        out[p] = True
        out[order[p]] = True
    clip = out.copy()
    if r64["dn"] is not None:
        clip |= np.abs(r64["dn"]) < 8 * E["e_dn"]
    return out, clip


def case_rows(r64s, advs, oris, E, cap=0.05):
    """rows_out for every cloud of a case, and the condition on the choice of inputs: at most `cap` of the rows are out."""
    outs = [rows_out(r, a, o, E) for r, a, o in zip(r64s, advs, oris)]
    total = sum(len(o[1]) for o in outs)
    share = sum(int(o[1].sum()) for o in outs) / float(total)
    assert share <= cap, "%.2f %% of the rows are out: choose other inputs" % (100 * share)
    return outs, share
