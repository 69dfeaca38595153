"""Test oracle of the DGCNN input gradient (include/ifd_dgcnn_atk.h), one cloud at a time.

(a) ``run_cloud``: the reference-form gradient.  dgcnn_oracle._forward_batch's operations in its order (graph_feature, conv2d,
    batch_norm, leaky_relu, max over the neighbours; conv1d, the two pools, the head) with autograd on and the four neighbour
    tables forced or left to topk, whose indices carry no gradient either way; the adversarial losses are atk_oracle.adv_loss.
    Unlike _forward_batch it keeps every pre-activation, which the checks below need; tests/test_dgcnn_grad_cpu.py holds its
    logits and gradient to _forward_batch's bit for bit.  Runs in float32 (the reference's rounding) and float64.
(b) ``explicit``: the gradient as a fixed linear map of GIVEN discrete choices, on the BN-folded weights in split form: per edge
    convolution P = Wa x, Q = (Wb - Wa) x + b, pre_i[c] = P[win_edge[i][c]][c] + Q_i[c], out = pre * (1 | 0.2) by a given sign
    mask; conv5's slopes from a given mask, its max-pool through a given win_pool.  Only the head's two LeakyReLUs, the hinge
    and the runner-up class are the oracle's own (``head_exclusion`` names the clouds where those are within rounding of
    flipping).  In float64 it is the yardstick of a GPU gradient, fed the GPU's choices; in float32 its distance from the
    float64 run on the same choices is e_32, the error float32 arithmetic makes on this very map.
(c) ``choices_valid``: the GPU's choices held against the float64 reference-form run: a reported winner's float64 value within
    8 e_act of its channel's float64 maximum; a sign that disagrees with float64 only where |pre-activation| <= 8 e_act.  e_act is
    the float32 run's own distance from the float64 run, layer by layer (``layer_errors``), as in atk_oracle."""
import numpy as np
import torch
import torch.nn.functional as F

import atk_oracle as AO
import dgcnn_oracle as DO
from ifdefense_amd.weights import dgcnn_layers, fold_dgcnn

WIDTHS = (64, 64, 128, 256)
OUT_COLS = ((0, 64), (64, 128), (128, 256), (256, 512))
LAYERS = ("edge1", "edge2", "edge3", "edge4", "conv5", "fc1", "fc2")


def _t(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t if dtype is None else t.to(dtype)


# ---------------------------------------------------------------------------------------------- (a) the reference form
def _reference(W, x, k, idx):
    """dgcnn_oracle._forward_batch on x [1,3,n], keeping the pre-activations: edge[l] [1,Cout,n,k] (per neighbour, in the order
    of idx[l]'s row), conv5 [1,1024,n], fc1 [1,512], fc2 [1,256]."""
    L = dgcnn_layers()
    chosen, xs, edge = [], [], []
    h = x
    for l in range(4):
        lin, bn, (co, ci), _, _ = L[l]
        e, ix = DO.graph_feature(h, k, None if idx is None or idx[l] is None else idx[l])
        chosen.append(ix)
        e = DO._bn(W, F.conv2d(e, W[lin + ".weight"].reshape(co, ci, 1, 1), W.get(lin + ".bias")), bn)
        edge.append(e)
        h = F.leaky_relu(e, negative_slope=0.2).max(dim=-1, keepdim=False)[0]
        xs.append(h)
    feat = torch.cat(xs, dim=1)
    lin, bn, (co, ci), _, _ = L[4]
    p5 = DO._bn(W, F.conv1d(feat, W[lin + ".weight"].reshape(co, ci, 1), W.get(lin + ".bias")), bn)
    y = F.leaky_relu(p5, negative_slope=0.2)
    g = torch.cat((F.adaptive_max_pool1d(y, 1).view(1, -1), F.adaptive_avg_pool1d(y, 1).view(1, -1)), 1)
    p1 = DO._bn(W, F.linear(g, W[L[5][0] + ".weight"], W.get(L[5][0] + ".bias")), L[5][1])
    p2 = DO._bn(W, F.linear(F.leaky_relu(p1, negative_slope=0.2), W[L[6][0] + ".weight"], W.get(L[6][0] + ".bias")), L[6][1])
    lo = F.linear(F.leaky_relu(p2, negative_slope=0.2), W["linear3.weight"], W["linear3.bias"])
    return {"logits": lo, "feat": feat, "global_feat": g, "idx": chosen, "edge": edge, "conv5": p5, "fc1": p1, "fc2": p2}


def _loss_fields(logits, target, loss, kappa, scale):
    lv, h, oi = AO.adv_loss(logits, torch.as_tensor([int(target)]), loss, kappa)
    (lv.sum() * scale).backward()
    return {"target": int(target), "logits": logits[0].detach().numpy(), "loss": float(lv[0].detach()),
            "hinge": None if h is None else float(h[0].detach()), "other": None if oi is None else int(oi[0])}


def run_cloud(W, pts, target, loss="logits", kappa=0., scale=1., k=DO.K_DEFAULT, idx=None, dtype=torch.float64):
    """One cloud [n,3].  W: dgcnn_oracle.to_torch(state dict, dtype).  idx: None or four [n,k] tables.  -> dict: grad [n,3] =
    scale * d loss / d pts, logits [40], loss, hinge, other, idx (four [n,k]), edge (four [Cout,n,k]), conv5 [1024,n], fc1, fc2,
    feat [n,512], global_feat [2048], and the run's own discrete choices in the GPU's form: win_edge (four [n,Cout], the POINT
    index torch.max took), feat_pos [n,512], act5 [n,1024] (bool), win_pool [1024] (torch.max: the lowest index among equals)."""
    x0 = _t(pts, dtype)[None, :, :3].transpose(1, 2).contiguous().requires_grad_()
    ib = None if idx is None else [None if t is None else _t(t)[None] for t in idx]
    o = _reference(W, x0, k, ib)
    r = _loss_fields(o["logits"], target, loss, kappa, scale)
    r["grad"] = x0.grad[0].t().contiguous().numpy()
    with torch.no_grad():
        r["idx"] = [t[0].numpy() for t in o["idx"]]
        r["edge"] = [e[0].numpy() for e in o["edge"]]
        r["win_edge"] = [torch.gather(ix[0], 1, e[0].max(dim=-1)[1].t()).numpy() for e, ix in zip(o["edge"], o["idx"])]
        r["conv5"], r["fc1"], r["fc2"] = o["conv5"][0].numpy(), o["fc1"][0].numpy(), o["fc2"][0].numpy()
        r["feat"] = o["feat"][0].t().contiguous().numpy()
        r["global_feat"] = o["global_feat"][0].numpy()
        r["feat_pos"], r["act5"] = r["feat"] > 0, r["conv5"].T > 0
        r["win_pool"] = F.leaky_relu(o["conv5"][0], negative_slope=0.2).max(1)[1].numpy()
    return r


# ---------------------------------------------------------------------------------------------- (b) the explicit-choice form
def folded(sd, dtype=torch.float64):
    """The BN-folded layers of a state dict (weights.fold_dgcnn, float64), as tensors of ``dtype``: {name: tensor}."""
    return {k: torch.as_tensor(v).to(dtype) for k, v in fold_dgcnn(sd)}


def explicit(Wf, pts, target, win_edge, feat_pos, act5, win_pool, loss="logits", kappa=0., scale=1., dtype=torch.float64):
    """One cloud [n,3] with every discrete choice of the point layers given (module docstring).  -> dict: grad [n,3], logits,
    loss, hinge, other, fc1 [512], fc2 [256] (the head's pre-activations)."""
    L = dgcnn_layers()
    x0 = _t(pts, dtype)[:, :3].contiguous().requires_grad_()
    one, fifth = torch.tensor(1.0, dtype=dtype), torch.tensor(0.2, dtype=dtype)
    slope = lambda m: torch.where(_t(m).bool(), one, fifth)                  # noqa: E731
    h, xs = x0, []
    for l in range(4):
        w, b = Wf[L[l][0] + ".weight"], Wf[L[l][0] + ".bias"]
        C = w.shape[1] // 2
        P, Q = h @ w[:, :C].t(), h @ (w[:, C:] - w[:, :C]).t() + b
        a, c = OUT_COLS[l]
        h = (torch.gather(P, 0, _t(win_edge[l]).long()) + Q) * slope(np.asarray(feat_pos)[:, a:c])
        xs.append(h)
    feat = torch.cat(xs, dim=1)
    y = (feat @ Wf["conv5.0.weight"].t() + Wf["conv5.0.bias"]) * slope(act5)
    g = torch.cat((y[_t(win_pool).long(), torch.arange(y.shape[1])], y.mean(0)))[None]
    p1 = F.linear(g, Wf["linear1.0.weight"], Wf["linear1.0.bias"])
    p2 = F.linear(F.leaky_relu(p1, negative_slope=0.2), Wf["linear2.0.weight"], Wf["linear2.0.bias"])
    lo = F.linear(F.leaky_relu(p2, negative_slope=0.2), Wf["linear3.weight"], Wf["linear3.bias"])
    r = _loss_fields(lo, target, loss, kappa, scale)
    r["grad"] = (x0.grad if x0.grad is not None else torch.zeros_like(x0)).numpy()
    r["fc1"], r["fc2"] = p1[0].detach().numpy(), p2[0].detach().numpy()
    return r


def explicit_from(Wf, pts, target, r, **kw):
    """explicit() fed the choices of a run_cloud result, or of ``gpu_choices``."""
    return explicit(Wf, pts, target, r["win_edge"], r["feat_pos"], r["act5"], r["win_pool"], **kw)


def unpack_act5(words, n):
    """act5 [N,32] int32 / uint32 words -> bool [n,1024]: bit c % 32 of word c // 32."""
    w = np.asarray(words)[:n].astype(np.int64) & 0xffffffff
    return ((w[:, :, None] >> np.arange(32)[None, None, :]) & 1).astype(bool).reshape(n, 1024)


def gpu_choices(aux, b, n):
    """Cloud b (n points) of DgcnnClassifier.input_grad's diagnostics, on the CPU, in run_cloud's form."""
    return {"idx": [t[b, :n].cpu().numpy().astype(np.int64) for t in aux["idx"]],
            "win_edge": [t[b, :n].cpu().numpy().astype(np.int64) for t in aux["win_edge"]],
            "feat_pos": aux["feat"][b, :n].cpu().numpy() > 0, "act5": unpack_act5(aux["act5"][b].cpu().numpy(), n),
            "win_pool": aux["win_pool"][b].cpu().numpy().astype(np.int64)}


# ---------------------------------------------------------------------------------------------- (c) errors, validity, exclusion
def _edge_pre(r, l):
    return r["edge"][l].max(-1)                                           # [Cout,n]: the pre-activation the layer's LeakyReLU sees


def layer_errors(r32, r64):
    """e_act per layer: max |float32 run - float64 run| of the pre-activations over lists of clouds run with the SAME neighbour
    tables (edge layers: per neighbour); 'logits' too."""
    e = {}
    for l in range(4):
        e["edge%d" % (l + 1)] = max(float(np.abs(a["edge"][l].astype(np.float64) - b["edge"][l]).max()) for a, b in zip(r32, r64))
    for k in ("conv5", "fc1", "fc2", "logits"):
        e[k] = max(float(np.abs(a[k].astype(np.float64) - b[k]).max()) for a, b in zip(r32, r64))
    return e


def choices_valid(ch, r64, e, what=""):
    """``ch`` (gpu_choices) against the float64 run r64 made with ch's neighbour tables.  -> the worst ratio to e_act seen."""
    n = r64["grad"].shape[0]
    worst = 0.0
    for l in range(4):
        E, ix, win, ea = r64["edge"][l], r64["idx"][l], np.asarray(ch["win_edge"][l]), e["edge%d" % (l + 1)]
        hit = ix[:, None, :] == win[:, :, None]                             # [n,Cout,k]
        assert hit.any(-1).all(), "%s: edge %d: a winner that is not a neighbour" % (what, l + 1)
        at = np.take_along_axis(E.transpose(1, 0, 2), hit.argmax(-1)[:, :, None], 2)[:, :, 0]      # [n,Cout]
        short = float((E.max(-1).T - at).max())
        assert short <= 8 * ea, "%s: edge %d: winner %.3e below the maximum (8 e_act = %.3e)" % (what, l + 1, short, 8 * ea)
        a, c = OUT_COLS[l]
        pre = _edge_pre(r64, l).T
        off = np.asarray(ch["feat_pos"])[:, a:c] != (pre > 0)
        gap = float(np.abs(pre[off]).max()) if off.any() else 0.0
        assert gap <= 8 * ea, "%s: edge %d: a sign differs at |pre| = %.3e (8 e_act = %.3e)" % (what, l + 1, gap, 8 * ea)
        worst = max(worst, short / ea if ea > 0 else 0.0, gap / ea if ea > 0 else 0.0)
    p5 = r64["conv5"]
    act = np.where(p5 > 0, p5, 0.2 * p5)
    worst = max(worst, AO.winners_valid(ch["win_pool"], act, e["conv5"], what + ": conv5 pool"))
    off = np.asarray(ch["act5"]) != (p5.T > 0)
    gap = float(np.abs(p5.T[off]).max()) if off.any() else 0.0
    assert gap <= 8 * e["conv5"], "%s: conv5: a sign differs at |pre| = %.3e (8 e_act = %.3e)" % (what, gap, 8 * e["conv5"])
    assert n == len(ch["feat_pos"])
    return max(worst, gap / e["conv5"] if e["conv5"] > 0 else 0.0)


def head_exclusion(r64, e, loss="logits"):
    """Reasons (empty: none) for which the float64 oracle alone leaves a cloud out: the gates that cannot be forced - an fc1 / fc2
    pre-activation, the hinge, or the runner-up gap within 8 e_act of flipping."""
    why = ["unit:" + k for k in ("fc1", "fc2") if np.abs(r64[k]).min() < 8 * e[k]]
    if loss == "logits":
        if abs(r64["hinge"]) < 8 * e["logits"]:
            why.append("hinge")
        o = np.sort(np.delete(r64["logits"], r64["target"]))
        if o[-1] - o[-2] < 8 * e["logits"]:
            why.append("runner-up")
    return why


E32_FLOOR = 1e-7


def grad_e32(g32, g64):
    """e_32 of a case: max over its clouds of max |g32 - g64| / max |g64| (explicit() in the two precisions on the same choices),
    floored at 1e-7."""
    e = E32_FLOOR
    for a, b in zip(g32, g64):
        s = np.abs(b).max()
        if s > 0:
            e = max(e, float(np.abs(np.asarray(a, np.float64) - b).max() / s))
    return e


def oracle_case(sd, clouds, targets, loss="logits", kappa=0., scale=1., k=DO.K_DEFAULT, idx=None):
    """Both reference-form runs of a list of clouds (the float32 run with ITS OWN tables forced into the float64 run unless idx
    gives them per cloud) -> (r32, r64, e_act, exclusions): what a parity case needs that does not depend on the GPU."""
    W32, W64 = DO.to_torch(sd, torch.float32), DO.to_torch(sd, torch.float64)
    r32 = [run_cloud(W32, c, t, loss, kappa, scale, k, None if idx is None else idx[i], torch.float32)
           for i, (c, t) in enumerate(zip(clouds, targets))]
    r64 = [run_cloud(W64, c, t, loss, kappa, scale, k, a["idx"], torch.float64) for c, t, a in zip(clouds, targets, r32)]
    e = layer_errors(r32, r64)
    return r32, r64, e, [head_exclusion(r, e, loss) for r in r64]
