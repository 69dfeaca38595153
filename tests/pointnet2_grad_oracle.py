"""Test oracle of the PointNet++ input gradient (include/ifd_pn2_atk.h), one cloud at a time.

(a) ``run_cloud``: the reference-form gradient.  pointnet2_oracle._forward_batch's operations in its order (index the centroids,
    gather the balls, subtract the centroid, cat, linear -> batch_norm -> relu on the grouped rows, max over the samples; the
    group-all level; the head) with autograd on and the four index tables forced - farthest_point_sample and query_ball_point
    return indices, which carry no gradient; the centroids' coordinates do, through x[fps] and the subtraction.  The adversarial
    losses are atk_oracle.adv_loss.  Unlike _forward_batch it keeps every pre-activation, which the checks below need;
    tests/test_pointnet2_grad_cpu.py holds its logits and features to _forward_batch's bit for bit.  float32 and float64.
(b) ``explicit``: the gradient as a fixed linear map of GIVEN discrete choices, on the BN-folded weights: per level the hidden
    layers' gates as masks (act1 [512,32,128], act2 [128,64,256], act3 [128,768]: the first hidden layer's channels, then the
    second's), the group maxima through given winners (win1 [512,128], win2 [128,256] sample positions, win3 [1024] rows) and the
    last layer's gate as the sign of a given feature (pos1, pos2, pos3).  Only the head's two ReLUs, the hinge and the runner-up
    class are the oracle's own (``head_exclusion`` names the clouds where those are within rounding of flipping).  In float64 it
    is the yardstick of a GPU gradient, fed the GPU's choices; in float32 its distance from the float64 run on the same choices
    is e_32, the error float32 arithmetic makes on this very map.
(c) ``choices_valid``: the GPU's choices held against the float64 reference-form run on the GPU's tables: a reported winner's
    float64 value within 8 e_act of its channel's float64 maximum; a gate that disagrees with float64 only where
    |pre-activation| <= 8 e_act.  e_act is the float32 run's own distance from the float64 run, layer by layer
    (``layer_errors``), as in atk_oracle."""
import numpy as np
import torch
import torch.nn.functional as F

import atk_oracle as AO
import pointnet2_oracle as PO
from ifdefense_amd.weights import fold_pointnet2, pointnet2_layers

NP1, NS1, NP2, NS2 = PO.NP1, PO.NS1, PO.NP2, PO.NS2
TABLES = ("fps1", "fps2", "ball1", "ball2")
PRE = ("sa1_0", "sa1_1", "sa1_2", "sa2_0", "sa2_1", "sa2_2", "sa3_0", "sa3_1", "sa3_2", "fc1", "fc2")
CHOICES = ("win1", "win2", "win3", "act1", "act2", "act3", "pos1", "pos2", "pos3")


def _t(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t if dtype is None else t.to(dtype)


def _long(a):
    return torch.as_tensor(np.asarray(a).astype(np.int64))


# ---------------------------------------------------------------------------------------------- (a) the reference form
def _mlp(W, layers, rows, pre, tag):
    """The level's conv -> bn -> relu stack on rows [..., C]; the pre-activations go to pre[tag_k]."""
    h = rows
    for k, (lin, bn, (co, ci), _) in enumerate(layers):
        p = PO._bn(W, F.linear(h.reshape(-1, ci), W[lin + ".weight"].reshape(co, ci), W[lin + ".bias"]), bn).view(h.shape[:-1] + (co,))
        pre["%s_%d" % (tag, k)] = p
        h = F.relu(p)
    return h


def _reference(W, x, t):
    """pointnet2_oracle._forward_batch on one cloud x [n,3] with the tables t, keeping the pre-activations."""
    L = pointnet2_layers()
    f1, f2, b1, b2 = (_long(t[k]) for k in TABLES)
    pre = {}
    c1 = x[f1]                                                                 # [512, 3]
    l1 = _mlp(W, L[0:3], x[b1] - c1.view(NP1, 1, 3), pre, "sa1").max(1)[0]     # [512, 128]
    c2 = c1[f2]                                                                # [128, 3]
    g2 = torch.cat([c1[b2] - c2.view(NP2, 1, 3), l1[b2]], dim=-1)
    l2 = _mlp(W, L[3:6], g2, pre, "sa2").max(1)[0]                             # [128, 256]
    g = _mlp(W, L[6:9], torch.cat([c2, l2], dim=-1), pre, "sa3").max(0)[0][None]    # [1, 1024]
    pre["fc1"] = PO._bn(W, F.linear(g, W["fc1.weight"], W["fc1.bias"]), "bn1")
    pre["fc2"] = PO._bn(W, F.linear(F.relu(pre["fc1"]), W["fc2.weight"], W["fc2.bias"]), "bn2")
    lo = F.linear(F.relu(pre["fc2"]), W["fc3.weight"], W["fc3.bias"])
    return {"logits": lo, "l1_feat": l1, "l2_feat": l2, "global_feat": g[0], "pre": pre}


def _loss_fields(logits, target, loss, kappa, scale):
    lv, h, oi = AO.adv_loss(logits, torch.as_tensor([int(target)]), loss, kappa)
    (lv.sum() * scale).backward()
    return {"target": int(target), "logits": logits[0].detach().numpy(), "loss": float(lv[0].detach()),
            "hinge": None if h is None else float(h[0].detach()), "other": None if oi is None else int(oi[0])}


def run_cloud(W, pts, target, tables, loss="logits", kappa=0., scale=1., dtype=torch.float64):
    """One cloud [n,3].  W: pointnet2_oracle.to_torch(state dict, dtype).  tables: the four index tables of the cloud.  -> dict:
    grad [n,3] = scale * d loss / d pts, logits [40], loss, hinge, other, tables, pre {name: pre-activation} (sa1_k [512,32,C],
    sa2_k [128,64,C], sa3_k [128,C], fc1 [512], fc2 [256]), l1_feat, l2_feat, global_feat, and the run's own discrete choices in
    the GPU's form (module docstring; torch.max on the CPU takes the lowest index among equal values)."""
    x0 = _t(pts, dtype)[:, :3].contiguous().requires_grad_()
    o = _reference(W, x0, tables)
    r = _loss_fields(o["logits"], target, loss, kappa, scale)
    r["grad"] = (x0.grad if x0.grad is not None else torch.zeros_like(x0)).numpy()
    r["tables"] = {k: np.asarray(tables[k]).astype(np.int64) for k in TABLES}
    with torch.no_grad():
        p = {k: v.numpy() for k, v in o["pre"].items()}
        r["pre"] = {k: (v[0] if k in ("fc1", "fc2") else v) for k, v in p.items()}
        for k in ("l1_feat", "l2_feat", "global_feat"):
            r[k] = o[k].numpy()
        r["win1"], r["win2"] = o["pre"]["sa1_2"].max(1)[1].numpy(), o["pre"]["sa2_2"].max(1)[1].numpy()
        r["win3"] = o["pre"]["sa3_2"].max(0)[1].numpy()
        r["act1"] = np.concatenate([p["sa1_0"] > 0, p["sa1_1"] > 0], -1)
        r["act2"] = np.concatenate([p["sa2_0"] > 0, p["sa2_1"] > 0], -1)
        r["act3"] = np.concatenate([p["sa3_0"] > 0, p["sa3_1"] > 0], -1)
        r["pos1"], r["pos2"], r["pos3"] = r["l1_feat"] > 0, r["l2_feat"] > 0, r["global_feat"] > 0
    return r


# ---------------------------------------------------------------------------------------------- (b) the explicit-choice form
def folded(sd, dtype=torch.float64):
    """The BN-folded layers of a state dict (weights.fold_pointnet2, float64), as tensors of ``dtype``: {name: tensor}."""
    return {k: torch.as_tensor(v).to(dtype) for k, v in fold_pointnet2(sd)}


def _level(Wf, layers, rows, act, win, pos, dtype, over):
    """A level of given choices: two gated hidden layers, the last layer gathered at the winners (``over``: the axis of the
    maximum, 1 = the samples of a group, 0 = the rows of sa3) and gated by pos."""
    (l0, _, (c0, _), _), (l1, _, _, _), (l2, _, _, _) = layers
    m = _t(act).to(dtype)
    h = (rows @ Wf[l0 + ".weight"].t() + Wf[l0 + ".bias"]) * m[..., :c0]
    h = (h @ Wf[l1 + ".weight"].t() + Wf[l1 + ".bias"]) * m[..., c0:]
    p = h @ Wf[l2 + ".weight"].t() + Wf[l2 + ".bias"]
    w = _long(win)
    top = torch.gather(p, 1, w[:, None, :])[:, 0, :] if over == 1 else p[w, torch.arange(p.shape[1])]
    return top * _t(pos).to(dtype)


def explicit(Wf, pts, target, tables, ch, loss="logits", kappa=0., scale=1., dtype=torch.float64):
    """One cloud [n,3] with every discrete choice of the three levels given (module docstring): ch holds CHOICES.  -> dict: grad
    [n,3], logits, loss, hinge, other, fc1 [512], fc2 [256] (the head's pre-activations), l1_feat, l2_feat, global_feat."""
    L = pointnet2_layers()
    x0 = _t(pts, dtype)[:, :3].contiguous().requires_grad_()
    f1, f2, b1, b2 = (_long(tables[k]) for k in TABLES)
    c1 = x0[f1]
    l1 = _level(Wf, L[0:3], x0[b1] - c1.view(NP1, 1, 3), ch["act1"], ch["win1"], ch["pos1"], dtype, 1)
    c2 = c1[f2]
    l2 = _level(Wf, L[3:6], torch.cat([c1[b2] - c2.view(NP2, 1, 3), l1[b2]], dim=-1), ch["act2"], ch["win2"], ch["pos2"], dtype, 1)
    g = _level(Wf, L[6:9], torch.cat([c2, l2], dim=-1), ch["act3"], ch["win3"], ch["pos3"], dtype, 0)[None]
    p1 = F.linear(g, Wf["fc1.weight"], Wf["fc1.bias"])
    p2 = F.linear(F.relu(p1), Wf["fc2.weight"], Wf["fc2.bias"])
    lo = F.linear(F.relu(p2), Wf["fc3.weight"], Wf["fc3.bias"])
    r = _loss_fields(lo, target, loss, kappa, scale)
    r["grad"] = (x0.grad if x0.grad is not None else torch.zeros_like(x0)).numpy()
    r["fc1"], r["fc2"] = p1[0].detach().numpy(), p2[0].detach().numpy()
    r["l1_feat"], r["l2_feat"], r["global_feat"] = l1.detach().numpy(), l2.detach().numpy(), g[0].detach().numpy()
    return r


def explicit_from(Wf, pts, target, r, **kw):
    """explicit() fed the tables and choices of a run_cloud result, or of ``gpu_choices``."""
    return explicit(Wf, pts, target, r["tables"], r, **kw)


def unpack_bits(words, channels):
    """[..., W] int32 / uint32 words -> bool [..., channels]: bit c % 32 of word c // 32."""
    w = np.asarray(words).astype(np.int64) & 0xffffffff
    b = ((w[..., None] >> np.arange(32)) & 1).astype(bool)
    return b.reshape(w.shape[:-1] + (w.shape[-1] * 32,))[..., :channels]


def gpu_choices(aux, b):
    """Cloud b of PointNet2Classifier.input_grad's diagnostics, on the CPU, in run_cloud's form."""
    get = lambda k: aux[k][b].cpu().numpy()                                  # noqa: E731
    ch = {"tables": {k: get(k).astype(np.int64) for k in TABLES}}
    for k in ("win1", "win2", "win3"):
        ch[k] = get(k).astype(np.int64)
    ch["act1"], ch["act2"], ch["act3"] = unpack_bits(get("act1"), 128), unpack_bits(get("act2"), 256), unpack_bits(get("act3"), 768)
    ch["pos1"], ch["pos2"], ch["pos3"] = get("l1_feat") > 0, get("l2_feat") > 0, get("global_feat") > 0
    return ch


# ---------------------------------------------------------------------------------------------- (c) errors, validity, exclusion
def layer_errors(r32, r64):
    """e_act per layer: max |float32 run - float64 run| of the pre-activations over lists of clouds run with the SAME tables;
    'logits' too."""
    e = {k: max(float(np.abs(a["pre"][k].astype(np.float64) - b["pre"][k]).max()) for a, b in zip(r32, r64)) for k in PRE}
    e["logits"] = max(float(np.abs(a["logits"].astype(np.float64) - b["logits"]).max()) for a, b in zip(r32, r64))
    return e


def _gates_valid(got, pre, ea, what):
    off = np.asarray(got) != (pre > 0)
    gap = float(np.abs(pre[off]).max()) if off.any() else 0.0
    assert gap <= 8 * ea, "%s: a gate differs at |pre| = %.3e (8 e_act = %.3e)" % (what, gap, 8 * ea)
    return gap / ea if ea > 0 else 0.0


def _winners_valid(win, pre, axis, ea, what):
    win = np.asarray(win)
    assert win.min() >= 0 and win.max() < pre.shape[axis], "%s: a winner outside its range" % what
    act = np.maximum(pre, 0.0)                                                # the maximum is taken behind the ReLU: a channel that is
    at = np.take_along_axis(act, np.expand_dims(win, axis), axis).squeeze(axis)   # negative in every row ties at 0
    short = float((act.max(axis) - at).max())
    assert short <= 8 * ea, "%s: winner %.3e below the maximum (8 e_act = %.3e)" % (what, short, 8 * ea)
    return short / ea if ea > 0 else 0.0


def choices_valid(ch, r64, e, what=""):
    """``ch`` (gpu_choices) against the float64 run r64 made with ch's tables.  -> the worst ratio to e_act seen."""
    p, worst = r64["pre"], 0.0
    for lv, axis, c0 in ((1, 1, 64), (2, 1, 128), (3, 0, 256)):
        tag, act = "sa%d" % lv, np.asarray(ch["act%d" % lv])
        worst = max(worst, _gates_valid(act[..., :c0], p[tag + "_0"], e[tag + "_0"], "%s: %s layer 1" % (what, tag)),
                    _gates_valid(act[..., c0:], p[tag + "_1"], e[tag + "_1"], "%s: %s layer 2" % (what, tag)),
                    _winners_valid(ch["win%d" % lv], p[tag + "_2"], axis, e[tag + "_2"], "%s: %s" % (what, tag)),
                    _gates_valid(ch["pos%d" % lv], p[tag + "_2"].max(axis), e[tag + "_2"], "%s: %s last layer" % (what, tag)))
    return worst


def head_exclusion(r64, e, loss="logits"):
    """Reasons (empty: none) for which the float64 oracle alone leaves a cloud out: the gates that cannot be forced - an fc1 / fc2
    pre-activation, the hinge, or the runner-up gap within 8 e_act of flipping."""
    why = ["unit:" + k for k in ("fc1", "fc2") if np.abs(r64["pre"][k]).min() < 8 * e[k]]
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


def oracle_case(sd, clouds, targets, loss="logits", kappa=0., scale=1., starts=None, tables=None):
    """Both reference-form runs of a list of clouds on the same tables (per cloud: ``tables``, else the oracle's own float32
    selection from ``starts``) -> (r32, r64, e_act, exclusions): what a parity case needs that does not depend on the GPU."""
    W32, W64 = PO.to_torch(sd, torch.float32), PO.to_torch(sd, torch.float64)
    if tables is None:
        tables = [PO.tables_of_cloud(c, (0, 0) if starts is None else tuple(int(v) for v in starts[i])) for i, c in enumerate(clouds)]
    r32 = [run_cloud(W32, c, t, tb, loss, kappa, scale, torch.float32) for c, t, tb in zip(clouds, targets, tables)]
    r64 = [run_cloud(W64, c, t, tb, loss, kappa, scale, torch.float64) for c, t, tb in zip(clouds, targets, tables)]
    e = layer_errors(r32, r64)
    return r32, r64, e, [head_exclusion(r, e, loss) for r in r64]
