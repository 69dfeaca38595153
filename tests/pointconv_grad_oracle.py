"""Test oracle of the PointConv input gradient (include/ifd_pc_atk.h), one cloud at a time.

(a) ``run_cloud``: the reference-form gradient.  pointconv_oracle._forward_cloud's operations in its order (the reference's own
    matrix-form density -> DensityNet with ReLU after all three layers; gather, subtract the centroid, cat; conv -> batch_norm ->
    relu on the grouped rows; WeightNet on the differences; features times the density scale; matmul over the members; the level's
    linear; sa3 on the 128 centroids minus their mean; the head) with autograd on and the four index tables forced -
    farthest_point_sample and knn_point return indices, which carry no gradient; everything else does.  The adversarial losses are
    atk_oracle.adv_loss.  It keeps every pre-activation, which the checks below need; tests/test_pointconv_grad_cpu.py holds its
    logits and features to pointconv_oracle.forward's bit for bit.  float32 and float64.
(b) ``explicit``: the gradient as a fixed map of GIVEN discrete choices, on the BN-folded weights and the header's difference-form
    density: every ReLU of the three levels is a given mask - per level DensityNet's three layers (``dn{l}`` [n, 17]), WeightNet's
    (``wn{l}`` [S, K, 32]), the MLP's (``mg{l}`` [S, K, C0 + C1 + C2]) and the wide linear's as the sign of a given feature
    (``pos{l}``).  Only the head's two ReLUs, the hinge and the runner-up class are the oracle's own (``head_exclusion`` names the
    clouds where those are within rounding of flipping).  In float64 it is the yardstick of a GPU gradient, fed the GPU's choices;
    in float32 its distance from the float64 run on the same choices is e_32.  ``cut`` detaches one of the five paths of the
    coordinates (include/ifd_pc_atk.h): "wn" (a)'s WeightNet part, "mlp" (a)'s MLP-xyz part, "b" the centroids in the differences,
    "c" sa3's mean, "d" the densities.
(c) ``choices_valid``: the GPU's choices held against the float64 reference-form run: the tables must be the run's, and a gate
    may disagree with float64 only where |pre-activation| <= 8 e_act.  e_act is the float32 run's own distance from the float64
    run, layer by layer (``layer_errors``), as in atk_oracle."""
import numpy as np
import torch
import torch.nn.functional as F

import pointconv_oracle as PCO
from ifdefense_amd.weights import fold_pointconv, pointconv_layers
from pointnet2_grad_oracle import E32_FLOOR, _gates_valid, _long, _loss_fields, _t, grad_e32, head_exclusion, unpack_bits  # noqa: F401

NP1, K1, NP2, K2 = PCO.NP1, PCO.K1, PCO.NP2, PCO.K2
BW = (PCO.BW1, PCO.BW2, PCO.BW3)
TABLES = PCO.TABLES
MLP = ((64, 64, 128), (128, 128, 256), (256, 512, 1024))
LEVEL_PRE = tuple("%s%d_%d" % (net, lv, k) for lv in (1, 2, 3) for net in ("dn", "mlp", "wn") for k in range(3)) + ("lin1", "lin2", "lin3")
PRE = LEVEL_PRE + ("fc1", "fc2")
CHOICES = tuple("%s%d" % (n, lv) for lv in (1, 2, 3) for n in ("dn", "wn", "mg", "pos"))
CUTS = ("wn", "mlp", "b", "c", "d")


# ---------------------------------------------------------------------------------------------- (a) the reference form
def _stack(W, layers, h, pre, tag):
    """pointconv_oracle._stack on the rows h [rows, C]; the pre-activations go to pre[tag_k] (a single layer: pre[tag])."""
    for k, (lin, bn, (co, ci), _) in enumerate(layers):
        p = PCO._bn(W, F.linear(h, W[lin + ".weight"].reshape(co, ci), W[lin + ".bias"]), bn)
        pre[tag if len(layers) == 1 else "%s_%d" % (tag, k)] = p
        h = F.relu(p)
    return h


def _density_scale(W, layers, xyz, bw, pre, tag):
    sq = (xyz * xyz).sum(-1)
    d = (sq[:, None] + sq[None, :]) - 2.0 * (xyz @ xyz.t())
    rho = (torch.exp(-d / (2.0 * bw * bw)) / (2.5 * bw)).mean(-1)
    return _stack(W, layers, rho[:, None], pre, tag)[:, 0]


def _level(W, L, lv, grouped_xyz, feats, scale, pre):
    S, K, _ = grouped_xyz.shape
    rows = grouped_xyz if feats is None else torch.cat([grouped_xyz, feats], dim=-1)
    h = _stack(W, L[3:6], rows.reshape(S * K, -1), pre, "mlp%d" % lv).view(S, K, -1)
    wn = _stack(W, L[6:9], grouped_xyz.reshape(S * K, 3), pre, "wn%d" % lv).view(S, K, 16)
    h = h * scale[:, :, None]
    g = torch.matmul(h.permute(0, 2, 1), wn).reshape(S, -1)
    return _stack(W, L[9:10], g, pre, "lin%d" % lv)


def _reference(W, x, t):
    L = pointconv_layers()
    f1, f2, k1, k2 = (_long(t[k]) for k in TABLES)
    pre = {}
    s1 = _density_scale(W, L[0:3], x, BW[0], pre, "dn1")
    c1 = x[f1]
    p1 = _level(W, L[0:10], 1, x[k1] - c1[:, None, :], None, s1[k1], pre)
    s2 = _density_scale(W, L[10:13], c1, BW[1], pre, "dn2")
    c2 = c1[f2]
    l2 = _level(W, L[10:20], 2, c1[k2] - c2[:, None, :], p1[k2], s2[k2], pre)
    s3 = _density_scale(W, L[20:23], c2, BW[2], pre, "dn3")
    centred = c2 - c2.mean(dim=0, keepdim=True)
    g = _level(W, L[20:30], 3, centred[None], l2[None], s3[None], pre)
    pre["fc1"] = PCO._bn(W, F.linear(g, W["fc1.weight"], W["fc1.bias"]), "bn1")
    pre["fc2"] = PCO._bn(W, F.linear(F.relu(pre["fc1"]), W["fc2.weight"], W["fc2.bias"]), "bn2")
    lo = F.linear(F.relu(pre["fc2"]), W["fc3.weight"], W["fc3.bias"])
    return {"logits": lo, "dens1": s1, "dens2": s2, "dens3": s3, "l1_feat": p1, "l2_feat": l2, "global_feat": g[0], "pre": pre}


def _shape_pre(p):
    """The pre-activations in the choices' shapes: mlp / wn of sa1 [512,32,C], of sa2 [128,64,C], of sa3 [128,C]; fc [C]."""
    out = {}
    for k, v in p.items():
        if k.startswith(("mlp1", "wn1")):
            v = v.reshape(NP1, K1, -1)
        elif k.startswith(("mlp2", "wn2")):
            v = v.reshape(NP2, K2, -1)
        elif k in ("fc1", "fc2", "lin3"):
            v = v[0]
        out[k] = v
    return out


def choices_of(pre, feats):
    """The discrete choices of a set of pre-activations (``_shape_pre``'s form) in explicit()'s form."""
    ch = {}
    for lv in (1, 2, 3):
        for net, name in (("dn", "dn"), ("wn", "wn"), ("mlp", "mg")):
            ch["%s%d" % (name, lv)] = np.concatenate([pre["%s%d_%d" % (net, lv, k)] > 0 for k in range(3)], -1)
    ch["pos1"], ch["pos2"], ch["pos3"] = feats["l1_feat"] > 0, feats["l2_feat"] > 0, feats["global_feat"] > 0
    return ch


def run_cloud(W, pts, target, tables, loss="logits", kappa=0., scale=1., dtype=torch.float64):
    """One cloud [n,3].  W: pointconv_oracle.to_torch(state dict, dtype).  tables: the four index tables of the cloud.  -> dict:
    grad [n,3] = scale * d loss / d pts, logits [40], loss, hinge, other, tables, pre {name: pre-activation} (PRE), dens1 .. dens3,
    l1_feat, l2_feat, global_feat, and the run's own discrete choices in explicit()'s form (CHOICES)."""
    x0 = _t(pts, dtype)[:, :3].contiguous().requires_grad_()
    o = _reference(W, x0, tables)
    r = _loss_fields(o["logits"], target, loss, kappa, scale)
    r["grad"] = (x0.grad if x0.grad is not None else torch.zeros_like(x0)).numpy()
    r["tables"] = {k: np.asarray(tables[k]).astype(np.int64) for k in TABLES}
    with torch.no_grad():
        r["pre"] = _shape_pre({k: v.numpy() for k, v in o["pre"].items()})
        for k in ("dens1", "dens2", "dens3", "l1_feat", "l2_feat", "global_feat"):
            r[k] = o[k].numpy()
    r.update(choices_of(r["pre"], r))
    return r


# ---------------------------------------------------------------------------------------------- (b) the explicit-choice form
def folded(sd, dtype=torch.float64):
    """The BN-folded layers of a state dict (weights.fold_pointconv, float64), as tensors of ``dtype``: {name: tensor}."""
    return {k: torch.as_tensor(v).to(dtype) for k, v in fold_pointconv(sd)}


def _masked(Wf, layers, h, mask, dtype):
    """The layers on the rows h [..., C] with every ReLU replaced by its given mask [..., sum of the widths]."""
    m, at = _t(mask).to(dtype), 0
    for lin, _, (co, _), _ in layers:
        h = (h @ Wf[lin + ".weight"].t() + Wf[lin + ".bias"]) * m[..., at:at + co]
        at += co
    return h


def _density_masked(Wf, layers, xyz, bw, mask, dtype):
    """The header's density (difference form) and DensityNet under its given gates."""
    d = ((xyz[None, :, :] - xyz[:, None, :]) ** 2).sum(-1)
    rho = torch.exp(-(d / (2.0 * bw * bw))).mean(-1) / (2.5 * bw)
    return _masked(Wf, layers, rho[:, None], mask, dtype)[:, 0]


def _level_masked(Wf, L, delta_mlp, delta_wn, feats, scale, ch, lv, dtype):
    rows = delta_mlp if feats is None else torch.cat([delta_mlp, feats], dim=-1)
    h = _masked(Wf, L[3:6], rows, ch["mg%d" % lv], dtype)
    wn = _masked(Wf, L[6:9], delta_wn, ch["wn%d" % lv], dtype)
    g = torch.matmul((h * scale[..., None]).transpose(-1, -2), wn)            # [S, C, 16]
    lin = L[9][0]
    return (g.reshape(g.shape[0], -1) @ Wf[lin + ".weight"].t() + Wf[lin + ".bias"]) * _t(ch["pos%d" % lv]).to(dtype).reshape(g.shape[0], -1)


def explicit(Wf, pts, target, tables, ch, loss="logits", kappa=0., scale=1., dtype=torch.float64, cut=None):
    """One cloud [n,3] with every discrete choice of the three levels given (module docstring): ch holds CHOICES.  cut: None or one
    of CUTS, the path of the coordinates that is detached.  -> dict: grad [n,3], logits, loss, hinge, other, fc1 [512], fc2 [256]
    (the head's pre-activations), dens1 .. dens3, l1_feat, l2_feat, global_feat."""
    assert cut is None or cut in CUTS
    L = pointconv_layers()
    x0 = _t(pts, dtype)[:, :3].contiguous().requires_grad_()
    f1, f2, k1, k2 = (_long(tables[k]) for k in TABLES)
    det = lambda v, name: v.detach() if cut == name else v                    # noqa: E731
    c1 = x0[f1]
    c2 = c1[f2]
    s1 = _density_masked(Wf, L[0:3], det(x0, "d"), BW[0], ch["dn1"], dtype)
    s2 = _density_masked(Wf, L[10:13], det(c1, "d"), BW[1], ch["dn2"], dtype)
    s3 = _density_masked(Wf, L[20:23], det(c2, "d"), BW[2], ch["dn3"], dtype)
    d1 = x0[k1] - det(c1, "b")[:, None, :]
    l1 = _level_masked(Wf, L[0:10], det(d1, "mlp"), det(d1, "wn"), None, s1[k1], ch, 1, dtype)
    d2 = c1[k2] - det(c2, "b")[:, None, :]
    l2 = _level_masked(Wf, L[10:20], det(d2, "mlp"), det(d2, "wn"), l1[k2], s2[k2], ch, 2, dtype)
    d3 = (c2 - det(c2.mean(dim=0, keepdim=True), "c"))[None]
    g = _level_masked(Wf, L[20:30], det(d3, "mlp"), det(d3, "wn"), l2[None], s3[None], ch, 3, dtype)
    p1 = F.linear(g, Wf["fc1.weight"], Wf["fc1.bias"])
    p2 = F.linear(F.relu(p1), Wf["fc2.weight"], Wf["fc2.bias"])
    lo = F.linear(F.relu(p2), Wf["fc3.weight"], Wf["fc3.bias"])
    r = _loss_fields(lo, target, loss, kappa, scale)
    r["grad"] = (x0.grad if x0.grad is not None else torch.zeros_like(x0)).numpy()
    r["fc1"], r["fc2"] = p1[0].detach().numpy(), p2[0].detach().numpy()
    for k, v in (("dens1", s1), ("dens2", s2), ("dens3", s3), ("l1_feat", l1), ("l2_feat", l2), ("global_feat", g[0])):
        r[k] = v.detach().numpy()
    return r


def explicit_from(Wf, pts, target, r, **kw):
    """explicit() fed the tables and choices of a run_cloud result, or of ``gpu_choices``."""
    return explicit(Wf, pts, target, r["tables"], r, **kw)


def _dn_bits(words):
    """[n] words -> bool [n, 17]: bits 0 .. 7, 8 .. 15, 16."""
    return unpack_bits(np.asarray(words)[..., None], 17)


def gpu_choices(aux, b, n):
    """Cloud b (of n points) of PointConvClassifier.input_grad's diagnostics, on the CPU, in run_cloud's form."""
    get = lambda k: aux[k][b].cpu().numpy()                                  # noqa: E731
    ch = {"tables": {k: get(k).astype(np.int64) for k in TABLES}}
    ch["dn1"], ch["dn2"], ch["dn3"] = _dn_bits(get("dgate1")[:n]), _dn_bits(get("dgate2")), _dn_bits(get("dgate3"))
    for lv in (1, 2, 3):
        ch["wn%d" % lv] = unpack_bits(get("wgate%d" % lv)[..., None], 32)
        ch["mg%d" % lv] = unpack_bits(get("mgate%d" % lv), sum(MLP[lv - 1]))
    ch["pos1"], ch["pos2"], ch["pos3"] = get("l1_feat") > 0, get("l2_feat") > 0, get("global_feat") > 0
    return ch


# ---------------------------------------------------------------------------------------------- (c) errors, validity
def layer_errors(r32, r64):
    """e_act per layer: max |float32 run - float64 run| of the pre-activations over lists of clouds run with the SAME tables;
    'logits' too."""
    e = {k: max(float(np.abs(a["pre"][k].astype(np.float64) - b["pre"][k]).max()) for a, b in zip(r32, r64)) for k in PRE}
    e["logits"] = max(float(np.abs(a["logits"].astype(np.float64) - b["logits"]).max()) for a, b in zip(r32, r64))
    return e


def choices_valid(ch, r64, e, what=""):
    """``ch`` (gpu_choices) against the float64 run r64: the same tables, and every gate float64's own but where the
    pre-activation lies within 8 e_act of zero.  -> the worst ratio to e_act seen."""
    for k in TABLES:
        assert np.array_equal(np.asarray(ch["tables"][k]), r64["tables"][k]), "%s: table %s is not the float64 run's" % (what, k)
    p, worst = r64["pre"], 0.0
    for lv in (1, 2, 3):
        for net, name in (("dn", "dn"), ("wn", "wn"), ("mlp", "mg")):
            got, at = np.asarray(ch["%s%d" % (name, lv)]), 0
            for k in range(3):
                key = "%s%d_%d" % (net, lv, k)
                co = p[key].shape[-1]
                worst = max(worst, _gates_valid(got[..., at:at + co], p[key], e[key], "%s: %s" % (what, key)))
                at += co
            assert at == got.shape[-1], (what, name, lv, got.shape)
        worst = max(worst, _gates_valid(ch["pos%d" % lv], p["lin%d" % lv], e["lin%d" % lv], "%s: lin%d" % (what, lv)))
    return worst


def oracle_case(sd, clouds, targets, loss="logits", kappa=0., scale=1., starts=None, tables=None):
    """Both reference-form runs of a list of clouds on the same tables (per cloud: ``tables``, else the oracle's own float32
    selection from ``starts``) -> (r32, r64, e_act, exclusions): what a parity case needs that does not depend on the GPU."""
    W32, W64 = PCO.to_torch(sd, torch.float32), PCO.to_torch(sd, torch.float64)
    if tables is None:
        tables = [PCO.tables_of_cloud(c, (0, 0) if starts is None else tuple(int(v) for v in starts[i])) for i, c in enumerate(clouds)]
    r32 = [run_cloud(W32, c, t, tb, loss, kappa, scale, torch.float32) for c, t, tb in zip(clouds, targets, tables)]
    r64 = [run_cloud(W64, c, t, tb, loss, kappa, scale, torch.float64) for c, t, tb in zip(clouds, targets, tables)]
    e = layer_errors(r32, r64)
    return r32, r64, e, [head_exclusion(r, e, loss) for r in r64]
