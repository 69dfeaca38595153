"""Torch-CPU restatement of the reference's PU-Net forward (baselines/defense/DUP_Net/pu_net.py:88-132, pu_modules.py,
pu_utils.py; PUNet(npoint=1024, up_ratio=4, use_bn=False, use_res=False)) for the parity tests of ifd_punet_forward.

Test infrastructure only (product code never imports it).  Runs in float32 or float64; every discrete decision (FPS
indices, ball-query members, FP 3-NN) can be injected, so the float64 run can follow the GPU's decisions and measure only
its arithmetic.  dist_form selects the squared distances of the ball query and the 3-NN: "torch" is the reference's
expanded form -2 s.d + |s|^2 + |d|^2 (pu_utils.py:24-27), "elementwise" the direct sum of squared differences.
dist_dtype computes those distances in a type of their own: float32 distances under float64 arithmetic are "the
reference's distances, exact arithmetic after them", which keeps the expanded form's float32 noise at coinciding points (it
decides the 3-NN weights 1 / (d + 1e-8) there) out of the error a float64 comparison measures.  make_weights gives dense
seeded weights: the shipped checkpoint leaves a third of its channels dead, and a dead channel hides a wrong column map.
"""
import glob
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
NPOINTS = (1024, 512, 256, 128)
RADII = (0.05, 0.1, 0.2, 0.3)
NSAMPLE = 32
LEVEL_OFF = (0, 1024, 1536, 1792)
# (name, out channels, in channels) of every 1x1 conv in state_dict order; each has .conv.weight [out,in,1,1], .conv.bias [out]
LAYERS = tuple(
    [("SA_modules.%d.mlps.0.layer%d" % (v, j), o, i) for v, io in enumerate((((32, 3), (32, 32), (64, 32)),
                                                                            ((64, 67), (64, 64), (128, 64)),
                                                                            ((128, 131), (128, 128), (256, 128)),
                                                                            ((256, 259), (256, 256), (512, 256))))
     for j, (o, i) in enumerate(io)] +
    [("FP_Modules.%d.mlp.layer0" % f, 64, c) for f, c in enumerate((128, 256, 512))] +
    [("FC_Modules.%d.layer%d" % (k, j), o, i) for k in range(4) for j, (o, i) in enumerate(((256, 259), (128, 256)))] +
    [("pcd_layer.0.layer0", 64, 128), ("pcd_layer.1.layer0", 3, 64)])
DEAD = 1e-6


def load_weights():
    """The shipped checkpoint pu-in_1024-up_4.pth as {name: float32 array} (tests/golden/punet_weights_*.npz)."""
    sd = {}
    for f in sorted(glob.glob(os.path.join(HERE, "golden", "punet_weights_*.npz"))):
        with np.load(f) as z:
            sd.update({k: z[k] for k in z.files})
    return sd


def dead_channels(w, eps=DEAD):
    """(dead output rows, dead input columns) of a [out,in,1,1] weight: indices whose largest magnitude is below eps."""
    m = np.abs(np.asarray(w).reshape(w.shape[0], -1))
    return np.flatnonzero(m.max(1) < eps), np.flatnonzero(m.max(0) < eps)


def make_weights(seed):
    """A dense PU-Net state dict with the shipped checkpoint's names and shapes: weights uniform in +-sqrt(6 / fan_in),
    biases uniform in +-0.1, float32, drawn in state_dict order from numpy.random.default_rng(seed).  No dead row or column."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, o, i in LAYERS:
        a = np.sqrt(6.0 / i)
        w = rng.uniform(-a, a, (o, i, 1, 1)).astype(np.float32)
        rows, cols = dead_channels(w)
        assert rows.size == 0 and cols.size == 0, "%s: dead rows %s, dead columns %s" % (name, rows, cols)
        sd[name + ".conv.weight"] = w
        sd[name + ".conv.bias"] = rng.uniform(-0.1, 0.1, o).astype(np.float32)
    return sd


def square_distance(src, dst, dist_form="torch"):
    """pu_utils.py:7-31 ([B,N,3] x [B,M,3] -> [B,N,M])."""
    if dist_form == "elementwise":
        return ((src[:, :, None, :] - dst[:, None, :, :]) ** 2).sum(-1)
    B, N, _ = src.shape
    M = dst.shape[1]
    dist = -2 * torch.matmul(src, dst.permute(0, 2, 1))
    dist += torch.sum(src ** 2, -1).view(B, N, 1)
    dist += torch.sum(dst ** 2, -1).view(B, 1, M)
    return dist


def index_points(points, idx):
    """pu_utils.py:34-52."""
    B = points.shape[0]
    view = [B] + [1] * (idx.dim() - 1)
    return points[torch.arange(B, device=points.device).view(view).expand_as(idx), idx]


def farthest_point_sample(xyz, npoint, start):
    """pu_utils.py:55-74 with the start index given (torch.randint(0, N, (B,)) of the reference)."""
    B, N, _ = xyz.shape
    start = torch.as_tensor(start)
    if bool((start < 0).any()) or bool((start >= N).any()):       # checked here: a GPU gather does not check its indices
        raise ValueError("FPS start index outside [0, %d)" % N)
    centroids = torch.zeros(B, npoint, dtype=torch.long, device=xyz.device)
    distance = torch.ones(B, N, dtype=xyz.dtype, device=xyz.device) * 1e10
    farthest = start.long().to(xyz.device).clone()
    bi = torch.arange(B, device=xyz.device)
    for i in range(npoint):
        centroids[:, i] = farthest
        c = xyz[bi, farthest, :].view(B, 1, 3)
        dist = torch.sum((xyz - c) ** 2, -1)
        mask = dist < distance
        distance[mask] = dist[mask]
        farthest = torch.max(distance, -1)[1]
    return centroids


def distance_in(src, dst, dist_form, dist_dtype):
    """square_distance computed in dist_dtype (None: the operands' own type); the caller casts the result."""
    if dist_dtype is None:
        return square_distance(src, dst, dist_form)
    return square_distance(src.to(dist_dtype), dst.to(dist_dtype), dist_form)


def query_ball_point(radius, xyz, new_xyz, dist_form="torch", dist_dtype=None):
    """pu_utils.py:77-98 (the comparison with radius^2 is made in the distances' own type)."""
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    group_idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat([B, S, 1])
    d = distance_in(new_xyz, xyz, dist_form, dist_dtype)
    group_idx[d > radius ** 2] = N
    group_idx = group_idx.sort(dim=-1)[0][:, :, :NSAMPLE]
    first = group_idx[:, :, 0].view(B, S, 1).repeat([1, 1, NSAMPLE])
    mask = group_idx == N
    group_idx[mask] = first[mask]
    return group_idx


def shared_mlp(x, layers, last_relu=True, log=None, names=()):
    """SharedMLP of 1x1 Conv2d with bias (pytorch_modules.py), x [B, C, n, s].  log[names[i]] (optional) receives each
    layer's largest output per channel [C]: a unit whose entry is 0 after its ReLU never fires on these clouds."""
    for i, (w, b) in enumerate(layers):
        x = F.conv2d(x, w, b)
        if last_relu or i < len(layers) - 1:
            x = F.relu(x)
        if log is not None:
            log[names[i]] = x.amax(dim=(0, 2, 3))
    return x


def _layers(W, names):
    return [(W[n + ".conv.weight"], W[n + ".conv.bias"]) for n in names]


def to_torch(sd, dtype=torch.float32):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}


def three_nn(xyz, known, dtype, dist_form="torch", dist_dtype=None, idx=None):
    """The 3 nearest `known` of every point (pu_modules.py:157-171): (squared distances cast to dtype, indices)."""
    d = distance_in(xyz, known, dist_form, dist_dtype)
    if idx is not None:
        d = torch.gather(d, 2, idx)
    else:
        d, idx = d.sort(dim=-1)
        d, idx = d[:, :, :3], idx[:, :, :3]
    return d.to(dtype), idx


def decisions(xyz, fps_start=None, dtype=torch.float32, dist_form="torch", dist_dtype=None, fps_idx=None):
    """The discrete decisions forward() takes on xyz, without the MLPs (none depends on the weights): the same record
    keys and layouts, plus "l_xyz", the list of the five levels' coordinates."""
    xyz = torch.as_tensor(xyz).to(dtype)
    rec = {"fps_idx": [], "ball_idx": [], "knn_idx": []}
    l_xyz = [xyz]
    for k in range(4):
        x, S = l_xyz[k], NPOINTS[k]
        if fps_idx is not None:
            fi = torch.as_tensor(fps_idx)[:, LEVEL_OFF[k]:LEVEL_OFF[k] + S].long()
        else:
            fi = farthest_point_sample(x, S, torch.as_tensor(fps_start)[:, k])
        new_xyz = index_points(x, fi)
        rec["fps_idx"].append(fi)
        rec["ball_idx"].append(query_ball_point(RADII[k], x, new_xyz, dist_form, dist_dtype))
        l_xyz.append(new_xyz)
    for k in range(3):
        rec["knn_idx"].append(three_nn(xyz, l_xyz[k + 2], dtype, dist_form, dist_dtype)[1])
    return {"fps_idx": torch.cat(rec["fps_idx"], 1).int(), "ball_idx": torch.cat(rec["ball_idx"], 1).int(),
            "knn_idx": torch.stack(rec["knn_idx"], 1).int(), "l_xyz": l_xyz}


def forward(W, xyz, fps_start=None, dtype=torch.float32, dist_form="torch", fps_idx=None, ball_idx=None, knn_idx=None,
            dist_dtype=None):
    """PUNet.forward (pu_net.py:88-132): xyz [B,1024,3] -> ([B,4096,3], record).  fps_start [B,4] (the reference's draws);
    fps_idx [B,1920], ball_idx [B,1920,32], knn_idx [B,3,1024,3] (optional): inject the decisions.  dist_dtype (optional):
    the squared distances of the 3-NN weights (and of the ball query and the 3-NN order where those are not injected) are
    computed in it, in dist_form, and then cast to dtype.  record holds the decisions taken: fps_idx, ball_idx, knn_idx
    (same layouts as ifd_punet_aux), and the float-valued intermediates: l_feats (l_feats[1..4], each [B,C,S]), up (the
    three FP outputs [B,64,1024]), knn_w (the normalised 3-NN weights [B,3,1024,3]) and act_max ({layer name: each output
    channel's largest value over these clouds})."""
    W = {k: v.to(dtype) for k, v in W.items()}
    xyz = torch.as_tensor(xyz).to(dtype)
    B = xyz.shape[0]
    rec = {"fps_idx": [], "ball_idx": [], "knn_idx": [], "knn_w": []}
    act = {}
    l_xyz, l_feats = [xyz], [None]
    for k in range(4):
        x, feats = l_xyz[k], l_feats[k]
        S = NPOINTS[k]
        if fps_idx is not None:
            fi = torch.as_tensor(fps_idx)[:, LEVEL_OFF[k]:LEVEL_OFF[k] + S].long()
        else:
            fi = farthest_point_sample(x, S, torch.as_tensor(fps_start)[:, k])
        new_xyz = index_points(x, fi)
        if ball_idx is not None:
            gi = torch.as_tensor(ball_idx)[:, LEVEL_OFF[k]:LEVEL_OFF[k] + S].long()
        else:
            gi = query_ball_point(RADII[k], x, new_xyz, dist_form, dist_dtype)
        grouped = index_points(x, gi) - new_xyz.unsqueeze(2)
        if feats is not None:
            grouped = torch.cat([grouped, index_points(feats.transpose(1, 2).contiguous(), gi)], dim=-1)
        g = grouped.permute(0, 3, 1, 2)
        names = ["SA_modules.%d.mlps.0.layer%d" % (k, j) for j in range(3)]
        nf = F.max_pool2d(shared_mlp(g, _layers(W, names), log=act, names=names), kernel_size=[1, NSAMPLE]).squeeze(-1)
        l_xyz.append(new_xyz)
        l_feats.append(nf)
        rec["fps_idx"].append(fi)
        rec["ball_idx"].append(gi)
    up = []
    for k in range(3):
        known, kf = l_xyz[k + 2], l_feats[k + 2].permute(0, 2, 1)
        d, idx = three_nn(xyz, known, dtype, dist_form, dist_dtype,
                          None if knn_idx is None else torch.as_tensor(knn_idx)[:, k].long())
        w = 1.0 / (d + 1e-8)
        w = w / torch.sum(w, dim=-1).view(B, -1, 1)
        rec["knn_w"].append(w)
        interp = torch.sum(index_points(kf, idx) * w.view(B, -1, 3, 1), dim=2)
        f = interp.permute(0, 2, 1).unsqueeze(-1)
        names = ["FP_Modules.%d.mlp.layer0" % k]
        up.append(shared_mlp(f, _layers(W, names), log=act, names=names).squeeze(-1))
        rec["knn_idx"].append(idx)
    feats = torch.cat([xyz.transpose(1, 2).contiguous(), l_feats[1], *up], dim=1).unsqueeze(-1)
    r = []
    for k in range(4):
        names = ["FC_Modules.%d.layer%d" % (k, j) for j in range(2)]
        r.append(shared_mlp(feats, _layers(W, names), log=act, names=names))
    r = torch.cat(r, dim=2)
    out = shared_mlp(r, _layers(W, ["pcd_layer.0.layer0"]), log=act, names=["pcd_layer.0.layer0"])
    out = shared_mlp(out, _layers(W, ["pcd_layer.1.layer0"]), last_relu=False, log=act, names=["pcd_layer.1.layer0"])
    rec = {"fps_idx": torch.cat(rec["fps_idx"], 1).int(), "ball_idx": torch.cat(rec["ball_idx"], 1).int(),
           "knn_idx": torch.stack(rec["knn_idx"], 1).int(), "knn_w": torch.stack(rec["knn_w"], 1),
           "l_feats": l_feats[1:], "up": up, "act_max": act}
    return out.squeeze(-1).transpose(1, 2).contiguous(), rec


# ---------------------------------------------------------------------------------------------- decisions, attributed
def level_inputs(l_xyz):
    """(query points, candidate points, radius or None) of the seven distance matrices of one forward: the four ball
    queries (centroids of level k against level k's input) and the three 3-NN searches (input points against centroids)."""
    return [(l_xyz[k + 1], l_xyz[k], RADII[k]) for k in range(4)] + [(l_xyz[0], l_xyz[k + 2], None) for k in range(3)]


def exact_distances(l_xyz):
    """The seven distance matrices in float64, direct form: what the decisions would be taken on without rounding."""
    return [square_distance(q.double(), c.double(), "elementwise") for q, c, _ in level_inputs(l_xyz)]


def distance_band(l_xyz, exact=None):
    """Per cloud [B]: twice the largest |float32 expanded form - float64| over that cloud's seven distance matrices.  A
    decision may go either way only where the float64 distances are closer than this to the threshold or to each other."""
    exact = exact_distances(l_xyz) if exact is None else exact
    worst = torch.zeros(l_xyz[0].shape[0], dtype=torch.float64)
    for (q, c, _), e in zip(level_inputs(l_xyz), exact):
        d32 = square_distance(q.float(), c.float(), "torch").double()
        worst = torch.maximum(worst, (d32 - e).abs().flatten(1).max(1)[0])
    return 2 * worst


def ball_row_allowed(row, d, r2, band):
    """Is `row` (32 indices) a ball-query answer for the float64 distances d [N] when membership is free only within
    band of r2?  Members ascend strictly, then the first member fills; no member is surely outside; no point before the
    last member (before the end, if the ball did not fill) is surely inside and left out."""
    row = np.asarray(row).astype(np.int64)
    d = np.asarray(d)
    N = d.shape[0]
    if row.min() < 0 or row.max() >= N:
        return False
    c = 1
    while c < NSAMPLE and row[c] > row[c - 1]:
        c += 1
    if not (row[c:] == row[0]).all():
        return False
    mem = row[:c]
    if (d[mem] > r2 + band).any():
        return False
    end = mem[-1] + 1 if c == NSAMPLE else N
    skipped = np.ones(end, bool)
    skipped[mem] = False
    return not (d[:end][skipped] < r2 - band).any()


def knn_row_allowed(row, d, band):
    """Is `row` (3 indices) a 3-NN answer for the float64 distances d [M] when order is free only among distances within
    band of each other?  Distinct, ascending up to band, and nothing left out is nearer than the third by more than band."""
    row = np.asarray(row).astype(np.int64)
    d = np.asarray(d)
    if row.min() < 0 or row.max() >= d.shape[0] or len(set(row.tolist())) != 3:
        return False
    a, b, c = d[row]
    if a > b + band or b > c + band or a > c + band:
        return False
    rest = np.ones(d.shape[0], bool)
    rest[row] = False
    return not (d[rest] < c - band).any()


def first_coinciding(pts):
    """[M,3] -> [M]: for each point the lowest index of a point with the same coordinates, bit for bit."""
    _, inv = np.unique(np.asarray(pts), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    first = np.full(inv.max() + 1, len(inv))
    np.minimum.at(first, inv, np.arange(len(inv)))
    return first[inv]


def attribute_decisions(got, ref, exact, band, l_xyz):
    """Compare decisions `got` with `ref` (records of the same clouds, same fps_idx) row by row.  Returns
    (ball rows differing, knn rows differing, list of unattributable rows as text): a differing row is attributable when
    ball_row_allowed / knn_row_allowed accepts it on the float64 distances `exact` with the cloud's `band`.

    3-NN rows are compared after each index is replaced by the lowest index of a coinciding centroid (first_coinciding).
    Coinciding centroids have equal distances in every form and equal features (same coordinates, same ball), and the
    reference's own choice among them is not defined: its torch.sort is unstable, and on an all-equal row of 128 or more it
    returns neither index order nor any order a kernel could restate (512 zeros -> 336, 351, 350, ...)."""
    bad = []
    gb, rb = got["ball_idx"].numpy(), ref["ball_idx"].numpy()
    bd = np.argwhere((gb != rb).any(-1))
    for b, w in bd:
        k = max(v for v in range(4) if LEVEL_OFF[v] <= w)
        d = exact[k][b, w - LEVEL_OFF[k]].numpy()
        if not ball_row_allowed(gb[b, w], d, RADII[k] ** 2, float(band[b])):
            bad.append("cloud %d level %d centroid %d (band %.3e, r^2 %.6e):\n  got %s\n  ref %s\n  d64(got) %s" % (
                b, k, w - LEVEL_OFF[k], float(band[b]), RADII[k] ** 2, gb[b, w].tolist(), rb[b, w].tolist(),
                d[np.clip(gb[b, w], 0, d.shape[0] - 1)].tolist()))
    gk, rk = got["knn_idx"].numpy(), ref["knn_idx"].numpy()
    same = np.ones(gk.shape[:3], bool)
    for b in range(gk.shape[0]):
        for f in range(3):
            canon = first_coinciding(l_xyz[f + 2][b].numpy())
            same[b, f] = (canon[np.clip(gk[b, f], 0, len(canon) - 1)] == canon[rk[b, f]]).all(-1) & \
                ((gk[b, f] >= 0) & (gk[b, f] < len(canon))).all(-1)
    kd = np.argwhere(~same)
    for b, f, i in kd:
        d = exact[4 + f][b, i].numpy()
        if not knn_row_allowed(gk[b, f, i], d, float(band[b])):
            bad.append("cloud %d FP %d point %d (band %.3e): got %s d64 %s, ref %s d64 %s" % (
                b, f, i, float(band[b]), gk[b, f, i].tolist(), d[np.clip(gk[b, f, i], 0, d.shape[0] - 1)].tolist(),
                rk[b, f, i].tolist(), d[rk[b, f, i]].tolist()))
    return len(bd), len(kd), bad
