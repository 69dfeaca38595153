"""Torch-CPU restatement of the reference's PU-Net forward (baselines/defense/DUP_Net/pu_net.py:88-132, pu_modules.py,
pu_utils.py; PUNet(npoint=1024, up_ratio=4, use_bn=False, use_res=False)) for the parity tests of ifd_punet_forward.

Test infrastructure only (product code never imports it).  Runs in float32 or float64; every discrete decision (FPS
indices, ball-query members, FP 3-NN) can be injected, so the float64 run can follow the GPU's decisions and measure only
its arithmetic.  dist_form selects the squared distances of the ball query and the 3-NN: "torch" is the reference's
expanded form -2 s.d + |s|^2 + |d|^2 (pu_utils.py:24-27), "elementwise" the direct sum of squared differences.
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


def load_weights():
    """The shipped checkpoint pu-in_1024-up_4.pth as {name: float32 array} (tests/golden/punet_weights_*.npz)."""
    sd = {}
    for f in sorted(glob.glob(os.path.join(HERE, "golden", "punet_weights_*.npz"))):
        with np.load(f) as z:
            sd.update({k: z[k] for k in z.files})
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


def query_ball_point(radius, xyz, new_xyz, dist_form="torch"):
    """pu_utils.py:77-98."""
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    group_idx = torch.arange(N, device=xyz.device).view(1, 1, N).repeat([B, S, 1])
    d = square_distance(new_xyz, xyz, dist_form)
    group_idx[d > radius ** 2] = N
    group_idx = group_idx.sort(dim=-1)[0][:, :, :NSAMPLE]
    first = group_idx[:, :, 0].view(B, S, 1).repeat([1, 1, NSAMPLE])
    mask = group_idx == N
    group_idx[mask] = first[mask]
    return group_idx


def shared_mlp(x, layers, last_relu=True):
    """SharedMLP of 1x1 Conv2d with bias (pytorch_modules.py), x [B, C, n, s]."""
    for i, (w, b) in enumerate(layers):
        x = F.conv2d(x, w, b)
        if last_relu or i < len(layers) - 1:
            x = F.relu(x)
    return x


def to_torch(sd, dtype=torch.float32):
    return {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}


def forward(W, xyz, fps_start=None, dtype=torch.float32, dist_form="torch", fps_idx=None, ball_idx=None, knn_idx=None):
    """PUNet.forward (pu_net.py:88-132): xyz [B,1024,3] -> ([B,4096,3], record).  fps_start [B,4] (the reference's draws);
    fps_idx [B,1920], ball_idx [B,1920,32], knn_idx [B,3,1024,3] (optional): inject the decisions.  record holds the
    decisions taken: fps_idx, ball_idx, knn_idx (same layouts as ifd_punet_aux)."""
    W = {k: v.to(dtype) for k, v in W.items()}
    xyz = torch.as_tensor(xyz).to(dtype)
    B = xyz.shape[0]
    rec = {"fps_idx": [], "ball_idx": [], "knn_idx": []}
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
            gi = query_ball_point(RADII[k], x, new_xyz, dist_form)
        grouped = index_points(x, gi) - new_xyz.unsqueeze(2)
        if feats is not None:
            grouped = torch.cat([grouped, index_points(feats.transpose(1, 2).contiguous(), gi)], dim=-1)
        g = grouped.permute(0, 3, 1, 2)
        layers = [(W["SA_modules.%d.mlps.0.layer%d.conv.weight" % (k, j)], W["SA_modules.%d.mlps.0.layer%d.conv.bias" % (k, j)])
                  for j in range(3)]
        nf = F.max_pool2d(shared_mlp(g, layers), kernel_size=[1, NSAMPLE]).squeeze(-1)
        l_xyz.append(new_xyz)
        l_feats.append(nf)
        rec["fps_idx"].append(fi)
        rec["ball_idx"].append(gi)
    up = []
    for k in range(3):
        known, kf = l_xyz[k + 2], l_feats[k + 2].permute(0, 2, 1)
        d = square_distance(xyz, known, dist_form)
        if knn_idx is not None:
            idx = torch.as_tensor(knn_idx)[:, k].long()
            d = torch.gather(d, 2, idx)
        else:
            d, idx = d.sort(dim=-1)
            d, idx = d[:, :, :3], idx[:, :, :3]
        w = 1.0 / (d + 1e-8)
        w = w / torch.sum(w, dim=-1).view(B, -1, 1)
        interp = torch.sum(index_points(kf, idx) * w.view(B, -1, 3, 1), dim=2)
        f = interp.permute(0, 2, 1).unsqueeze(-1)
        up.append(shared_mlp(f, [(W["FP_Modules.%d.mlp.layer0.conv.weight" % k], W["FP_Modules.%d.mlp.layer0.conv.bias" % k])])
                  .squeeze(-1))
        rec["knn_idx"].append(idx)
    feats = torch.cat([xyz.transpose(1, 2).contiguous(), l_feats[1], *up], dim=1).unsqueeze(-1)
    r = [shared_mlp(feats, [(W["FC_Modules.%d.layer%d.conv.weight" % (k, j)], W["FC_Modules.%d.layer%d.conv.bias" % (k, j)])
                            for j in range(2)]) for k in range(4)]
    r = torch.cat(r, dim=2)
    out = shared_mlp(r, [(W["pcd_layer.0.layer0.conv.weight"], W["pcd_layer.0.layer0.conv.bias"])])
    out = shared_mlp(out, [(W["pcd_layer.1.layer0.conv.weight"], W["pcd_layer.1.layer0.conv.bias"])], last_relu=False)
    rec = {"fps_idx": torch.cat(rec["fps_idx"], 1).int(), "ball_idx": torch.cat(rec["ball_idx"], 1).int(),
           "knn_idx": torch.stack(rec["knn_idx"], 1).int()}
    return out.squeeze(-1).transpose(1, 2).contiguous(), rec
