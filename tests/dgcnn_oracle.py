"""DGCNN(emb_dims=1024, k, output_channels=40, use_bn=True) in eval mode restated in torch functional ops, the test oracle of
the DGCNN victim (include/ifd_dgcnn.h).  It follows baselines/model/dgcnn.py op for op (pairwise_distance and topk; gather, cat
of (x_j - x_i, x_i), conv2d -> batch_norm -> leaky_relu, max over the neighbours; conv1d, max and average pooling, the linear
head) so that in float32 it repeats the reference's rounding, and runs in float64 as the yardstick of the GPU's arithmetic.  It
is device-free (the reference hard-codes torch.device('cuda') in get_graph_feature).

``idx``: the neighbour sets of the four edge convolutions can be forced, the seam the reference's get_graph_feature(idx=...)
has.  A flipped neighbour moves the logits by far more than the arithmetic does, so the arithmetic of an implementation is judged
with ITS choice of neighbours forced into the float32 and the float64 oracle alike.

Weights: ``make_weights(seed)`` draws the un-folded state_dict from numpy's default_rng(seed + 9101), layers in network order
(ifdefense_amd.weights.dgcnn_layers): weight (and bias where the layer has one) U(+-1/sqrt(fan_in)), then the layer's BatchNorm,
under its module key ``bnN``: gamma 1 + U(+-0.2), beta U(+-0.1), running_mean N(0, 0.1), running_var U(0.5, 1.25).  A dict
WITHOUT BatchNorm keys (weights.fold_dgcnn's output) runs the same network with the BatchNorms left out.

``make_calibrated_weights(seed)``: make_weights with linear3 alone replaced, by the recipe of pointnet_oracle.make_calibrated_weights:
with h [140,256] the float64 oracle's post-LeakyReLU linear2 output on bench.synth_clouds(140, seed=31)[:, :128], mu = h.mean(0),
s = h.std(0), live = s > 1e-6 max(s):
    linear3.weight <- linear3.weight * where(live, 1/s, 0)[None,:] * sqrt(3 * 256 / live.sum()),  linear3.bias <- -(linear3.weight @ mu),
rounded to float32, so that the predicted class varies from cloud to cloud.  ``make_tied_weights`` copies linear3's rows 0..19
onto 20..39: 20 exact ties in every cloud's logits."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from ifdefense_amd.weights import BN_EPS, dgcnn_layers

K_DEFAULT = 20


def make_weights(seed=0):
    rng = np.random.default_rng(seed + 9101)
    w = {}
    for lin, bn, (co, ci), ones, has_bias in dgcnn_layers():
        b = 1.0 / np.sqrt(ci)
        w[lin + ".weight"] = rng.uniform(-b, b, size=(co, ci) + (1,) * ones).astype(np.float32)
        if has_bias:
            w[lin + ".bias"] = rng.uniform(-b, b, size=(co,)).astype(np.float32)
        if bn:
            w[bn[0] + ".weight"] = (1.0 + rng.uniform(-0.2, 0.2, co)).astype(np.float32)
            w[bn[0] + ".bias"] = rng.uniform(-0.1, 0.1, co).astype(np.float32)
            w[bn[0] + ".running_mean"] = rng.normal(0.0, 0.1, co).astype(np.float32)
            w[bn[0] + ".running_var"] = rng.uniform(0.5, 1.25, co).astype(np.float32)
    return w


CALIBRATION_CLOUDS, CALIBRATION_SEED, CALIBRATION_POINTS = 140, 31, 128


@functools.lru_cache(maxsize=None)
def _calibrated_linear3(seed, k):
    import bench
    w = make_weights(seed)
    W = to_torch(w, torch.float64)
    x = bench.synth_clouds(CALIBRATION_CLOUDS, seed=CALIBRATION_SEED)[:, :CALIBRATION_POINTS]
    h = torch.cat([forward(W, x[a:a + 28], dtype=torch.float64, k=k)["h2"] for a in range(0, len(x), 28)]).numpy()
    mu, s = h.mean(0), h.std(0)
    live = s > 1e-6 * s.max()
    inv = np.where(live, 1.0 / np.where(live, s, 1.0), 0.0)
    w3 = w["linear3.weight"].astype(np.float64) * inv[None, :] * np.sqrt(3.0 * 256 / live.sum())
    return w3.astype(np.float32), (-(w3 @ mu)).astype(np.float32), int(live.sum())


def make_calibrated_weights(seed=0, k=K_DEFAULT):
    """make_weights(seed) with linear3 rescaled so that the predicted class varies from cloud to cloud (module docstring).
    Deterministic; the calibration pass is computed once per (seed, k) and cached."""
    w = make_weights(seed)
    w3, b3, _ = _calibrated_linear3(int(seed), int(k))
    w["linear3.weight"], w["linear3.bias"] = w3.copy(), b3.copy()
    return w


def make_tied_weights(w):
    """A copy of ``w`` in which classes 20..39 are bit-identical twins of classes 0..19 (linear3's rows and biases copied)."""
    w = {k: np.array(v, copy=True) for k, v in w.items()}
    w["linear3.weight"][20:40] = w["linear3.weight"][0:20]
    w["linear3.bias"][20:40] = w["linear3.bias"][0:20]
    return w


def reference_state_dict(w):
    """make_weights' dict as nn.DataParallel saves the reference's model: torch tensors, ``module.`` prefix, every BatchNorm under
    both of its keys (``bnN.*`` and the Sequential's ``convN.1.*`` / ``linearN.1.*``), num_batches_tracked counters."""
    both = {}
    for _, bn, _, _, _ in dgcnn_layers():
        if bn:
            both[bn[0]] = bn[1]
    sd = {}
    for k, v in w.items():
        names = [k]
        head, _, field = k.rpartition(".")
        if head in both:
            names.append(both[head] + "." + field)
        for n in names:
            sd["module." + n] = torch.from_numpy(np.asarray(v))
            if n.endswith(".running_var"):
                sd["module." + n[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    return sd


def to_torch(w, dtype=torch.float32):
    return {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items()}


def _tensor(t):
    return t if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))


def knn(x, k):
    """x [B,C,N] -> idx [B,N,k], the reference's knn()."""
    inner = -2 * torch.matmul(x.transpose(2, 1), x)
    xx = torch.sum(x ** 2, dim=1, keepdim=True)
    pairwise_distance = -xx - inner - xx.transpose(2, 1)
    return pairwise_distance.topk(k=k, dim=-1)[1]


def graph_feature(x, k, idx=None):
    """x [B,C,N] -> ([B,2C,N,k] = (x_j - x_i, x_i), idx [B,N,k])."""
    B, C, N = x.shape
    if idx is None:
        idx = knn(x, k)
    idx = idx.long()
    flat = (idx + torch.arange(0, B, device=x.device).view(-1, 1, 1) * N).view(-1)
    xt = x.transpose(2, 1).contiguous()
    feature = xt.view(B * N, -1)[flat, :].view(B, N, k, C)
    xr = xt.view(B, N, 1, C).repeat(1, 1, k, 1)
    return torch.cat((feature - xr, xr), dim=3).permute(0, 3, 1, 2), idx


def _bn(W, x, bn):
    for name in bn or ():
        if (name + ".running_var") in W:
            return F.batch_norm(x, W[name + ".running_mean"], W[name + ".running_var"], W[name + ".weight"], W[name + ".bias"],
                                False, 0.0, BN_EPS)
    return x


def _forward_batch(W, x, k, idx):
    L = dgcnn_layers()
    chosen, xs = [], []
    h = x
    for l in range(4):
        lin, bn, (co, ci), _, _ = L[l]
        e, ix = graph_feature(h, k, None if idx is None or idx[l] is None else idx[l])
        chosen.append(ix)
        e = F.conv2d(e, W[lin + ".weight"].reshape(co, ci, 1, 1), W.get(lin + ".bias"))
        e = F.leaky_relu(_bn(W, e, bn), negative_slope=0.2)
        h = e.max(dim=-1, keepdim=False)[0]
        xs.append(h)
    feat = torch.cat(xs, dim=1)
    lin, bn, (co, ci), _, _ = L[4]
    y = F.leaky_relu(_bn(W, F.conv1d(feat, W[lin + ".weight"].reshape(co, ci, 1), W.get(lin + ".bias")), bn), negative_slope=0.2)
    B = y.shape[0]
    g = torch.cat((F.adaptive_max_pool1d(y, 1).view(B, -1), F.adaptive_avg_pool1d(y, 1).view(B, -1)), 1)
    h1 = F.leaky_relu(_bn(W, F.linear(g, W[L[5][0] + ".weight"], W.get(L[5][0] + ".bias")), L[5][1]), negative_slope=0.2)
    h2 = F.leaky_relu(_bn(W, F.linear(h1, W[L[6][0] + ".weight"], W.get(L[6][0] + ".bias")), L[6][1]), negative_slope=0.2)
    lo = F.linear(h2, W["linear3.weight"], W["linear3.bias"])
    return {"logits": lo, "feat": feat.transpose(1, 2).contiguous(), "global_feat": g, "idx": chosen, "h2": h2}


def forward(W, x, n_points=None, dtype=torch.float32, k=K_DEFAULT, idx=None):
    """x: [B,N,3] (point-major) or a list of [K_i,3]; n_points: [B] valid rows of each cloud.  idx: None, or four [B,N,k] index
    tensors (None entries are left to the oracle) that force the neighbour sets; of a ragged batch the first n_points[b] rows of
    cloud b are used.  -> {"logits" [B,40], "feat" [B,N,512] (a list of [K_i,512] for ragged input), "global_feat" [B,2048],
    "idx" four [B,N,k] (lists for ragged input), "h2" [B,256]} in ``dtype`` (W must be in it)."""
    with torch.no_grad():
        if isinstance(x, (list, tuple)) or n_points is not None:
            clouds = [c if torch.is_tensor(c) else torch.as_tensor(np.asarray(c)) for c in x]
            if n_points is not None:
                clouds = [c[:int(n)] for c, n in zip(clouds, n_points)]
            outs = []
            for b, c in enumerate(clouds):
                ib = None if idx is None else [None if t is None else _tensor(t[b])[None, :len(c)] for t in idx]
                outs.append(_forward_batch(W, c.to(dtype)[None, :, :3].transpose(1, 2).contiguous(), k, ib))
            return {"logits": torch.cat([o["logits"] for o in outs]), "global_feat": torch.cat([o["global_feat"] for o in outs]),
                    "h2": torch.cat([o["h2"] for o in outs]), "feat": [o["feat"][0] for o in outs],
                    "idx": [[o["idx"][l][0] for o in outs] for l in range(4)]}
        x = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(dtype)
        ib = None if idx is None else [None if t is None else _tensor(t) for t in idx]
        return _forward_batch(W, x[:, :, :3].transpose(1, 2).contiguous(), k, ib)


# ---- the neighbour-validity check shared by tests/test_dgcnn_cpu.py and tests/test_gpu_dgcnn.py -------------------------
def exact_scores(x):
    """x [n,C] (any float dtype) -> s [n,n] float64, s_ij = 2 <x_i, x_j> - |x_j|^2."""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 * (x @ x.T) - (x * x).sum(1)[None, :]


def gamma(m):
    u = m * 2.0 ** -24
    return u / (1.0 - u)


def check_neighbours(x, idx, k, what=""):
    """idx [n,k] chosen for the layer input x [n,C] (f32 values): every row holds k distinct indices in [0, n), and the smallest
    exact score chosen is >= the largest exact score left out - 2 tau_i, tau_i = gamma_{C+2} (|x_i| + max_j |x_j|)^2: the standard
    bound of a C-term dot product and the three-term combination in f32, whatever the summation order."""
    x = np.asarray(x, dtype=np.float64)
    idx = np.asarray(idx).astype(np.int64)
    n, C = x.shape
    assert idx.shape == (n, k), (what, idx.shape)
    assert idx.min() >= 0 and idx.max() < n, (what, int(idx.min()), int(idx.max()))
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), (what, "a repeated neighbour")
    if k == n:
        return 0.0
    s = exact_scores(x)
    chosen = np.zeros((n, n), bool)
    chosen[np.arange(n)[:, None], idx] = True
    lo = np.where(chosen, s, np.inf).min(1)
    hi = np.where(chosen, -np.inf, s).max(1)
    nrm = np.sqrt((x * x).sum(1))
    tau = gamma(C + 2) * (nrm + nrm.max()) ** 2
    worst = float(((hi - lo) / (2 * tau)).max())
    bad = np.nonzero(lo < hi - 2 * tau)[0]
    assert bad.size == 0, (what, "rows with a better candidate left out", bad[:10], (hi - lo)[bad[:10]], tau[bad[:10]])
    return worst
