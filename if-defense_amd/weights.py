"""Checkpoint handling: the reference's ``state_dict`` -> the canonical flat order of include/ifd.h."""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np


def canonical_keys() -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of every tensor, in the order ifd_create expects (names as in pretrain/convonet.pth;
    schema: SURVEY.md section 8 R0, ConvONet/src/conv_onet/models/decoder.py:29-40,
    src/encoder/pointnet.py:37-47, src/encoder/unet.py:184-209)."""
    k: List[Tuple[str, Tuple[int, ...]]] = []
    k += [("decoder.fc_p.weight", (32, 3)), ("decoder.fc_p.bias", (32,))]
    for i in range(5):
        k += [(f"decoder.fc_c.{i}.weight", (32, 32)), (f"decoder.fc_c.{i}.bias", (32,))]
    for i in range(5):
        k += [(f"decoder.blocks.{i}.fc_0.weight", (32, 32)), (f"decoder.blocks.{i}.fc_0.bias", (32,)),
              (f"decoder.blocks.{i}.fc_1.weight", (32, 32)), (f"decoder.blocks.{i}.fc_1.bias", (32,))]
    k += [("decoder.fc_out.weight", (1, 32)), ("decoder.fc_out.bias", (1,))]
    k += [("encoder.fc_pos.weight", (64, 3)), ("encoder.fc_pos.bias", (64,))]
    for i in range(5):
        k += [(f"encoder.blocks.{i}.fc_0.weight", (32, 64)), (f"encoder.blocks.{i}.fc_0.bias", (32,)),
              (f"encoder.blocks.{i}.fc_1.weight", (32, 32)), (f"encoder.blocks.{i}.fc_1.bias", (32,)),
              (f"encoder.blocks.{i}.shortcut.weight", (32, 64))]
    k += [("encoder.fc_c.weight", (32, 32)), ("encoder.fc_c.bias", (32,))]
    chans = [32, 64, 128, 256]
    cin = 32
    for i, co in enumerate(chans):
        k += [(f"encoder.unet.down_convs.{i}.conv1.weight", (co, cin, 3, 3)),
              (f"encoder.unet.down_convs.{i}.conv1.bias", (co,)),
              (f"encoder.unet.down_convs.{i}.conv2.weight", (co, co, 3, 3)),
              (f"encoder.unet.down_convs.{i}.conv2.bias", (co,))]
        cin = co
    for i in range(3):
        co = cin // 2
        k += [(f"encoder.unet.up_convs.{i}.upconv.weight", (cin, co, 2, 2)),
              (f"encoder.unet.up_convs.{i}.upconv.bias", (co,)),
              (f"encoder.unet.up_convs.{i}.conv1.weight", (co, 2 * co, 3, 3)),
              (f"encoder.unet.up_convs.{i}.conv1.bias", (co,)),
              (f"encoder.unet.up_convs.{i}.conv2.weight", (co, co, 3, 3)),
              (f"encoder.unet.up_convs.{i}.conv2.bias", (co,))]
        cin = co
    k += [("encoder.unet.conv_final.weight", (32, 32, 1, 1)), ("encoder.unet.conv_final.bias", (32,))]
    return k


def onet_canonical_keys() -> List[Tuple[str, Tuple[int, ...]]]:
    """ONet-Opt (ONet/configs/onet_mn40.yaml): the reference checkpoint's state_dict order without the BatchNorm
    ``num_batches_tracked`` scalars (include/ifd.h, ONet section).  Conv1d kernels keep their trailing 1."""
    k: List[Tuple[str, Tuple[int, ...]]] = [("decoder.fc_p.weight", (256, 3, 1)), ("decoder.fc_p.bias", (256,))]

    def cbn(pre):
        return [(pre + ".conv_gamma.weight", (256, 512, 1)), (pre + ".conv_gamma.bias", (256,)),
                (pre + ".conv_beta.weight", (256, 512, 1)), (pre + ".conv_beta.bias", (256,)),
                (pre + ".bn.running_mean", (256,)), (pre + ".bn.running_var", (256,))]

    for i in range(5):
        k += cbn(f"decoder.block{i}.bn_0") + cbn(f"decoder.block{i}.bn_1")
        k += [(f"decoder.block{i}.fc_0.weight", (256, 256, 1)), (f"decoder.block{i}.fc_0.bias", (256,)),
              (f"decoder.block{i}.fc_1.weight", (256, 256, 1)), (f"decoder.block{i}.fc_1.bias", (256,))]
    k += cbn("decoder.bn") + [("decoder.fc_out.weight", (1, 256, 1)), ("decoder.fc_out.bias", (1,))]
    k += [("encoder.fc_pos.weight", (1024, 3)), ("encoder.fc_pos.bias", (1024,))]
    for i in range(5):
        k += [(f"encoder.block_{i}.fc_0.weight", (512, 1024)), (f"encoder.block_{i}.fc_0.bias", (512,)),
              (f"encoder.block_{i}.fc_1.weight", (512, 512)), (f"encoder.block_{i}.fc_1.bias", (512,)),
              (f"encoder.block_{i}.shortcut.weight", (512, 1024))]
    k += [("encoder.fc_c.weight", (512, 512)), ("encoder.fc_c.bias", (512,))]
    return k


def punet_canonical_keys() -> List[Tuple[str, Tuple[int, ...]]]:
    """PU-Net of DUP-Net (baselines/defense/DUP_Net/pu_net.py, npoint 1024, up_ratio 4, no BN): the state_dict order of
    pu-in_1024-up_4.pth (include/ifd_dup.h).  1x1 Conv2d kernels keep their trailing [1, 1]."""
    k: List[Tuple[str, Tuple[int, ...]]] = []

    def conv(pre, co, ci):
        return [(pre + ".conv.weight", (co, ci, 1, 1)), (pre + ".conv.bias", (co,))]

    sa = [[3, 32, 32, 64], [67, 64, 64, 128], [131, 128, 128, 256], [259, 256, 256, 512]]
    for i, m in enumerate(sa):
        for j in range(3):
            k += conv(f"SA_modules.{i}.mlps.0.layer{j}", m[j + 1], m[j])
    for i, c in enumerate([128, 256, 512]):
        k += conv(f"FP_Modules.{i}.mlp.layer0", 64, c)
    for i in range(4):
        k += conv(f"FC_Modules.{i}.layer0", 256, 259) + conv(f"FC_Modules.{i}.layer1", 128, 256)
    k += conv("pcd_layer.0.layer0", 64, 128) + conv("pcd_layer.1.layer0", 3, 64)
    return k


BN_EPS = 1e-5


def pointnet_layers(feature_transform: bool = False) -> List[Tuple[str, object, Tuple[int, int], bool]]:
    """The conv / linear layers of PointNetCls(k=40, use_bn=True) (baselines/model/pointnet.py) in network order, which is
    the canonical order of include/ifd_cls.h: (layer key, its BatchNorm's key or None, (out, in), is a Conv1d).  The
    Sequential members are ``.0`` (conv / linear) and ``.1`` (BatchNorm); STNkd names its layers conv1..3 / fc1..3 / bn1..5."""
    def seq(pre, dims, conv):
        return [(pre + ".0", pre + ".1", dims, conv)]

    k = (seq("feat.stn.conv1", (64, 3), True) + seq("feat.stn.conv2", (128, 64), True) + seq("feat.stn.conv3", (1024, 128), True)
         + seq("feat.stn.fc1", (512, 1024), False) + seq("feat.stn.fc2", (256, 512), False)
         + [("feat.stn.fc3", None, (9, 256), False)] + seq("feat.conv1", (64, 3), True))
    if feature_transform:
        f = "feat.fstn."
        k += [(f + "conv1", f + "bn1", (64, 64), True), (f + "conv2", f + "bn2", (128, 64), True),
              (f + "conv3", f + "bn3", (1024, 128), True), (f + "fc1", f + "bn4", (512, 1024), False),
              (f + "fc2", f + "bn5", (256, 512), False), (f + "fc3", None, (4096, 256), False)]
    k += seq("feat.conv2", (128, 64), True) + seq("feat.conv3", (1024, 128), True) + seq("fc1", (512, 1024), False)
    k += [("fc2", "bn2", (256, 512), False), ("fc3", None, (40, 256), False)]
    return k


def pointnet_canonical_keys(feature_transform: bool = False) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the BN-folded tensors ifd_cls_create expects, in order (include/ifd_cls.h)."""
    k: List[Tuple[str, Tuple[int, ...]]] = []
    for lin, _, (co, ci), _ in pointnet_layers(feature_transform):
        k += [(lin + ".weight", (co, ci)), (lin + ".bias", (co,))]
    return k


def pointnet_state_keys(feature_transform: bool = False) -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the un-folded state_dict tensors the packer reads (no ``module.`` prefix, no num_batches_tracked)."""
    k: List[Tuple[str, Tuple[int, ...]]] = []
    for lin, bn, (co, ci), conv in pointnet_layers(feature_transform):
        k += [(lin + ".weight", (co, ci, 1) if conv else (co, ci)), (lin + ".bias", (co,))]
        if bn:
            k += [(bn + "." + n, (co,)) for n in ("weight", "bias", "running_mean", "running_var")]
    return k


def strip_module_prefix(state: Dict[str, object]) -> Dict[str, object]:
    """Keys of a state_dict saved from nn.DataParallel carry ``module.``; accept both forms."""
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}


def fold_pointnet(state: Dict[str, object], feature_transform=None) -> List[Tuple[str, np.ndarray]]:
    """Fold every eval-mode BatchNorm into its layer in float64: w' = w g / sqrt(var + eps), b' = (b - mean) g / sqrt(var +
    eps) + beta.  -> [(canonical name, float64 array)] in canonical order.  feature_transform None: judged from the keys."""
    state = strip_module_prefix(state)
    if feature_transform is None:
        feature_transform = "feat.fstn.conv1.weight" in state

    def get(name, shape):
        if name not in state:
            raise KeyError("checkpoint lacks %r" % name)
        t = state[name]
        a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s: expected shape %s, got %s" % (name, shape, tuple(a.shape)))
        return a.astype(np.float64)

    out: List[Tuple[str, np.ndarray]] = []
    for lin, bn, (co, ci), conv in pointnet_layers(bool(feature_transform)):
        w = get(lin + ".weight", (co, ci, 1) if conv else (co, ci)).reshape(co, ci)
        b = get(lin + ".bias", (co,))
        if bn:
            g, beta = get(bn + ".weight", (co,)), get(bn + ".bias", (co,))
            mean, var = get(bn + ".running_mean", (co,)), get(bn + ".running_var", (co,))
            sc = g / np.sqrt(var + BN_EPS)
            w, b = w * sc[:, None], (b - mean) * sc + beta
        out += [(lin + ".weight", w), (lin + ".bias", b)]
    return out


def pack_pointnet(state: Dict[str, object], feature_transform=None) -> np.ndarray:
    """fold_pointnet, rounded to float32 and flattened in canonical order (num_batches_tracked is ignored)."""
    return np.concatenate([a.astype(np.float32).reshape(-1) for _, a in fold_pointnet(state, feature_transform)])


def _keys(model: str):
    if model == "pointnet":
        return pointnet_canonical_keys(False)
    if model == "dgcnn":
        return dgcnn_canonical_keys()
    if model == "pointnet2":
        return pointnet2_canonical_keys()
    if model == "pointconv":
        return pointconv_canonical_keys()
    if model == "onet":
        return onet_canonical_keys()
    if model == "punet":
        return punet_canonical_keys()
    return canonical_keys()


def pack_state_dict(state: Dict[str, object], model: str = "convonet", feature_transform=None) -> np.ndarray:
    """Flatten a state_dict (torch tensors or numpy arrays) into one float32 vector.  Missing or
    mis-shaped tensors raise KeyError / ValueError, like ``load_state_dict(strict=True)``.  "pointnet": BatchNorm is
    folded on the way (pack_pointnet); feature_transform None means judged from the keys."""
    if model == "pointnet":
        return pack_pointnet(state, feature_transform)
    if model == "dgcnn":
        return pack_dgcnn(state)
    if model == "pointnet2":
        return pack_pointnet2(state)
    if model == "pointconv":
        return pack_pointconv(state)
    parts = []
    for name, shape in _keys(model):
        if name not in state:
            raise KeyError("checkpoint lacks %r" % name)
        t = state[name]
        a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s: expected shape %s, got %s" % (name, shape, tuple(a.shape)))
        parts.append(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
    return np.concatenate(parts)


def load_checkpoint(path: str, model: str = "convonet", feature_transform=None) -> np.ndarray:
    """``torch.load`` a reference checkpoint (ConvONet/opt_defense.py:65) and pack it.  Accepts a bare
    state_dict or the training checkpoints' {'model': state_dict, ...} wrapper."""
    if model == "pointnet":
        # pretrain/<dataset>/pointnet.pth (baselines/config.py BEST_WEIGHTS; saved from nn.DataParallel) or an .npz of its arrays
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                return pack_pointnet({n: z[n] for n in z.files}, feature_transform)
        import torch
        return pack_pointnet(torch.load(path, map_location="cpu", weights_only=True), feature_transform)
    if model == "dgcnn":
        # pretrain/<dataset>/dgcnn.pth (saved from nn.DataParallel) or an .npz of its arrays
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                return pack_dgcnn({n: z[n] for n in z.files})
        import torch
        return pack_dgcnn(torch.load(path, map_location="cpu", weights_only=True))
    if model == "pointnet2":
        # pretrain/<dataset>/pointnet2.pth (saved from nn.DataParallel) or an .npz of its arrays
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                return pack_pointnet2({n: z[n] for n in z.files})
        import torch
        return pack_pointnet2(torch.load(path, map_location="cpu", weights_only=True))
    if model == "pointconv":
        # pretrain/<dataset>/pointconv.pth (saved from nn.DataParallel) or an .npz of its arrays
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                return pack_pointconv({n: z[n] for n in z.files})
        import torch
        return pack_pointconv(torch.load(path, map_location="cpu", weights_only=True))
    if model == "punet":
        # pu-in_1024-up_4.pth (baselines/config.py PU_NET_WEIGHT) or an .npz of the same arrays
        if path.endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                return pack_state_dict({n: z[n] for n in z.files}, model)
        import torch
        return pack_state_dict(torch.load(path, map_location="cpu", weights_only=True), model)
    import torch
    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "model" in sd and "decoder.fc_p.weight" not in sd:
        sd = sd["model"]
    return pack_state_dict(sd, model)


def random_state_dict(seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random weights of the shipped architecture (benchmarks / smoke runs; the trained
    pretrain/convonet.pth is a Google-Drive download).  Linear layers: U(-1/sqrt(fan_in), +); convs:
    Xavier-normal with a small uniform bias; fc_1 is NOT zero-initialised (src/layers.py:37 would make
    every residual branch constant)."""
    import math
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}
    def uni(shape, bound):
        return rng.uniform(-bound, bound, size=shape).astype(np.float32)

    def linear(name, n_out, n_in, bias=True):
        b = 1.0 / math.sqrt(n_in)
        w[name + ".weight"] = uni((n_out, n_in), b)
        if bias:
            w[name + ".bias"] = uni((n_out,), b)

    def conv(name, c_out, c_in, k, transpose=False):
        shape = (c_in, c_out, k, k) if transpose else (c_out, c_in, k, k)
        std = math.sqrt(2.0 / (c_in * k * k + c_out * k * k))
        w[name + ".weight"] = (rng.standard_normal(shape) * std).astype(np.float32)
        w[name + ".bias"] = uni((c_out,), 0.05)

    linear("decoder.fc_p", 32, 3)
    for i in range(5):
        linear(f"decoder.fc_c.{i}", 32, 32)
    for i in range(5):
        linear(f"decoder.blocks.{i}.fc_0", 32, 32)
        linear(f"decoder.blocks.{i}.fc_1", 32, 32)
    linear("decoder.fc_out", 1, 32)
    linear("encoder.fc_pos", 64, 3)
    for i in range(5):
        linear(f"encoder.blocks.{i}.fc_0", 32, 64)
        linear(f"encoder.blocks.{i}.fc_1", 32, 32)
        linear(f"encoder.blocks.{i}.shortcut", 32, 64, bias=False)
    linear("encoder.fc_c", 32, 32)
    c_in = 32
    for i, c_out in enumerate([32, 64, 128, 256]):
        conv(f"encoder.unet.down_convs.{i}.conv1", c_out, c_in, 3)
        conv(f"encoder.unet.down_convs.{i}.conv2", c_out, c_out, 3)
        c_in = c_out
    for i in range(3):
        c_out = c_in // 2
        conv(f"encoder.unet.up_convs.{i}.upconv", c_out, c_in, 2, transpose=True)
        conv(f"encoder.unet.up_convs.{i}.conv1", c_out, 2 * c_out, 3)
        conv(f"encoder.unet.up_convs.{i}.conv2", c_out, c_out, 3)
        c_in = c_out
    conv("encoder.unet.conv_final", 32, c_in, 1)
    return w


def onet_random_state_dict(seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random ONet weights (same streams as the test oracle's: Linear / 1x1-conv U(+-1/sqrt(fan_in)); what
    the reference zero-initialises - fc_1, CBN gamma/beta convs - is randomised; non-trivial BatchNorm statistics)."""
    rng = np.random.default_rng(seed + 7001)
    w: Dict[str, np.ndarray] = {}

    def lin(key, n_out, n_in, bias=True, conv=False, scale=1.0):
        b = scale / np.sqrt(n_in)
        shape = (n_out, n_in, 1) if conv else (n_out, n_in)
        w[key + ".weight"] = rng.uniform(-b, b, size=shape).astype(np.float32)
        if bias:
            w[key + ".bias"] = rng.uniform(-b, b, size=(n_out,)).astype(np.float32)

    lin("encoder.fc_pos", 1024, 3)
    for i in range(5):
        lin(f"encoder.block_{i}.fc_0", 512, 1024)
        lin(f"encoder.block_{i}.fc_1", 512, 512)
        lin(f"encoder.block_{i}.shortcut", 512, 1024, bias=False)
    lin("encoder.fc_c", 512, 512)

    def cbn(key):
        lin(key + ".conv_gamma", 256, 512, conv=True, scale=8.0)
        w[key + ".conv_gamma.bias"] = (1.0 + rng.uniform(-0.2, 0.2, 256)).astype(np.float32)
        lin(key + ".conv_beta", 256, 512, conv=True, scale=8.0)
        w[key + ".bn.running_mean"] = rng.normal(0.0, 0.3, 256).astype(np.float32)
        w[key + ".bn.running_var"] = rng.uniform(0.5, 1.5, 256).astype(np.float32)

    lin("decoder.fc_p", 256, 3, conv=True)
    for i in range(5):
        cbn(f"decoder.block{i}.bn_0")
        cbn(f"decoder.block{i}.bn_1")
        lin(f"decoder.block{i}.fc_0", 256, 256, conv=True)
        lin(f"decoder.block{i}.fc_1", 256, 256, conv=True)
    cbn("decoder.bn")
    lin("decoder.fc_out", 1, 256, conv=True)
    return w


def pointnet_random_state_dict(seed: int = 0, feature_transform: bool = False) -> Dict[str, np.ndarray]:
    """Seeded random un-folded PointNet weights for smoke / benchmark runs (no victim checkpoint ships: pretrain/mn40/
    pointnet.pth is a download).  Per layer in network order: weight and bias U(+-1/sqrt(fan_in)); each BatchNorm after
    its layer: gamma 1 + U(+-0.2), beta U(+-0.1), running_mean N(0, 0.1), running_var U(0.5, 1.25) - never the init
    values.  The recipe (and so the numbers) is that of tests/pointnet_oracle.py make_weights."""
    rng = np.random.default_rng(seed + 9001)
    w: Dict[str, np.ndarray] = {}
    for lin, bn, (co, ci), conv in pointnet_layers(feature_transform):
        b = 1.0 / np.sqrt(ci)
        w[lin + ".weight"] = rng.uniform(-b, b, size=(co, ci, 1) if conv else (co, ci)).astype(np.float32)
        w[lin + ".bias"] = rng.uniform(-b, b, size=(co,)).astype(np.float32)
        if bn:
            w[bn + ".weight"] = (1.0 + rng.uniform(-0.2, 0.2, co)).astype(np.float32)
            w[bn + ".bias"] = rng.uniform(-0.1, 0.1, co).astype(np.float32)
            w[bn + ".running_mean"] = rng.normal(0.0, 0.1, co).astype(np.float32)
            w[bn + ".running_var"] = rng.uniform(0.5, 1.25, co).astype(np.float32)
    return w


# ---- the DGCNN victim (include/ifd_dgcnn.h) --------------------------------------------------------------------------
def dgcnn_layers() -> List[Tuple[str, Tuple[str, str], Tuple[int, int], int, bool]]:
    """The layers of DGCNN(emb_dims=1024, k, output_channels=40, use_bn=True) (baselines/model/dgcnn.py) in network order,
    which is the canonical order of include/ifd_dgcnn.h: (layer key, the two keys its BatchNorm is registered under - the
    module attribute first, the Sequential's member second - or None, (out, in), trailing singleton dims of the weight, has a
    bias).  The reference builds ``self.bn1`` and then puts the same module into ``self.conv1``, so a state_dict holds every
    BatchNorm twice: ``bn1.*`` and ``conv1.1.*``."""
    k = []
    for i, dims in enumerate([(64, 6), (64, 128), (128, 128), (256, 256)], 1):
        k.append(("conv%d.0" % i, ("bn%d" % i, "conv%d.1" % i), dims, 2, False))
    k.append(("conv5.0", ("bn5", "conv5.1"), (1024, 512), 1, False))
    k.append(("linear1.0", ("bn6", "linear1.1"), (512, 2048), 0, False))
    k.append(("linear2.0", ("bn7", "linear2.1"), (256, 512), 0, True))
    k.append(("linear3", None, (40, 256), 0, True))
    return k


def dgcnn_canonical_keys() -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the BN-folded tensors ifd_dgcnn_create expects, in order (include/ifd_dgcnn.h)."""
    k: List[Tuple[str, Tuple[int, ...]]] = []
    for lin, _, (co, ci), _, _ in dgcnn_layers():
        k += [(lin + ".weight", (co, ci)), (lin + ".bias", (co,))]
    return k


def fold_dgcnn(state: Dict[str, object]) -> List[Tuple[str, np.ndarray]]:
    """Fold every eval-mode BatchNorm into its layer in float64 (the formulas of fold_pointnet; a layer without a bias has
    b = 0, so its folded bias is the BatchNorm's shift).  -> [(canonical name, float64 array)] in canonical order.  Each
    BatchNorm tensor is read from ``bnN.*``, else from the Sequential's key; both present and different is a ValueError."""
    state = strip_module_prefix(state)

    def arr(name):
        t = state[name]
        return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)

    def get(name, shape):
        if name not in state:
            raise KeyError("checkpoint lacks %r" % name)
        a = arr(name)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s: expected shape %s, got %s" % (name, shape, tuple(a.shape)))
        return a.astype(np.float64)

    def get_bn(names, field, shape):
        first, second = (n + "." + field for n in names)
        if first in state and second in state and not np.array_equal(arr(first), arr(second)):
            raise ValueError("%s and %s name one BatchNorm tensor but differ" % (first, second))
        return get(first if first in state or second not in state else second, shape)

    out: List[Tuple[str, np.ndarray]] = []
    for lin, bn, (co, ci), ones, has_bias in dgcnn_layers():
        w = get(lin + ".weight", (co, ci) + (1,) * ones).reshape(co, ci)
        b = get(lin + ".bias", (co,)) if has_bias else np.zeros(co)
        if bn:
            g, beta = get_bn(bn, "weight", (co,)), get_bn(bn, "bias", (co,))
            mean, var = get_bn(bn, "running_mean", (co,)), get_bn(bn, "running_var", (co,))
            sc = g / np.sqrt(var + BN_EPS)
            w, b = w * sc[:, None], (b - mean) * sc + beta
        out += [(lin + ".weight", w), (lin + ".bias", b)]
    return out


def pack_dgcnn(state: Dict[str, object]) -> np.ndarray:
    """fold_dgcnn, rounded to float32 and flattened in canonical order (num_batches_tracked is ignored)."""
    return np.concatenate([a.astype(np.float32).reshape(-1) for _, a in fold_dgcnn(state)])


def dgcnn_random_state_dict(seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random un-folded DGCNN weights for smoke / benchmark runs (pretrain/mn40/dgcnn.pth is a download), under the
    BatchNorms' module keys (``bnN.*``).  Per layer in network order: weight (and bias, where the layer has one)
    U(+-1/sqrt(fan_in)); each BatchNorm after its layer: gamma 1 + U(+-0.2), beta U(+-0.1), running_mean N(0, 0.1),
    running_var U(0.5, 1.25).  The recipe (and so the numbers) is that of tests/dgcnn_oracle.py make_weights."""
    rng = np.random.default_rng(seed + 9101)
    w: Dict[str, np.ndarray] = {}
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


# ---- the PointNet++ victim (include/ifd_pn2.h) -----------------------------------------------------------------------
def pointnet2_layers() -> List[Tuple[str, object, Tuple[int, int], int]]:
    """The layers of PointNet2ClsSsg(num_classes=40) (baselines/model/pointnet2.py) in network order, which is the canonical
    order of include/ifd_pn2.h: (layer key, its BatchNorm's key or None, (out, in), trailing singleton dims of the weight).
    Every layer has a bias."""
    k = []
    for sa, dims in (("sa1", [(64, 3), (64, 64), (128, 64)]), ("sa2", [(128, 131), (128, 128), (256, 128)]),
                     ("sa3", [(256, 259), (512, 256), (1024, 512)])):
        for i, d in enumerate(dims):
            k.append(("%s.mlp_convs.%d" % (sa, i), "%s.mlp_bns.%d" % (sa, i), d, 2))
    k.append(("fc1", "bn1", (512, 1024), 0))
    k.append(("fc2", "bn2", (256, 512), 0))
    k.append(("fc3", None, (40, 256), 0))
    return k


def pointnet2_canonical_keys() -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the BN-folded tensors ifd_pn2_create expects, in order (include/ifd_pn2.h)."""
    k: List[Tuple[str, Tuple[int, ...]]] = []
    for lin, _, (co, ci), _ in pointnet2_layers():
        k += [(lin + ".weight", (co, ci)), (lin + ".bias", (co,))]
    return k


def fold_pointnet2(state: Dict[str, object]) -> List[Tuple[str, np.ndarray]]:
    """Fold every eval-mode BatchNorm into its layer in float64 (the formulas of fold_pointnet).  -> [(canonical name, float64
    array)] in canonical order.  A key that is there both with and without the ``module.`` prefix is a ValueError."""
    doubled = [k for k in state if not k.startswith("module.") and ("module." + k) in state]
    if doubled:
        raise ValueError("checkpoint holds %r with and without the module. prefix" % doubled[0])
    state = strip_module_prefix(state)

    def get(name, shape):
        if name not in state:
            raise KeyError("checkpoint lacks %r" % name)
        t = state[name]
        a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s: expected shape %s, got %s" % (name, shape, tuple(a.shape)))
        return a.astype(np.float64)

    out: List[Tuple[str, np.ndarray]] = []
    for lin, bn, (co, ci), ones in pointnet2_layers():
        w = get(lin + ".weight", (co, ci) + (1,) * ones).reshape(co, ci)
        b = get(lin + ".bias", (co,))
        if bn:
            g, beta = get(bn + ".weight", (co,)), get(bn + ".bias", (co,))
            mean, var = get(bn + ".running_mean", (co,)), get(bn + ".running_var", (co,))
            sc = g / np.sqrt(var + BN_EPS)
            w, b = w * sc[:, None], (b - mean) * sc + beta
        out += [(lin + ".weight", w), (lin + ".bias", b)]
    return out


def pack_pointnet2(state: Dict[str, object]) -> np.ndarray:
    """fold_pointnet2, rounded to float32 and flattened in canonical order (num_batches_tracked is ignored)."""
    return np.concatenate([a.astype(np.float32).reshape(-1) for _, a in fold_pointnet2(state)])


def pointnet2_random_state_dict(seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random un-folded PointNet++ weights for smoke / benchmark runs (pretrain/mn40/pointnet2.pth is a download).  Per
    layer in network order: weight and bias U(+-1/sqrt(fan_in)); each BatchNorm after its layer: gamma 1 + U(+-0.2), beta
    U(+-0.1), running_mean N(0, 0.1), running_var U(0.5, 1.25).  The recipe (and so the numbers) is that of
    tests/pointnet2_oracle.py make_weights."""
    rng = np.random.default_rng(seed + 9201)
    w: Dict[str, np.ndarray] = {}
    for lin, bn, (co, ci), ones in pointnet2_layers():
        b = 1.0 / np.sqrt(ci)
        w[lin + ".weight"] = rng.uniform(-b, b, size=(co, ci) + (1,) * ones).astype(np.float32)
        w[lin + ".bias"] = rng.uniform(-b, b, size=(co,)).astype(np.float32)
        if bn:
            w[bn + ".weight"] = (1.0 + rng.uniform(-0.2, 0.2, co)).astype(np.float32)
            w[bn + ".bias"] = rng.uniform(-0.1, 0.1, co).astype(np.float32)
            w[bn + ".running_mean"] = rng.normal(0.0, 0.1, co).astype(np.float32)
            w[bn + ".running_var"] = rng.uniform(0.5, 1.25, co).astype(np.float32)
    return w


# ---- the PointConv victim (include/ifd_pc.h) -------------------------------------------------------------------------
def pointconv_layers() -> List[Tuple[str, object, Tuple[int, int], int]]:
    """The layers of PointConvDensityClsSsg(num_classes=40) (baselines/model/pointconv.py) in the canonical order of
    include/ifd_pc.h - per level densitynet x 3 (Conv1d), mlp x 3 (Conv2d), weightnet x 3 (Conv2d), linear (Linear); then the
    head: (layer key, its BatchNorm's key or None, (out, in), trailing singleton dims of the weight).  Every layer has a bias."""
    k = []
    for sa, cin, mlp in (("sa1", 3, (64, 64, 128)), ("sa2", 131, (128, 128, 256)), ("sa3", 259, (256, 512, 1024))):
        for i, d in enumerate([(8, 1), (8, 8), (1, 8)]):
            k.append(("%s.densitynet.mlp_convs.%d" % (sa, i), "%s.densitynet.mlp_bns.%d" % (sa, i), d, 1))
        last = cin
        for i, co in enumerate(mlp):
            k.append(("%s.mlp_convs.%d" % (sa, i), "%s.mlp_bns.%d" % (sa, i), (co, last), 2))
            last = co
        for i, d in enumerate([(8, 3), (8, 8), (16, 8)]):
            k.append(("%s.weightnet.mlp_convs.%d" % (sa, i), "%s.weightnet.mlp_bns.%d" % (sa, i), d, 2))
        k.append((sa + ".linear", sa + ".bn_linear", (last, 16 * last), 0))
    k.append(("fc1", "bn1", (512, 1024), 0))
    k.append(("fc2", "bn2", (256, 512), 0))
    k.append(("fc3", None, (40, 256), 0))
    return k


def pointconv_canonical_keys() -> List[Tuple[str, Tuple[int, ...]]]:
    """(name, shape) of the BN-folded tensors ifd_pc_create expects, in order (include/ifd_pc.h): 19,559,411 floats."""
    k: List[Tuple[str, Tuple[int, ...]]] = []
    for lin, _, (co, ci), _ in pointconv_layers():
        k += [(lin + ".weight", (co, ci)), (lin + ".bias", (co,))]
    return k


def pointconv_weight_count() -> int:
    return sum(int(np.prod(shape)) for _, shape in pointconv_canonical_keys())


def fold_pointconv(state: Dict[str, object]) -> List[Tuple[str, np.ndarray]]:
    """Fold every eval-mode BatchNorm into its layer in float64 (the formulas of fold_pointnet).  -> [(canonical name, float64
    array)] in canonical order.  A key that is there both with and without the ``module.`` prefix is a ValueError."""
    doubled = [k for k in state if not k.startswith("module.") and ("module." + k) in state]
    if doubled:
        raise ValueError("checkpoint holds %r with and without the module. prefix" % doubled[0])
    state = strip_module_prefix(state)

    def get(name, shape):
        if name not in state:
            raise KeyError("checkpoint lacks %r" % name)
        t = state[name]
        a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s: expected shape %s, got %s" % (name, shape, tuple(a.shape)))
        return a.astype(np.float64)

    out: List[Tuple[str, np.ndarray]] = []
    for lin, bn, (co, ci), ones in pointconv_layers():
        w = get(lin + ".weight", (co, ci) + (1,) * ones).reshape(co, ci)
        b = get(lin + ".bias", (co,))
        if bn:
            g, beta = get(bn + ".weight", (co,)), get(bn + ".bias", (co,))
            mean, var = get(bn + ".running_mean", (co,)), get(bn + ".running_var", (co,))
            sc = g / np.sqrt(var + BN_EPS)
            w, b = w * sc[:, None], (b - mean) * sc + beta
        out += [(lin + ".weight", w), (lin + ".bias", b)]
    return out


def pack_pointconv(state: Dict[str, object]) -> np.ndarray:
    """fold_pointconv, rounded to float32 and flattened in canonical order (num_batches_tracked is ignored)."""
    return np.concatenate([a.astype(np.float32).reshape(-1) for _, a in fold_pointconv(state)])


def pointconv_random_state_dict(seed: int = 0) -> Dict[str, np.ndarray]:
    """Seeded random un-folded PointConv weights for smoke / benchmark runs (pretrain/mn40/pointconv.pth is a download).  Per
    layer in canonical order: weight and bias U(+-1/sqrt(fan_in)); each BatchNorm after its layer: gamma 1 + U(+-0.2), beta
    U(+-0.1), running_mean N(0, 0.1), running_var U(0.5, 1.25).  A DensityNet ends in a ReLU and a net of fan-in 1 and 8 drawn
    this way is dead as often as not, so the DensityNets' tensors are then made positive: weights and biases by their absolute
    values, running_mean by minus its absolute value - every density scale s_j is positive.  The recipe (and so the numbers) is
    that of tests/pointconv_oracle.py make_weights."""
    rng = np.random.default_rng(seed + 9301)
    w: Dict[str, np.ndarray] = {}
    for lin, bn, (co, ci), ones in pointconv_layers():
        b = 1.0 / np.sqrt(ci)
        w[lin + ".weight"] = rng.uniform(-b, b, size=(co, ci) + (1,) * ones).astype(np.float32)
        w[lin + ".bias"] = rng.uniform(-b, b, size=(co,)).astype(np.float32)
        if bn:
            w[bn + ".weight"] = (1.0 + rng.uniform(-0.2, 0.2, co)).astype(np.float32)
            w[bn + ".bias"] = rng.uniform(-0.1, 0.1, co).astype(np.float32)
            w[bn + ".running_mean"] = rng.normal(0.0, 0.1, co).astype(np.float32)
            w[bn + ".running_var"] = rng.uniform(0.5, 1.25, co).astype(np.float32)
        if ".densitynet." in lin:
            for key in (lin + ".weight", lin + ".bias", bn + ".bias"):
                w[key] = np.abs(w[key])
            w[bn + ".running_mean"] = -np.abs(w[bn + ".running_mean"])
    return w
