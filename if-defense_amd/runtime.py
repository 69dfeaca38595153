"""Host-side mirror of the reference's call seams for the ConvONet-Opt path.

The reference exposes the path through module-level globals (``generator.model.encode_inputs`` /
``.decode`` / ``repulsion_loss`` / ``optimize_points``, ConvONet/opt_defense.py:212,221,300,182).
``Restorer`` offers the same calls with the same argument meaning, backed by libifd.so's HIP kernels;
PyTorch is used only for device memory and streams.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import IfdConfig, IfdMeshParams, IfdOptParams, IfdPrepParams

PLANE_ORDER = ("xz", "xy", "yz")
# measurement hook: IFD_SPLIT=1|2|4 overrides the automatic choice of ifd_opt_params.split (results do not depend on it)
import os as _os
_ENV_SPLIT = int(_os.environ.get("IFD_SPLIT", "0"))
# ifd_opt_params.precision by name.  Where a caller passes None the module default applies: "f32" unless a test / measurement
# set another one (set_default_precision; tests/conftest.py runs the parity matrix in both modes that way).  The environment's
# IFD_PRECISION is honoured only together with IFD_ENABLE_TEST_HOOKS=1 (round-5 advisor: a stray variable must not switch a
# production process to another arithmetic); the CLIs and pipeline.py always pass an explicit precision.
PRECISIONS = {"f32": 0, "bf16x6": 1, "bf16x3": 2}
_DEFAULT_PRECISION = "f32"
if _os.environ.get("IFD_ENABLE_TEST_HOOKS", "") == "1" and _os.environ.get("IFD_PRECISION"):
    _DEFAULT_PRECISION = _os.environ["IFD_PRECISION"]


def default_precision() -> str:
    return _DEFAULT_PRECISION


def set_default_precision(name: str) -> str:
    """Test / measurement hook: the precision used where a caller passes None.  Returns the previous default."""
    global _DEFAULT_PRECISION
    if name not in PRECISIONS:
        raise ValueError("precision must be one of %s" % sorted(PRECISIONS))
    prev, _DEFAULT_PRECISION = _DEFAULT_PRECISION, name
    return prev


def precision_code(precision) -> int:
    if precision is None:
        precision = _DEFAULT_PRECISION
    if isinstance(precision, str):
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(PRECISIONS))
        return PRECISIONS[precision]
    return int(precision)


class IfdError(RuntimeError):
    pass


def planes_to_channel_last(planes: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Reference layout {'xz','xy','yz': [B,32,64,64]} -> device layout [B,3,64,64,32] (include/ifd.h)."""
    return torch.stack([planes[k] for k in PLANE_ORDER], dim=1).permute(0, 1, 3, 4, 2).contiguous()


def planes_from_channel_last(planes: torch.Tensor) -> Dict[str, torch.Tensor]:
    return {k: planes[:, i].permute(0, 3, 1, 2).contiguous() for i, k in enumerate(PLANE_ORDER)}


def _f32(t: torch.Tensor, device: torch.device) -> torch.Tensor:
    return t.to(device=device, dtype=torch.float32).contiguous()


class Restorer:
    """One context = one model on one GPU (ifd_create ... ifd_destroy)."""
    model_name = "convonet"

    def __init__(self, weights: np.ndarray, device=None, padding: float = 0.1, threshold: float = 0.2):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise IfdError("no GPU visible: the restoration path only runs on an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise IfdError("Restorer needs a cuda (ROCm) device, got %s" % self.device)
        self.threshold = float(threshold)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.size != self.lib.ifd_weight_count():
            raise IfdError("expected %d weights, got %d" % (self.lib.ifd_weight_count(), w.size))
        cfg = IfdConfig(C.sizeof(IfdConfig), 64, 32, 32, 5, 4, 32, float(padding))
        with torch.cuda.device(self.device):
            self.ctx = self.lib.ifd_create(w.ctypes.data, w.size, C.byref(cfg), self.device.index or 0)
        if not self.ctx:
            raise IfdError((self.lib.ifd_last_error(None) or b"ifd_create failed").decode())
        self._fn_decode, self._fn_optimize = self.lib.ifd_decode_ex, self.lib.ifd_optimize
        self.n_sel = 600                  # encoder subset (convonet_3plane_mn40.yaml:7 pointcloud_n)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ifd_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    # ---------------------------------------------------------------- helpers
    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc: int):
        if rc != _lib.IFD_OK:
            raise IfdError("libifd error %d: %s" % (rc, (self.lib.ifd_last_error(self.ctx) or b"").decode()))

    @staticmethod
    def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
        return None if t is None else t.data_ptr()

    def _cond(self, c) -> torch.Tensor:
        """The conditioning code in device layout (planes here; the latent code in OnetRestorer)."""
        return self._planes(c)

    def _planes(self, c) -> torch.Tensor:
        if isinstance(c, dict):
            c = planes_to_channel_last({k: _f32(v, self.device) for k, v in c.items()})
        c = _f32(c, self.device)
        if c.dim() != 5 or tuple(c.shape[1:]) != (3, 64, 64, 32):
            raise IfdError("planes must be [B,3,64,64,32] channel-last or the reference's dict of [B,32,64,64]")
        return c

    # ---------------------------------------------------------------- pre-processing
    def sor(self, pc: torch.Tensor, k: int = 2, alpha: float = 1.1, want_value: bool = False):
        """SORDefense(k, alpha) keep-mask (defense/SOR.py:22-49): pc [B,K,3] -> uint8 [B,K] (and float64 value)."""
        pc = _f32(pc, self.device)
        B, K = pc.shape[:2]
        keep = torch.empty(B, K, device=self.device, dtype=torch.uint8)
        val = torch.empty(B, K, device=self.device, dtype=torch.float64) if want_value else None
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_sor(self.ctx, pc.data_ptr(), B, K, int(k), float(alpha), keep.data_ptr(),
                                         self._ptr(val), self._stream()))
        return (keep, val) if want_value else keep

    def prepare(self, pc: torch.Tensor, keep: Optional[torch.Tensor] = None, n_sel: int = 600, n_opt: int = 1024,
                padding_scale: float = 0.9, init_sigma: float = 0.01, seed: int = 0, cloud_index_base: int = 0,
                sel_idx: Optional[torch.Tensor] = None, init_idx: Optional[torch.Tensor] = None,
                noise: Optional[torch.Tensor] = None, want_proc: bool = False):
        """preprocess_pc + init_points (opt_defense.py:114-179) for a batch.  Returns a dict with
        sel [B,n_sel,3], t_per_cloud [B], init [B,n_opt,3], n_kept [B] (and proc [B,K,3] if asked)."""
        pc = _f32(pc, self.device)
        B, K = pc.shape[:2]
        i32 = lambda t: None if t is None else t.to(device=self.device, dtype=torch.int32).contiguous()
        sel_idx, init_idx = i32(sel_idx), i32(init_idx)
        noise = None if noise is None else _f32(noise, self.device)
        keep = None if keep is None else keep.to(device=self.device, dtype=torch.uint8).contiguous()
        sel = torch.empty(B, n_sel, 3, device=self.device, dtype=torch.float32)
        tpc = torch.empty(B, device=self.device, dtype=torch.int32)
        init = torch.empty(B, n_opt, 3, device=self.device, dtype=torch.float32)
        nk = torch.empty(B, device=self.device, dtype=torch.int32)
        proc = torch.zeros(B, K, 3, device=self.device, dtype=torch.float32) if want_proc else None
        prm = IfdPrepParams(C.sizeof(IfdPrepParams), int(n_sel), int(n_opt), float(padding_scale), float(init_sigma),
                            int(seed) & 0xFFFFFFFFFFFFFFFF, int(cloud_index_base))
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_prepare(self.ctx, pc.data_ptr(), self._ptr(keep), B, K, C.byref(prm),
                                             self._ptr(sel_idx), self._ptr(init_idx), self._ptr(noise), sel.data_ptr(),
                                             tpc.data_ptr(), init.data_ptr(), nk.data_ptr(), self._ptr(proc),
                                             self._stream()))
        out = {"sel": sel, "t_per_cloud": tpc, "init": init, "n_kept": nk}
        if want_proc:
            out["proc"] = proc
        return out

    # ---------------------------------------------------------------- encoder
    def encode_points(self, sel: torch.Tensor, t_per_cloud: Optional[torch.Tensor] = None, want_c: bool = False):
        """Point-wise half of encode_inputs (pointnet.py:124-156 + scatter_mean): sel [B,T,3] -> pre-U-Net
        planes [B,3,64,64,32] channel-last (and the per-point features c [B,T,32])."""
        sel = _f32(sel, self.device)
        B, T = sel.shape[:2]
        tpc = None if t_per_cloud is None else t_per_cloud.to(device=self.device, dtype=torch.int32).contiguous()
        pre = torch.empty(B, 3, 64, 64, 32, device=self.device, dtype=torch.float32)
        c = torch.empty(B, T, 32, device=self.device, dtype=torch.float32) if want_c else None
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_encode_points(self.ctx, sel.data_ptr(), self._ptr(tpc), B, T, pre.data_ptr(),
                                                   self._ptr(c), self._stream()))
        return (pre, c) if want_c else pre

    def encode_inputs(self, sel: torch.Tensor, t_per_cloud: Optional[torch.Tensor] = None) -> torch.Tensor:
        """generator.model.encode_inputs(x) (opt_defense.py:300): [B,T,3] -> planes [B,3,64,64,32] channel-last
        (use planes_from_channel_last for the reference's dict of [B,32,64,64])."""
        sel = _f32(sel, self.device)
        B, T = sel.shape[:2]
        tpc = None if t_per_cloud is None else t_per_cloud.to(device=self.device, dtype=torch.int32).contiguous()
        planes = torch.empty(B, 3, 64, 64, 32, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_encode_planes(self.ctx, sel.data_ptr(), self._ptr(tpc), B, T, planes.data_ptr(),
                                                   self._stream()))
        return planes

    def unet(self, planes_pre: torch.Tensor) -> torch.Tensor:
        """The shared U-Net on pre-U-Net planes [B,3,64,64,32] (src/encoder/unet.py:225-239)."""
        pre = _f32(planes_pre, self.device)
        out = torch.empty_like(pre)
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_unet(self.ctx, pre.data_ptr(), pre.shape[0], out.data_ptr(), self._stream()))
        return out

    # ---------------------------------------------------------------- call seams
    def decode(self, p: torch.Tensor, c, want_grad: bool = False, precision=None):
        """generator.model.decode(p, c).logits -> [B,K]; with want_grad also d(sum logits)/dp [B,K,3].  precision as in
        optimize_points (None: the module default): the seam computes in the arithmetic the optimiser would (ifd_decode_ex)."""
        planes = self._cond(c)
        p = _f32(p, self.device)
        B, K = p.shape[:2]
        logits = torch.empty(B, K, device=self.device, dtype=torch.float32)
        grad = torch.empty(B, K, 3, device=self.device, dtype=torch.float32) if want_grad else None
        with torch.cuda.device(self.device):
            self._check(self._fn_decode(self.ctx, planes.data_ptr(), p.data_ptr(), B, K, precision_code(precision),
                                            logits.data_ptr(), self._ptr(grad), self._stream()))
        return (logits, grad) if want_grad else logits

    def repulsion_loss(self, p: torch.Tensor, want_grad: bool = False, want_idx: bool = False):
        """repulsion_loss(p) -> [B] (defense/repulsion_loss.py:18-54)."""
        p = _f32(p, self.device)
        B, K = p.shape[:2]
        loss = torch.empty(B, device=self.device, dtype=torch.float32)
        grad = torch.empty(B, K, 3, device=self.device, dtype=torch.float32) if want_grad else None
        idx = torch.empty(B, K, 5, device=self.device, dtype=torch.int32) if want_idx else None
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_repulsion(self.ctx, p.data_ptr(), B, K, loss.data_ptr(), self._ptr(grad),
                                               self._ptr(idx), self._stream()))
        out = (loss,) + ((grad,) if want_grad else ()) + ((idx,) if want_idx else ())
        return out if len(out) > 1 else loss

    def optimize_points(self, opt_points: torch.Tensor, c, rep_weight: float = 1.0, iterations: int = 1000,
                        lr: float = 1e-3, loss_batch=None, normalize: bool = True,
                        state: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
                        return_state: bool = False, return_loss: bool = False, steps: Optional[int] = None,
                        knn_scan_every_step: bool = False, printing: bool = False, split: int = 0,
                        planes_shared: bool = False, rep_radius: float = 0.07, rep_h: float = 0.03, check: bool = True,
                        precision=None, knn_reference_form: bool = False):
        """optimize_points(opt_points, z, c, rep_weight, iterations) (opt_defense.py:182-239).

        Runs ``iterations + 1`` Adam steps (the reference's ``range(iterations + 1)``) unless ``steps``
        is given.  ``loss_batch`` is the reference batch size whose 1/B factor scales both losses
        (default: the number of clouds passed in); an int, or an int32 tensor [B] with one value per cloud.  ``state=(m, v, t0)`` resumes / teacher-forces.
        ``split``: CUs per cloud (ifd_opt_params.split: 0 automatic, 1 / 2 / 4 forced; same results).
        ``knn_reference_form``: validation only - the reference's neighbour choice bug for bug (ifd_opt_params.knn_reference_form:
        float32 expanded-form distances, top-6 minus column 0, pn_utils.py:72-83) instead of the exact 5-NN.
        ``precision``: arithmetic of the decoder's dense layers (ifd_opt_params.precision): "f32" / 0 (default), "bf16x6" / 1
        (f32-equivalent on the bf16 matrix core), "bf16x3" / 2 (reduced); None takes the module default ("f32"; set_default_precision).
        ``rep_radius`` / ``rep_h``: RepulsionLoss(radius, h) (defense/repulsion_loss.py:9-10; the reference never changes them).
        ``check`` (default on): synchronise and raise IfdError on a device-side failure (``check_status``: a split cloud's
        bounded wait that gave up, repulsion sums near their range) - a caller that gets points back can trust them.  The drivers
        of pipeline.py pass ``check=False`` and check once per file instead, where the result is consumed (no synchronisation
        inside the streamed passes).
        Returns the points as a torch tensor on the device ([B,K,3]); the reference's ``.cpu().numpy()``
        is left to the caller.
        """
        if printing and state is None and not return_state and not return_loss:
            return self._optimize_points_printing(opt_points, c, rep_weight, int(iterations) + 1 if steps is None else int(steps),
                                                  lr, loss_batch, normalize, knn_scan_every_step, precision, check)
        planes = self._cond(c)
        p = _f32(opt_points, self.device).clone()
        B, K = p.shape[:2]
        n_steps = int(iterations) + 1 if steps is None else int(steps)
        t0 = 0
        m = v = None
        if state is not None:
            m, v, t0 = _f32(state[0], self.device).clone(), _f32(state[1], self.device).clone(), int(state[2])
        elif return_state:
            m, v = torch.zeros_like(p), torch.zeros_like(p)
        loss = torch.empty(B, 2, device=self.device, dtype=torch.float32) if return_loss else None
        lb_arr = None
        if torch.is_tensor(loss_batch):
            lb_arr = loss_batch.to(device=self.device, dtype=torch.int32).contiguous()
            if lb_arr.numel() != B:
                raise IfdError("loss_batch tensor must have one entry per cloud")
            loss_batch = B
        prm = IfdOptParams(C.sizeof(IfdOptParams), n_steps, t0, int(loss_batch or B), int(bool(normalize)),
                           float(lr), float(rep_weight), self.threshold, float(rep_radius), float(rep_h), 1e-12,
                           int(bool(knn_scan_every_step)), int(split or _ENV_SPLIT), int(bool(planes_shared)),
                           int(bool(knn_reference_form)), precision_code(precision))
        with torch.cuda.device(self.device):
            self._check(self._fn_optimize(self.ctx, planes.data_ptr(), p.data_ptr(), B, K, C.byref(prm),
                                              self._ptr(lb_arr), self._ptr(m), self._ptr(v), self._ptr(loss),
                                              self._stream()))
        if check:
            self.check_status()
        out = (p,)
        if return_state:
            out += ((m, v, t0 + n_steps),)
        if return_loss:
            out += (loss,)
        return out if len(out) > 1 else p

    def _optimize_points_printing(self, opt_points, c, rep_weight, n_steps, lr, loss_batch, normalize, scan, precision=None, check=True):
        """printing=True of the reference's optimize_points (opt_defense.py:229-236): at iterations 0, 100, 200, ... it
        prints the loss, the two loss terms and the mean occupancy probability, all evaluated at that iteration's
        pre-update points.  The run is cut so that every such iteration is a launch of its own (the kernel reports the
        losses of a launch's last step; the probability comes from one ifd_decode of the points it starts from) and the
        Adam state is carried across: the result is bit-identical to the uncut run (the neighbour lists are exact at every
        step, the moments are passed on as they are).
        Scaling: the reference prints per BATCH of `batch_size` clouds; a device pass here may hold several reference
        batches (or a shard of one), so the printed terms are the means over this pass's clouds of the per-cloud terms -
        equal to the reference's scalars when the pass is exactly one reference batch, their average otherwise."""
        p, st, t = opt_points, None, 0
        B = opt_points.shape[0]
        while t < n_steps:
            nxt = t if t % 100 == 0 else min(n_steps, (t // 100 + 1) * 100)     # next printing iteration (or the end)
            if nxt > t:                                                          # plain steps up to it
                last = nxt == n_steps
                p, st = self.optimize_points(p, c, rep_weight=rep_weight, steps=nxt - t, lr=lr, loss_batch=loss_batch,
                                             normalize=normalize and last, state=st, return_state=True,
                                             knn_scan_every_step=scan, precision=precision, check=check)
                t = nxt
                continue
            prob = float(torch.sigmoid(self.decode(p, c, precision=precision)).mean())   # occ_value of iteration t (pre-update points)
            last = t + 1 == n_steps
            p, st, loss = self.optimize_points(p, c, rep_weight=rep_weight, steps=1, lr=lr, loss_batch=loss_batch,
                                               normalize=normalize and last, state=st, return_state=True, return_loss=True,
                                               knn_scan_every_step=scan, precision=precision, check=check)
            l = loss.double().cpu()
            if torch.is_tensor(loss_batch):
                lbv = loss_batch.double().cpu()
            else:
                lbv = torch.full((B,), float(loss_batch or B), dtype=torch.float64)
            # per-cloud terms carry their own 1/B; the reference's scalars are sums over the batch of B clouds
            occ = float((l[:, 0]).sum()) * float(B) / float(lbv.sum()) if lbv.numel() else 0.0
            rep = float(l[:, 1].mean()) * rep_weight
            print('iter {}, loss {:.4f}'.format(t, occ + rep))
            print('occ loss: {:.4f}, rep loss: {:.4f}\nocc value mean: {:.4f}'.format(occ, rep, prob))
            t += 1
        return p

    def check_status(self):
        """ifd_optimize_status: raise IfdError if an optimise launch since the last check failed on the device - a cross-CU
        wait of a split cloud that gave up, fixed-point repulsion sums near their range (include/ifd.h).  Synchronises the
        current stream."""
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_optimize_status(self.ctx, self._stream()))

    def counters(self) -> Dict[str, int]:
        """Diagnostic counters of the last optimize_points call (synchronises)."""
        buf = (C.c_uint64 * 16)()
        self._check(self.lib.ifd_get_counters(self.ctx, buf, 16))
        return {"knn_rebuilds": int(buf[0]), "knn_brute_scans": int(buf[1]), "knn_passes": int(buf[2]),
                "cloud0_shader_cycles": int(buf[3]), "knn_ring_evals": int(buf[4]), "knn_exact_evals": int(buf[5]), "knn_refresh_waves": int(buf[6]), "knn_lists_built": int(buf[7]),
                "mesh_points": int(buf[8]), "mesh_rounds": int(buf[9]),
                "prof_cycles": [int(buf[i]) for i in range(8, 16)]}      # only in -DIFD_PROF diagnostic builds

    def wave_trace(self):
        """Time stamps (shader cycles) of one optimiser step of cloud 0, [8 waves][32 slots] - only filled by a
        -DIFD_TRACE diagnostic build of libifd.so (scripts/trace_step.py)."""
        buf = (C.c_uint64 * (16 + 8 * 32))()
        self._check(self.lib.ifd_get_counters(self.ctx, buf, 16 + 8 * 32))
        return [[int(buf[16 + w * 32 + i]) for i in range(32)] for w in range(8)]

    def tile_trace(self):
        """Time stamps (shader cycles) inside ONE decoder tile per wave of the traced step, [8 waves][128 slots] - only filled
        by a -DIFD_TRACE -DIFD_TRACE2=<n> diagnostic build (scripts/tile_trace.py; slot map in optimize.hip decoder_tile3)."""
        base = 16 + 8 * 32 + 3          # behind the three status words (ifd_internal.h TRACE2_BASE)
        buf = (C.c_uint64 * (base + 8 * 128))()
        self._check(self.lib.ifd_get_counters(self.ctx, buf, base + 8 * 128))
        return [[int(buf[base + w * 128 + i]) for i in range(128)] for w in range(8)]

    def normalize_batch_pc(self, points: torch.Tensor) -> torch.Tensor:
        """normalize_batch_pc (opt_defense.py:76-83); returns a new tensor."""
        p = _f32(points, self.device).clone()
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_normalize_unit_sphere(self.ctx, p.data_ptr(), p.shape[0], p.shape[1],
                                                           self._stream()))
        return p


class OnetRestorer(Restorer):
    """ONet-Opt (ONet/opt_defense.py): same call seams, Occupancy-Network model (ifd_onet_create).

    ``encode_inputs`` returns the latent code c [B,512] (generator.model.encode_inputs, :300); ``decode`` and
    ``optimize_points`` take it where ConvONet takes the planes (z is empty: z_dim 0 in configs/onet_mn40.yaml)."""
    model_name = "onet"

    def __init__(self, weights: np.ndarray, device=None, threshold: float = 0.2):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise IfdError("no GPU visible: the restoration path only runs on an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise IfdError("OnetRestorer needs a cuda (ROCm) device, got %s" % self.device)
        self.threshold = float(threshold)
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.size != self.lib.ifd_onet_weight_count():
            raise IfdError("expected %d weights, got %d" % (self.lib.ifd_onet_weight_count(), w.size))
        with torch.cuda.device(self.device):
            self.ctx = self.lib.ifd_onet_create(w.ctypes.data, w.size, self.device.index or 0)
        if not self.ctx:
            raise IfdError((self.lib.ifd_last_error(None) or b"ifd_onet_create failed").decode())
        self._fn_decode, self._fn_optimize = self.lib.ifd_onet_decode_ex, self.lib.ifd_onet_optimize
        self.n_sel = 300                  # onet_mn40.yaml:6 pointcloud_n

    def _cond(self, c) -> torch.Tensor:
        c = _f32(c, self.device)
        if c.dim() != 2 or c.shape[1] != 512:
            raise IfdError("the ONet conditioning code must be [B,512]")
        return c

    def encode_inputs(self, sel: torch.Tensor, t_per_cloud: Optional[torch.Tensor] = None) -> torch.Tensor:
        sel = _f32(sel, self.device)
        B, T = sel.shape[:2]
        tpc = None if t_per_cloud is None else t_per_cloud.to(device=self.device, dtype=torch.int32).contiguous()
        c = torch.empty(B, 512, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_onet_encode(self.ctx, sel.data_ptr(), self._ptr(tpc), B, T, c.data_ptr(),
                                                 self._stream()))
        return c

    def mesh_sample(self, c: torch.Tensor, n_sample: int = 1024, resolution0: int = 32, upsampling_steps: int = 2,
                    padding: float = 0.1, seed: int = 0, cloud_index_base: int = 0, max_triangles: int = 400000,
                    want_grid: bool = False, want_triangles: bool = False, threshold: Optional[float] = None, precision=None):
        """reconstruct_mesh + trimesh.sample.sample_surface (ONet/remesh_defense.py:128-157) for a batch of latent codes:
        c [B,512] -> dict(points [B,n_sample,3] (not normalised), n_triangles [B] int32, optionally grid [B,P,P,P] and
        triangles [B,max_triangles,9]).  ``n_triangles`` is the uncapped total of a cloud's surface: the valid rows of
        ``triangles`` are the first min(n_triangles, max_triangles), and where n_triangles > max_triangles the samples cover
        those triangles only (the lowest-x slabs) - call again with a larger ``max_triangles``.  ``precision``: arithmetic of the grid evaluation's decoder layers (ifd_mesh_params.precision,
        "f32" default / "bf16x6" / "bf16x3")."""
        c = self._cond(c)
        B = c.shape[0]
        P = (resolution0 << upsampling_steps) + 1
        pts = torch.zeros(B, n_sample, 3, device=self.device, dtype=torch.float32)
        ntri = torch.zeros(B, device=self.device, dtype=torch.int32)
        grid = torch.empty(B, P, P, P, device=self.device, dtype=torch.float32) if want_grid else None
        tris = torch.zeros(B, max_triangles, 9, device=self.device, dtype=torch.float32) if want_triangles else None
        prm = IfdMeshParams(C.sizeof(IfdMeshParams), int(resolution0), int(upsampling_steps), int(n_sample), int(max_triangles),
                            float(padding), float(self.threshold if threshold is None else threshold), int(seed),
                            int(cloud_index_base), precision_code(precision), 0)
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_onet_mesh_sample(self.ctx, c.data_ptr(), B, C.byref(prm), pts.data_ptr(), ntri.data_ptr(),
                                                      self._ptr(grid), self._ptr(tris), self._stream()))
        out = {"points": pts, "n_triangles": ntri}
        if want_grid:
            out["grid"] = grid
        if want_triangles:
            out["triangles"] = tris
        return out

    def mesh_from_grid(self, grid: torch.Tensor, iso: float = 0.0, padding: float = 0.1, max_triangles: int = 400000,
                       n_sample: int = 1024, seed: int = 0, cloud_index_base: int = 0, points: Optional[torch.Tensor] = None,
                       triangles: Optional[torch.Tensor] = None, cum_area: Optional[torch.Tensor] = None):
        """Validation seam (ifd_mesh_from_grid): marching cubes + surface sampling of caller-supplied grids [B,P,P,P] at the
        iso-value ``iso`` (used as is), by the production code.  Returns dict(points, n_triangles); ``points`` [B,n_sample,3],
        ``triangles`` [B,max_triangles,9] float32 and ``cum_area`` [B,max_triangles] float64 may be passed in - the library writes
        the valid rows only - and are returned under their names."""
        grid = _f32(grid, self.device)
        if grid.dim() != 4 or not (grid.shape[1] == grid.shape[2] == grid.shape[3]):
            raise IfdError("mesh_from_grid takes grids [B,P,P,P]")
        B, P = int(grid.shape[0]), int(grid.shape[1])
        pts = torch.zeros(B, n_sample, 3, device=self.device, dtype=torch.float32) if points is None else points
        ntri = torch.zeros(B, device=self.device, dtype=torch.int32)
        for t, shape, dt in ((pts, (B, n_sample, 3), torch.float32), (triangles, (B, max_triangles, 9), torch.float32),
                             (cum_area, (B, max_triangles), torch.float64)):
            if t is not None and (tuple(t.shape) != shape or t.dtype != dt or t.device != self.device or not t.is_contiguous()):
                raise IfdError("mesh_from_grid: an output tensor must be contiguous %s %s on %s" % (shape, dt, self.device))
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_mesh_from_grid(self.ctx, grid.data_ptr(), B, P, float(iso), float(padding), int(max_triangles),
                                                    int(n_sample), int(seed), int(cloud_index_base), pts.data_ptr(), ntri.data_ptr(),
                                                    self._ptr(triangles), self._ptr(cum_area), self._stream()))
        out = {"points": pts, "n_triangles": ntri}
        if triangles is not None:
            out["triangles"] = triangles
        if cum_area is not None:
            out["cum_area"] = cum_area
        return out

    def mise_from_field(self, field: torch.Tensor, resolution0: int, upsampling_steps: int, threshold: float = 0.0):
        """Validation seam (ifd_mise_from_field): the production MISE loop on caller-supplied fields [B,P,P,P]
        (P = (resolution0 << upsampling_steps) + 1) in place of the decoder, ``threshold`` compared as is.  Returns
        dict(grid [B,P,P,P] (to_dense), rounds, points): the rounds of the call and the grid points it evaluated."""
        field = _f32(field, self.device)
        if field.dim() != 4 or not (field.shape[1] == field.shape[2] == field.shape[3]):
            raise IfdError("mise_from_field takes fields [B,P,P,P]")
        B, P = int(field.shape[0]), int(field.shape[1])
        grid = torch.empty_like(field)
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_mise_from_field(self.ctx, field.data_ptr(), B, P, int(resolution0), int(upsampling_steps),
                                                     float(threshold), grid.data_ptr(), self._stream()))
        cnt = self.counters()
        return {"grid": grid, "rounds": cnt["mesh_rounds"], "points": cnt["mesh_points"]}

    def encode_points(self, *a, **k):
        raise IfdError("encode_points / unet belong to the ConvONet model")

    unet = encode_points


class DupNet:
    """The reference's baseline defenses on one GPU (include/ifd_dup.h): SRSDefense, SORDefense and DUPNet
    (baselines/defense/drop_points/SRS.py, SOR.py, DUP_Net/DUP_Net.py) behind their call seams.

    ``weights``: the packed PU-Net checkpoint (``weights.load_checkpoint(path, "punet")``), or None for SRS / SOR only.
    Draws are the library's, keyed by ``seed`` and the global cloud index (``cloud_index_base`` + row), so a file gives the
    same result however it is batched; every method also takes explicit draws.  Batches are processed in chunks of
    ``chunk`` clouds, which bounds the context workspace (PU-Net: 1.4 MB per cloud of a chunk)."""

    NPOINT = 1024
    UP_RATIO = 4

    def __init__(self, weights: Optional[np.ndarray] = None, device=None, seed: int = 0, chunk: int = 512):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise IfdError("no GPU visible: the baseline defenses only run on an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.seed, self.chunk = int(seed), int(chunk)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        if w is not None and w.size != self.lib.ifd_punet_weight_count():
            raise IfdError("expected %d PU-Net weights, got %d" % (self.lib.ifd_punet_weight_count(), w.size))
        with torch.cuda.device(self.device):
            self.ctx = self.lib.ifd_dup_create(None if w is None else w.ctypes.data, 0 if w is None else w.size,
                                               self.device.index or 0)
        if not self.ctx:
            raise IfdError((self.lib.ifd_last_error(None) or b"ifd_dup_create failed").decode())
        self.has_punet = w is not None

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ifd_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc: int):
        if rc != _lib.IFD_OK:
            raise IfdError("libifd error %d: %s" % (rc, (self.lib.ifd_last_error(self.ctx) or b"").decode()))

    def _i32(self, t, shape) -> Optional[torch.Tensor]:
        if t is None:
            return None
        t = torch.as_tensor(t).to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise IfdError("explicit draws must have shape %s, got %s" % (tuple(shape), tuple(t.shape)))
        return t

    def _chunks(self, B: int):
        for c0 in range(0, B, self.chunk):
            yield c0, min(B, c0 + self.chunk)

    # ------------------------------------------------------------------ SRS
    def srs(self, pc: torch.Tensor, drop_num: int = 500, idx=None, cloud_index_base: int = 0) -> torch.Tensor:
        """SRSDefense(drop_num).random_drop: [B,K,3] -> [B,K-drop_num,3], rows in draw order.  idx: [B,K-drop_num]."""
        pc = _f32(pc, self.device)
        B, K = pc.shape[:2]
        m = K - int(drop_num)
        if m < 1 or drop_num < 0:
            raise IfdError("SRS: drop_num must leave at least one point (K=%d, drop_num=%d)" % (K, drop_num))
        idx = self._i32(idx, (B, m))
        out = torch.empty(B, m, 3, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            for a, b in self._chunks(B):
                self._check(self.lib.ifd_srs(self.ctx, pc[a:b].data_ptr(), b - a, K, int(drop_num), self.seed,
                                             int(cloud_index_base) + a, None if idx is None else idx[a:b].data_ptr(),
                                             out[a:b].data_ptr(), self._stream()))
        return out

    # ------------------------------------------------------------------ SOR
    def sor_mask(self, pc: torch.Tensor, k: int = 2, alpha: float = 1.1) -> torch.Tensor:
        """SORDefense(k, alpha) keep mask [B,K] uint8 (ifd_sor)."""
        pc = _f32(pc, self.device)
        B, K = pc.shape[:2]
        keep = torch.empty(B, K, device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            for a, b in self._chunks(B):
                self._check(self.lib.ifd_sor(self.ctx, pc[a:b].data_ptr(), b - a, K, int(k), float(alpha),
                                             keep[a:b].data_ptr(), None, self._stream()))
        return keep

    def sor(self, pc: torch.Tensor, k: int = 2, alpha: float = 1.1):
        """SORDefense.forward: a list of [N_i,3] tensors, the kept points in their original order."""
        pc = _f32(pc, self.device)
        keep = self.sor_mask(pc, k, alpha).bool()
        return [pc[i][keep[i]] for i in range(pc.shape[0])]

    # ------------------------------------------------------------------ DUP-Net
    def process_data(self, pc: torch.Tensor, keep: torch.Tensor, draws=None, cloud_index_base: int = 0):
        """DUPNet.process_data on SOR's output given as (pc [B,K,3], keep mask [B,K]) -> ([B,1024,3], n_kept [B]).
        draws: [B,1024] explicit choices into each cloud's kept rows."""
        pc = _f32(pc, self.device)
        B, K = pc.shape[:2]
        keep = keep.to(device=self.device, dtype=torch.uint8).contiguous()
        draws = self._i32(draws, (B, self.NPOINT))
        out = torch.empty(B, self.NPOINT, 3, device=self.device, dtype=torch.float32)
        n = torch.empty(B, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            for a, b in self._chunks(B):
                self._check(self.lib.ifd_dup_fill(self.ctx, pc[a:b].data_ptr(), keep[a:b].data_ptr(), b - a, K, self.NPOINT,
                                                  self.seed, int(cloud_index_base) + a,
                                                  None if draws is None else draws[a:b].data_ptr(), out[a:b].data_ptr(),
                                                  n[a:b].data_ptr(), self._stream()))
        return out, n

    def pu_net(self, x: torch.Tensor, fps_start=None, cloud_index_base: int = 0, want_aux: bool = False):
        """PUNet(npoint=1024, up_ratio=4).forward: [B,1024,3] -> [B,4096,3] (row k*1024+i = branch k, point i).
        fps_start: [B,4] start index of each level's FPS.  want_aux: also return the discrete decisions
        {"fps_idx" [B,1920], "ball_idx" [B,1920,32], "knn_idx" [B,3,1024,3]}."""
        if not self.has_punet:
            raise IfdError("this DupNet was made without PU-Net weights")
        x = _f32(x, self.device)
        B = x.shape[0]
        if tuple(x.shape[1:]) != (self.NPOINT, 3):
            raise IfdError("PU-Net input must be [B,1024,3], got %s" % (tuple(x.shape),))
        fps_start = self._i32(fps_start, (B, 4))
        out = torch.empty(B, self.NPOINT * self.UP_RATIO, 3, device=self.device, dtype=torch.float32)
        aux = None
        if want_aux:
            aux = {"fps_idx": torch.empty(B, 1920, device=self.device, dtype=torch.int32),
                   "ball_idx": torch.empty(B, 1920, 32, device=self.device, dtype=torch.int32),
                   "knn_idx": torch.empty(B, 3, self.NPOINT, 3, device=self.device, dtype=torch.int32)}
        with torch.cuda.device(self.device):
            for a, b in self._chunks(B):
                st = None if aux is None else C.byref(_lib.IfdPunetAux(aux["fps_idx"][a:b].data_ptr(),
                                                                       aux["ball_idx"][a:b].data_ptr(),
                                                                       aux["knn_idx"][a:b].data_ptr()))
                self._check(self.lib.ifd_punet_forward(self.ctx, x[a:b].data_ptr(), b - a, self.NPOINT, self.UP_RATIO,
                                                       None if fps_start is None else fps_start[a:b].data_ptr(), self.seed,
                                                       int(cloud_index_base) + a, out[a:b].data_ptr(), st, self._stream()))
        return (out, aux) if want_aux else out

    def dup(self, pc: torch.Tensor, k: int = 2, alpha: float = 1.1, fill_draws=None, fps_start=None,
            cloud_index_base: int = 0) -> torch.Tensor:
        """DUPNet.forward: SOR, process_data, PU-Net -> [B,4096,3]."""
        pc = _f32(pc, self.device)
        keep = self.sor_mask(pc, k, alpha)
        x, _ = self.process_data(pc, keep, fill_draws, cloud_index_base)
        return self.pu_net(x, fps_start, cloud_index_base)


class Classifier:
    """A victim classifier of the reference on one GPU (include/ifd_cls.h): PointNetCls(k=40, feature_transform, use_bn) in
    eval mode, what baselines/inference.py runs on a restored cloud file.

    ``weights``: the BN-folded canonical vector (``weights.load_checkpoint(path, "pointnet")`` or
    ``weights.pack_state_dict(state_dict, "pointnet")``).  Clouds go in point-major, [B,N,3] - the layout of the .npz files -
    not the [B,3,N] the reference's model takes.  A cloud's logits do not depend on how it is batched or padded."""

    N_CLASSES = 40
    MODELS = {"pointnet": _lib.CLS_POINTNET, "pointnet2": _lib.CLS_POINTNET2, "dgcnn": _lib.CLS_DGCNN,
              "pointconv": _lib.CLS_POINTCONV}

    def __init__(self, weights: np.ndarray, model: str = "pointnet", feature_transform: bool = False, device=None):
        if model not in self.MODELS:
            raise IfdError("unknown victim model %r" % (model,))
        self.lib = _lib.load()
        self.feature_transform = bool(feature_transform)
        want = self.lib.ifd_cls_weight_count(self.MODELS[model], int(self.feature_transform))
        if want == 0:
            raise IfdError("victim model %r is not built (only pointnet is)" % model)
        self._create("ifd_cls_create", want, "%s weights (feature_transform=%s)" % (model, self.feature_transform), weights, device,
                     self.MODELS[model], int(self.feature_transform))

    def _create(self, create_fn: str, want: int, label: str, weights, device, *args):
        """The creation every victim shares: ``want`` weights of the kind ``label`` names, a GPU, the device, then
        lib.<create_fn>(weights, count, *args, N_CLASSES, device index) -> self.ctx."""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.size != want:
            raise IfdError("expected %d %s, got %d" % (want, label, w.size))
        if not torch.cuda.is_available():
            raise IfdError("no GPU visible: the classifier only runs on an MI355X (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        with torch.cuda.device(self.device):
            self.ctx = getattr(self.lib, create_fn)(w.ctypes.data, w.size, *args, self.N_CLASSES, self.device.index or 0)
        if not self.ctx:
            raise IfdError((self.lib.ifd_last_error(None) or create_fn.encode() + b" failed").decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ifd_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _check(self, rc: int):
        if rc != _lib.IFD_OK:
            raise IfdError("libifd error %d: %s" % (rc, (self.lib.ifd_last_error(self.ctx) or b"").decode()))

    def _batch(self, pc, n_points):
        """-> (pc [B,stride,3] f32 on the device, n_points [B] int32 on the device or None)."""
        if isinstance(pc, (list, tuple)) or (isinstance(pc, np.ndarray) and pc.dtype == object):
            if n_points is not None:
                raise IfdError("n_points comes from the clouds themselves when a list of clouds is passed")
            clouds = [np.asarray(c.detach().cpu() if hasattr(c, "detach") else c, dtype=np.float32)[:, :3] for c in pc]
            if not clouds:
                raise IfdError("no clouds")
            counts = np.array([len(c) for c in clouds], dtype=np.int32)
            if len(set(counts.tolist())) == 1:
                return torch.from_numpy(np.ascontiguousarray(np.stack(clouds))).to(self.device), None
            padded = np.zeros((len(clouds), max(int(counts.max()), 1), 3), np.float32)
            for i, c in enumerate(clouds):
                padded[i, :len(c)] = c
            return torch.from_numpy(padded).to(self.device), torch.from_numpy(counts).to(self.device)
        pc = _f32(torch.as_tensor(pc), self.device)
        if pc.dim() != 3 or pc.shape[2] != 3:
            raise IfdError("clouds must be [B,N,3] (point-major), got %s" % (tuple(pc.shape),))
        return pc, self._counts(n_points, int(pc.shape[0]))

    def logits(self, pc, n_points=None, want_aux: bool = False, want_pred: bool = False):
        """pc: [B,N,3] tensor / array, or a list (or object array) of ragged [K_i,3] clouds, which are padded into one strided
        batch.  n_points: [B] valid rows of each cloud of a [B,N,3] batch.  Returns logits [B,40]; with want_aux also
        {"trans" [B,3,3], "trans_feat" [B,64,64] (feature_transform only), "global_feat" [B,1024], "pred" [B] int32}."""
        def aux_table(B, stride):
            f32 = dict(device=self.device, dtype=torch.float32)
            aux = {"trans": torch.empty(B, 3, 3, **f32), "global_feat": torch.empty(B, 1024, **f32)}
            if self.feature_transform:
                aux["trans_feat"] = torch.empty(B, 64, 64, **f32)
            return aux
        return self._forward("ifd_cls_forward", pc, n_points, _lib.IfdClsAux, aux_table, want_aux, want_pred)

    def _forward(self, fn: str, pc, n_points, aux_struct, aux_table, want_aux: bool, want_pred: bool, extra=None):
        """The forward call every victim shares: the batch, the logits, and - with want_aux or want_pred - the aux struct filled
        with "pred" and, with want_aux, the tensors of aux_table(B, stride): a member of aux_struct per name, a list filling an
        array member.  ``extra(B)``: the arguments lib.<fn> takes between n_points and B, as device tensors or None."""
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        between = extra(B) if extra else ()
        out = torch.empty(B, self.N_CLASSES, device=self.device, dtype=torch.float32)
        aux, st = None, None
        if want_aux or want_pred:
            aux = {"pred": torch.empty(B, device=self.device, dtype=torch.int32)}
            if want_aux:
                aux.update(aux_table(B, stride))
            a = aux_struct()
            for name, t in aux.items():
                if isinstance(t, list):
                    for i, ti in enumerate(t):
                        getattr(a, name)[i] = ti.data_ptr()
                else:
                    setattr(a, name, t.data_ptr())
            st = C.byref(a)
        ptr = lambda t: None if t is None else t.data_ptr()        # noqa: E731
        with torch.cuda.device(self.device):
            self._check(getattr(self.lib, fn)(self.ctx, pc.data_ptr(), ptr(n_points), *[ptr(t) for t in between], B, stride,
                                              out.data_ptr(), st, torch.cuda.current_stream(self.device).cuda_stream))
        return (out, aux) if aux is not None else out

    def predict(self, pc, n_points=None) -> torch.Tensor:
        """argmax of the logits, [B] int64 (the lowest class among equal logits, as torch.argmax on the CPU)."""
        _, aux = self.logits(pc, n_points, want_pred=True)
        return aux["pred"].long()

    # ---- include/ifd_atk.h: input gradients and the FGM family (models without feature_transform) ----
    LOSSES = {"logits": _lib.ATK_LOSS_LOGITS, "cross_entropy": _lib.ATK_LOSS_CE, "ce": _lib.ATK_LOSS_CE}
    FGM_KINDS = {"fgm": _lib.FGM_FGM, "ifgm": _lib.FGM_IFGM, "mifgm": _lib.FGM_MIFGM, "pgd": _lib.FGM_PGD}

    def _loss_kind(self, loss):
        if loss not in self.LOSSES:
            raise IfdError("unknown adversarial loss %r (logits | cross_entropy)" % (loss,))
        return self.LOSSES[loss]

    def _target(self, target, B):
        t = torch.as_tensor(target).to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(t.shape) != (B,):
            raise IfdError("target must be [B]")
        return t

    def _counts(self, n, B):
        """n_points / n_ori as [B] int32 on the device, or None."""
        if n is None:
            return None
        n = torch.as_tensor(n).to(device=self.device, dtype=torch.int32).contiguous()
        if tuple(n.shape) != (B,):
            raise IfdError("n_points must be [B]")
        return n

    def _vec(self, x, B, dtype, name):
        """pred / loss as [B] of dtype on the device, or None."""
        if x is None:
            return None
        x = torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()
        if tuple(x.shape) != (B,):
            raise IfdError("%s must be [B]" % name)
        return x

    def _diag(self, want, shapes, names_text):
        """The diagnostics named in ``want`` as a dict of device tensors, NaN / -1 where the library leaves them untouched."""
        out = {}
        for k in want:
            if k not in shapes:
                raise IfdError("unknown diagnostic %r (%s)" % (k, names_text))
            shape, dt = shapes[k]
            out[k] = torch.full(shape, float("nan") if dt == torch.float32 else -1, device=self.device, dtype=dt)
        return out

    @staticmethod
    def _bounds(bounds):
        return {"weight": bounds[0], "lower": bounds[1], "upper": bounds[2]}

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    # the library calls behind input_grad, fgm_update and fgm_attack; a victim with its own (DgcnnClassifier) names them here
    ATK_FNS = {"input_grad": "ifd_cls_input_grad", "fgm_update": "ifd_fgm_update", "fgm_attack": "ifd_fgm_attack"}
    # and behind the Perturb, kNN and Drop calls: PointNet's own entry points here, include/ifd_victim_atk.h's on the other victims
    LOOP_FNS = {"cw_step": "ifd_cw_step", "cw_adjust": "ifd_cw_adjust", "cw_perturb_attack": "ifd_cw_perturb_attack",
                "knn_step": "ifd_knn_step", "knn_project_clip": "ifd_knn_project_clip", "knn_attack": "ifd_knn_attack",
                "drop_step": "ifd_drop_step", "drop_attack": "ifd_drop_attack"}
    VICTIM_LOOP_FNS = {"cw_step": "ifd_victim_cw_step", "cw_adjust": "ifd_victim_cw_adjust",
                      "cw_perturb_attack": "ifd_victim_cw_perturb_attack", "knn_step": "ifd_victim_knn_step",
                      "knn_project_clip": "ifd_victim_knn_project_clip", "knn_attack": "ifd_victim_knn_attack",
                      "drop_step": "ifd_victim_drop_step", "drop_attack": "ifd_victim_drop_attack"}

    def _fn(self, name):
        return getattr(self.lib, self.LOOP_FNS[name])

    def _loop_starts(self, fps_start, B):
        """The fps_start argument of a whole-loop call as a list of device tensors (or None) that the call takes behind n_points:
        PointNet's own calls have none."""
        if fps_start is not None:
            raise IfdError("this victim does not sample: it takes no fps_start")
        return []

    GRAD_OUT = _lib.IfdAtkOut            # the library's struct of input_grad's diagnostics: a member per name of _grad_spec

    def _grad_spec(self, B, stride):
        """input_grad's diagnostics: name -> (shape, dtype, fill), or a list of those for an array member; fill None: the library
        writes every element."""
        f, i = torch.float32, torch.int32
        return {"logits": ((B, self.N_CLASSES), f, None), "loss": ((B,), f, None), "pred": ((B,), i, None),
                "win_feat": ((B, 1024), i, None), "win_stn": ((B, 1024), i, None), "global_feat": ((B, 1024), f, None)}

    def _make(self, entry):
        """The device tensor(s) of one entry of a spec."""
        if isinstance(entry, list):
            return [self._make(e) for e in entry]
        shape, dt, fill = entry
        return torch.empty(shape, device=self.device, dtype=dt) if fill is None else torch.full(shape, fill, device=self.device, dtype=dt)

    def _grad_aux(self, B, stride, names=None):
        """-> (the diagnostics of input_grad as a dict of device tensors, the library's struct pointing at them).  names: only
        those are allocated and filled; None: all of them."""
        spec = self._grad_spec(B, stride)
        if names is not None:
            for n in names:
                if n not in spec:
                    raise IfdError("unknown diagnostic %r of input_grad (%s)" % (n, " | ".join(spec)))
            spec = {n: e for n, e in spec.items() if n in names}
        aux = {n: self._make(e) for n, e in spec.items()}
        st = self.GRAD_OUT()
        for name, t in aux.items():
            if isinstance(t, list):
                for j, tj in enumerate(t):
                    getattr(st, name)[j] = tj.data_ptr()
            else:
                setattr(st, name, t.data_ptr())
        return aux, st

    def input_grad(self, pc, target, loss="logits", kappa=0., scale=1., n_points=None, want_aux: bool = False):
        """scale * d loss_b / d pc[b] of an adversarial loss on the logits (FGM.get_gradient without its normalisation):
        grad [B,N,3], zeros in the rows beyond a cloud's points.  pc: as ``logits`` takes it, ragged lists included; target [B].
        loss: "logits" (LogitsAdvLoss(kappa)) or "cross_entropy".  With want_aux also {"logits" [B,40], "loss" [B], "pred" [B],
        "win_feat" / "win_stn" [B,1024] int32 (the point each max-pool channel came from), "global_feat" [B,1024]}.  want_aux may
        also be a tuple of those names, e.g. ("pred", "loss"): then only they are allocated, filled and returned."""
        return self._input_grad(pc, target, loss, kappa, scale, n_points, want_aux)

    def _input_grad(self, pc, target, loss, kappa, scale, n_points, want_aux, extra=None):
        """input_grad's call; ``extra(B)``: the arguments the library call takes between n_points and B, device tensors or None."""
        kind = self._loss_kind(loss)
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        target = self._target(target, B)
        held = extra(B) if extra else ()                               # the tensors stay alive until the call has been made
        between = [None if t is None else t.data_ptr() for t in held]
        grad = torch.empty(B, stride, 3, device=self.device, dtype=torch.float32)
        aux, st = None, None
        if want_aux:
            aux, struct = self._grad_aux(B, stride, tuple(want_aux) if isinstance(want_aux, (tuple, list)) else None)
            st = C.byref(struct)
        with torch.cuda.device(self.device):
            self._check(getattr(self.lib, self.ATK_FNS["input_grad"])(
                self.ctx, pc.data_ptr(), None if n_points is None else n_points.data_ptr(), *between, B, stride, target.data_ptr(), kind,
                float(kappa), float(scale), grad.data_ptr(), st, self._stream()))
        return (grad, aux) if want_aux else grad

    def fgm_update(self, kind, grad, pc, ori_pc=None, momentum=None, step_size=0., budget=0., mu=1., n_points=None):
        """One update of FGM.py IN PLACE on ``pc`` (and ``momentum``): contiguous float32 [B,N,3] tensors on the device."""
        if kind not in self.FGM_KINDS:
            raise IfdError("unknown attack %r (fgm | ifgm | mifgm | pgd)" % (kind,))
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        for t in (grad, pc, ori_pc, momentum):
            if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, stride, 3)):
                raise IfdError("fgm_update works in place on contiguous float32 [B,N,3] device tensors")
        n_points = self._counts(n_points, B)
        ptr = lambda t: None if t is None else t.data_ptr()        # noqa: E731
        with torch.cuda.device(self.device):
            self._check(getattr(self.lib, self.ATK_FNS["fgm_update"])(
                self.ctx, self.FGM_KINDS[kind], ptr(grad), ptr(pc), ptr(ori_pc), ptr(momentum), float(step_size), float(budget), float(mu),
                ptr(n_points), B, stride, self._stream()))
        return pc

    def fgm_attack(self, kind, pc, target, budget, step_size, num_iter=1, mu=1., loss="logits", kappa=0., scale=1., n_points=None):
        """The whole loop on the device (ifd_fgm_attack): -> (adversarial clouds [B,N,3], success [B] bool).  ``pc`` is the
        start AND the centre of the clip: pass it with the start noise already added."""
        return self._fgm_attack(kind, pc, target, budget, step_size, num_iter, mu, loss, kappa, scale, n_points)

    def _fgm_attack(self, kind, pc, target, budget, step_size, num_iter, mu, loss, kappa, scale, n_points, extra=None):
        """fgm_attack's call; ``extra(B)``: the arguments the library call takes between n_points and target."""
        if kind not in self.FGM_KINDS:
            raise IfdError("unknown attack %r (fgm | ifgm | mifgm | pgd)" % (kind,))
        loss_kind = self._loss_kind(loss)
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        target = self._target(target, B)
        held = extra(B) if extra else ()                               # the tensors stay alive until the call has been made
        between = [None if t is None else t.data_ptr() for t in held]
        out = torch.empty_like(pc)
        success = torch.empty(B, device=self.device, dtype=torch.int32)
        P = _lib.IfdFgmParams(C.sizeof(_lib.IfdFgmParams), self.FGM_KINDS[kind], loss_kind, int(num_iter), float(kappa), float(scale),
                              float(step_size), float(budget), float(mu))
        with torch.cuda.device(self.device):
            self._check(getattr(self.lib, self.ATK_FNS["fgm_attack"])(
                self.ctx, C.byref(P), pc.data_ptr(), None if n_points is None else n_points.data_ptr(), *between, target.data_ptr(), B, stride,
                out.data_ptr(), success.data_ptr(), self._stream()))
        return out, success.bool()

    # ---- include/ifd_cw.h: the CW point-perturbation attack (models without feature_transform) ----
    CW_STATE = (("m", torch.float32, 3), ("v", torch.float32, 3), ("bestdist", torch.float32, 1), ("bestscore", torch.int32, 1),
                ("o_bestdist", torch.float32, 1), ("o_bestscore", torch.int32, 1), ("o_bestattack", torch.float32, 3),
                ("weight", torch.float64, 1), ("lower", torch.float64, 1), ("upper", torch.float64, 1))

    def cw_state(self, B, stride, init_weight=10., max_weight=80.):
        """The state of a fresh attack (ifd_cw_state) as a dict of device tensors: Perturb.py:59-66, 74-76."""
        f = lambda shape, v, dt: torch.full(shape, v, device=self.device, dtype=dt)      # noqa: E731
        return {"m": f((B, stride, 3), 0., torch.float32), "v": f((B, stride, 3), 0., torch.float32),
                "bestdist": f((B,), 1e10, torch.float32), "bestscore": f((B,), -1, torch.int32),
                "o_bestdist": f((B,), 1e10, torch.float32), "o_bestscore": f((B,), -1, torch.int32),
                "o_bestattack": f((B, stride, 3), 0., torch.float32), "weight": f((B,), float(init_weight), torch.float64),
                "lower": f((B,), 0., torch.float64), "upper": f((B,), float(max_weight), torch.float64)}

    def _cw_struct(self, state, B, stride):
        ptrs = []
        for key, dt, rank in self.CW_STATE:
            t = state.get(key)
            want = (B, stride, 3) if rank == 3 else (B,)
            if t is None or not (t.is_cuda and t.dtype == dt and t.is_contiguous() and tuple(t.shape) == want):
                raise IfdError("cw state %r must be a contiguous %s device tensor of shape %s" % (key, dt, want))
            ptrs.append(t.data_ptr())
        return _lib.IfdCwState(*ptrs)

    def _cw_cloud(self, t, B, stride, what):
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, stride, 3)):
            raise IfdError("%s must be a contiguous float32 [B,N,3] device tensor" % what)
        return None if t is None else t.data_ptr()

    def cw_step(self, state, grad, pred, target, adv, ori, t, lr, scale=1., loss=None, last_input=None, n_points=None,
                want_info: bool = False):
        """One iteration of the CW attack behind ``input_grad`` (ifd_cw_step), IN PLACE on ``adv`` and ``state`` (a dict as
        ``cw_state`` makes it).  grad, pred, loss: as ``input_grad`` returned them for ``adv``.  With want_info returns
        [B,3] = (adversarial loss, dist * weight, dist) per cloud."""
        B, stride = int(adv.shape[0]), int(adv.shape[1])
        st = self._cw_struct(state, B, stride)
        ptrs = [self._cw_cloud(x, B, stride, n) for x, n in ((grad, "grad"), (adv, "adv"), (ori, "ori"), (last_input, "last_input"))]
        pred = self._vec(pred, B, torch.int32, "pred")
        target = self._target(target, B)
        loss = self._vec(loss, B, torch.float32, "loss")
        n_points = self._counts(n_points, B)
        info = torch.empty(B, 3, device=self.device, dtype=torch.float32) if want_info else None
        ptr = lambda x: None if x is None else x.data_ptr()        # noqa: E731
        with torch.cuda.device(self.device):
            self._check(self._fn("cw_step")(self.ctx, C.byref(st), ptrs[0], pred.data_ptr(), ptr(loss), target.data_ptr(), ptrs[1], ptrs[2],
                                             ptrs[3], ptr(info), int(t), float(lr), float(scale), ptr(n_points), B, stride, self._stream()))
        return info

    def cw_adjust(self, state, target, n_points=None):
        """The end of a search step (ifd_cw_adjust), IN PLACE on ``state``: the weight's binary search, then the reset of
        bestdist, bestscore, m and v."""
        B, stride = int(state["m"].shape[0]), int(state["m"].shape[1])
        st = self._cw_struct(state, B, stride)
        target = self._target(target, B)
        n_points = self._counts(n_points, B)
        with torch.cuda.device(self.device):
            self._check(self._fn("cw_adjust")(self.ctx, C.byref(st), target.data_ptr(), None if n_points is None else n_points.data_ptr(),
                                               B, stride, self._stream()))
        return state

    def cw_perturb_attack(self, pc, target, noise=None, loss="logits", kappa=0., scale=1., attack_lr=1e-2, init_weight=10.,
                          max_weight=80., binary_step=10, num_iter=500, n_points=None, want_bounds: bool = False, fps_start=None):
        """The whole CW point-perturbation attack on the device (ifd_cw_perturb_attack): -> (adversarial clouds [B,N,3],
        best_dist [B] (1e10 where no iteration reached the target), success [B] bool) and with want_bounds also
        {"weight", "lower", "upper"} [B] float64.  noise: [binary_step,B,N,3], the start noise of every search step, or None."""
        loss_kind = self._loss_kind(loss)
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        target = self._target(target, B)
        starts = self._loop_starts(fps_start, B)
        if noise is not None:
            noise = _f32(torch.as_tensor(noise), self.device)
            if tuple(noise.shape) != (int(binary_step), B, stride, 3):
                raise IfdError("noise must be [binary_step,B,N,3]")
        out = torch.empty_like(pc)
        best = torch.empty(B, device=self.device, dtype=torch.float32)
        success = torch.empty(B, device=self.device, dtype=torch.int32)
        bounds = torch.empty(3, B, device=self.device, dtype=torch.float64) if want_bounds else None
        P = _lib.IfdCwParams(C.sizeof(_lib.IfdCwParams), loss_kind, int(binary_step), int(num_iter), float(kappa), float(scale),
                             float(attack_lr), float(init_weight), float(max_weight))
        with torch.cuda.device(self.device):
            self._check(self._fn("cw_perturb_attack")(self.ctx, C.byref(P), pc.data_ptr(),
                                                       None if n_points is None else n_points.data_ptr(),
                                                       *[None if t is None else t.data_ptr() for t in starts],
                                                       target.data_ptr(), None if noise is None else noise.data_ptr(), B, stride,
                                                       out.data_ptr(), best.data_ptr(), success.data_ptr(),
                                                       None if bounds is None else bounds.data_ptr(), self._stream()))
        if want_bounds:
            return out, best, success.bool(), self._bounds(bounds)
        return out, best, success.bool()

    # ---- include/ifd_knn.h: the kNN attack (models without feature_transform) ----
    def _knn_params(self, loss_kind=_lib.ATK_LOSS_LOGITS, num_iter=1, kappa=0., scale=1., attack_lr=1e-3, chamfer_weight=5., knn_weight=3.,
                    alpha=1.05, budget=0.1):
        return _lib.IfdKnnParams(C.sizeof(_lib.IfdKnnParams), int(loss_kind), int(num_iter), float(kappa), float(scale), float(attack_lr),
                                 float(chamfer_weight), float(knn_weight), float(alpha), float(budget))

    def knn_step(self, grad, adv, ori, m, v, t, lr, scale=1., normal=None, loss=None, n_points=None, chamfer_weight=5., knn_weight=3.,
                 alpha=1.05, budget=0.1, want=()):
        """One iteration of the kNN attack behind ``input_grad`` (ifd_knn_step), IN PLACE on ``adv``, ``m`` and ``v``: contiguous
        float32 [B,N,3] device tensors, 6 <= N <= 2048.  grad, loss: as ``input_grad`` returned them for ``adv``; normal [B,N,3] or
        None (then the clip alone follows Adam).  ``want``: names of diagnostics to return as a dict - "info" [B,4] (adversarial
        loss, cd, knn, n (w1 cd + w2 knn)), "dist_grad" [B,N,3], "nn_ori" [B,N], "nn5" [B,N,5], "mask" [B,N] (int32; rows beyond a
        cloud's count, and clouds below 6 points, are left as they were allocated: -1 / NaN)."""
        if not torch.is_tensor(adv) or adv.dim() != 3:
            raise IfdError("adv must be a contiguous float32 [B,N,3] device tensor")
        B, stride = int(adv.shape[0]), int(adv.shape[1])
        names = (("grad", grad), ("adv", adv), ("ori", ori), ("m", m), ("v", v), ("normal", normal))
        for name, x in names:
            if x is None and name != "normal":
                raise IfdError("%s is missing" % name)
        ptrs = {name: self._cw_cloud(x, B, stride, name) for name, x in names}
        loss = self._vec(loss, B, torch.float32, "loss")
        n_points = self._counts(n_points, B)
        shapes = {"info": ((B, 4), torch.float32), "dist_grad": ((B, stride, 3), torch.float32), "nn_ori": ((B, stride), torch.int32),
                  "nn5": ((B, stride, 5), torch.int32), "mask": ((B, stride), torch.int32)}
        out = self._diag(want, shapes, "info | dist_grad | nn_ori | nn5 | mask")
        ptr = lambda x: None if x is None else x.data_ptr()        # noqa: E731
        diag = _lib.IfdKnnDiag(*[ptr(out.get(k)) for k in ("info", "dist_grad", "nn_ori", "nn5", "mask")])
        P = self._knn_params(chamfer_weight=chamfer_weight, knn_weight=knn_weight, alpha=alpha, budget=budget)
        with torch.cuda.device(self.device):
            self._check(self._fn("knn_step")(self.ctx, C.byref(P), ptrs["grad"], ptr(loss), ptrs["adv"], ptrs["ori"], ptrs["normal"],
                                              ptrs["m"], ptrs["v"], int(t), float(lr), float(scale), C.byref(diag) if out else None,
                                              ptr(n_points), B, stride, self._stream()))
        return out

    def knn_project_clip(self, adv, ori, normal=None, budget=0.1, n_points=None):
        """ProjectInnerClipLinf(budget) IN PLACE on ``adv`` (ifd_knn_project_clip): contiguous float32 [B,N,3] device tensors;
        normal None: the clip alone."""
        if not torch.is_tensor(adv) or adv.dim() != 3:
            raise IfdError("adv must be a contiguous float32 [B,N,3] device tensor")
        B, stride = int(adv.shape[0]), int(adv.shape[1])
        if ori is None:
            raise IfdError("ori is missing")
        ptrs = [self._cw_cloud(x, B, stride, name) for name, x in (("adv", adv), ("ori", ori), ("normal", normal))]
        n_points = self._counts(n_points, B)
        with torch.cuda.device(self.device):
            self._check(self._fn("knn_project_clip")(self.ctx, ptrs[0], ptrs[1], ptrs[2], float(budget),
                                                      None if n_points is None else n_points.data_ptr(), B, stride, self._stream()))
        return adv

    def knn_attack(self, pc, target, normal=None, noise=None, loss="logits", kappa=15., scale=1., attack_lr=1e-3, num_iter=2500,
                   n_points=None, chamfer_weight=5., knn_weight=3., alpha=1.05, budget=0.1, fps_start=None):
        """The whole kNN attack on the device (ifd_knn_attack): -> (adversarial clouds [B,N,3], pred [B] int64, success [B] bool).
        pc [B,N,3]; normal [B,N,3] or None (the clip alone); noise [B,N,3], the start noise, or None."""
        loss_kind = self._loss_kind(loss)
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        target = self._target(target, B)
        starts = self._loop_starts(fps_start, B)
        extra = {}
        for name, x in (("normal", normal), ("noise", noise)):
            if x is not None:
                x = _f32(torch.as_tensor(x), self.device)
                if tuple(x.shape) != (B, stride, 3):
                    raise IfdError("%s must be [B,N,3]" % name)
            extra[name] = x
        out = torch.empty_like(pc)
        pred = torch.empty(B, device=self.device, dtype=torch.int32)
        success = torch.empty(B, device=self.device, dtype=torch.int32)
        P = self._knn_params(loss_kind, num_iter, kappa, scale, attack_lr, chamfer_weight, knn_weight, alpha, budget)
        ptr = lambda x: None if x is None else x.data_ptr()        # noqa: E731
        with torch.cuda.device(self.device):
            self._check(self._fn("knn_attack")(self.ctx, C.byref(P), pc.data_ptr(), ptr(extra["normal"]), ptr(n_points),
                                            *[ptr(t) for t in starts], target.data_ptr(),
                                                ptr(extra["noise"]), B, stride, out.data_ptr(), pred.data_ptr(), success.data_ptr(),
                                                self._stream()))
        return out, pred.long(), success.bool()

    # ---- include/ifd_add.h: the CW point-adding attack (models without feature_transform) ----
    ADD_KINDS = {"chamfer": _lib.ADD_CHAMFER, "hausdorff": _lib.ADD_HAUSDORFF}

    def _add_kind(self, kind):
        if kind not in self.ADD_KINDS:
            raise IfdError("unknown set distance %r (chamfer | hausdorff)" % (kind,))
        return self.ADD_KINDS[kind]

    def _add_num(self, num_add):
        num_add = int(num_add)
        if not 1 <= num_add <= _lib.ADD_MAX_ADD:
            raise IfdError("num_add must be in [1, %d]" % _lib.ADD_MAX_ADD)
        return num_add

    # what add_*, cluster_* and object_* share (include/ifd_add.h, ifd_cluster.h, ifd_object.h)
    def _group_rows(self, num_add, per, word):
        """-> (num_add, per, A = num_add * per) of clusters or objects of ``per`` points; word: how ``per`` reads in the refusal."""
        num_add, per = int(num_add), int(per)
        if num_add < 1 or per < 1 or not 1 <= num_add * per <= _lib.ADD_MAX_ADD:
            raise IfdError("num_add and %s must be at least 1 and num_add * %s in [1, %d]" % (word, word, _lib.ADD_MAX_ADD))
        return num_add, per, num_add * per

    @staticmethod
    def _cat_dims(cat):
        if not torch.is_tensor(cat) or cat.dim() != 3:
            raise IfdError("cat must be a contiguous float32 [B,N,3] device tensor")
        return int(cat.shape[0]), int(cat.shape[1])

    def _shaped(self, x, shape, message):
        """x as a float32 device tensor of that shape, or None."""
        if x is None:
            return None
        x = _f32(torch.as_tensor(x), self.device)
        if tuple(x.shape) != tuple(shape):
            raise IfdError(message)
        return x

    def _adding_step(self, fn, lead, counts, A, shapes, diag_type, grad, pred, target, cat, t, lr, scale, loss, last_input, n_ori,
                     want_info, want):
        """The body of add_step, cluster_step and object_step.  lead: the library call's arguments in front of grad (the kind, the
        state struct, the object template), counts: those behind the stride (num_add, the points per group); A: added rows a cloud;
        shapes: the diagnostics {name: (shape, dtype)} in the order of diag_type's members."""
        B, stride = self._cat_dims(cat)
        ptrs = [self._cw_cloud(x, B, stride, n) for x, n in ((grad, "grad"), (cat, "cat"))]
        if grad is None:
            raise IfdError("grad is missing")
        li = self._cw_cloud(last_input, B, A, "last_input")
        pred = self._vec(pred, B, torch.int32, "pred")
        target = self._target(target, B)
        loss = self._vec(loss, B, torch.float32, "loss")
        n_ori = self._counts(n_ori, B)
        out = self._diag(want, shapes, " | ".join(shapes))
        ptr = lambda x: None if x is None else x.data_ptr()        # noqa: E731
        diag = diag_type(*[ptr(out.get(k)) for k in shapes])
        info = torch.empty(B, 3, device=self.device, dtype=torch.float32) if want_info else None
        with torch.cuda.device(self.device):
            self._check(fn(self.ctx, *lead, ptrs[0], pred.data_ptr(), ptr(loss), target.data_ptr(), ptrs[1], ptr(n_ori), li, ptr(info),
                           C.byref(diag) if out else None, int(t), float(lr), float(scale), B, stride, *counts, self._stream()))
        if want_info:
            out["info"] = info
        return out

    def _adding_inputs(self, loss, pc, n_points, target):
        """The front of add_attack, cluster_attack and object_attack -> (loss_kind, pc, n_points, B, stride, target)."""
        loss_kind = self._loss_kind(loss)
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        return loss_kind, pc, n_points, B, stride, self._target(target, B)

    def _adding_attack(self, fn, params, pc, n_points, target, between, A, out_stride, want_bounds):
        """... and their end: the outputs of A added rows a cloud and the library call.  params: the call's struct; between: its
        tensors (or None) between target and B."""
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        out_stride = stride + A if out_stride is None else int(out_stride)
        if out_stride < 1:
            raise IfdError("out_stride must be positive")
        out = torch.zeros(B, out_stride, 3, device=self.device, dtype=torch.float32)
        best = torch.empty(B, device=self.device, dtype=torch.float32)
        success = torch.empty(B, device=self.device, dtype=torch.int32)
        bounds = torch.empty(3, B, device=self.device, dtype=torch.float64) if want_bounds else None
        ptr = lambda x: None if x is None else x.data_ptr()        # noqa: E731
        with torch.cuda.device(self.device):
            self._check(fn(self.ctx, C.byref(params), pc.data_ptr(), ptr(n_points), target.data_ptr(), *[ptr(x) for x in between], B, stride,
                           out_stride, out.data_ptr(), best.data_ptr(), success.data_ptr(), ptr(bounds), self._stream()))
        if want_bounds:
            return out, best, success.bool(), self._bounds(bounds)
        return out, best, success.bool()

    def add_select(self, grad, pc, num_add, n_points=None, want_idx: bool = False):
        """The num_add rows of ``pc`` [B,N,3] with the largest gradient norm (ifd_add_select), in descending order of the score
        (gx*gx + gy*gy) + gz*gz, the lowest index first among equal scores: -> cri [B,num_add,3], with want_idx also idx
        [B,num_add] int32.  grad [B,N,3] as ``input_grad`` returns it; num_add <= n <= 2048 rows per cloud."""
        num_add = self._add_num(num_add)
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        grad = _f32(torch.as_tensor(grad), self.device)
        if tuple(grad.shape) != (B, stride, 3):
            raise IfdError("grad must have the clouds' shape [B,N,3]")
        cri = torch.empty(B, num_add, 3, device=self.device, dtype=torch.float32)
        idx = torch.empty(B, num_add, device=self.device, dtype=torch.int32) if want_idx else None
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_add_select(self.ctx, grad.data_ptr(), pc.data_ptr(), None if n_points is None else n_points.data_ptr(),
                                                B, stride, num_add, cri.data_ptr(), None if idx is None else idx.data_ptr(),
                                                self._stream()))
        return (cri, idx) if want_idx else cri

    def add_critical_points(self, pc, target, num_add, scale=1., n_points=None, want_idx: bool = False):
        """Add.py get_critical_points (ifd_add_critical_points): ``add_select`` on the gradient of scale * cross_entropy(logits,
        target) -> cri [B,num_add,3], with want_idx also idx [B,num_add] int32."""
        num_add = self._add_num(num_add)
        pc, n_points = self._batch(pc, n_points)
        B, stride = int(pc.shape[0]), int(pc.shape[1])
        target = self._target(target, B)
        cri = torch.empty(B, num_add, 3, device=self.device, dtype=torch.float32)
        idx = torch.empty(B, num_add, device=self.device, dtype=torch.int32) if want_idx else None
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_add_critical_points(self.ctx, pc.data_ptr(), None if n_points is None else n_points.data_ptr(),
                                                         target.data_ptr(), B, stride, num_add, float(scale), cri.data_ptr(),
                                                         None if idx is None else idx.data_ptr(), self._stream()))
        return (cri, idx) if want_idx else cri

    def add_step(self, kind, state, grad, pred, target, cat, num_add, t, lr, scale=1., loss=None, last_input=None, n_ori=None,
                 want_info: bool = False, want=()):
        """One iteration of the point-adding attack behind ``input_grad`` on the concatenated clouds (ifd_add_step), IN PLACE on
        the added rows of ``cat`` [B,N,3] (cloud b: n_ori[b] originals, then num_add added rows; n_ori None: N - num_add) and on
        ``state`` (``cw_state(B, num_add, ...)``).  grad [B,N,3], pred, loss: as ``input_grad`` returned them for ``cat`` with
        n_points = n_ori + num_add; last_input [B,num_add,3] or None.  Returns a dict: with want_info "info" [B,3] (adversarial loss,
        dist * weight, dist), and the diagnostics named in ``want``: "dist_grad" [B,num_add,3], "nn_ori" [B,num_add] int32, "far" [B]
        int32 (clouds outside the limits are left as allocated: NaN / -1)."""
        kind = self._add_kind(kind)
        num_add = self._add_num(num_add)
        B, _ = self._cat_dims(cat)
        st = self._cw_struct(state, B, num_add)
        shapes = {"dist_grad": ((B, num_add, 3), torch.float32), "nn_ori": ((B, num_add), torch.int32), "far": ((B,), torch.int32)}
        return self._adding_step(self.lib.ifd_add_step, [kind, C.byref(st)], [num_add], num_add, shapes, _lib.IfdAddDiag, grad, pred, target,
                                 cat, t, lr, scale, loss, last_input, n_ori, want_info, want)

    def add_attack(self, kind, pc, target, num_add, noise=None, loss="logits", kappa=0., scale=1., attack_lr=1e-2, init_weight=5e3,
                   max_weight=4e4, binary_step=10, num_iter=500, n_points=None, out_stride=None, want_bounds: bool = False):
        """The whole CW point-adding attack on the device (ifd_add_attack): -> (clouds [B,out_stride,3]: each cloud's originals bit
        for bit, then its num_add added points; best_dist [B] (1e10 where no iteration reached the target); success [B] bool) and
        with want_bounds also {"weight", "lower", "upper"} [B] float64.  noise: [binary_step,B,num_add,3], the start noise of every
        search step, or None.  out_stride: rows of the output, default N + num_add (rows beyond a cloud's n + num_add are zero)."""
        kind = self._add_kind(kind)
        num_add = self._add_num(num_add)
        loss_kind, pc, n_points, B, stride, target = self._adding_inputs(loss, pc, n_points, target)
        noise = self._shaped(noise, (int(binary_step), B, num_add, 3), "noise must be [binary_step,B,num_add,3]")
        P = _lib.IfdAddParams(C.sizeof(_lib.IfdAddParams), kind, loss_kind, int(binary_step), int(num_iter), num_add, float(kappa),
                              float(scale), float(attack_lr), float(init_weight), float(max_weight))
        return self._adding_attack(self.lib.ifd_add_attack, P, pc, n_points, target, [noise], num_add, out_stride, want_bounds)

    # ---- include/ifd_cluster.h: the CW cluster-adding attack (models without feature_transform) ----
    def cluster_dbscan(self, pts, eps=0.2, min_samples=3, n_pts=None, want_count: bool = False):
        """DBSCAN of every cloud of ``pts`` [B,N,3] (or a ragged list) by the definition in include/ifd_cluster.h
        (ifd_cluster_dbscan): -> labels [B,N] int32 - clusters 0, 1, ... by ascending lowest core point, -1 for outliers and in the
        rows beyond a cloud's points - and with want_count also the number of clusters [B] int32.  1 <= n <= 256 points a cloud."""
        pts, n_pts = self._batch(pts, n_pts)
        B, stride = int(pts.shape[0]), int(pts.shape[1])
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        labels = torch.full((B, stride), -1, device=self.device, dtype=torch.int32)
        count = torch.zeros(B, device=self.device, dtype=torch.int32) if want_count else None
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_cluster_dbscan(self.ctx, pts.data_ptr(), None if n_pts is None else n_pts.data_ptr(), B, stride,
                                                    float(eps), int(min_samples), labels.data_ptr(),
                                                    None if count is None else count.data_ptr(), self._stream()))
        return (labels, count) if want_count else labels

    def cluster_step(self, state, grad, pred, target, cat, num_add, cl_num_p, t, lr, scale=1., loss=None, last_input=None, n_ori=None,
                     want_info: bool = False, want=()):
        """One iteration of the cluster-adding attack behind ``input_grad`` on the concatenated clouds (ifd_cluster_step), IN PLACE
        on the added rows of ``cat`` [B,N,3] (cloud b: n_ori[b] originals, then A = num_add * cl_num_p added rows, cluster c the rows
        [c * cl_num_p, (c + 1) * cl_num_p); n_ori None: N - A) and on ``state`` (``cw_state(B, A, ...)``).  grad, pred, loss, last_input
        [B,A,3]: as ``add_step`` takes them.  Returns a dict: with want_info "info" [B,3] (adversarial loss, dist * weight, dist), and
        the diagnostics named in ``want``: "dist_grad" [B,A,3], "nn_ori" [B,A] int32, "far_i" / "far_j" [B,num_add] int32, "far_val"
        [B,num_add] (clouds outside the limits are left as allocated: NaN / -1)."""
        num_add, cl_num_p, A = self._group_rows(num_add, cl_num_p, "cl_num_p")
        B, _ = self._cat_dims(cat)
        st = self._cw_struct(state, B, A)
        shapes = {"dist_grad": ((B, A, 3), torch.float32), "nn_ori": ((B, A), torch.int32), "far_i": ((B, num_add), torch.int32),
                  "far_j": ((B, num_add), torch.int32), "far_val": ((B, num_add), torch.float32)}
        return self._adding_step(self.lib.ifd_cluster_step, [C.byref(st)], [num_add, cl_num_p], A, shapes, _lib.IfdClusterDiag, grad, pred,
                                 target, cat, t, lr, scale, loss, last_input, n_ori, want_info, want)

    def cluster_attack(self, pc, target, clusters, num_add, cl_num_p, noise=None, loss="logits", kappa=0., scale=1., attack_lr=1e-2,
                       init_weight=5., max_weight=30., binary_step=5, num_iter=500, n_points=None, out_stride=None,
                       want_bounds: bool = False):
        """The whole CW cluster-adding attack on the device (ifd_cluster_attack) from the start ``clusters`` [B,A,3], A = num_add *
        cl_num_p: -> (clouds [B,out_stride,3]: each cloud's originals bit for bit, then its A added points; best_dist [B] (1e10 where
        no iteration reached the target); success [B] bool) and with want_bounds also {"weight", "lower", "upper"} [B] float64.
        noise: [binary_step,B,A,3], the start noise of every search step, or None.  out_stride: rows of the output, default N + A."""
        num_add, cl_num_p, A = self._group_rows(num_add, cl_num_p, "cl_num_p")
        loss_kind, pc, n_points, B, stride, target = self._adding_inputs(loss, pc, n_points, target)
        clusters = self._shaped(torch.as_tensor(clusters), (B, A, 3), "clusters must be [B,num_add*cl_num_p,3]")
        noise = self._shaped(noise, (int(binary_step), B, A, 3), "noise must be [binary_step,B,num_add*cl_num_p,3]")
        P = _lib.IfdClusterParams(C.sizeof(_lib.IfdClusterParams), loss_kind, int(binary_step), int(num_iter), num_add, cl_num_p,
                                  float(kappa), float(scale), float(attack_lr), float(init_weight), float(max_weight))
        return self._adding_attack(self.lib.ifd_cluster_attack, P, pc, n_points, target, [clusters, noise], A, out_stride, want_bounds)

    # ---- include/ifd_object.h: the CW object-adding attack (models without feature_transform) ----
    OBJECT_POSE = (("shift", 3), ("angle", 1), ("shift_m", 3), ("shift_v", 3), ("angle_m", 1), ("angle_v", 1))

    def _object_template(self, objects, num_add, obj_num_p):
        objects = _f32(torch.as_tensor(objects), self.device)
        if tuple(objects.shape) != (num_add, obj_num_p, 3):
            raise IfdError("objects must be [num_add,obj_num_p,3]")
        return objects

    def object_state(self, B, num_add, obj_num_p, init_weight=5., max_weight=40.):
        """The state of a fresh attack (ifd_object_state) as a dict of device tensors: ``cw_state(B, A, ...)`` - "m" and "v" belong to
        the object rows, "o_bestattack" holds world rows - and "obj" [B,A,3], "shift" [B,num_add,3], "angle" [B,num_add] with the pose
        moments "shift_m", "shift_v", "angle_m", "angle_v", all zero.  ``cw_adjust`` works on it as it is; the pose moments are the
        caller's to zero at the start of a search step."""
        num_add, obj_num_p, A = self._group_rows(num_add, obj_num_p, "obj_num_p")
        state = self.cw_state(B, A, init_weight, max_weight)
        state["obj"] = torch.zeros(B, A, 3, device=self.device, dtype=torch.float32)
        for key, width in self.OBJECT_POSE:
            state[key] = torch.zeros((B, num_add, 3) if width == 3 else (B, num_add), device=self.device, dtype=torch.float32)
        return state

    def _object_struct(self, state, B, num_add, A):
        ptrs = [self._cw_cloud(state.get("obj"), B, A, "object state 'obj'")]
        if ptrs[0] is None:
            raise IfdError("object state 'obj' is missing")
        for key, width in self.OBJECT_POSE:
            t = state.get(key)
            want = (B, num_add, 3) if width == 3 else (B, num_add)
            if t is None or not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == want):
                raise IfdError("object state %r must be a contiguous float32 device tensor of shape %s" % (key, want))
            ptrs.append(t.data_ptr())
        return _lib.IfdObjectState(self._cw_struct(state, B, A), *ptrs)

    def object_place(self, obj, angle, shift, cat, num_add, obj_num_p, n_ori=None):
        """world = rotate_shift(obj, angle, shift) (ifd_object_place) IN PLACE into the added rows of ``cat`` [B,N,3]: obj [B,A,3],
        angle [B,num_add] about the y axis, shift [B,num_add,3]; cloud b has n_ori[b] originals (None: N - A) in front of its A =
        num_add * obj_num_p added rows.  Returns ``cat``."""
        num_add, obj_num_p, A = self._group_rows(num_add, obj_num_p, "obj_num_p")
        B, stride = self._cat_dims(cat)
        self._cw_cloud(cat, B, stride, "cat")
        obj = _f32(torch.as_tensor(obj), self.device)
        angle = _f32(torch.as_tensor(angle), self.device)
        shift = _f32(torch.as_tensor(shift), self.device)
        if tuple(obj.shape) != (B, A, 3) or tuple(angle.shape) != (B, num_add) or tuple(shift.shape) != (B, num_add, 3):
            raise IfdError("obj must be [B,num_add*obj_num_p,3], angle [B,num_add] and shift [B,num_add,3]")
        n_ori = self._counts(n_ori, B)
        with torch.cuda.device(self.device):
            self._check(self.lib.ifd_object_place(self.ctx, obj.data_ptr(), angle.data_ptr(), shift.data_ptr(), cat.data_ptr(),
                                                  None if n_ori is None else n_ori.data_ptr(), B, stride, num_add, obj_num_p,
                                                  self._stream()))
        return cat

    def object_step(self, state, objects, grad, pred, target, cat, num_add, obj_num_p, t, lr, scale=1., loss=None, last_input=None,
                    n_ori=None, want_info: bool = False, want=()):
        """One iteration of the object-adding attack behind ``input_grad`` on the concatenated clouds (ifd_object_step), IN PLACE on
        ``state`` (``object_state``) and on the added rows of ``cat`` [B,N,3], which must hold the placement of the state when called
        and hold the placement of the new state afterwards.  objects [num_add,obj_num_p,3]: the template shared by the batch.  grad,
        pred, loss, last_input [B,A,3]: as ``add_step`` takes them.  Returns a dict: with want_info "info" [B,3] (adversarial loss,
        dist * weight, dist), and the diagnostics named in ``want``: "obj_grad" [B,A,3], "nn_ori" [B,A] int32, "g_shift" [B,num_add,3],
        "g_angle" [B,num_add], "l2" [B], "cd" [B] (clouds outside the limits are left as allocated: NaN / -1)."""
        num_add, obj_num_p, A = self._group_rows(num_add, obj_num_p, "obj_num_p")
        B, _ = self._cat_dims(cat)
        st = self._object_struct(state, B, num_add, A)
        objects = self._object_template(objects, num_add, obj_num_p)
        shapes = {"obj_grad": ((B, A, 3), torch.float32), "nn_ori": ((B, A), torch.int32), "g_shift": ((B, num_add, 3), torch.float32),
                  "g_angle": ((B, num_add), torch.float32), "l2": ((B,), torch.float32), "cd": ((B,), torch.float32)}
        return self._adding_step(self.lib.ifd_object_step, [C.byref(st), objects.data_ptr()], [num_add, obj_num_p], A, shapes,
                                 _lib.IfdObjectDiag, grad, pred, target, cat, t, lr, scale, loss, last_input, n_ori, want_info, want)

    def object_attack(self, pc, target, objects, centers, angles0, noise_obj=None, noise_shift=None, loss="logits", kappa=0., scale=1.,
                      attack_lr=1e-2, init_weight=5., max_weight=40., binary_step=5, num_iter=500, n_points=None, out_stride=None,
                      want_bounds: bool = False):
        """The whole CW object-adding attack on the device (ifd_object_attack): objects [num_add,obj_num_p,3] the template, centers
        [B,num_add,3] the start shifts, angles0 [binary_step,B,num_add] the start angles of every search step, noise_obj
        [binary_step,B,A,3] and noise_shift [binary_step,B,num_add,3] the start noise or None.  -> (clouds [B,out_stride,3]: each
        cloud's originals bit for bit, then its A = num_add * obj_num_p added points; best_dist [B] (1e10 where no iteration reached
        the target); success [B] bool) and with want_bounds also {"weight", "lower", "upper"} [B] float64.  out_stride: rows of the
        output, default N + A."""
        objects = _f32(torch.as_tensor(objects), self.device)
        if objects.dim() != 3 or int(objects.shape[2]) != 3:
            raise IfdError("objects must be [num_add,obj_num_p,3]")
        num_add, obj_num_p, A = self._group_rows(objects.shape[0], objects.shape[1], "obj_num_p")
        loss_kind, pc, n_points, B, stride, target = self._adding_inputs(loss, pc, n_points, target)
        steps = int(binary_step)
        arr = lambda x, shape, what: self._shaped(x, shape, "%s must be %s" % (what, list(shape)))       # noqa: E731
        centers = arr(centers, (B, num_add, 3), "centers")
        angles0 = arr(angles0, (steps, B, num_add), "angles0")
        if centers is None or angles0 is None:
            raise IfdError("centers and angles0 are needed")
        noise_obj = arr(noise_obj, (steps, B, A, 3), "noise_obj")
        noise_shift = arr(noise_shift, (steps, B, num_add, 3), "noise_shift")
        P = _lib.IfdObjectParams(C.sizeof(_lib.IfdObjectParams), loss_kind, steps, int(num_iter), num_add, obj_num_p, float(kappa),
                                 float(scale), float(attack_lr), float(init_weight), float(max_weight))
        return self._adding_attack(self.lib.ifd_object_attack, P, pc, n_points, target, [objects, centers, noise_obj, noise_shift, angles0],
                                   A, out_stride, want_bounds)

    # ---- include/ifd_drop.h: the saliency Drop attack (models without feature_transform) ----
    def drop_step(self, grad, pc, n_points, k, alpha=1., index=None, want=()):
        """One round of the Drop attack behind ``input_grad`` (ifd_drop_step), IN PLACE on ``pc`` [B,N,3] float32, ``n_points`` [B]
        int32 and ``index`` [B,N] int32 (or None), contiguous device tensors: every cloud with k < n <= 2048 loses its k rows of
        highest saliency (the lowest row first among equal saliencies), the survivors move up in their order, the rows it lost
        become zeros (-1 in ``index``) and its count n - k; any other cloud is left untouched.  grad [B,N,3] as ``input_grad``
        returned it.  Returns the diagnostics named in ``want``: "saliency" [B,N] (the first n rows, before the drop), "center" [B,3],
        "dropped" [B,k] int32 in drop order (NaN / -1 where the library writes nothing)."""
        if not torch.is_tensor(pc) or pc.dim() != 3:
            raise IfdError("pc must be a contiguous float32 [B,N,3] device tensor")
        B, stride, k = int(pc.shape[0]), int(pc.shape[1]), int(k)
        if grad is None:
            raise IfdError("grad is missing")
        ptrs = [self._cw_cloud(x, B, stride, n) for x, n in ((grad, "grad"), (pc, "pc"))]
        for t, shape, name in ((n_points, (B,), "n_points"), (index, (B, stride), "index")):
            if t is None and name == "index":
                continue
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape):
                raise IfdError("%s must be a contiguous int32 %s device tensor (updated in place)" % (name, list(shape)))
        shapes = {"saliency": ((B, stride), torch.float32), "center": ((B, 3), torch.float32), "dropped": ((B, max(k, 1)), torch.int32)}
        out = self._diag(want, shapes, "saliency | center | dropped")
        ptr = lambda x: None if x is None else x.data_ptr()        # noqa: E731
        diag = _lib.IfdDropOut(*[ptr(out.get(n)) for n in ("saliency", "center", "dropped")])
        with torch.cuda.device(self.device):
            self._check(self._fn("drop_step")(self.ctx, ptrs[0], ptrs[1], n_points.data_ptr(), ptr(index), B, stride, k, float(alpha),
                                               C.byref(diag) if out else None, self._stream()))
        return out

    def drop_attack(self, pc, label, num_drop, k=5, alpha=1., scale=1., n_points=None, want_kept: bool = False, fps_start=None):
        """The whole Drop attack on the device (ifd_drop_attack): ceil(num_drop / k) rounds of the gradient of scale *
        cross_entropy(logits, label) and ``drop_step``, then a forward.  -> (clouds [B,N - num_drop,3], correct [B] bool: the
        clouds the victim STILL classifies as ``label``) and with want_kept also kept [B,N - num_drop] int32, the surviving rows'
        indices into ``pc``.  With n_points, cloud b is the first n_points[b] - num_drop rows of its output (zeros behind them)."""
        pc, n_points = self._batch(pc, n_points)
        B, stride, num_drop = int(pc.shape[0]), int(pc.shape[1]), int(num_drop)
        if B < 1 or stride < 1:
            raise IfdError("empty batch")
        label = self._target(label, B)
        starts = self._loop_starts(fps_start, B)
        out = torch.empty_like(pc)
        n_out = torch.empty(B, device=self.device, dtype=torch.int32)
        correct = torch.empty(B, device=self.device, dtype=torch.int32)
        kept = torch.empty(B, stride, device=self.device, dtype=torch.int32) if want_kept else None
        P = _lib.IfdDropParams(C.sizeof(_lib.IfdDropParams), num_drop, int(k), float(alpha), float(scale))
        with torch.cuda.device(self.device):
            self._check(self._fn("drop_attack")(self.ctx, C.byref(P), pc.data_ptr(), None if n_points is None else n_points.data_ptr(),
                                                *[None if t is None else t.data_ptr() for t in starts], label.data_ptr(), B, stride,
                                                out.data_ptr(), n_out.data_ptr(), None if kept is None else kept.data_ptr(),
                                                correct.data_ptr(), self._stream()))
        m = max(stride - num_drop, 0)
        if want_kept:
            return out[:, :m].contiguous(), correct.bool(), kept[:, :m].contiguous()
        return out[:, :m].contiguous(), correct.bool()


class DgcnnClassifier(Classifier):
    """The DGCNN victim of the reference on one GPU (include/ifd_dgcnn.h): DGCNN(emb_dims=1024, k, output_channels=40) in eval
    mode.  ``weights``: the BN-folded canonical vector (``weights.load_checkpoint(path, "dgcnn")`` or
    ``weights.pack_state_dict(state_dict, "dgcnn")``).  Inputs are Classifier's: [B,N,3] batches (point-major), lists and
    object arrays of ragged clouds; every cloud needs at least k points and at most 2048.  A cloud's outputs do not depend on
    how it is batched or padded.

    Of the attack entry points, ``input_grad``, ``fgm_update`` and ``fgm_attack`` run on this victim (include/ifd_dgcnn_atk.h),
    with Classifier's signatures and return shapes, so attack.FGM / IFGM / MIFGM / PGD work on it unchanged; the gradient is
    the one of the network with its neighbour tables held fixed.  ``cw_state``, ``cw_step``, ``cw_adjust``, ``cw_perturb_attack``,
    ``knn_step``, ``knn_project_clip``, ``knn_attack``, ``drop_step`` and ``drop_attack`` run on it too (include/ifd_victim_atk.h),
    so attack.CWPerturb / CWKNN / SaliencyDrop work on it unchanged.  The point-adding attacks (add_*, cluster_*, object_*) are
    PointNet's, and the library refuses them on a DGCNN context."""

    MAX_POINTS = _lib.DGCNN_MAX_POINTS
    ATK_FNS = {"input_grad": "ifd_dgcnn_input_grad", "fgm_update": "ifd_dgcnn_fgm_update", "fgm_attack": "ifd_dgcnn_fgm_attack"}
    LOOP_FNS = Classifier.VICTIM_LOOP_FNS
    EDGE_WIDTHS = (64, 64, 128, 256)

    def __init__(self, weights: np.ndarray, k: int = 20, device=None):
        self.lib = _lib.load()
        self.feature_transform = False
        self.k = int(k)
        if not 1 <= self.k <= _lib.DGCNN_MAX_K:
            raise IfdError("k must lie in [1, %d], got %d" % (_lib.DGCNN_MAX_K, self.k))
        self._create("ifd_dgcnn_create", self.lib.ifd_dgcnn_weight_count(), "dgcnn weights", weights, device, self.k)

    def logits(self, pc, n_points=None, want_aux: bool = False, want_pred: bool = False):
        """pc, n_points: as Classifier.logits.  Returns logits [B,40]; with want_aux also {"idx": four [B,N,k] int32 (the
        neighbours each edge convolution chose; rows beyond a cloud's count are -1), "feat" [B,N,512] (x1|x2|x3|x4; zero
        beyond a cloud's count), "global_feat" [B,2048] (max | mean of conv5), "pred" [B] int32}."""
        def aux_table(B, stride):
            return {"idx": [torch.full((B, stride, self.k), -1, device=self.device, dtype=torch.int32) for _ in range(4)],
                    "feat": torch.zeros(B, stride, 512, device=self.device, dtype=torch.float32),
                    "global_feat": torch.empty(B, 2048, device=self.device, dtype=torch.float32)}
        return self._forward("ifd_dgcnn_forward", pc, n_points, _lib.IfdDgcnnAux, aux_table, want_aux, want_pred)

    GRAD_OUT = _lib.IfdDgcnnGradOut

    def _loop_starts(self, fps_start, B):
        return super()._loop_starts(fps_start, B) + [None]             # the ifd_victim_* loops take a (NULL) fps_start

    def _grad_spec(self, B, stride):
        """input_grad's diagnostics on this victim: {"logits" [B,40], "loss" [B], "pred" [B], "idx": four [B,N,k] int32, "feat"
        [B,N,512], "global_feat" [B,2048], "win_pool" [B,1024] int32 (the point of each conv5 max-pool channel), "win_edge": four
        [B,N,Cout] int32 (the neighbour holding each channel's maximum), "act5" [B,N,32] int32 (bit c % 32 of word c // 32: conv5's
        pre-activation of channel c is > 0)}.  Rows beyond a cloud's count: -1 in idx and win_edge, zero in feat and act5."""
        f, i = torch.float32, torch.int32
        return {"logits": ((B, self.N_CLASSES), f, None), "loss": ((B,), f, None), "pred": ((B,), i, None),
                "idx": [((B, stride, self.k), i, -1) for _ in range(4)],
                "feat": ((B, stride, 512), f, 0.), "global_feat": ((B, 2048), f, None), "win_pool": ((B, 1024), i, None),
                "win_edge": [((B, stride, c), i, -1) for c in self.EDGE_WIDTHS], "act5": ((B, stride, 32), i, 0)}


class _SampledVictim(Classifier):
    """What the two victims that sample share (PointNet++, PointConv): how ``fps_start`` reaches the library."""

    def _starts(self, fps_start):
        """-> extra(B) of _forward / _input_grad / _fgm_attack: fps_start as [B,2] int32 on the device, or None."""
        def starts(B):
            if fps_start is None:
                return (None,)
            t = torch.as_tensor(fps_start).to(device=self.device, dtype=torch.int32).contiguous()
            if tuple(t.shape) != (B, 2):
                raise IfdError("fps_start must be [B,2], got %s" % (tuple(t.shape),))
            return (t,)
        return starts

    def _loop_starts(self, fps_start, B):
        return list(self._starts(fps_start)(B))


class PointNet2Classifier(_SampledVictim):
    """The PointNet++ victim of the reference on one GPU (include/ifd_pn2.h): PointNet2ClsSsg(num_classes=40) in eval mode.
    ``weights``: the BN-folded canonical vector (``weights.load_checkpoint(path, "pointnet2")`` or
    ``weights.pack_state_dict(state_dict, "pointnet2")``).  Inputs are Classifier's: [B,N,3] batches (point-major), lists and
    object arrays of ragged clouds of 1 to 2048 points.  ``fps_start`` [B,2] int: the first pick of the level-1 sampling (below
    the cloud's count) and of the level-2 sampling (below 512); None means 0, 0 - the reference draws them at random, here
    they are an input.  A cloud's outputs do not depend on how it is batched or padded.

    Of the attack entry points, ``input_grad``, ``fgm_update`` and ``fgm_attack`` run on this victim (include/ifd_pn2_atk.h),
    with Classifier's signatures and return shapes plus ``fps_start=None``, so attack.FGM / IFGM / MIFGM / PGD work on it
    unchanged; the gradient is the one of the network with its four index tables held fixed, the tables being the forward's on
    the current cloud.  ``cw_state``, ``cw_step``, ``cw_adjust``, ``cw_perturb_attack``, ``knn_step``, ``knn_project_clip``,
    ``knn_attack``, ``drop_step`` and ``drop_attack`` run on it too (include/ifd_victim_atk.h); the three whole loops take
    ``fps_start=None`` and use the same starts in every gradient and in the closing forward - for ``drop_attack`` they must be valid
    for the clouds that are written, fps_start[b][0] < n_points[b] - num_drop.  The point-adding attacks (add_*, cluster_*,
    object_*) are PointNet's, and the library refuses them on a PointNet++ context."""

    MAX_POINTS = _lib.PN2_MAX_POINTS
    ATK_FNS = {"input_grad": "ifd_pn2_input_grad", "fgm_update": "ifd_pn2_fgm_update", "fgm_attack": "ifd_pn2_fgm_attack"}
    LOOP_FNS = Classifier.VICTIM_LOOP_FNS

    def __init__(self, weights: np.ndarray, device=None):
        self.lib = _lib.load()
        self.feature_transform = False
        self._create("ifd_pn2_create", self.lib.ifd_pn2_weight_count(), "pointnet2 weights", weights, device)

    GRAD_OUT = _lib.IfdPn2GradOut

    def _grad_spec(self, B, stride):
        """input_grad's diagnostics on this victim: {"logits" [B,40], "loss" [B], "pred" [B], the tables and features of
        ``logits``' aux, "win1" [B,512,128], "win2" [B,128,256], "win3" [B,1024] int32 (the sample position, resp. row, holding each
        group maximum), "act1" [B,512,32,4], "act2" [B,128,64,8], "act3" [B,128,24] int32 (gate bits of the hidden layers: bit c % 32
        of a layer's word c // 32 is set where its pre-activation of channel c is > 0)}."""
        n1, s1, n2, s2 = _lib.PN2_NPOINT1, _lib.PN2_NSAMPLE1, _lib.PN2_NPOINT2, _lib.PN2_NSAMPLE2
        f, i = torch.float32, torch.int32
        shapes = dict(logits=((B, self.N_CLASSES), f), loss=((B,), f), pred=((B,), i), fps1=((B, n1), i), fps2=((B, n2), i),
                      ball1=((B, n1, s1), i), ball2=((B, n2, s2), i), l1_feat=((B, n1, 128), f), l2_feat=((B, n2, 256), f),
                      global_feat=((B, 1024), f), win1=((B, n1, 128), i), win2=((B, n2, 256), i), win3=((B, 1024), i),
                      act1=((B, n1, s1, 4), i), act2=((B, n2, s2, 8), i), act3=((B, n2, 24), i))
        return {n: (shape, dt, None) for n, (shape, dt) in shapes.items()}

    def input_grad(self, pc, target, loss="logits", kappa=0., scale=1., n_points=None, want_aux: bool = False, fps_start=None):
        """Classifier.input_grad on this victim (ifd_pn2_input_grad); fps_start as ``logits`` takes it; want_aux: see _grad_aux."""
        return self._input_grad(pc, target, loss, kappa, scale, n_points, want_aux, extra=self._starts(fps_start))

    def fgm_attack(self, kind, pc, target, budget, step_size, num_iter=1, mu=1., loss="logits", kappa=0., scale=1., n_points=None,
                   fps_start=None):
        """Classifier.fgm_attack on this victim (ifd_pn2_fgm_attack): the same fps_start in every iteration and in the last forward."""
        return self._fgm_attack(kind, pc, target, budget, step_size, num_iter, mu, loss, kappa, scale, n_points,
                                extra=self._starts(fps_start))

    def fgm_update(self, kind, grad, pc, ori_pc=None, momentum=None, step_size=0., budget=0., mu=1., n_points=None, fps_start=None):
        """Classifier.fgm_update on this victim (ifd_pn2_fgm_update); the update does not sample, fps_start is accepted and unused."""
        return super().fgm_update(kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points)

    def logits(self, pc, n_points=None, fps_start=None, want_aux: bool = False, want_pred: bool = False):
        """pc, n_points: as Classifier.logits.  Returns logits [B,40]; with want_aux also {"fps1" [B,512], "fps2" [B,128],
        "ball1" [B,512,32], "ball2" [B,128,64] (int32), "l1_feat" [B,512,128], "l2_feat" [B,128,256], "global_feat" [B,1024],
        "pred" [B] int32}."""
        starts = self._starts(fps_start)

        def aux_table(B, stride):
            n1, s1, n2, s2 = _lib.PN2_NPOINT1, _lib.PN2_NSAMPLE1, _lib.PN2_NPOINT2, _lib.PN2_NSAMPLE2
            i32, f32 = dict(device=self.device, dtype=torch.int32), dict(device=self.device, dtype=torch.float32)
            return dict(fps1=torch.empty(B, n1, **i32), fps2=torch.empty(B, n2, **i32), ball1=torch.empty(B, n1, s1, **i32),
                        ball2=torch.empty(B, n2, s2, **i32), l1_feat=torch.empty(B, n1, 128, **f32),
                        l2_feat=torch.empty(B, n2, 256, **f32), global_feat=torch.empty(B, 1024, **f32))
        return self._forward("ifd_pn2_forward", pc, n_points, _lib.IfdPn2Aux, aux_table, want_aux, want_pred, extra=starts)

    def predict(self, pc, n_points=None, fps_start=None) -> torch.Tensor:
        """argmax of the logits, [B] int64 (the lowest class among equal logits)."""
        _, aux = self.logits(pc, n_points, fps_start=fps_start, want_pred=True)
        return aux["pred"].long()


class PointConvClassifier(_SampledVictim):
    """The PointConv victim of the reference on one GPU (include/ifd_pc.h): PointConvDensityClsSsg(num_classes=40) in eval mode.
    ``weights``: the BN-folded canonical vector (``weights.load_checkpoint(path, "pointconv")`` or
    ``weights.pack_state_dict(state_dict, "pointconv")``).  Inputs are Classifier's: [B,N,3] batches (point-major), lists and
    object arrays of ragged clouds of 32 to 2048 points.  ``fps_start`` [B,2] int: the first pick of the level-1 sampling (below
    the cloud's count) and of the level-2 sampling (below 512); None means 0, 0 - the reference draws them at random, here
    they are an input.  A cloud's outputs do not depend on how it is batched or padded.

    Of the attack entry points, ``input_grad``, ``fgm_update`` and ``fgm_attack`` run on this victim (include/ifd_pc_atk.h),
    with Classifier's signatures and return shapes plus ``fps_start=None``, so attack.FGM / IFGM / MIFGM / PGD work on it
    unchanged; the gradient is the one of the network with its four index tables held fixed, the tables being the forward's on
    the current cloud.  ``cw_state``, ``cw_step``, ``cw_adjust``, ``cw_perturb_attack``, ``knn_step``, ``knn_project_clip``,
    ``knn_attack``, ``drop_step`` and ``drop_attack`` run on it too (include/ifd_victim_atk.h); the three whole loops take
    ``fps_start=None`` and use the same starts in every gradient and in the closing forward - for ``drop_attack`` they must be valid
    for the clouds that are written, fps_start[b][0] < n_points[b] - num_drop.  The point-adding attacks (add_*, cluster_*,
    object_*) are PointNet's, and the library refuses them on a PointConv context."""

    MAX_POINTS = _lib.PC_MAX_POINTS
    MIN_POINTS = _lib.PC_MIN_POINTS
    CHUNK = _lib.PC_CHUNK
    ATK_FNS = {"input_grad": "ifd_pc_input_grad", "fgm_update": "ifd_pc_fgm_update", "fgm_attack": "ifd_pc_fgm_attack"}
    LOOP_FNS = Classifier.VICTIM_LOOP_FNS

    def __init__(self, weights: np.ndarray, device=None):
        self.lib = _lib.load()
        self.feature_transform = False
        self._create("ifd_pc_create", self.lib.ifd_pc_weight_count(), "pointconv weights", weights, device)

    GRAD_OUT = _lib.IfdPcGradOut

    def _aux_spec(self, B, stride):
        n1, k1, n2, k2 = _lib.PC_NPOINT1, _lib.PC_K1, _lib.PC_NPOINT2, _lib.PC_K2
        f, i = torch.float32, torch.int32
        return dict(fps1=((B, n1), i, None), fps2=((B, n2), i, None), knn1=((B, n1, k1), i, None), knn2=((B, n2, k2), i, None),
                    dens1=((B, stride), f, 0.), dens2=((B, n1), f, None), dens3=((B, n2), f, None), l1_feat=((B, n1, 128), f, None),
                    l2_feat=((B, n2, 256), f, None), global_feat=((B, 1024), f, None))

    def _aux_table(self, B, stride):
        return {n: self._make(e) for n, e in self._aux_spec(B, stride).items()}

    def _grad_spec(self, B, stride):
        """input_grad's diagnostics on this victim: {"logits" [B,40], "loss" [B], "pred" [B], the tables, densities and features of
        ``logits``' aux, and the gate bits of the backward pass as int32 words (include/ifd_pc_atk.h): "dgate1" [B,N] (zero beyond a
        cloud's count), "dgate2" [B,512], "dgate3" [B,128] (DensityNet), "wgate1" [B,512,32], "wgate2" [B,128,64], "wgate3" [B,128]
        (WeightNet), "mgate1" [B,512,32,8], "mgate2" [B,128,64,16], "mgate3" [B,128,56] (the MLPs)}."""
        n1, k1, n2, k2 = _lib.PC_NPOINT1, _lib.PC_K1, _lib.PC_NPOINT2, _lib.PC_K2
        f, i = torch.float32, torch.int32
        return dict(logits=((B, self.N_CLASSES), f, None), loss=((B,), f, None), pred=((B,), i, None), **self._aux_spec(B, stride),
                    dgate1=((B, stride), i, 0), dgate2=((B, n1), i, None), dgate3=((B, n2), i, None),
                    wgate1=((B, n1, k1), i, None), wgate2=((B, n2, k2), i, None), wgate3=((B, n2), i, None),
                    mgate1=((B, n1, k1, 8), i, None), mgate2=((B, n2, k2, 16), i, None), mgate3=((B, n2, 56), i, None))

    def input_grad(self, pc, target, loss="logits", kappa=0., scale=1., n_points=None, want_aux: bool = False, fps_start=None):
        """Classifier.input_grad on this victim (ifd_pc_input_grad); fps_start as ``logits`` takes it; want_aux: see _grad_aux."""
        return self._input_grad(pc, target, loss, kappa, scale, n_points, want_aux, extra=self._starts(fps_start))

    def fgm_attack(self, kind, pc, target, budget, step_size, num_iter=1, mu=1., loss="logits", kappa=0., scale=1., n_points=None,
                   fps_start=None):
        """Classifier.fgm_attack on this victim (ifd_pc_fgm_attack): the same fps_start in every iteration and in the last forward."""
        return self._fgm_attack(kind, pc, target, budget, step_size, num_iter, mu, loss, kappa, scale, n_points,
                                extra=self._starts(fps_start))

    def fgm_update(self, kind, grad, pc, ori_pc=None, momentum=None, step_size=0., budget=0., mu=1., n_points=None, fps_start=None):
        """Classifier.fgm_update on this victim (ifd_pc_fgm_update); the update does not sample, fps_start is accepted and unused."""
        return super().fgm_update(kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points)

    def logits(self, pc, n_points=None, fps_start=None, want_aux: bool = False, want_pred: bool = False):
        """pc, n_points: as Classifier.logits.  Returns logits [B,40]; with want_aux also {"fps1" [B,512], "fps2" [B,128],
        "knn1" [B,512,32], "knn2" [B,128,64] (int32), "dens1" [B,N] (zero beyond a cloud's count), "dens2" [B,512], "dens3"
        [B,128] (DensityNet's outputs), "l1_feat" [B,512,128], "l2_feat" [B,128,256], "global_feat" [B,1024], "pred" [B] int32}."""
        return self._forward("ifd_pc_forward", pc, n_points, _lib.IfdPcAux, self._aux_table, want_aux, want_pred,
                             extra=self._starts(fps_start))

    def predict(self, pc, n_points=None, fps_start=None) -> torch.Tensor:
        """argmax of the logits, [B] int64 (the lowest class among equal logits)."""
        _, aux = self.logits(pc, n_points, fps_start=fps_start, want_pred=True)
        return aux["pred"].long()
