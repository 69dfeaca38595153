"""The FGM family of the reference's attacks (baselines/attack/FGM/FGM.py: FGM, IFGM, MIFGM, PGD) on the PointNet victim - the
loop runs on the device (include/ifd_atk.h ifd_fgm_attack).

The classes take the reference's constructor arguments, except that ``model`` is a ``runtime.Classifier`` (anything with its
``fgm_attack`` and ``predict``), ``adv_func`` is the loss by name - "logits" (LogitsAdvLoss(kappa)) or "cross_entropy" - and the
clip is ClipPointsL2(budget), the only one the reference's script uses.  ``attack(data [B,K,3], target [B])`` returns the
reference's pair (adversarial clouds [B,K,3] as a numpy array, success_num) and prints its progress lines.  With the
per-iteration lines (``verbose=True``, the default) the loop is driven from the host, one gradient and one update call an
iteration; ``verbose=False`` prints the last line only and runs the whole loop in one library call.  Both give the same bits.

Start noise: IFGM / MIFGM add randn * 1e-7, PGD adds uniform(-eps, eps), eps = budget / sqrt(3 K), and the perturbed cloud is the
centre of the clip (FGM.py:131-134, 275-281).  The noise is drawn here from a seeded HOST torch.Generator, PGD's first: the
reference draws on the GPU from the global CUDA stream, which cannot be reproduced, so clouds agree with a reference run in
distribution only, not number for number.

The reference's loss is a mean over the batch it was called with; pass that batch size as ``ref_batch`` (scale = 1 / ref_batch) to
reproduce how its ``+ 1e-9`` terms weigh against the gradient's norm.  The default is the batch passed to ``attack``.
"""
from __future__ import annotations

import numpy as np
import torch


class FGM:
    KIND = "fgm"

    def __init__(self, model, adv_func="logits", budget=0.08, dist_metric="l2", kappa=0., seed=1, ref_batch=None, verbose=True):
        if dist_metric.lower() != "l2":
            raise ValueError("only the l2 constraint of the reference's script is built")
        self.model, self.adv_func, self.kappa = model, adv_func, float(kappa)
        self.budget, self.step_size, self.num_iter, self.mu = float(budget), float(budget), 1, 1.0
        self.ref_batch, self.verbose = ref_batch, verbose
        self.generator = torch.Generator().manual_seed(int(seed))

    def start(self, data: torch.Tensor) -> torch.Tensor:
        """The cloud the loop starts from and clips against (plain FGM: the data themselves)."""
        return data

    def _scale(self, B):
        return 1.0 / float(self.ref_batch or B)

    def _loop(self, pc, target):
        """The reference's loop from the host, one ifd_cls_input_grad and one ifd_fgm_update an iteration: the same kernels as
        ifd_fgm_attack on the same numbers, with the prediction of every iteration at hand for the progress lines."""
        B = int(pc.shape[0])
        dev = self.model.device
        ori = pc.to(dev).contiguous()
        cur = ori.clone()
        tgt = target.to(dev)
        mom = torch.zeros_like(cur) if self.KIND == "mifgm" else None
        for it in range(self.num_iter):
            grad, aux = self.model.input_grad(cur, tgt, self.adv_func, self.kappa, self._scale(B), want_aux=True)
            if it % max(self.num_iter // 5, 1) == 0:
                print('iter {}/{}, success: {}/{}'.format(it, self.num_iter, int((aux["pred"].long() == tgt).sum()), B))
            self.model.fgm_update(self.KIND, grad, cur, ori, mom, self.step_size, self.budget, self.mu)
        return cur, self.model.predict(cur).to(tgt.device) == tgt

    def attack(self, data, target):
        data = torch.as_tensor(np.asarray(data) if not torch.is_tensor(data) else data).float().cpu()
        target = torch.as_tensor(np.asarray(target) if not torch.is_tensor(target) else target).long().cpu()
        B = int(data.shape[0])
        pc = self.start(data)
        if self.KIND != "fgm" and self.verbose:
            adv, ok = self._loop(pc, target)
        else:
            adv, ok = self.model.fgm_attack(self.KIND, pc, target, self.budget, self.step_size, self.num_iter, self.mu, self.adv_func,
                                            self.kappa, self._scale(B))
        success_num = int(ok.sum())
        if self.KIND == "fgm":
            print('Successfully attack {}/{}'.format(success_num, B))
        else:
            print('Final success: {}/{}'.format(success_num, B))
        return adv.cpu().numpy(), success_num


class IFGM(FGM):
    KIND = "ifgm"

    def __init__(self, model, adv_func="logits", clip_func=None, budget=0.08, step_size=None, num_iter=50, dist_metric="l2", **kw):
        super().__init__(model, adv_func, budget, dist_metric, **kw)
        self.num_iter = int(num_iter)
        self.step_size = float(budget) / self.num_iter if step_size is None else float(step_size)

    def start(self, data):
        return data + torch.randn(data.shape, generator=self.generator) * 1e-7


class MIFGM(IFGM):
    KIND = "mifgm"

    def __init__(self, model, adv_func="logits", clip_func=None, budget=0.08, step_size=None, num_iter=50, mu=1., dist_metric="l2", **kw):
        super().__init__(model, adv_func, clip_func, budget, step_size, num_iter, dist_metric, **kw)
        self.mu = float(mu)


class PGD(IFGM):
    KIND = "pgd"

    def start(self, data):
        eps = self.budget / ((data.shape[1] * data.shape[2]) ** 0.5)
        init = data + (torch.rand(data.shape, generator=self.generator) * 2 - 1) * eps
        return super().start(init)


ATTACKS = {"fgm": FGM, "ifgm": IFGM, "mifgm": MIFGM, "pgd": PGD}
