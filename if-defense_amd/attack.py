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

``CWPerturb`` is the reference's Carlini-Wagner point-perturbation attack (baselines/attack/CW/Perturb.py, include/ifd_cw.h), on the
same two loop forms; it is not one of ``ATTACKS``, which names the FGM family for the fgm_attack CLI.  ``CWKNN`` is the reference's
kNN attack (baselines/attack/CW/kNN.py, include/ifd_knn.h), likewise, and ``CWAdd`` its point-adding attack
(baselines/attack/CW/Add.py, include/ifd_add.h), whose clouds come back larger than they went in.  ``SaliencyDrop`` is the
reference's untargeted point-dropping attack (baselines/attack/Saliency/Drop.py, include/ifd_drop.h), whose clouds come back
smaller; it draws no noise.  ``CWAddClusters`` is the reference's cluster-adding attack (baselines/attack/CW/Add_Cluster.py,
include/ifd_cluster.h): ``num_add`` clusters of ``cl_num_p`` points, started on DBSCAN clusters of the 128 critical points.
``CWAddObjects`` is its object-adding attack (baselines/attack/CW/Add_Objects.py, include/ifd_object.h): ``num_add`` copies of an
object, each placed by a shift and a rotation about the y axis that are optimised with the object's points.

``CWPerturb``, ``CWKNN`` and ``SaliencyDrop`` also run on ``runtime.DgcnnClassifier`` and, through ``victim_atk_cli.BoundLoopStarts``,
on ``PointNet2Classifier`` and ``PointConvClassifier`` (include/ifd_victim_atk.h).  The host-driven loops ask ``input_grad`` for the
diagnostics they read only (``want_aux=("pred", "loss")``).
"""
from __future__ import annotations

import numpy as np
import torch


class _Attack:
    """What the attack classes share: the seeded host generator, the loss scale, the coercion of attack()'s arguments and the
    reference's progress and closing lines."""

    STEP_LINES = 'Step {}, iteration {}, success {}/{}\nadv_loss: {:.4f}, dist_loss: {:.4f}'

    def _common(self, seed, ref_batch, verbose):
        self.ref_batch, self.verbose = ref_batch, verbose
        self.generator = torch.Generator().manual_seed(int(seed))

    def _scale(self, B):
        return 1.0 / float(self.ref_batch or B)

    @staticmethod
    def _tensors(data, target):
        """(data, target) as CPU float / long tensors."""
        data = torch.as_tensor(np.asarray(data) if not torch.is_tensor(data) else data).float().cpu()
        target = torch.as_tensor(np.asarray(target) if not torch.is_tensor(target) else target).long().cpu()
        return data, target

    @staticmethod
    def _progress(fmt, a, b, pred, tgt, info, dist_col):
        """The reference's two lines: fmt filled with (a, b, hits, B, adv_loss, dist_loss), the two losses the batch means of
        info[:, 0] and info[:, dist_col] of the previous iteration, zero without one."""
        adv_loss, dist_loss = (0., 0.) if info is None else (float(info[:, 0].mean()), float(info[:, dist_col].mean()))
        print(fmt.format(a, b, int((pred.long() == tgt.long()).sum()), int(tgt.shape[0]), adv_loss, dist_loss))

    @staticmethod
    def _finish(ok, B, fmt='Successfully attack {}/{}'):
        success_num = int(ok.sum())
        print(fmt.format(success_num, B))
        return success_num

    def _search(self, tgt, state, last, want_aux, start, step):
        """The Carlini-Wagner search from the host, shared by CWPerturb and the adding attacks: ``binary_step`` search steps of
        ``num_iter`` iterations - one ``input_grad`` (with ``want_aux``) and one step call each, the reference's lines every
        num_iter // 5 iterations - and ``cw_adjust`` behind each.  start(search_step) -> the cloud the victim sees in that step;
        step(cloud, grad, aux, t, last_input, want_info) -> the step call's info or None, last_input being ``last`` in the very last
        iteration.  -> (o_bestattack, or ``last`` where the search never succeeded; o_bestdist; success)."""
        net = self.model
        B = int(tgt.shape[0])
        every = max(self.num_iter // 5, 1)
        for s in range(self.binary_step):
            cloud = start(s)
            info = None
            for it in range(self.num_iter):
                grad, aux = net.input_grad(cloud, tgt, self.adv_func, self.kappa, self._scale(B), want_aux=want_aux)
                if it % every == 0:
                    self._progress(self.STEP_LINES, s, it, aux["pred"], tgt, info, 1)
                final = s == self.binary_step - 1 and it == self.num_iter - 1
                info = step(cloud, grad, aux, it + 1, last if final else None, it % every == every - 1)
            net.cw_adjust(state, tgt)
        ok = state["lower"] > 0
        return torch.where(ok[:, None, None], state["o_bestattack"], last), state["o_bestdist"], ok


class FGM(_Attack):
    KIND = "fgm"

    def __init__(self, model, adv_func="logits", budget=0.08, dist_metric="l2", kappa=0., seed=1, ref_batch=None, verbose=True):
        if dist_metric.lower() != "l2":
            raise ValueError("only the l2 constraint of the reference's script is built")
        self.model, self.adv_func, self.kappa = model, adv_func, float(kappa)
        self.budget, self.step_size, self.num_iter, self.mu = float(budget), float(budget), 1, 1.0
        self._common(seed, ref_batch, verbose)

    def start(self, data: torch.Tensor) -> torch.Tensor:
        """The cloud the loop starts from and clips against (plain FGM: the data themselves)."""
        return data

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
            grad, aux = self.model.input_grad(cur, tgt, self.adv_func, self.kappa, self._scale(B), want_aux=("pred",))
            if it % max(self.num_iter // 5, 1) == 0:
                print('iter {}/{}, success: {}/{}'.format(it, self.num_iter, int((aux["pred"].long() == tgt).sum()), B))
            self.model.fgm_update(self.KIND, grad, cur, ori, mom, self.step_size, self.budget, self.mu)
        return cur, self.model.predict(cur).to(tgt.device) == tgt

    def attack(self, data, target):
        data, target = self._tensors(data, target)
        B = int(data.shape[0])
        pc = self.start(data)
        if self.KIND != "fgm" and self.verbose:
            adv, ok = self._loop(pc, target)
        else:
            adv, ok = self.model.fgm_attack(self.KIND, pc, target, self.budget, self.step_size, self.num_iter, self.mu, self.adv_func,
                                            self.kappa, self._scale(B))
        success_num = self._finish(ok, B) if self.KIND == "fgm" else self._finish(ok, B, 'Final success: {}/{}')
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


class CWPerturb(_Attack):
    """CW attack by perturbing points (Perturb.py CWPerturb): ``binary_step`` search steps on the weight of the L2 distance term,
    ``num_iter`` Adam iterations each.  ``model`` is a ``runtime.Classifier`` (anything with its ``input_grad``, ``cw_state``,
    ``cw_step``, ``cw_adjust`` and ``cw_perturb_attack``), ``adv_func`` the loss by name ("logits": LogitsAdvLoss(kappa), or
    "cross_entropy"), ``dist_func`` "l2" (L2Dist, the only one built).  ``attack(data [B,K,3], target [B])`` returns the reference's
    triple (o_bestdist [B], o_bestattack [B,K,3], success_num) as numpy arrays and prints its progress lines without the wall-clock
    ones.  ``verbose=True`` drives the loop from the host, one ``input_grad`` and one ``cw_step`` an iteration, with the reference's
    lines every num_iter // 5 iterations (the two losses are the batch means of the previous iteration, zero at iteration 0, as in
    the reference); ``verbose=False`` is one library call and prints the last line only.  Both give the same bits.

    Every search step starts from data + randn * 1e-7, drawn here once per search step from a seeded HOST torch.Generator: the
    reference draws on the GPU from the global CUDA stream, which cannot be reproduced, so clouds agree with a reference run in
    distribution only, not number for number.  ``ref_batch``: the batch the reference's losses are a mean over (scale =
    1 / ref_batch); the default is the batch passed to ``attack``."""

    def __init__(self, model, adv_func="logits", dist_func="l2", attack_lr=1e-2, init_weight=10., max_weight=80., binary_step=10,
                 num_iter=500, kappa=0., seed=1, ref_batch=None, verbose=True):
        if str(dist_func).lower() != "l2":
            raise ValueError("only the l2 distance of the reference's script is built")
        if int(binary_step) < 1 or int(num_iter) < 1:
            raise ValueError("binary_step and num_iter must be at least 1")
        self.model, self.adv_func, self.kappa = model, adv_func, float(kappa)
        self.attack_lr, self.init_weight, self.max_weight = float(attack_lr), float(init_weight), float(max_weight)
        self.binary_step, self.num_iter = int(binary_step), int(num_iter)
        self._common(seed, ref_batch, verbose)

    def noise(self, data: torch.Tensor) -> torch.Tensor:
        """[binary_step,B,K,3]: the start noise, one draw per search step."""
        return torch.stack([torch.randn(data.shape, generator=self.generator) * 1e-7 for _ in range(self.binary_step)])

    def _loop(self, data, target, noise):
        """Perturb.py:69-175 from the host: the kernels of ifd_cw_perturb_attack on the same numbers."""
        net = self.model
        dev = net.device
        B, K = int(data.shape[0]), int(data.shape[1])
        ori = data.to(dev).contiguous()
        tgt = target.to(dev)
        state = net.cw_state(B, K, self.init_weight, self.max_weight)

        def step(adv, grad, aux, t, last_input, want_info):
            return net.cw_step(state, grad, aux["pred"], tgt, adv, ori, t, self.attack_lr, self._scale(B), loss=aux["loss"],
                               last_input=last_input, want_info=want_info)
        return self._search(tgt, state, torch.empty_like(ori), ("pred", "loss"), lambda s: ori + noise[s].to(dev), step)

    def attack(self, data, target):
        data, target = self._tensors(data, target)
        B = int(data.shape[0])
        noise = self.noise(data)
        if self.verbose:
            adv, dist, ok = self._loop(data, target, noise)
        else:
            adv, dist, ok = self.model.cw_perturb_attack(data, target, noise, self.adv_func, self.kappa, self._scale(B), self.attack_lr,
                                                         self.init_weight, self.max_weight, self.binary_step, self.num_iter)
        return dist.cpu().numpy().astype(np.float64), adv.cpu().numpy(), self._finish(ok, B)


class CWKNN(_Attack):
    """The kNN attack (kNN.py CWKNN): ``num_iter`` Adam iterations on the adversarial loss plus ChamferkNNDist('adv2ori', 5, 1.05, 5.,
    3.), each followed by ProjectInnerClipLinf(0.1); no binary search, no records.  ``model`` is a ``runtime.Classifier`` (anything
    with its ``input_grad``, ``knn_step``, ``knn_attack`` and ``predict``), ``adv_func`` the loss by name ("logits":
    LogitsAdvLoss(kappa), or "cross_entropy"); ``dist_func`` "chamfer_knn" and ``clip_func`` "project_inner_clip_linf" are the only
    ones built.  ``attack(data, target [B])`` takes data [B,K,6] (points and normals) or [B,K,3] (no projection, the clip alone, as
    the reference does without normals) and returns the reference's pair (adversarial clouds [B,K,3] as a numpy array,
    success_num).  ``verbose=True`` drives the loop from the host, one ``input_grad`` and one ``knn_step`` an iteration, with the
    reference's two lines every num_iter // 5 iterations (every iteration when num_iter < 5; the two losses are the batch means of the
    previous iteration, zero at iteration 0) but not its wall-clock lines; ``verbose=False`` is one library call and prints the last
    line only.  Both give the same bits.

    The start is data + randn * 1e-7, drawn here from a seeded HOST torch.Generator: agreement with a reference run in distribution
    only.  ``ref_batch``: the batch the reference's losses are a mean over (scale = 1 / ref_batch); default: the batch passed."""

    CHAMFER_WEIGHT, KNN_WEIGHT, ALPHA, BUDGET = 5., 3., 1.05, 0.1

    def __init__(self, model, adv_func="logits", dist_func="chamfer_knn", clip_func="project_inner_clip_linf", attack_lr=1e-3,
                 num_iter=2500, kappa=15., seed=1, ref_batch=None, verbose=True):
        if str(dist_func).lower() != "chamfer_knn":
            raise ValueError("only the chamfer_knn distance of the reference's script is built")
        if str(clip_func).lower() != "project_inner_clip_linf":
            raise ValueError("only the project_inner_clip_linf clip of the reference's script is built")
        if int(num_iter) < 1:
            raise ValueError("num_iter must be at least 1")
        self.model, self.adv_func, self.kappa = model, adv_func, float(kappa)
        self.attack_lr, self.num_iter = float(attack_lr), int(num_iter)
        self._common(seed, ref_batch, verbose)

    def noise(self, data: torch.Tensor) -> torch.Tensor:
        """[B,K,3]: the start noise, one draw."""
        return torch.randn((int(data.shape[0]), int(data.shape[1]), 3), generator=self.generator) * 1e-7

    def _hyper(self):
        return dict(chamfer_weight=self.CHAMFER_WEIGHT, knn_weight=self.KNN_WEIGHT, alpha=self.ALPHA, budget=self.BUDGET)

    def _loop(self, pts, normal, target, noise):
        """kNN.py:77-140 from the host: the kernels of ifd_knn_attack on the same numbers."""
        net = self.model
        dev = net.device
        B = int(pts.shape[0])
        ori = pts.to(dev).contiguous()
        nrm = None if normal is None else normal.to(dev).contiguous()
        tgt = target.to(dev)
        adv = ori + noise.to(dev)
        m, v = torch.zeros_like(ori), torch.zeros_like(ori)
        every = max(self.num_iter // 5, 1)
        info = None
        for it in range(self.num_iter):
            grad, aux = net.input_grad(adv, tgt, self.adv_func, self.kappa, self._scale(B), want_aux=("pred", "loss"))
            if it % every == 0:
                self._progress('Iteration {}/{}, success {}/{}\nadv_loss: {:.4f}, dist_loss: {:.4f}', it, self.num_iter, aux["pred"], tgt,
                               info, 3)
            want = ("info",) if it % every == every - 1 else ()
            info = net.knn_step(grad, adv, ori, m, v, it + 1, self.attack_lr, self._scale(B), normal=nrm, loss=aux["loss"], want=want,
                                **self._hyper()).get("info")
        return adv, net.predict(adv).to(tgt.device) == tgt

    def attack(self, data, target):
        data, target = self._tensors(data, target)
        if data.dim() != 3 or int(data.shape[2]) not in (3, 6):
            raise ValueError("data must be [B,K,6] (points and normals) or [B,K,3]")
        B = int(data.shape[0])
        pts = data[:, :, :3].contiguous()
        normal = data[:, :, 3:].contiguous() if int(data.shape[2]) == 6 else None
        noise = self.noise(data)
        if self.verbose:
            adv, ok = self._loop(pts, normal, target, noise)
        else:
            adv, _, ok = self.model.knn_attack(pts, target, normal, noise, self.adv_func, self.kappa, self._scale(B), self.attack_lr,
                                               self.num_iter, **self._hyper())
        return adv.cpu().numpy(), self._finish(ok, B)


class _CWAdding(_Attack):
    """What CWAdd, CWAddClusters and CWAddObjects share: the checks and the end of ``attack`` and, around their own step calls, the
    host-driven loop.  A subclass has ``_run(data, target)`` -> (clouds, o_bestdist, success), on either loop form."""

    NUM_CRI, EPS, MIN_SAMPLES = 128, 0.2, 3        # clusters and objects start from DBSCAN on 128 critical points
    FEWEST = "128"                                 # the fewest points of a cloud, as the refusal names them

    def _fewest(self):
        return self.NUM_CRI

    def _host_loop(self, ori, tgt, state, cat, start, step):
        """``_search`` on ``cat``, the originals ``ori`` with the added rows behind them -> (ori with the rows the search ends on,
        o_bestdist, success)."""
        last = torch.empty(int(cat.shape[0]), int(cat.shape[1]) - int(ori.shape[1]), 3, device=cat.device, dtype=torch.float32)
        added, dist, ok = self._search(tgt, state, last, True, start, step)
        return torch.cat([ori, added], dim=1), dist, ok

    def attack(self, data, target):
        data, target = self._tensors(data, target)
        if data.dim() != 3 or int(data.shape[2]) != 3:
            raise ValueError("data must be [B,K,3]")
        if not self._fewest() <= int(data.shape[1]) <= 2048:
            raise ValueError("clouds must have between %s and 2048 points" % self.FEWEST)
        adv, dist, ok = self._run(data, target)
        return dist.cpu().numpy().astype(np.float64), adv.cpu().numpy(), self._finish(ok, int(data.shape[0]))


class CWAdd(_CWAdding):
    """CW attack by adding points (Add.py CWAdd): ``num_add`` points start on the cloud's critical points - the rows with the largest
    gradient of cross_entropy(logits, target) - and are optimised by ``binary_step`` search steps on the weight of the set distance,
    ``num_iter`` Adam iterations each, while the victim sees the original cloud with the added points behind it.  ``model`` is a
    ``runtime.Classifier`` (anything with its ``input_grad``, ``add_critical_points``, ``cw_state``, ``add_step``, ``cw_adjust`` and
    ``add_attack``), ``adv_func`` the loss by name ("logits": LogitsAdvLoss(kappa), or "cross_entropy"), ``dist_func`` "chamfer"
    (ChamferDist('adv2ori')) or "hausdorff" (HausdorffDist('adv2ori')).  ``attack(data [B,K,3], target [B])`` returns the reference's
    triple (o_bestdist [B], clouds [B,K+num_add,3]: the originals, then the best added points, or the last forwarded ones where the
    search never succeeded; success_num) as numpy arrays.  ``verbose=True`` drives the loop from the host, one ``input_grad`` and
    one ``add_step`` an iteration, with the reference's progress lines every num_iter // 5 iterations (the two losses are the batch
    means of the previous iteration, zero at iteration 0, as in the reference) - its wall-clock lines ("total time: ...") are left
    out; ``verbose=False`` is one library call and prints the last line only.  Both give the same bits.

    Every search step starts from critical points + randn * 1e-7, drawn here once per search step from a seeded HOST
    torch.Generator: agreement with a reference run in distribution only.  Where torch.topk leaves the order among equal scores
    open, the library's selection takes the lowest index first (include/ifd_add.h).  ``ref_batch``: the batch the reference's losses
    are a mean over (scale = 1 / ref_batch); the default is the batch passed to ``attack``."""

    def __init__(self, model, adv_func="logits", dist_func="chamfer", attack_lr=1e-2, init_weight=5e3, max_weight=4e4, binary_step=10,
                 num_iter=500, num_add=512, kappa=0., seed=1, ref_batch=None, verbose=True):
        self.dist_func = str(dist_func).lower()
        if self.dist_func not in ("chamfer", "hausdorff"):
            raise ValueError("dist_func must be chamfer or hausdorff")
        if int(binary_step) < 1 or int(num_iter) < 1:
            raise ValueError("binary_step and num_iter must be at least 1")
        if not 1 <= int(num_add) <= 1024:
            raise ValueError("num_add must be in [1, 1024]")
        self.model, self.adv_func, self.kappa = model, adv_func, float(kappa)
        self.attack_lr, self.init_weight, self.max_weight = float(attack_lr), float(init_weight), float(max_weight)
        self.binary_step, self.num_iter, self.num_add = int(binary_step), int(num_iter), int(num_add)
        self._common(seed, ref_batch, verbose)

    FEWEST = "num_add"                             # the critical points are rows of the cloud

    def _fewest(self):
        return self.num_add

    def noise(self, data: torch.Tensor) -> torch.Tensor:
        """[binary_step,B,num_add,3]: the start noise, one draw per search step."""
        shape = (int(data.shape[0]), self.num_add, 3)
        return torch.stack([torch.randn(shape, generator=self.generator) * 1e-7 for _ in range(self.binary_step)])

    def _loop(self, data, target, noise):
        """Add.py:85-220 from the host: the kernels of ifd_add_attack on the same numbers."""
        net = self.model
        dev = net.device
        B, K, A = int(data.shape[0]), int(data.shape[1]), self.num_add
        ori = data.to(dev).contiguous()
        tgt = target.to(dev)
        cri = net.add_critical_points(ori, tgt, A, self._scale(B))
        state = net.cw_state(B, A, self.init_weight, self.max_weight)
        cat = torch.cat([ori, cri], dim=1).contiguous()

        def start(s):
            cat[:, K:] = cri + noise[s].to(dev)
            return cat

        def step(cat, grad, aux, t, last_input, want_info):
            return net.add_step(self.dist_func, state, grad, aux["pred"], tgt, cat, A, t, self.attack_lr, self._scale(B), loss=aux["loss"],
                                last_input=last_input, want_info=want_info).get("info")
        return self._host_loop(ori, tgt, state, cat, start, step)

    def _run(self, data, target):
        noise = self.noise(data)
        if self.verbose:
            return self._loop(data, target, noise)
        return self.model.add_attack(self.dist_func, data, target, self.num_add, noise, self.adv_func, self.kappa,
                                     self._scale(int(data.shape[0])), self.attack_lr, self.init_weight, self.max_weight, self.binary_step,
                                     self.num_iter)


def init_clusters(points, labels, num_add, cl_num_p, rng):
    """Add_Cluster.py:103-127 on one cloud, the reference's numpy calls in its order on ``rng`` (a np.random.RandomState; the
    reference uses the global one): points [n,3] the critical points, labels [n] their DBSCAN labels -> [num_add,cl_num_p,3].  The
    ``num_add`` largest clusters in ascending order of their counts (a stable argsort), from each ``cl_num_p`` rows drawn with
    replacement unless it has more; then, while clusters are missing, a random non-outlier point and its ``cl_num_p`` nearest
    non-outlier points.  Where the reference raises: with no non-outlier point at all, every point counts as one for the fallback;
    a fallback with fewer than ``cl_num_p`` candidates repeats their sorted list cyclically."""
    points, result = np.asarray(points), np.asarray(labels)
    filter_idx = result > -0.5
    result = result[filter_idx]
    if filter_idx.any():
        points = points[filter_idx]
    out = []
    labels, counts = np.unique(result, return_counts=True)
    for one_label in labels[np.argsort(counts, kind="stable")[-num_add:]]:
        cluster_points = points[result == one_label]
        replace = not (len(cluster_points) > cl_num_p)
        out.append(cluster_points[rng.choice(len(cluster_points), cl_num_p, replace=replace)].copy())
    while len(out) < num_add:
        rand_point = points[rng.choice(len(points), 1)[0]]
        dist_matrix = np.sum((points - rand_point[None, :]) ** 2, axis=1)
        out.append(points[np.resize(np.argsort(dist_matrix)[:cl_num_p], cl_num_p)].copy())
    return np.array(out)


class CWAddClusters(_CWAdding):
    """CW attack by adding clusters (Add_Cluster.py CWAddClusters with FarChamferDist(num_add, 'adv2ori', 0.1)): ``num_add`` clusters
    of ``cl_num_p`` points are optimised by ``binary_step`` search steps on the weight of the distance - the farthest pair inside
    every cluster plus 0.1 x Chamfer - ``num_iter`` Adam iterations each, while the victim sees the original cloud with the clusters
    behind it.  ``model`` is a ``runtime.Classifier`` (anything with its ``input_grad``, ``add_critical_points``, ``cluster_dbscan``,
    ``cw_state``, ``cluster_step``, ``cw_adjust`` and ``cluster_attack``), ``adv_func`` the loss by name ("logits":
    LogitsAdvLoss(kappa), or "cross_entropy"), ``dist_func`` "far_chamfer" (the only one built).  ``attack(data [B,K,3], target
    [B])``, 128 <= K <= 2048, returns the reference's triple (o_bestdist [B], clouds [B,K+num_add*cl_num_p,3]: the originals, then
    the best added points, or the last forwarded ones where the search never succeeded; success_num) as numpy arrays.
    ``verbose=True`` drives the loop from the host, one ``input_grad`` and one ``cluster_step`` an iteration, with the reference's
    progress lines every num_iter // 5 iterations (the two losses are the batch means of the previous iteration, zero at iteration 0)
    - its wall-clock lines ("total: ...") are left out; ``verbose=False`` is one library call and prints the last line only.  Both
    give the same bits.

    The start (``_init_centers``): the 128 critical points of ``add_critical_points`` towards the TARGET labels, as the reference
    takes them, clustered on the device by ``cluster_dbscan(eps=0.2, min_samples=3)`` - include/ifd_cluster.h's definition, which is
    sklearn's result wherever no pair lies within float32 rounding of eps - the labels copied back once per batch, then
    ``init_clusters``: the reference's numpy calls in its order on ONE np.random.RandomState(seed) kept across ``attack`` calls, so
    that, given equal labels, the clusters are the reference's under np.random.seed(seed), number for number.  Two cases in which
    the reference raises are defined here: a cloud whose 128 critical points are all outliers uses all 128 as the candidate points
    of the fallback; a fallback with fewer than ``cl_num_p`` candidate points repeats their sorted list cyclically.

    Every search step starts from clusters + randn * 1e-7, drawn here once per search step from a seeded HOST torch.Generator:
    agreement with a reference run in distribution only.  ``ref_batch``: the batch the reference's losses are a mean over (scale =
    1 / ref_batch); the default is the batch passed to ``attack``."""

    def __init__(self, model, adv_func="logits", dist_func="far_chamfer", attack_lr=1e-2, init_weight=5., max_weight=30., binary_step=5,
                 num_iter=500, num_add=3, cl_num_p=32, kappa=0., seed=1, ref_batch=None, verbose=True):
        if str(dist_func).lower() != "far_chamfer":
            raise ValueError("only the far_chamfer distance of the reference's script is built")
        if int(binary_step) < 1 or int(num_iter) < 1:
            raise ValueError("binary_step and num_iter must be at least 1")
        if int(num_add) < 1 or int(cl_num_p) < 1 or not 1 <= int(num_add) * int(cl_num_p) <= 1024:
            raise ValueError("num_add and cl_num_p must be at least 1 and num_add * cl_num_p in [1, 1024]")
        self.model, self.adv_func, self.kappa = model, adv_func, float(kappa)
        self.attack_lr, self.init_weight, self.max_weight = float(attack_lr), float(init_weight), float(max_weight)
        self.binary_step, self.num_iter, self.num_add, self.cl_num_p = int(binary_step), int(num_iter), int(num_add), int(cl_num_p)
        self.rng = np.random.RandomState(int(seed))
        self._common(seed, ref_batch, verbose)

    def noise(self, data: torch.Tensor) -> torch.Tensor:
        """[binary_step,B,num_add*cl_num_p,3]: the start noise, one draw per search step."""
        shape = (int(data.shape[0]), self.num_add * self.cl_num_p, 3)
        return torch.stack([torch.randn(shape, generator=self.generator) * 1e-7 for _ in range(self.binary_step)])

    def _init_centers(self, data, target):
        """Add_Cluster.py:83-130 -> clusters [B,num_add*cl_num_p,3] float32 (a CPU tensor)."""
        net = self.model
        B = int(data.shape[0])
        cri = net.add_critical_points(data, target, self.NUM_CRI, self._scale(B))
        labels = net.cluster_dbscan(cri, self.EPS, self.MIN_SAMPLES).cpu().numpy()
        cri = cri.cpu().numpy()
        out = np.stack([init_clusters(cri[b], labels[b], self.num_add, self.cl_num_p, self.rng) for b in range(B)])
        return torch.from_numpy(out.reshape(B, self.num_add * self.cl_num_p, 3).astype(np.float32))

    def _loop(self, data, target, clusters, noise):
        """Add_Cluster.py:165-278 from the host: the kernels of ifd_cluster_attack on the same numbers."""
        net = self.model
        dev = net.device
        B, K = int(data.shape[0]), int(data.shape[1])
        ori = data.to(dev).contiguous()
        tgt = target.to(dev)
        start = clusters.to(dev)
        state = net.cw_state(B, self.num_add * self.cl_num_p, self.init_weight, self.max_weight)
        cat = torch.cat([ori, start], dim=1).contiguous()

        def begin(s):
            cat[:, K:] = start + noise[s].to(dev)
            return cat

        def step(cat, grad, aux, t, last_input, want_info):
            return net.cluster_step(state, grad, aux["pred"], tgt, cat, self.num_add, self.cl_num_p, t, self.attack_lr, self._scale(B),
                                    loss=aux["loss"], last_input=last_input, want_info=want_info).get("info")
        return self._host_loop(ori, tgt, state, cat, begin, step)

    def _run(self, data, target):
        clusters = self._init_centers(data, target)
        noise = self.noise(data)
        if self.verbose:
            return self._loop(data, target, clusters, noise)
        return self.model.cluster_attack(data, target, clusters, self.num_add, self.cl_num_p, noise, self.adv_func, self.kappa,
                                         self._scale(int(data.shape[0])), self.attack_lr, self.init_weight, self.max_weight,
                                         self.binary_step, self.num_iter)


def prepare_objects(object_pc, scaling, num_add, obj_num_p, rng):
    """Add_Objects.py:86-98, the reference's numpy calls in its order on ``rng`` (a np.random.RandomState; the reference uses the
    global one): object_pc [M,3] -> [num_add,obj_num_p,3] float64.  The object is centred, scaled to the unit sphere and by
    ``scaling`` in its own dtype (float32 for a float32 file), then shuffled in place once per object - the shuffles accumulate - and
    the first ``obj_num_p`` rows are taken.  The caller's array is not changed.  Refused with ValueError (the reference fails on a
    broadcast or an assert): an array that is not [M,3], fewer than ``obj_num_p`` rows, a non-finite or single-point object."""
    pc = np.asarray(object_pc)
    if pc.ndim != 2 or pc.shape[1] != 3:
        raise ValueError("the object must be an [M,3] array, got %s" % (tuple(pc.shape),))
    if len(pc) < int(obj_num_p):
        raise ValueError("the object has %d points, fewer than obj_num_p = %d" % (len(pc), int(obj_num_p)))
    pc = pc - np.mean(pc, axis=0)[None, :]                             # normalize_points_np
    with np.errstate(all="ignore"):
        pc = pc / np.max(np.sqrt(np.sum(pc ** 2, axis=1)), 0)
    if not np.isfinite(pc).all():
        raise ValueError("the object cannot be normalised (all points equal, or non-finite coordinates)")
    pc = pc * scaling
    out = np.zeros((int(num_add), int(obj_num_p), 3))
    for i in range(int(num_add)):
        rng.shuffle(pc)
        out[i] = pc[:int(obj_num_p)].copy()
    return out


def init_centers(points, labels, num_add, rng):
    """Add_Objects.py:116-143 on one cloud, the reference's numpy calls in its order on ``rng`` (np.random.RandomState): points [n,3]
    the critical points, labels [n] their DBSCAN labels -> [num_add,3].  From each of the ``num_add`` largest clusters, in ascending
    order of their counts (a stable argsort), the cluster point nearest to the cluster's mean (the lowest index among equals); then,
    while centres are missing, one random non-outlier point.  Where the reference raises - no non-outlier point at all - every point
    counts as one for the fallback."""
    points, result = np.asarray(points), np.asarray(labels)
    filter_idx = result > -0.5
    result = result[filter_idx]
    if filter_idx.any():
        points = points[filter_idx]
    out = []
    labels, counts = np.unique(result, return_counts=True)
    for one_label in labels[np.argsort(counts, kind="stable")[-num_add:]]:
        cluster_points = points[result == one_label]
        cluster_center = np.mean(cluster_points, axis=0)
        dist = np.sum((cluster_points - cluster_center[None, :]) ** 2, axis=1)
        out.append(cluster_points[np.argmin(dist)].copy())
    while len(out) < num_add:
        out.append(points[rng.choice(len(points), 1)[0]].copy())
    return np.array(out)


class CWAddObjects(_CWAdding):
    """CW attack by adding objects (Add_Objects.py CWAddObjects with L2ChamferDist(num_add, 'adv2ori', 0.2)): ``num_add`` copies of
    ``obj_num_p`` points of one object are placed into the cloud by a rotation about the y axis and a shift each; the object-frame
    points, the shifts and the angles are optimised by ``binary_step`` search steps on the weight of the distance - the L2 norm of
    the points' displacement from the object plus 0.2 x Chamfer of the placed points to the cloud - ``num_iter`` Adam iterations each.
    ``model`` is a ``runtime.Classifier`` (anything with its ``input_grad``, ``add_critical_points``, ``cluster_dbscan``,
    ``object_state``, ``object_place``, ``object_step``, ``cw_adjust`` and ``object_attack``), ``object_pc`` the object [M,3] (the
    reference's data/airplane.npy), ``adv_func`` the loss by name ("logits": LogitsAdvLoss(kappa), or "cross_entropy"), ``dist_func``
    "l2_chamfer" (the only one built).  ``attack(data [B,K,3], target [B])``, 128 <= K <= 2048, returns the reference's triple
    (o_bestdist [B], clouds [B,K+num_add*obj_num_p,3]: the originals, then the best placed points, or the last forwarded ones where
    the search never succeeded; success_num) as numpy arrays.  ``verbose=True`` drives the loop from the host, one ``input_grad`` and
    one ``object_step`` an iteration, with the reference's progress lines every num_iter // 5 iterations (the two losses are the batch
    means of the previous iteration, zero at iteration 0) - its wall-clock lines ("total: ...") are left out; ``verbose=False`` is one
    library call and prints the last line only.  Both give the same bits.

    ONE np.random.RandomState(seed) does the object's shuffles at construction (``prepare_objects``) and then the fallback draws of
    ``init_centers``, kept across ``attack`` calls: given equal DBSCAN labels, objects and centres are the reference's under
    np.random.seed(seed), number for number.  The centres (``_init_centers``): the 128 critical points of ``add_critical_points``
    towards the TARGET labels, clustered on the device by ``cluster_dbscan(eps=0.2, min_samples=3)`` (include/ifd_cluster.h's
    definition, sklearn's result wherever no pair lies within float32 rounding of eps), then ``init_centers``.  Defined where the
    reference raises or leaves the order open: a cloud whose 128 critical points are all outliers uses all of them as fallback
    candidates; the argsort of the cluster counts is stable; an object with fewer than ``obj_num_p`` rows, or not [M,3], is refused
    with ValueError.

    Every search step starts from objects + randn * 1e-7, centres + randn * 1e-7 and angles rand * pi, drawn here in the reference's
    order from a seeded HOST torch.Generator: agreement with a reference run in distribution only.  The reference draws three angles
    per object and rotates by the first alone; the other two never move and reach no output, so one angle per object is kept.
    ``ref_batch``: the batch the reference's losses are a mean over (scale = 1 / ref_batch); the default is the batch passed to
    ``attack``."""

    def __init__(self, model, object_pc, adv_func="logits", dist_func="l2_chamfer", attack_lr=1e-2, init_weight=5., max_weight=40.,
                 binary_step=5, num_iter=500, num_add=3, obj_num_p=64, scaling=0.3, kappa=0., seed=1, ref_batch=None, verbose=True):
        if str(dist_func).lower() != "l2_chamfer":
            raise ValueError("only the l2_chamfer distance of the reference's script is built")
        if int(binary_step) < 1 or int(num_iter) < 1:
            raise ValueError("binary_step and num_iter must be at least 1")
        if int(num_add) < 1 or int(obj_num_p) < 1 or not 1 <= int(num_add) * int(obj_num_p) <= 1024:
            raise ValueError("num_add and obj_num_p must be at least 1 and num_add * obj_num_p in [1, 1024]")
        self.model, self.adv_func, self.kappa = model, adv_func, float(kappa)
        self.attack_lr, self.init_weight, self.max_weight = float(attack_lr), float(init_weight), float(max_weight)
        self.binary_step, self.num_iter, self.num_add, self.obj_num_p = int(binary_step), int(num_iter), int(num_add), int(obj_num_p)
        self.rng = np.random.RandomState(int(seed))
        self.object_pc = prepare_objects(object_pc, scaling, self.num_add, self.obj_num_p, self.rng)
        self._common(seed, ref_batch, verbose)

    def draws(self, data: torch.Tensor):
        """(noise_obj [binary_step,B,A,3], noise_shift [binary_step,B,num_add,3], angles0 [binary_step,B,num_add]): per search step
        the reference's three draws in its order (Add_Objects.py:229-240)."""
        B, na, A = int(data.shape[0]), self.num_add, self.num_add * self.obj_num_p
        no, ns, an = [], [], []
        for _ in range(self.binary_step):
            no.append(torch.randn((B, A, 3), generator=self.generator) * 1e-7)
            ns.append(torch.randn((B, na, 3), generator=self.generator) * 1e-7)
            an.append((torch.rand((B, na, 3), generator=self.generator) * np.pi)[..., 0].contiguous())
        return torch.stack(no), torch.stack(ns), torch.stack(an)

    def _init_centers(self, data, target):
        """Add_Objects.py:100-146 -> centres [B,num_add,3] float32 (a CPU tensor)."""
        net = self.model
        B = int(data.shape[0])
        cri = net.add_critical_points(data, target, self.NUM_CRI, self._scale(B))
        labels = net.cluster_dbscan(cri, self.EPS, self.MIN_SAMPLES).cpu().numpy()
        cri = cri.cpu().numpy()
        out = np.stack([init_centers(cri[b], labels[b], self.num_add, self.rng) for b in range(B)])
        return torch.from_numpy(out.astype(np.float32))

    def _loop(self, data, target, objects, centers, noise_obj, noise_shift, angles0):
        """Add_Objects.py:227-367 from the host: the kernels of ifd_object_attack on the same numbers."""
        net = self.model
        dev = net.device
        B, K, na, P = int(data.shape[0]), int(data.shape[1]), self.num_add, self.obj_num_p
        A = na * P
        ori = data.to(dev).contiguous()
        tgt = target.to(dev)
        objects, centers = objects.to(dev), centers.to(dev)
        state = net.object_state(B, na, P, self.init_weight, self.max_weight)
        cat = torch.cat([ori, torch.zeros(B, A, 3, device=dev)], dim=1).contiguous()

        def start(s):
            state["obj"].copy_(objects.reshape(1, A, 3) + noise_obj[s].to(dev))
            state["shift"].copy_(centers + noise_shift[s].to(dev))
            state["angle"].copy_(angles0[s].to(dev))
            for key in ("shift_m", "shift_v", "angle_m", "angle_v"):
                state[key].zero_()
            net.object_place(state["obj"], state["angle"], state["shift"], cat, na, P)
            return cat

        def step(cat, grad, aux, t, last_input, want_info):
            return net.object_step(state, objects, grad, aux["pred"], tgt, cat, na, P, t, self.attack_lr, self._scale(B), loss=aux["loss"],
                                   last_input=last_input, want_info=want_info).get("info")
        return self._host_loop(ori, tgt, state, cat, start, step)

    def _run(self, data, target):
        objects = torch.from_numpy(self.object_pc).float()
        centers = self._init_centers(data, target)
        noise_obj, noise_shift, angles0 = self.draws(data)
        if self.verbose:
            return self._loop(data, target, objects, centers, noise_obj, noise_shift, angles0)
        return self.model.object_attack(data, target, objects, centers, angles0, noise_obj, noise_shift, self.adv_func, self.kappa,
                                        self._scale(int(data.shape[0])), self.attack_lr, self.init_weight, self.max_weight,
                                        self.binary_step, self.num_iter)


class SaliencyDrop(_Attack):
    """The saliency point-dropping attack (Saliency/Drop.py SaliencyDrop): ceil(num_drop / k) rounds, each taking the gradient of
    cross_entropy(logits, label) and dropping the k points of highest saliency -(r ** alpha) * sum((x - centre) * grad), centre the
    per-coordinate median of the shrinking cloud.  ``model`` is a ``runtime.Classifier`` (anything with its ``input_grad``,
    ``drop_step``, ``drop_attack`` and ``predict``).  ``attack(data [B,K,3], target [B])`` - target the TRUE labels, the attack is
    untargeted - returns the reference's pair (clouds [B,K - num_drop,3] as a numpy array, success_num), where success_num counts
    the clouds the victim still classifies correctly.  ``verbose=True`` drives the rounds from the host, one ``input_grad`` and one
    ``drop_step`` a round, with the reference's two lines every max(num_rounds // 5, 1) rounds (the reference divides by
    num_rounds // 5 and fails below 5 rounds); ``verbose=False`` is one library call.  Both print the closing line and give the same
    bits.  No noise is drawn, so there is no seed.

    Where the reference leaves bits open the library decides (include/ifd_drop.h): among equal saliencies the lowest row is dropped
    first, and the survivors keep their input order - the reference returns them in topk's order, which cannot be reproduced.
    ``ref_batch``: the batch the reference's loss is a mean over (scale = 1 / ref_batch); default: the batch passed."""

    def __init__(self, model, num_drop, alpha=1, k=5, ref_batch=None, verbose=True):
        if int(num_drop) < 1 or int(k) < 1:
            raise ValueError("num_drop and k must be at least 1")
        if not float(alpha) > 0:
            raise ValueError("alpha must be positive")
        self.model, self.num_drop, self.alpha, self.k = model, int(num_drop), float(alpha), int(k)
        self._common(0, ref_batch, verbose)

    def _loop(self, data, target):
        """Drop.py:56-95 from the host: the kernels of ifd_drop_attack on the same numbers."""
        net = self.model
        dev = net.device
        B, K_ = int(data.shape[0]), int(data.shape[1])
        cur = data.to(dev).contiguous().clone()
        tgt = target.to(dev)
        n = torch.full((B,), K_, device=dev, dtype=torch.int32)
        num_rounds = -(-self.num_drop // self.k)
        every = max(num_rounds // 5, 1)
        for i in range(num_rounds):
            k = min(self.k, self.num_drop - i * self.k)
            grad, aux = net.input_grad(cur, tgt, "cross_entropy", 0., self._scale(B), n_points=n, want_aux=("pred",))
            if i % every == 0:
                print('Iteration {}/{}, success {}/{}\nPoint num: {}/{}'.format(i, num_rounds, int((aux["pred"].long() == tgt).sum()), B,
                                                                              K_ - i * self.k, K_))
            net.drop_step(grad, cur, n, k, self.alpha)
        out = cur[:, :K_ - self.num_drop].contiguous()
        return out, net.predict(out).to(tgt.device) == tgt

    def attack(self, data, target):
        data, target = self._tensors(data, target)
        if data.dim() != 3 or int(data.shape[2]) != 3:
            raise ValueError("data must be [B,K,3]")
        B, K_ = int(data.shape[0]), int(data.shape[1])
        if not self.num_drop < K_ <= 2048:
            raise ValueError("clouds must have more than num_drop and at most 2048 points")
        if self.verbose:
            adv, ok = self._loop(data, target)
        else:
            adv, ok = self.model.drop_attack(data, target, self.num_drop, self.k, self.alpha, self._scale(B))
        success_num = int(ok.sum())
        print('Final success: {}/{}, point num: {}/{}'.format(success_num, B, int(adv.shape[1]), K_))
        return adv.cpu().numpy(), success_num
