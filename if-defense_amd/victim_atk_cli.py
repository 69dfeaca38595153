"""What victim_perturb_attack, victim_knn_attack and victim_drop_attack share: the reference's Perturb, kNN and Drop scripts on
the DGCNN, PointNet++ and PointConv victims (include/ifd_victim_atk.h).  PointNet keeps its own scripts (perturb_attack,
knn_attack, drop_attack), which go on refusing every other --model.

The rules are those of pointnet2_fgm_attack: what the batches of a file share is taken from the FILE, so that --batch_size only
says how many clouds go through the library at once and the clouds written do not depend on it, bit for bit.
  - The loss is a mean over the whole file: scale = 1 / N in every batch.
  - The start noise is one seeded draw for the file: search step s of Perturb starts cloud i from data[i] + noise_s[i], where
    noise_0, noise_1, ... are consecutive randn([N,K,3]) * 1e-7 draws of one torch.Generator seeded with --seed; kNN has the one
    draw noise_0.  A batch replays the generator and keeps its own rows, one [N,K,3] draw at a time, so the host never holds
    [binary_step,N,K,3].
  - PointNet++ and PointConv: the starts of cloud i are ``pointnet2_inference.fps_starts(fps_seed, sizes)[i]`` by its place in the
    file, in every gradient and in the closing forward.  ``sizes`` are the sizes that are WRITTEN - for Drop K - num_drop - so that
    the rate in the file's name is what the victim's inference CLI reports on that file with the same --fps_seed.

Every refusal is a message and status 2, before the victim is made: --model pointnet (a pointer to its own CLI) or an unknown
one, --feature_transform, for DGCNN --emb_dims other than 1024 or --k outside [1, 32], and clouds outside the victim's range
(DGCNN [k, 2048], PointNet++ [1, 2048], PointConv [32, 2048]; kNN needs 6 points as well, and Drop what is left after the drop).
"""
from __future__ import annotations

import sys

import numpy as np

from . import attack_cli as C
from .inference import default_weight_path
from .pointnet2_fgm_attack import BoundStarts
from .pointnet2_inference import fps_starts

MAX_POINTS = 2048
# --model -> (the name in messages, the class in ifdefense_amd.runtime, the fewest points without --k, whether it samples)
VICTIMS = {'dgcnn': ('DGCNN', 'DgcnnClassifier', 1, False), 'pointnet2': ('PointNet++', 'PointNet2Classifier', 1, True),
           'pointconv': ('PointConv', 'PointConvClassifier', 32, True)}


class BoundLoopStarts(BoundStarts):
    """BoundStarts with the calls that attack.CWPerturb, CWKNN and SaliencyDrop make: the fps_start of the current batch goes
    to every call that runs the network, the step calls pass through."""

    def predict(self, pc, n_points=None):
        return self.classifier.predict(pc, n_points, fps_start=self._starts(pc))

    def input_grad(self, pc, target, loss="logits", kappa=0., scale=1., n_points=None, want_aux=False):
        return self.classifier.input_grad(pc, target, loss, kappa, scale, n_points=n_points, want_aux=want_aux, fps_start=self._starts(pc))

    def cw_perturb_attack(self, pc, *a, **kw):
        return self.classifier.cw_perturb_attack(pc, *a, fps_start=self._starts(pc), **kw)

    def knn_attack(self, pc, *a, **kw):
        return self.classifier.knn_attack(pc, *a, fps_start=self._starts(pc), **kw)

    def drop_attack(self, pc, *a, **kw):
        return self.classifier.drop_attack(pc, *a, fps_start=self._starts(pc), **kw)

    def __getattr__(self, name):
        if name in ("cw_state", "cw_step", "cw_adjust", "knn_step", "knn_project_clip", "drop_step"):
            return getattr(self.classifier, name)
        raise AttributeError(name)


def add_victim_flags(parser):
    parser.add_argument('--fps_seed', type=int, default=1,
                        help='seed of the start indices of the farthest point samplings (pointnet2, pointconv)')
    return parser


def refuse_victim(prog, args, pointnet_cli):
    """2 behind a message where the flags cannot be served, else 0."""
    model = args.model.lower()
    if model == 'pointnet':
        print("{}: the pointnet victim is attacked by `python -m ifdefense_amd.{}`".format(prog, pointnet_cli), file=sys.stderr)
        return 2
    if model not in VICTIMS:
        print("{}: unknown --model {} (dgcnn | pointnet2 | pointconv)".format(prog, args.model), file=sys.stderr)
        return 2
    if args.feature_transform:
        print("{}: --feature_transform belongs to pointnet".format(prog), file=sys.stderr)
        return 2
    if model == 'dgcnn':
        if args.emb_dims != 1024:
            print("{}: only --emb_dims 1024 is built, got {}".format(prog, args.emb_dims), file=sys.stderr)
            return 2
        if not 1 <= args.k <= 32:
            print("{}: --k must lie in [1, 32], got {}".format(prog, args.k), file=sys.stderr)
            return 2
    return 0


def min_points(args, floor=1):
    """The fewest points of a cloud that goes through the victim: its own minimum (DGCNN: --k), and the attack's ``floor``."""
    model = args.model.lower()
    return max(args.k if model == 'dgcnn' else VICTIMS[model][2], floor)


def refuse_clouds(prog, args, n, written=None, floor=1):
    """2 behind a message where clouds of n points (of which ``written`` reach the result, default all) are outside what the
    victim and the attack take, else 0."""
    label = VICTIMS[args.model.lower()][0]
    lo = min_points(args, floor)
    written = n if written is None else written
    if n > MAX_POINTS:
        print("{}: clouds of {} points, more than the {} the {} victim takes".format(prog, n, MAX_POINTS, label), file=sys.stderr)
        return 2
    if written < lo:
        print("{}: clouds of {} points, fewer than the {} the attack on the {} victim needs".format(prog, written, lo, label),
              file=sys.stderr)
        return 2
    return 0


def open_victim(args, make_classifier, sizes):
    """The victim of --model; ``sizes``: the sizes of the file's clouds as they are written, for the starts of a victim that
    samples.  make_classifier (test hook): (model, k, model_path) for dgcnn, (model, model_path) for the others."""
    model = args.model.lower()
    label, classifier_name, _, samples = VICTIMS[model]
    model_path = args.model_path or default_weight_path(args.dataset, model)
    print('Loading weight {}'.format(model_path))
    if make_classifier is None:
        from . import runtime
        from .weights import load_checkpoint
        kw = dict(k=args.k) if model == 'dgcnn' else {}
        net = getattr(runtime, classifier_name)(load_checkpoint(model_path, model), device=args.device, **kw)
    elif model == 'dgcnn':
        net = make_classifier(model, args.k, model_path)
    else:
        net = make_classifier(model, model_path)
    return BoundLoopStarts(net, fps_starts(args.fps_seed, sizes)) if samples else net


def file_noise(seed, shape, steps, a, n):
    """Rows [a, a + n) of the file's start noise: [steps, n, K, 3] of ``steps`` consecutive randn(shape) * 1e-7 draws, shape =
    (N, K, 3), of one generator seeded with ``seed``.  One draw is held at a time."""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return torch.stack([(torch.randn(shape, generator=g) * 1e-7)[a:a + n].clone() for _ in range(steps)])


def run_file(attacker, classifier, data, target, batch_size, noise_of=None):
    """attack_cli.run_batches over the file with the starts of every batch bound and its rows of the file's noise
    (``noise_of(a, n)``) in place of the attacker's own draw."""
    def on_batch(a, n):
        if isinstance(classifier, BoundStarts):
            classifier.at(a, n)
        if noise_of is not None:
            attacker.noise = lambda d: noise_of(a, n)
    return C.run_batches(attacker, data, target, batch_size, on_batch)
