"""Targeted FGM / I-FGM / MI-FGM / PGD attack on the PointNet++ victim - MI355X build of
baselines/attack_scripts/targeted_fgm_attack.py with --model pointnet2.

    python -m ifdefense_amd.pointnet2_fgm_attack --data_root=data/attack_data.npz --attack_type=ifgm --model_path=pointnet2.pth

The flags, the budget rules, the progress lines and the result file are those of ifdefense_amd.fgm_attack (imported, not
repeated); the file goes to <out_dir>/attack/results/{dataset}_{num_points}/FGM/pointnet2/{type}-budget_{delta}-iter_{n}-
success_{rate:.4f}-rank_{r}.npz, which ``ifdefense_amd.pointnet2_inference`` reads.  --model defaults to pointnet2 here and
anything else is refused (pointnet is attacked by ``ifdefense_amd.fgm_attack``, dgcnn by ``ifdefense_amd.dgcnn_fgm_attack``), as
are clouds of more than 2048 points.  Every refusal is a message and status 2, before the victim is made.  --model_path: the
checkpoint (.pth saved from nn.DataParallel, or an .npz of its arrays); empty means pretrain/{dataset}/pointnet2.pth.  The
gradient is the one of the network with its index tables held fixed (include/ifd_pn2_atk.h).

--batch_size only says how many clouds go through the library at once: the clouds written do not depend on it, bit for bit.  What
ifdefense_amd.fgm_attack takes per batch is taken here from the file, as its --batch_size -1 takes it: the loss is a mean over
the whole file (scale = 1 / N in every batch; the reference's mean over its batch differs from it only in how the updates' + 1e-9
weighs against the gradient's norm) and the start noise is one draw of the file's shape (``attack_file(by_file=True)``).

--fps_seed (default 1).  PointNet++ starts both of its farthest point samplings at a random point.  Here the starts of cloud i of
the file are ``pointnet2_inference.fps_starts(fps_seed, sizes)[i]``, however the file is batched, in every gradient, every
iteration and the closing prediction: the success rate in the file's name is what ``pointnet2_inference --fps_seed`` with the
same seed reports on that file.  The reference redraws its starts on every forward pass from the global random stream, which
also passes through its weight initialisation and its DataLoader and is NOT reproduced here: its attack sees other centroids in
every iteration, and its reported rate is one draw of them.
"""
from __future__ import annotations

import sys

from .fgm_attack import attack_file, build_parser
from .inference import default_weight_path
from .pointnet2_inference import MAX_POINTS, fps_starts

PROG = 'pointnet2_fgm_attack'
OTHER_CLI = {'pointnet': "`python -m ifdefense_amd.fgm_attack`", 'dgcnn': "`python -m ifdefense_amd.dgcnn_fgm_attack`",
             'pointconv': "`python -m ifdefense_amd.pointconv_fgm_attack`"}


class BoundStarts:
    """A PointNet2Classifier (anything with its calls) with the fps_start of the current batch bound to the calls the attack classes
    make, which know nothing of starts.  ``starts`` [N,2]: the whole file's; ``at(a, n)`` selects the batch of n clouds at offset a."""

    def __init__(self, classifier, starts):
        self.classifier, self.starts, self.device = classifier, starts, classifier.device
        self.batch = None

    def at(self, a, n):
        self.batch = self.starts[a:a + n]

    def _starts(self, pc):
        if self.batch is None or len(self.batch) != len(pc):
            raise ValueError("the batch of {} clouds does not match the {} starts bound to it".format(
                len(pc), 0 if self.batch is None else len(self.batch)))
        return self.batch

    def predict(self, pc):
        return self.classifier.predict(pc, fps_start=self._starts(pc))

    def input_grad(self, pc, target, loss="logits", kappa=0., scale=1., want_aux=False):
        return self.classifier.input_grad(pc, target, loss, kappa, scale, want_aux=want_aux, fps_start=self._starts(pc))

    def fgm_update(self, *a, **kw):
        return self.classifier.fgm_update(*a, **kw)

    def fgm_attack(self, kind, pc, target, budget, step_size, num_iter=1, mu=1., loss="logits", kappa=0., scale=1.):
        return self.classifier.fgm_attack(kind, pc, target, budget, step_size, num_iter, mu, loss, kappa, scale,
                                          fps_start=self._starts(pc))

    def close(self):
        if hasattr(self.classifier, "close"):
            self.classifier.close()


def sampled_main(prog, other_cli, model, label, classifier_name, min_points, max_points, argv, make_classifier) -> int:
    """main() of the CLI ``prog`` of a victim that samples: ``model`` its --model, ``label`` its name in messages,
    ``classifier_name`` its class in ifdefense_amd.runtime, [min_points, max_points] the clouds it takes."""
    parser = build_parser()
    parser.set_defaults(model=model)
    parser.add_argument('--fps_seed', type=int, default=1, help='seed of the start indices of the farthest point samplings')
    args = parser.parse_args(argv)
    if args.model.lower() != model:
        print("{}: only the {} victim is attacked here, not {}; attack it with {}".format(
            prog, model, args.model, other_cli.get(args.model.lower(), "the reference's targeted_fgm_attack.py")), file=sys.stderr)
        return 2
    if args.feature_transform:
        print("{}: --feature_transform belongs to pointnet".format(prog), file=sys.stderr)
        return 2
    sizes = []

    def check_data(data):
        n = data.shape[1]
        if n > max_points:
            return "clouds of {} points, more than the {} the {} victim takes".format(n, max_points, label)
        if n < min_points:
            return "empty clouds" if min_points == 1 else "clouds of {} points, fewer than the {} the {} victim needs".format(
                n, min_points, label)
        sizes[:] = [n] * len(data)
        return None

    def open_classifier():
        make = make_classifier
        if make is None:
            def make(model, model_path):
                from . import runtime
                from .weights import load_checkpoint
                return getattr(runtime, classifier_name)(load_checkpoint(model_path, model), device=args.device)
        model_path = args.model_path or default_weight_path(args.dataset, model)
        print('Loading weight {}'.format(model_path))
        return BoundStarts(make(model, model_path), fps_starts(args.fps_seed, sizes))

    return attack_file(prog, args, open_classifier, check_data, on_batch=lambda classifier, a, n: classifier.at(a, n), by_file=True)


def main(argv=None, make_classifier=None) -> int:
    return sampled_main(PROG, OTHER_CLI, 'pointnet2', 'PointNet++', 'PointNet2Classifier', 1, MAX_POINTS, argv, make_classifier)


if __name__ == '__main__':
    sys.exit(main())
