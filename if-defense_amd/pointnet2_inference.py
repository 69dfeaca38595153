"""Accuracy and attack success rate of the PointNet++ victim on a (restored) cloud file - MI355X build of baselines/inference.py
with --model pointnet2.

    python -m ifdefense_amd.pointnet2_inference --data_root=path/to/file-pointnet2-x.npz --mode=target --model_path=pointnet2.pth

The flags, the num-points rules, the evaluation and the printed lines are those of ifdefense_amd.inference (imported, not
repeated); the model comes from --model or from the file's path, and anything but pointnet2 is refused with a pointer to the CLI
that runs it.  --model_path: the checkpoint (.pth saved from nn.DataParallel, or an .npz of its arrays); empty means
pretrain/{dataset}/pointnet2.pth.  A file that holds a cloud of more than 2048 points is refused with a message.

--fps_seed (default 1, the reference's set_seed(1)).  PointNet++ starts both of its farthest-point samplings at a random point
(torch.randint in farthest_point_sample), so the reference's own accuracy varies with its random stream - which also passes
through the weight initialisation and the DataLoader and is NOT reproduced here.  Here the two start indices of a cloud are a
function of the seed, of the cloud's position in the file and of its point count only: one torch.Generator seeded with
--fps_seed draws two 62-bit integers per cloud for the whole file at once, and cloud i starts at (u[i,0] mod n_i, u[i,1] mod 512).
The result therefore does not depend on how the file is batched.
"""
from __future__ import annotations

import sys

import numpy as np

from .inference import ClosesClassifier, build_parser, default_weight_path, get_model_name, points_to_take, run_victim_cli

MAX_POINTS = 2048
OTHER_CLI = {'pointnet': "`python -m ifdefense_amd.inference`", 'dgcnn': "`python -m ifdefense_amd.dgcnn_inference`"}


def fps_starts(seed: int, sizes) -> np.ndarray:
    """[len(sizes), 2] int32: the level-1 and level-2 start index of every cloud of a file (module docstring)."""
    import torch
    g = torch.Generator()
    g.manual_seed(int(seed))
    u = torch.randint(0, 2 ** 62, (len(sizes), 2), generator=g, dtype=torch.int64).numpy()
    n = np.maximum(np.asarray(sizes, dtype=np.int64), 1)
    return np.stack([u[:, 0] % n, u[:, 1] % 512], axis=1).astype(np.int32)


class _CloudSizeError(ValueError):
    pass


class _Seeded(ClosesClassifier):
    """predict() of the wrapped classifier behind the check of the clouds' sizes, with the file's start indices."""

    def __init__(self, classifier, seed: int):
        super().__init__(classifier)
        self.seed = seed

    def predict(self, clouds):
        sizes = np.array([len(c) for c in clouds])
        if (sizes > MAX_POINTS).any():
            i = int(np.argmax(sizes > MAX_POINTS))
            raise _CloudSizeError("cloud %d has %d points, more than the %d the PointNet++ victim takes" % (i, int(sizes[i]), MAX_POINTS))
        if (sizes < 1).any():
            raise _CloudSizeError("cloud %d is empty" % int(np.argmax(sizes < 1)))
        return self.classifier.predict(clouds, fps_start=fps_starts(self.seed, sizes))


def main(argv=None, make_classifier=None) -> int:
    parser = build_parser()
    parser.add_argument('--fps_seed', type=int, default=1, help='seed of the start indices of the farthest point samplings')
    args = parser.parse_args(argv)
    if not args.model:
        args.model = get_model_name(args.data_root)
        if args.model is None:
            print('Victim model not recognized!', file=sys.stderr)
            return 2
    if args.model.lower() != 'pointnet2':
        print("pointnet2_inference: only the pointnet2 victim runs here, not {}; evaluate it with {}".format(
            args.model, OTHER_CLI.get(args.model.lower(), "the reference's baselines/inference.py")), file=sys.stderr)
        return 2
    num_points = points_to_take(args.data_root, args.num_points)
    if make_classifier is None:
        def make_classifier(model, model_path):
            from .runtime import PointNet2Classifier
            from .weights import load_checkpoint
            return PointNet2Classifier(load_checkpoint(model_path, model), device=args.device)
    model_path = args.model_path or default_weight_path(args.dataset, 'pointnet2')
    classifier = _Seeded(make_classifier('pointnet2', model_path), args.fps_seed)
    return run_victim_cli("pointnet2_inference", args, classifier, num_points, _CloudSizeError)


if __name__ == '__main__':
    sys.exit(main())
