"""Accuracy and attack success rate of the PointConv victim on a (restored) cloud file - MI355X build of baselines/inference.py
with --model pointconv.

    python -m ifdefense_amd.pointconv_inference --data_root=path/to/file-pointconv-x.npz --mode=target --model_path=pointconv.pth

The flags, the num-points rules, the evaluation and the printed lines are those of ifdefense_amd.inference (imported, not
repeated); the model comes from --model or from the file's path, and anything but pointconv is refused with a pointer to the CLI
that runs it.  --model_path: the checkpoint (.pth saved from nn.DataParallel, or an .npz of its arrays); empty means
pretrain/{dataset}/pointconv.pth.  A file that holds a cloud of fewer than 32 points (the reference's topk raises on it) or of
more than 2048 is refused with a message.

--fps_seed (default 1, the reference's set_seed(1)).  PointConv starts both of its farthest-point samplings at a random point
(torch.randint in farthest_point_sample), exactly as PointNet++ does; the start indices of a cloud are those of
ifdefense_amd.pointnet2_inference.fps_starts (imported, not repeated): a function of the seed, of the cloud's position in the file
and of its point count only, so the result does not depend on how the file is batched.
"""
from __future__ import annotations

import sys

import numpy as np

from .inference import ClosesClassifier, build_parser, default_weight_path, get_model_name, points_to_take, run_victim_cli
from .pointnet2_inference import fps_starts

MAX_POINTS, MIN_POINTS = 2048, 32
OTHER_CLI = {'pointnet': "`python -m ifdefense_amd.inference`", 'dgcnn': "`python -m ifdefense_amd.dgcnn_inference`",
             'pointnet2': "`python -m ifdefense_amd.pointnet2_inference`"}


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
            raise _CloudSizeError("cloud %d has %d points, more than the %d the PointConv victim takes" % (i, int(sizes[i]), MAX_POINTS))
        if (sizes < MIN_POINTS).any():
            i = int(np.argmax(sizes < MIN_POINTS))
            raise _CloudSizeError("cloud %d has %d points, fewer than the %d the PointConv victim needs (its first level takes "
                                  "the 32 nearest points of a centroid)" % (i, int(sizes[i]), MIN_POINTS))
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
    if args.model.lower() != 'pointconv':
        print("pointconv_inference: only the pointconv victim runs here, not {}; evaluate it with {}".format(
            args.model, OTHER_CLI.get(args.model.lower(), "the reference's baselines/inference.py")), file=sys.stderr)
        return 2
    num_points = points_to_take(args.data_root, args.num_points)
    if make_classifier is None:
        def make_classifier(model, model_path):
            from .runtime import PointConvClassifier
            from .weights import load_checkpoint
            return PointConvClassifier(load_checkpoint(model_path, model), device=args.device)
    model_path = args.model_path or default_weight_path(args.dataset, 'pointconv')
    classifier = _Seeded(make_classifier('pointconv', model_path), args.fps_seed)
    return run_victim_cli("pointconv_inference", args, classifier, num_points, _CloudSizeError)


if __name__ == '__main__':
    sys.exit(main())
