"""Targeted FGM / I-FGM / MI-FGM / PGD attack on the PointConv victim - MI355X build of
baselines/attack_scripts/targeted_fgm_attack.py with --model pointconv.

    python -m ifdefense_amd.pointconv_fgm_attack --data_root=data/attack_data.npz --attack_type=ifgm --model_path=pointconv.pth

The flags, the budget rules, the progress lines and the result file are those of ifdefense_amd.fgm_attack (imported, not
repeated); the file goes to <out_dir>/attack/results/{dataset}_{num_points}/FGM/pointconv/{type}-budget_{delta}-iter_{n}-
success_{rate:.4f}-rank_{r}.npz, which ``ifdefense_amd.pointconv_inference`` reads.  --model defaults to pointconv here and
anything else is refused (pointnet is attacked by ``ifdefense_amd.fgm_attack``, dgcnn by ``ifdefense_amd.dgcnn_fgm_attack``,
pointnet2 by ``ifdefense_amd.pointnet2_fgm_attack``), as are clouds of more than 2048 or fewer than 32 points.  Every refusal is a
message and status 2, before the victim is made.  --model_path: the checkpoint (.pth saved from nn.DataParallel, or an .npz of
its arrays); empty means pretrain/{dataset}/pointconv.pth.  The gradient is the one of the network with its index tables held
fixed (include/ifd_pc_atk.h).

--batch_size and --fps_seed mean what they mean in ``ifdefense_amd.pointnet2_fgm_attack``, whose adapter ``BoundStarts`` is
imported, not repeated: the clouds written do not depend on --batch_size, bit for bit (the loss scale and the start noise are the
file's, ``attack_file(by_file=True)``), and the starts of cloud i of the file are ``pointnet2_inference.fps_starts(fps_seed,
sizes)[i]`` in every gradient, every iteration and the closing prediction, so the success rate in the file's name is what
``pointconv_inference --fps_seed`` with the same seed reports on that file.
"""
from __future__ import annotations

import sys

from .fgm_attack import attack_file, build_parser
from .inference import default_weight_path
from .pointconv_inference import MAX_POINTS, MIN_POINTS
from .pointnet2_fgm_attack import BoundStarts
from .pointnet2_inference import fps_starts

PROG = 'pointconv_fgm_attack'
OTHER_CLI = {'pointnet': "`python -m ifdefense_amd.fgm_attack`", 'dgcnn': "`python -m ifdefense_amd.dgcnn_fgm_attack`",
             'pointnet2': "`python -m ifdefense_amd.pointnet2_fgm_attack`"}


def main(argv=None, make_classifier=None) -> int:
    parser = build_parser()
    parser.set_defaults(model='pointconv')
    parser.add_argument('--fps_seed', type=int, default=1, help='seed of the start indices of the farthest point samplings')
    args = parser.parse_args(argv)
    if args.model.lower() != 'pointconv':
        print("{}: only the pointconv victim is attacked here, not {}; attack it with {}".format(
            PROG, args.model, OTHER_CLI.get(args.model.lower(), "the reference's targeted_fgm_attack.py")), file=sys.stderr)
        return 2
    if args.feature_transform:
        print("{}: --feature_transform belongs to pointnet".format(PROG), file=sys.stderr)
        return 2
    sizes = []

    def check_data(data):
        n = data.shape[1]
        if n > MAX_POINTS:
            return "clouds of {} points, more than the {} the PointConv victim takes".format(n, MAX_POINTS)
        if n < MIN_POINTS:
            return "clouds of {} points, fewer than the {} the PointConv victim needs".format(n, MIN_POINTS)
        sizes[:] = [n] * len(data)
        return None

    def open_classifier():
        make = make_classifier
        if make is None:
            def make(model, model_path):
                from .runtime import PointConvClassifier
                from .weights import load_checkpoint
                return PointConvClassifier(load_checkpoint(model_path, model), device=args.device)
        model_path = args.model_path or default_weight_path(args.dataset, 'pointconv')
        print('Loading weight {}'.format(model_path))
        return BoundStarts(make('pointconv', model_path), fps_starts(args.fps_seed, sizes))

    return attack_file(PROG, args, open_classifier, check_data, on_batch=lambda classifier, a, n: classifier.at(a, n), by_file=True)


if __name__ == '__main__':
    sys.exit(main())
