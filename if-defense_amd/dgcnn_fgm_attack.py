"""Targeted FGM / I-FGM / MI-FGM / PGD attack on the DGCNN victim - MI355X build of baselines/attack_scripts/targeted_fgm_attack.py
with --model dgcnn.

    python -m ifdefense_amd.dgcnn_fgm_attack --data_root=data/attack_data.npz --attack_type=ifgm --model_path=dgcnn.pth

The flags, the budget rules, the progress lines and the result file are those of ifdefense_amd.fgm_attack (imported, not
repeated); the file goes to <out_dir>/attack/results/{dataset}_{num_points}/FGM/dgcnn/{type}-budget_{delta}-iter_{n}-
success_{rate:.4f}-rank_{r}.npz, which ``ifdefense_amd.dgcnn_inference`` reads.  --model defaults to dgcnn here and anything else
is refused (pointnet is attacked by ``ifdefense_amd.fgm_attack``).  --k is honoured (1 .. 32); --emb_dims other than 1024 is
refused, as are clouds of fewer than k or more than 2048 points.  Every refusal is a message and status 2, before the victim is
made.  --model_path: the checkpoint (.pth saved from nn.DataParallel, or an .npz of its arrays); empty means
pretrain/{dataset}/dgcnn.pth.  The gradient is the one of the network with its neighbour tables held fixed (include/ifd_dgcnn_atk.h).
"""
from __future__ import annotations

import sys

from .dgcnn_inference import MAX_POINTS
from .fgm_attack import attack_file, build_parser
from .inference import default_weight_path

PROG = 'dgcnn_fgm_attack'


def main(argv=None, make_classifier=None) -> int:
    parser = build_parser()
    parser.set_defaults(model='dgcnn')
    args = parser.parse_args(argv)
    if args.model.lower() != 'dgcnn':
        print("{}: only the dgcnn victim is attacked here, not {}; pointnet is attacked by `python -m ifdefense_amd.fgm_attack`"
              .format(PROG, args.model), file=sys.stderr)
        return 2
    if args.feature_transform:
        print("{}: --feature_transform belongs to pointnet".format(PROG), file=sys.stderr)
        return 2
    if args.emb_dims != 1024:
        print("{}: only --emb_dims 1024 is built, got {}".format(PROG, args.emb_dims), file=sys.stderr)
        return 2
    if not 1 <= args.k <= 32:
        print("{}: --k must lie in [1, 32], got {}".format(PROG, args.k), file=sys.stderr)
        return 2

    def check_data(data):
        n = data.shape[1]
        if n < args.k:
            return "clouds of {} points, fewer than k = {}: DGCNN needs k neighbours for every point".format(n, args.k)
        if n > MAX_POINTS:
            return "clouds of {} points, more than the {} the DGCNN victim takes".format(n, MAX_POINTS)
        return None

    def open_classifier():
        make = make_classifier
        if make is None:
            def make(model, k, model_path):
                from .runtime import DgcnnClassifier
                from .weights import load_checkpoint
                return DgcnnClassifier(load_checkpoint(model_path, model), k=k, device=args.device)
        model_path = args.model_path or default_weight_path(args.dataset, 'dgcnn')
        print('Loading weight {}'.format(model_path))
        return make('dgcnn', args.k, model_path)

    return attack_file(PROG, args, open_classifier, check_data)


if __name__ == '__main__':
    sys.exit(main())
