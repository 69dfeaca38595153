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

from .pointconv_inference import MAX_POINTS, MIN_POINTS
from .pointnet2_fgm_attack import BoundStarts, sampled_main  # noqa: F401  (BoundStarts: the tests and callers reach it here too)

PROG = 'pointconv_fgm_attack'
OTHER_CLI = {'pointnet': "`python -m ifdefense_amd.fgm_attack`", 'dgcnn': "`python -m ifdefense_amd.dgcnn_fgm_attack`",
             'pointnet2': "`python -m ifdefense_amd.pointnet2_fgm_attack`"}


def main(argv=None, make_classifier=None) -> int:
    return sampled_main(PROG, OTHER_CLI, 'pointconv', 'PointConv', 'PointConvClassifier', MIN_POINTS, MAX_POINTS, argv, make_classifier)


if __name__ == '__main__':
    sys.exit(main())
