"""Targeted CW point-perturbation attack on the DGCNN, PointNet++ and PointConv victims - MI355X build of
baselines/attack_scripts/targeted_perturb_attack.py with --model dgcnn | pointnet2 | pointconv.

    python -m ifdefense_amd.victim_perturb_attack --model=pointnet2 --data_root=data/attack_data.npz --model_path=pointnet2.pth

The flags, the settings (init_weight 10, max_weight 80) and the result file are those of ifdefense_amd.perturb_attack (imported,
not repeated): <out_dir>/attack/results/{dataset}_{num_points}/Perturb/Perturb-{model}-{adv_func}-success_{rate:.4f}-rank_{r}.npz,
which ``ifdefense_amd.dgcnn_inference`` / ``pointnet2_inference`` / ``pointconv_inference`` read.  --k is DGCNN's neighbour count
(1 .. 32), --fps_seed (default 1) seeds the sampling starts of PointNet++ and PointConv.  --model pointnet is refused with a
pointer to ``ifdefense_amd.perturb_attack``.  The refusals, and how the loss scale, the start noise and the starts are taken from
the file so that the clouds written do not depend on --batch_size: ifdefense_amd.victim_atk_cli.  The gradient is the one of the
network with its index tables held fixed (include/ifd_dgcnn_atk.h, ifd_pn2_atk.h, ifd_pc_atk.h).
"""
from __future__ import annotations

import sys

import numpy as np

from . import attack_cli as C
from . import victim_atk_cli as V
from .perturb_attack import build_parser, save_path

PROG = 'victim_perturb_attack'


def main(argv=None, make_classifier=None) -> int:
    from .attack import CWPerturb
    args = V.add_victim_flags(build_parser()).parse_args(argv)
    if V.refuse_victim(PROG, args, 'perturb_attack'):
        return 2
    if args.binary_step < 1 or args.num_iter < 1:
        print("{}: --binary_step and --num_iter must be at least 1".format(PROG), file=sys.stderr)
        return 2
    print(args)
    npz = np.load(args.data_root)
    data = C.load_points(npz, args.num_points)
    label, target = C.load_labels(npz)
    if V.refuse_clouds(PROG, args, data.shape[1]):
        return 2
    classifier = V.open_victim(args, make_classifier, [data.shape[1]] * len(data))
    try:
        attacker = CWPerturb(classifier, args.adv_func, 'l2', attack_lr=args.attack_lr, init_weight=10., max_weight=80.,
                             binary_step=args.binary_step, num_iter=args.num_iter, kappa=args.kappa, seed=args.seed,
                             ref_batch=len(data), verbose=args.verbose)
        adv, num = V.run_file(attacker, classifier, data, target, args.batch_size,
                              lambda a, n: V.file_noise(args.seed, data.shape, args.binary_step, a, n))
    finally:
        C.close_classifier(classifier)
    rate = float(num) / float(len(data))
    d, name = save_path(args.out_dir, args.dataset, args.num_points, args.model, args.adv_func, args.kappa, rate,
                        0 if args.local_rank < 0 else args.local_rank)
    C.save_npz(d, name, adv, label, target)
    return 0


if __name__ == '__main__':
    sys.exit(main())
