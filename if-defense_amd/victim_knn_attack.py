"""Targeted kNN attack on the DGCNN, PointNet++ and PointConv victims - MI355X build of
baselines/attack_scripts/targeted_knn_attack.py with --model dgcnn | pointnet2 | pointconv.

    python -m ifdefense_amd.victim_knn_attack --model=dgcnn --data_root=data/attack_data.npz --model_path=dgcnn.pth

The flags, the settings (kappa 15, attack_lr 1e-3, num_iter 2500, ChamferkNNDist('adv2ori', 5, 1.05, 5., 3.),
ProjectInnerClipLinf(0.1)), the clouds (six columns with normals, or three and the clip alone) and the result file are those of
ifdefense_amd.knn_attack (imported, not repeated):
<out_dir>/attack/results/{dataset}_{num_points}/kNN/kNN-{model}-{adv_func}-success_{rate:.4f}-rank_{r}.npz, which
``ifdefense_amd.dgcnn_inference`` / ``pointnet2_inference`` / ``pointconv_inference`` read.  --k is DGCNN's neighbour count
(1 .. 32), --fps_seed (default 1) seeds the sampling starts of PointNet++ and PointConv.  --model pointnet is refused with a
pointer to ``ifdefense_amd.knn_attack``.  Clouds need 6 points at least, as the attack's five neighbours do.  The refusals, and how
the loss scale, the start noise and the starts are taken from the file so that the clouds written do not depend on --batch_size:
ifdefense_amd.victim_atk_cli.
"""
from __future__ import annotations

import sys

import numpy as np

from . import attack_cli as C
from . import victim_atk_cli as V
from .knn_attack import build_parser, load_clouds, save_path

PROG = 'victim_knn_attack'
KNN_MIN_POINTS = 6


def main(argv=None, make_classifier=None) -> int:
    from .attack import CWKNN
    args = V.add_victim_flags(build_parser()).parse_args(argv)
    if V.refuse_victim(PROG, args, 'knn_attack'):
        return 2
    if args.num_iter < 1:
        print("{}: --num_iter must be at least 1".format(PROG), file=sys.stderr)
        return 2
    print(args)
    npz = np.load(args.data_root)
    data = load_clouds(npz['test_pc'], args.num_points)
    if data.shape[2] not in (3, 6):
        print("{}: clouds must have 6 columns (points and normals) or 3, got {}".format(PROG, data.shape[2]), file=sys.stderr)
        return 2
    if V.refuse_clouds(PROG, args, data.shape[1], floor=KNN_MIN_POINTS):
        return 2
    if data.shape[2] == 3:
        print("{}: the clouds carry no normals: running without the projection of inner points, the clip alone".format(PROG))
    label, target = C.load_labels(npz)
    classifier = V.open_victim(args, make_classifier, [data.shape[1]] * len(data))
    try:
        attacker = CWKNN(classifier, args.adv_func, 'chamfer_knn', 'project_inner_clip_linf', attack_lr=args.attack_lr,
                         num_iter=args.num_iter, kappa=args.kappa, seed=args.seed, ref_batch=len(data), verbose=args.verbose)
        shape = (data.shape[0], data.shape[1], 3)
        adv, num = V.run_file(attacker, classifier, data, target, args.batch_size,
                              lambda a, n: V.file_noise(args.seed, shape, 1, a, n)[0])
    finally:
        C.close_classifier(classifier)
    rate = float(num) / float(len(data))
    d, name = save_path(args.out_dir, args.dataset, args.num_points, args.model, args.adv_func, args.kappa, rate,
                        0 if args.local_rank < 0 else args.local_rank)
    C.save_npz(d, name, adv, label, target)
    return 0


if __name__ == '__main__':
    sys.exit(main())
