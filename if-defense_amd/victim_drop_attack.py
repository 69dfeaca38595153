"""Untargeted saliency point-dropping attack on the DGCNN, PointNet++ and PointConv victims - MI355X build of
baselines/attack_scripts/untargeted_drop_attack.py with --model dgcnn | pointnet2 | pointconv.

    python -m ifdefense_amd.victim_drop_attack --model=pointconv --data_root=data/attack_data.npz --num_drop=200 --model_path pointconv.pth

The flags, the settings (rounds of 5, alpha 1), the TRUE labels as targets and the result file are those of
ifdefense_amd.drop_attack (imported, not repeated):
<out_dir>/attack/results/{dataset}_{num_points}/Drop_{num_drop}/Drop-{model}-acc_{acc:.4f}.npz, which
``ifdefense_amd.dgcnn_inference`` / ``pointnet2_inference`` / ``pointconv_inference`` read.  --k is DGCNN's neighbour count
(1 .. 32), not the points dropped per round; --fps_seed (default 1) seeds the sampling starts of PointNet++ and PointConv.
--model pointnet is refused with a pointer to ``ifdefense_amd.drop_attack``.

The clouds shrink while one table of starts serves every round and the closing forward, so the starts are those of the clouds
that are WRITTEN: ``fps_starts(fps_seed, sizes - num_drop)``.  They name rows that every round still has, and {acc} in the file's
name is what the victim's inference CLI reports on that file with the same --fps_seed.  What is left of a cloud,
num_points - num_drop, must still be a cloud the victim takes (DGCNN: k points, PointConv: 32); less is refused with status 2 before
the victim is made.  The other refusals, and why the clouds written do not depend on --batch_size: ifdefense_amd.victim_atk_cli.
"""
from __future__ import annotations

import sys

import numpy as np

from . import attack_cli as C
from . import victim_atk_cli as V
from .drop_attack import ALPHA, DROP_PER_ROUND, build_parser, save_path

PROG = 'victim_drop_attack'


def main(argv=None, make_classifier=None) -> int:
    from .attack import SaliencyDrop
    args = V.add_victim_flags(build_parser()).parse_args(argv)
    if V.refuse_victim(PROG, args, 'drop_attack'):
        return 2
    if not 1 <= args.num_drop < args.num_points <= 2048:
        print("{}: 1 <= --num_drop < --num_points <= 2048 is needed".format(PROG), file=sys.stderr)
        return 2
    if args.num_points - args.num_drop < V.min_points(args):
        print("{}: --num_points {} less --num_drop {} leaves fewer than the {} points the {} victim needs".format(
            PROG, args.num_points, args.num_drop, V.min_points(args), V.VICTIMS[args.model.lower()][0]), file=sys.stderr)
        return 2
    print(args)
    npz = np.load(args.data_root)
    data = C.load_points(npz, args.num_points)
    label, target = C.load_labels(npz)
    left = data.shape[1] - args.num_drop
    if V.refuse_clouds(PROG, args, data.shape[1], written=left):
        return 2
    classifier = V.open_victim(args, make_classifier, [left] * len(data))
    try:
        attacker = SaliencyDrop(classifier, num_drop=args.num_drop, alpha=ALPHA, k=DROP_PER_ROUND, ref_batch=len(data),
                                verbose=args.verbose)
        adv, num = V.run_file(attacker, classifier, data, label, args.batch_size)      # the true labels: the attack is untargeted
    finally:
        C.close_classifier(classifier)
    acc = float(num) / float(len(data))
    d, name = save_path(args.out_dir, args.dataset, args.num_points, args.num_drop, args.model, acc)
    C.save_npz(d, name, adv, label, target)
    return 0


if __name__ == '__main__':
    sys.exit(main())
