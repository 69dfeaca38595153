"""Untargeted saliency point-dropping attack on the PointNet victim - MI355X build of
baselines/attack_scripts/untargeted_drop_attack.py.

    python -m ifdefense_amd.drop_attack --data_root=data/attack_data.npz --num_drop=200 --model_path pointnet.pth

Same flags and rules as the reference's script: --num_drop points are dropped (200) in rounds of 5 with alpha = 1 (the script's
fixed settings), every cloud is pc[:num_points, :3] normalised to the unit sphere (ModelNet40Attack(normalize=True)), the attack is
run against the TRUE labels (test_label), and the result goes to
<out_dir>/attack/results/{dataset}_{num_points}/Drop_{num_drop}/Drop-{model}-acc_{acc:.4f}.npz with test_pc float32
[N, num_points - num_drop, 3] and test_label / target_label uint8: a file the defenses and ``ifdefense_amd.inference`` read.
{acc} is the share of the clouds the victim still classifies correctly.  The surviving points keep their input order (the
reference writes them in topk's order; every reader treats a cloud as a set - include/ifd_drop.h).

Only the PointNet victim without feature_transform is built; anything else is refused with a message and a non-zero status.
--batch_size B_ref sets the batches the reference's loss is a mean over (scale = 1 / B_ref per batch, the last one smaller).  With
-1 the reference takes MAX_DROP_BATCH[num_points][model] from its config.py; here -1 means one batch of the whole file.  --k is
DGCNN's neighbour count, as in the reference (unused by PointNet), not the points dropped per round.  Additions: --model_path
(empty: BEST_WEIGHTS of baselines/config.py), --device, --out_dir, --verbose (the reference's progress lines, rounds driven from
the host; default: the whole attack in one library call).
"""
from __future__ import annotations

import os
import sys

import numpy as np

from . import attack_cli as C

ALPHA, DROP_PER_ROUND = 1, 5         # untargeted_drop_attack.py:109-110, "hyper-parameters from their official tensorflow code"


def build_parser():
    parser = C.parser_head(adv=False)
    parser.add_argument('--num_drop', type=int, default=200, metavar='N')
    return C.parser_tail(parser, local_rank=False, seed=False)


def save_path(out_dir, dataset, num_points, num_drop, model, acc):
    """untargeted_drop_attack.py:127-132."""
    d = os.path.join(out_dir, 'attack', 'results', '{}_{}'.format(dataset, num_points), 'Drop_{}'.format(num_drop))
    return d, 'Drop-{}-acc_{:.4f}.npz'.format(model, acc)


def main(argv=None, make_classifier=None) -> int:
    from .attack import SaliencyDrop
    args = build_parser().parse_args(argv)
    if C.refuse_unbuilt('drop_attack', args):
        return 2
    if not 1 <= args.num_drop < args.num_points <= 2048:
        print("drop_attack: 1 <= --num_drop < --num_points <= 2048 is needed", file=sys.stderr)
        return 2
    print(args)
    npz = np.load(args.data_root)
    data = C.load_points(npz, args.num_points)
    label, target = C.load_labels(npz)
    if data.shape[1] <= args.num_drop:
        print("drop_attack: the file's clouds have {} points, --num_drop {} leaves none".format(data.shape[1], args.num_drop),
              file=sys.stderr)
        return 2
    classifier = C.open_classifier(args, make_classifier)
    try:
        attacker = SaliencyDrop(classifier, num_drop=args.num_drop, alpha=ALPHA, k=DROP_PER_ROUND, verbose=args.verbose)
        adv, num = C.run_batches(attacker, data, label, args.batch_size)       # the true labels: the attack is untargeted
    finally:
        C.close_classifier(classifier)
    acc = float(num) / float(len(data))
    d, name = save_path(args.out_dir, args.dataset, args.num_points, args.num_drop, args.model, acc)
    C.save_npz(d, name, adv, label, target)
    return 0


if __name__ == '__main__':
    sys.exit(main())
