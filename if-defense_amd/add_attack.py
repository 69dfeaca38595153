"""Targeted CW point-adding attack on the PointNet victim - MI355X build of baselines/attack_scripts/targeted_add_attack.py.

    python -m ifdefense_amd.add_attack --data_root=data/attack_data.npz --model_path=pointnet.pth --dist_func=chamfer

Same flags and rules as the reference's script: --dist_func chamfer (init_weight 5e3, max_weight 4e4) or hausdorff (2e2, 9e2),
--num_add points are added (512), every cloud is pc[:num_points, :3] normalised to the unit sphere
(ModelNet40Attack(normalize=True)), and the result goes to
<out_dir>/attack/results/{dataset}_{num_points}/Add/{dist_func}/Add-{model}-{adv_func}-success_{rate:.4f}-rank_{r}.npz
({adv_func}: logits_kappa={kappa} or cross_entropy) with test_pc float32 [N, num_points + num_add, 3] - the original cloud, then
the added points - and test_label / target_label uint8: a file the defenses and ``ifdefense_amd.inference`` read.

Only the PointNet victim without feature_transform is built; anything else is refused with a message and a non-zero status.
Single process: --local_rank is accepted and only names the file, as rank 0 when it is left at -1 (the reference shards the data
over ranks).  --batch_size B_ref sets the batches the reference's losses are a mean over (scale = 1 / B_ref per batch, the last
one smaller) and the batches the start noise is drawn for.  With -1 the reference takes MAX_PERTURB_BATCH[num_points][model] from
its config.py; here -1 means one batch of the whole file.  Additions: --model_path (empty: BEST_WEIGHTS of baselines/config.py),
--seed (the start noise, see ``attack.CWAdd``), --device, --out_dir, --verbose (the reference's progress lines, loop driven
from the host; default: the whole loop in one library call).
"""
from __future__ import annotations

import os
import sys

from . import attack_cli as C


def build_parser():
    parser = C.parser_head()
    parser.add_argument('--dist_func', type=str, default='chamfer', choices=['chamfer', 'hausdorff'])
    parser.add_argument('--num_add', type=int, default=512, metavar='N')
    parser.add_argument('--attack_lr', type=float, default=1e-2)
    parser.add_argument('--binary_step', type=int, default=10, metavar='N')
    parser.add_argument('--num_iter', type=int, default=500, metavar='N')
    return C.parser_tail(parser)


WEIGHTS = {'chamfer': (5e3, 4e4), 'hausdorff': (2e2, 9e2)}        # targeted_add_attack.py:143-150: init_weight, max_weight


def save_path(out_dir, dataset, num_points, dist_func, model, adv_func, kappa, success_rate, local_rank):
    """targeted_add_attack.py:175-183."""
    d = os.path.join(out_dir, 'attack', 'results', '{}_{}'.format(dataset, num_points), 'Add', dist_func)
    if adv_func == 'logits':
        adv_func = 'logits_kappa={}'.format(kappa)
    return d, 'Add-{}-{}-success_{:.4f}-rank_{}.npz'.format(model, adv_func, success_rate, local_rank)


def main(argv=None, make_classifier=None) -> int:
    from .attack import CWAdd
    args = build_parser().parse_args(argv)
    if C.refuse_unbuilt('add_attack', args):
        return 2
    if args.binary_step < 1 or args.num_iter < 1:
        print("add_attack: --binary_step and --num_iter must be at least 1", file=sys.stderr)
        return 2
    if not 1 <= args.num_add <= 1024 or not args.num_add <= args.num_points <= 2048:
        print("add_attack: 1 <= --num_add <= 1024 and --num_add <= --num_points <= 2048 are needed", file=sys.stderr)
        return 2
    init_w, upper_w = WEIGHTS[args.dist_func]
    return C.run_attack(
        args, make_classifier,
        lambda classifier: CWAdd(classifier, args.adv_func, args.dist_func, attack_lr=args.attack_lr, init_weight=init_w, max_weight=upper_w,
                                 binary_step=args.binary_step, num_iter=args.num_iter, num_add=args.num_add, kappa=args.kappa,
                                 seed=args.seed, verbose=args.verbose),
        lambda rate, rank: save_path(args.out_dir, args.dataset, args.num_points, args.dist_func, args.model, args.adv_func, args.kappa,
                                     rate, rank))


if __name__ == '__main__':
    sys.exit(main())
