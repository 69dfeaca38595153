"""Targeted CW cluster-adding attack on the PointNet victim - MI355X build of baselines/attack_scripts/targeted_add_cluster_attack.py.

    python -m ifdefense_amd.cluster_attack --data_root=data/attack_data.npz --model_path=pointnet.pth

Same flags and rules as the reference's script: --num_add clusters (3) of --cl_num_p points (32) are added, the distance is
FarChamferDist(num_add, 'adv2ori', 0.1) with init_weight 5 and max_weight 30, every cloud is pc[:num_points, :3] normalised to the
unit sphere (ModelNet40Attack(normalize=True)), and the result goes to
<out_dir>/attack/results/{dataset}_{num_points}/Cluster/{num_add}-{cl_num_p}/Cluster-{model}-{adv_func}-success_{rate:.4f}-rank_{r}.npz
({adv_func}: logits_kappa={kappa} or cross_entropy) with test_pc float32 [N, num_points + num_add * cl_num_p, 3] - the original
cloud, then the added clusters - and test_label / target_label uint8: a file the defenses and ``ifdefense_amd.inference`` read.

Only the PointNet victim without feature_transform is built; anything else is refused with a message and a non-zero status, as
are --num_points outside [128, 2048] (the clusters start from 128 critical points), --num_add * --cl_num_p outside [1, 1024] and
--binary_step or --num_iter below 1.  Single process: --local_rank is accepted and only names the file, as rank 0 when it is left
at -1.  --batch_size B_ref sets the batches the reference's losses are a mean over (scale = 1 / B_ref per batch, the last one
smaller) and the batches the start noise is drawn for; -1 means one batch of the whole file (the reference takes BATCH_SIZE from
its config.py).  --seed seeds the start clusters' numpy draws, as the reference's set_seed does, and the start noise (see
``attack.CWAddClusters``).  Additions: --model_path (empty: BEST_WEIGHTS of baselines/config.py), --device, --out_dir, --verbose (the
reference's progress lines, loop driven from the host; default: the whole loop in one library call).
"""
from __future__ import annotations

import os
import sys

from . import attack_cli as C


def build_parser():
    parser = C.parser_head()
    parser.add_argument('--attack_lr', type=float, default=1e-2)
    parser.add_argument('--binary_step', type=int, default=5, metavar='N')
    parser.add_argument('--num_iter', type=int, default=500, metavar='N')
    parser.add_argument('--num_add', type=int, default=3, metavar='N')
    parser.add_argument('--cl_num_p', type=int, default=32, metavar='N')
    return C.parser_tail(parser)


INIT_WEIGHT, MAX_WEIGHT = 5., 30.                                  # targeted_add_cluster_attack.py:155-157


def save_path(out_dir, dataset, num_points, num_add, cl_num_p, model, adv_func, kappa, success_rate, local_rank):
    """targeted_add_cluster_attack.py:180-188."""
    d = os.path.join(out_dir, 'attack', 'results', '{}_{}'.format(dataset, num_points), 'Cluster', '{}-{}'.format(num_add, cl_num_p))
    if adv_func == 'logits':
        adv_func = 'logits_kappa={}'.format(kappa)
    return d, 'Cluster-{}-{}-success_{:.4f}-rank_{}.npz'.format(model, adv_func, success_rate, local_rank)


def main(argv=None, make_classifier=None) -> int:
    from .attack import CWAddClusters
    args = build_parser().parse_args(argv)
    if C.refuse_unbuilt('cluster_attack', args):
        return 2
    if args.binary_step < 1 or args.num_iter < 1:
        print("cluster_attack: --binary_step and --num_iter must be at least 1", file=sys.stderr)
        return 2
    if args.num_add < 1 or args.cl_num_p < 1 or not 1 <= args.num_add * args.cl_num_p <= 1024:
        print("cluster_attack: --num_add >= 1, --cl_num_p >= 1 and 1 <= --num_add * --cl_num_p <= 1024 are needed", file=sys.stderr)
        return 2
    if not 128 <= args.num_points <= 2048:
        print("cluster_attack: 128 <= --num_points <= 2048 is needed", file=sys.stderr)
        return 2
    return C.run_attack(
        args, make_classifier,
        lambda classifier: CWAddClusters(classifier, args.adv_func, "far_chamfer", attack_lr=args.attack_lr, init_weight=INIT_WEIGHT,
                                         max_weight=MAX_WEIGHT, binary_step=args.binary_step, num_iter=args.num_iter, num_add=args.num_add,
                                         cl_num_p=args.cl_num_p, kappa=args.kappa, seed=args.seed, verbose=args.verbose),
        lambda rate, rank: save_path(args.out_dir, args.dataset, args.num_points, args.num_add, args.cl_num_p, args.model, args.adv_func,
                                     args.kappa, rate, rank))


if __name__ == '__main__':
    sys.exit(main())
