"""Targeted CW object-adding attack on the PointNet victim - MI355X build of baselines/attack_scripts/targeted_add_object_attack.py.

    python -m ifdefense_amd.object_attack --data_root=data/attack_data.npz --obj_root=data/airplane.npy --model_path=pointnet.pth

Same flags and rules as the reference's script: --num_add copies (3) of --obj_num_p points (64) of the object in --obj_root (an
[M,3] .npy file, scaled to 0.3 of the unit sphere) are added, the distance is L2ChamferDist(num_add, 'adv2ori', 0.2) with init_weight
5 and max_weight 40, every cloud is pc[:num_points, :3] normalised to the unit sphere (ModelNet40Attack(normalize=True)), and the
result goes to
<out_dir>/attack/results/{dataset}_{num_points}/Object/{num_add}-{obj_num_p}/Object-{model}-{adv_func}-success_{rate:.4f}-rank_{r}.npz
({adv_func}: logits_kappa={kappa} or cross_entropy) with test_pc float32 [N, num_points + num_add * obj_num_p, 3] - the original
cloud, then the placed objects - and test_label / target_label uint8: a file the defenses and ``ifdefense_amd.inference`` read.

Only the PointNet victim without feature_transform is built; anything else is refused with a message and a non-zero status, as
are --num_points outside [128, 2048] (the centres start from 128 critical points), --num_add * --obj_num_p outside [1, 1024],
--binary_step or --num_iter below 1, and an object file that is missing, is not an [M,3] array or has fewer than --obj_num_p points.
Single process: --local_rank is accepted and only names the file, as rank 0 when it is left at -1.  --batch_size B_ref sets the
batches the reference's losses are a mean over (scale = 1 / B_ref per batch, the last one smaller) and the batches the start draws
are made for; -1 means one batch of the whole file (the reference takes BATCH_SIZE from its config.py).  --seed seeds the object's
shuffles and the centres' fallback draws, as the reference's set_seed does, and the start noise and angles (see
``attack.CWAddObjects``).  Additions: --model_path (empty: BEST_WEIGHTS of baselines/config.py), --device, --out_dir, --verbose (the
reference's progress lines, loop driven from the host; default: the whole loop in one library call).
"""
from __future__ import annotations

import os
import sys

import numpy as np

from . import attack_cli as C


def build_parser():
    parser = C.parser_head()
    parser.add_argument('--attack_lr', type=float, default=1e-2)
    parser.add_argument('--binary_step', type=int, default=5, metavar='N')
    parser.add_argument('--num_iter', type=int, default=500, metavar='N')
    parser.add_argument('--num_add', type=int, default=3, metavar='N')
    parser.add_argument('--obj_num_p', type=int, default=64, metavar='N')
    parser.add_argument('--obj_root', type=str, default='data/airplane.npy')
    return C.parser_tail(parser)


INIT_WEIGHT, MAX_WEIGHT, SCALING = 5., 40., 0.3                    # targeted_add_object_attack.py:157-165


def save_path(out_dir, dataset, num_points, num_add, obj_num_p, model, adv_func, kappa, success_rate, local_rank):
    """targeted_add_object_attack.py:184-192."""
    d = os.path.join(out_dir, 'attack', 'results', '{}_{}'.format(dataset, num_points), 'Object', '{}-{}'.format(num_add, obj_num_p))
    if adv_func == 'logits':
        adv_func = 'logits_kappa={}'.format(kappa)
    return d, 'Object-{}-{}-success_{:.4f}-rank_{}.npz'.format(model, adv_func, success_rate, local_rank)


def load_object(path, obj_num_p):
    """-> the object [M,3] as the file holds it, or None behind a message."""
    try:
        pc = np.load(path)
    except (OSError, ValueError) as e:
        print("object_attack: cannot read --obj_root {}: {}".format(path, e), file=sys.stderr)
        return None
    if not isinstance(pc, np.ndarray) or pc.ndim != 2 or pc.shape[1] != 3 or pc.dtype.kind != 'f' or len(pc) < obj_num_p:
        print("object_attack: --obj_root must hold a float [M,3] array with M >= --obj_num_p", file=sys.stderr)
        return None
    return pc


def main(argv=None, make_classifier=None) -> int:
    from .attack import CWAddObjects
    args = build_parser().parse_args(argv)
    if C.refuse_unbuilt('object_attack', args):
        return 2
    if args.binary_step < 1 or args.num_iter < 1:
        print("object_attack: --binary_step and --num_iter must be at least 1", file=sys.stderr)
        return 2
    if args.num_add < 1 or args.obj_num_p < 1 or not 1 <= args.num_add * args.obj_num_p <= 1024:
        print("object_attack: --num_add >= 1, --obj_num_p >= 1 and 1 <= --num_add * --obj_num_p <= 1024 are needed", file=sys.stderr)
        return 2
    if not 128 <= args.num_points <= 2048:
        print("object_attack: 128 <= --num_points <= 2048 is needed", file=sys.stderr)
        return 2
    object_pc = load_object(args.obj_root, args.obj_num_p)
    if object_pc is None:
        return 2

    def make_attacker(classifier):
        try:
            return CWAddObjects(classifier, object_pc, args.adv_func, "l2_chamfer", attack_lr=args.attack_lr, init_weight=INIT_WEIGHT,
                                max_weight=MAX_WEIGHT, binary_step=args.binary_step, num_iter=args.num_iter, num_add=args.num_add,
                                obj_num_p=args.obj_num_p, scaling=SCALING, kappa=args.kappa, seed=args.seed, verbose=args.verbose)
        except ValueError as e:
            print("object_attack: {}".format(e), file=sys.stderr)
            return None
    return C.run_attack(args, make_classifier, make_attacker,
                        lambda rate, rank: save_path(args.out_dir, args.dataset, args.num_points, args.num_add, args.obj_num_p, args.model,
                                                     args.adv_func, args.kappa, rate, rank))


if __name__ == '__main__':
    sys.exit(main())
