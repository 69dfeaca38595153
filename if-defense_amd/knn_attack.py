"""Targeted kNN attack on the PointNet victim - MI355X build of baselines/attack_scripts/targeted_knn_attack.py.

    python -m ifdefense_amd.knn_attack --data_root=data/attack_data.npz --model_path=pointnet.pth

Same flags and rules as the reference's script: kappa 15, attack_lr 1e-3, num_iter 2500, ChamferkNNDist('adv2ori', 5, 1.05, 5., 3.)
and ProjectInnerClipLinf(0.1); every cloud is pc[:num_points, :6] with columns 0-2 normalised to the unit sphere and columns 3-5,
the normals, left as they are (ModelNet40NormalAttack(normalize=True)), and the result goes to
<out_dir>/attack/results/{dataset}_{num_points}/kNN/kNN-{model}-{adv_func}-success_{rate:.4f}-rank_{r}.npz ({adv_func}:
logits_kappa={kappa} or cross_entropy) with test_pc float32 [N,K,3] and test_label / target_label uint8 - a file the defenses and
``ifdefense_amd.inference`` read.  A file whose clouds have only 3 columns runs without the projection (the clip alone, as the
reference's CWKNN does without normals) and one line says so.

Only the PointNet victim without feature_transform is built; anything else is refused with a message and a non-zero status.
Single process: --local_rank is accepted and only names the file, as rank 0 when it is left at -1.  --batch_size B_ref sets the
batches the reference's losses are a mean over (scale = 1 / B_ref per batch, the last one smaller) and the batches the start noise
is drawn for.  With -1 the reference takes MAX_KNN_BATCH[num_points][model] from its config.py; here -1 means one batch of the whole
file.  Additions: --model_path (empty: BEST_WEIGHTS of baselines/config.py), --seed (the start noise, see ``attack.CWKNN``),
--device, --out_dir, --verbose (the reference's progress lines, loop driven from the host; default: the whole loop in one library
call).
"""
from __future__ import annotations

import os
import sys

import numpy as np

from . import attack_cli as C
from .inference import normalize_points_np


def build_parser():
    parser = C.parser_head(kappa=15.)
    parser.add_argument('--attack_lr', type=float, default=1e-3)
    parser.add_argument('--num_iter', type=int, default=2500, metavar='N')
    return C.parser_tail(parser)


def save_path(out_dir, dataset, num_points, model, adv_func, kappa, success_rate, local_rank):
    """targeted_knn_attack.py:162-170."""
    d = os.path.join(out_dir, 'attack', 'results', '{}_{}'.format(dataset, num_points), 'kNN')
    if adv_func == 'logits':
        adv_func = 'logits_kappa={}'.format(kappa)
    return d, 'kNN-{}-{}-success_{:.4f}-rank_{}.npz'.format(model, adv_func, success_rate, local_rank)


def load_clouds(test_pc, num_points):
    """-> [N,K,6] or [N,K,3] float32: points normalised to the unit sphere, normals as they are."""
    out = []
    for c in test_pc:
        c = np.asarray(c, dtype=np.float32)[:num_points, :6]
        out.append(np.concatenate([normalize_points_np(c[:, :3]), c[:, 3:]], axis=1))
    return np.stack(out)


def main(argv=None, make_classifier=None) -> int:
    from .attack import CWKNN
    args = build_parser().parse_args(argv)
    if C.refuse_unbuilt('knn_attack', args):
        return 2
    if args.num_iter < 1:
        print("knn_attack: --num_iter must be at least 1", file=sys.stderr)
        return 2
    print(args)
    npz = np.load(args.data_root)
    data = load_clouds(npz['test_pc'], args.num_points)
    if data.shape[2] not in (3, 6):
        print("knn_attack: clouds must have 6 columns (points and normals) or 3, got {}".format(data.shape[2]), file=sys.stderr)
        return 2
    if data.shape[2] == 3:
        print("knn_attack: the clouds carry no normals: running without the projection of inner points, the clip alone")
    label, target = C.load_labels(npz)
    classifier = C.open_classifier(args, make_classifier)
    try:
        attacker = CWKNN(classifier, args.adv_func, 'chamfer_knn', 'project_inner_clip_linf', attack_lr=args.attack_lr,
                         num_iter=args.num_iter, kappa=args.kappa, seed=args.seed, verbose=args.verbose)
        adv, num = C.run_batches(attacker, data, target, args.batch_size)
    finally:
        C.close_classifier(classifier)
    rate = float(num) / float(len(data))
    d, name = save_path(args.out_dir, args.dataset, args.num_points, args.model, args.adv_func, args.kappa, rate,
                        0 if args.local_rank < 0 else args.local_rank)
    C.save_npz(d, name, adv, label, target)
    return 0


if __name__ == '__main__':
    sys.exit(main())
