"""Targeted FGM / I-FGM / MI-FGM / PGD attack on the PointNet victim - MI355X build of baselines/attack_scripts/targeted_fgm_attack.py.

    python -m ifdefense_amd.fgm_attack --data_root=data/attack_data.npz --attack_type=ifgm --model_path=pointnet.pth

Same flags and rules as the reference's script: budget *= sqrt(num_points * 3), step_size = budget / num_iter, every cloud is
pc[:num_points, :3] normalised to the unit sphere (ModelNet40Attack(normalize=True)), and the result goes to
<out_dir>/attack/results/{dataset}_{num_points}/FGM/{model}/{type}-budget_{delta}-iter_{n}-success_{rate:.4f}-rank_{r}.npz
with test_pc float32 and test_label / target_label uint8 - a file the defenses and ``ifdefense_amd.inference`` read.

Only the PointNet victim without feature_transform is built; anything else is refused with a message and a non-zero status.
Single process: --local_rank is accepted and only names the file (the reference shards the data over ranks).  --batch_size
B_ref sets the batches the reference's loss is a mean over (scale = 1 / B_ref per batch, the last one smaller).  With -1 the
reference takes MAX_FGM_PERTURB_BATCH[num_points][model] from its config.py; here -1 means one batch of the whole file.  Additions: --model_path
(empty: BEST_WEIGHTS of baselines/config.py), --seed (the start noise, see ``attack``), --device, --out_dir.
"""
from __future__ import annotations

import os
import sys

import numpy as np

from . import attack_cli as C


def build_parser():
    parser = C.parser_head()
    parser.add_argument('--attack_type', type=str, default='FGM', metavar='N')
    parser.add_argument('--budget', type=float, default=0.08)
    parser.add_argument('--num_iter', type=int, default=50)
    parser.add_argument('--mu', type=float, default=1.)
    return C.parser_tail(parser, verbose=False)


def attack_settings(budget: float, num_points: int, num_iter: int):
    """(budget, step_size) of targeted_fgm_attack.py:136-140."""
    b = budget * np.sqrt(num_points * 3)
    return float(b), float(b / float(num_iter))


def save_path(out_dir, dataset, num_points, model, attack_type, delta, num_iter, success_rate, local_rank):
    d = os.path.join(out_dir, 'attack', 'results', '{}_{}'.format(dataset, num_points), 'FGM', model)
    name = '{}-budget_{}-iter_{}-success_{:.4f}-rank_{}.npz'.format(attack_type.lower(), delta, num_iter, success_rate, local_rank)
    return d, name


def attack_file(prog, args, open_classifier, check_data=None, on_batch=None, by_file=False) -> int:
    """The script behind its refusals, shared with dgcnn_fgm_attack and pointnet2_fgm_attack: the settings, the data file, the
    victim that ``open_classifier()`` makes, the batches and the result file.  ``check_data(data)``: a message where the clouds
    [N,K,3] cannot be attacked (status 2, before the victim is made), else None.  ``on_batch(classifier, a, n)``, where given, is
    told the offset in the file and the size of every batch before it is attacked.  ``by_file``: what the batches of a file share
    is taken from the file, as --batch_size -1 takes it - the loss is a mean over the whole file (scale = 1 / N in every batch)
    and the start noise is ONE draw of the file's shape - so that --batch_size only says how many clouds go through the library at
    once and the clouds written do not depend on it.  Without it every batch has its own mean and its own draw, as before."""
    from .attack import ATTACKS
    kind = args.attack_type.lower()
    if kind not in ATTACKS:
        print("{}: unknown --attack_type {} (fgm | ifgm | mifgm | pgd)".format(prog, args.attack_type), file=sys.stderr)
        return 2
    print(args)
    delta = args.budget
    num_iter = int(args.num_iter)
    budget, step_size = attack_settings(args.budget, args.num_points, num_iter)
    npz = np.load(args.data_root)
    data = C.load_points(npz, args.num_points)
    label, target = C.load_labels(npz)
    why = check_data(data) if check_data else None
    if why:
        print("{}: {}".format(prog, why), file=sys.stderr)
        return 2
    classifier = open_classifier()
    try:
        kw = dict(kappa=args.kappa, seed=args.seed)
        if by_file:
            kw['ref_batch'] = len(data)
        if kind == 'fgm':
            attacker = ATTACKS[kind](classifier, args.adv_func, budget, **kw)
        elif kind == 'mifgm':
            attacker = ATTACKS[kind](classifier, args.adv_func, None, budget, step_size, num_iter, args.mu, **kw)
        else:
            attacker = ATTACKS[kind](classifier, args.adv_func, None, budget, step_size, num_iter, **kw)
        if by_file:                                                    # the file's start clouds, then loops that add nothing
            import torch
            data = attacker.start(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))).numpy()
            attacker.start = lambda d: d
        hook = None if on_batch is None else (lambda a, n: on_batch(classifier, a, n))
        adv, num = C.run_batches(attacker, data, target, args.batch_size, hook)
    finally:
        C.close_classifier(classifier)
    rate = float(num) / float(len(data))
    d, name = save_path(args.out_dir, args.dataset, args.num_points, args.model, kind, delta, num_iter, rate, args.local_rank)
    C.save_npz(d, name, adv, label, target)
    return 0


def main(argv=None, make_classifier=None) -> int:
    args = build_parser().parse_args(argv)
    if C.refuse_unbuilt('fgm_attack', args):
        return 2
    return attack_file('fgm_attack', args, lambda: C.open_classifier(args, make_classifier))


if __name__ == '__main__':
    sys.exit(main())
