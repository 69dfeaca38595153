"""What the attack scripts (fgm_attack, perturb_attack, knn_attack, add_attack, drop_attack, cluster_attack, object_attack) share: the reference's common flags, the two
refusals, the data file, the victim, the batch loop and the result file.  Each script adds its own flags between ``parser_head``
and ``parser_tail``, so ``print(args)`` lists them in the reference's order."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

from .inference import DATASETS, default_weight_path, normalize_points_np, str2bool


def parser_head(kappa=0., adv=True):
    """--data_root ... --kappa; adv=False: up to --k (the untargeted drop script has neither --adv_func nor --kappa)."""
    parser = argparse.ArgumentParser(description='Point Cloud Recognition')
    parser.add_argument('--data_root', type=str, default='data/attack_data.npz')
    parser.add_argument('--model', type=str, default='pointnet', metavar='N', choices=['pointnet', 'pointnet2', 'dgcnn', 'pointconv'])
    parser.add_argument('--feature_transform', type=str2bool, default=False)
    parser.add_argument('--dataset', type=str, default='mn40', metavar='N', choices=list(DATASETS))
    parser.add_argument('--batch_size', type=int, default=-1, metavar='BS', help="the reference's batch (loss mean); -1: the whole file")
    parser.add_argument('--num_points', type=int, default=1024)
    parser.add_argument('--emb_dims', type=int, default=1024, help='unused by PointNet')
    parser.add_argument('--k', type=int, default=20, help='unused by PointNet')
    if adv:
        parser.add_argument('--adv_func', type=str, default='logits', choices=['logits', 'cross_entropy'])
        parser.add_argument('--kappa', type=float, default=kappa)
    return parser


def parser_tail(parser, verbose=True, local_rank=True, seed=True):
    """--local_rank ... --out_dir, and --verbose where the script has the two loop forms; local_rank=False, seed=False: without
    those two (the drop script is single-process and draws no noise)."""
    if local_rank:
        parser.add_argument('--local_rank', default=-1, type=int, help='accepted; only names the output file')
    parser.add_argument('--model_path', type=str, default='')
    if seed:
        parser.add_argument('--seed', type=int, default=1)
    parser.add_argument('--device', type=str, default='cuda:0')
    parser.add_argument('--out_dir', type=str, default='.')
    if verbose:
        parser.add_argument('--verbose', type=str2bool, default=False)
    return parser


def refuse_unbuilt(prog, args) -> int:
    """2 behind a message where args ask for a victim that is not built, else 0."""
    if args.model.lower() != 'pointnet':
        print("{}: the {} victim is not built here (only pointnet is)".format(prog, args.model), file=sys.stderr)
        return 2
    if args.feature_transform:
        print("{}: input gradients through the feature transform are not built here (--feature_transform false only)".format(prog),
              file=sys.stderr)
        return 2
    return 0


def load_points(npz, num_points):
    """-> [N,K,3] float32: every cloud's first num_points points, normalised to the unit sphere."""
    return np.stack([normalize_points_np(np.asarray(c, dtype=np.float32)[:num_points, :3]) for c in npz['test_pc']])


def load_labels(npz):
    return np.asarray(npz['test_label']).reshape(-1), np.asarray(npz['target_label']).reshape(-1)


def open_classifier(args, make_classifier=None):
    if make_classifier is None:
        def make_classifier(model, feature_transform, model_path):
            from .runtime import Classifier
            from .weights import load_checkpoint
            return Classifier(load_checkpoint(model_path, model, feature_transform), model, feature_transform, device=args.device)
    model_path = args.model_path or default_weight_path(args.dataset, args.model)
    print('Loading weight {}'.format(model_path))
    return make_classifier(args.model, False, model_path)


def close_classifier(classifier):
    if hasattr(classifier, "close"):
        classifier.close()


def run_batches(attacker, data, target, batch_size, on_batch=None):
    """-> (adversarial clouds of the whole file, successes): attack() returns (..., clouds, success_num).  ``on_batch(a, n)``,
    where given, is told the offset and the size of every batch before it is attacked."""
    bs = len(data) if batch_size < 1 else batch_size
    adv, num = [], 0
    for a in range(0, len(data), bs):
        if on_batch is not None:
            on_batch(a, len(data[a:a + bs]))
        *_, pc, n_ok = attacker.attack(data[a:a + bs], target[a:a + bs].astype(np.int64))
        adv.append(pc)
        num += n_ok
    return np.concatenate(adv, axis=0), num


def save_npz(d, name, adv, label, target):
    os.makedirs(d, exist_ok=True)
    np.savez(os.path.join(d, name), test_pc=adv.astype(np.float32), test_label=label.astype(np.uint8), target_label=target.astype(np.uint8))


def run_attack(args, make_classifier, make_attacker, name_file) -> int:
    """A script's main behind its own refusals (add_attack, cluster_attack, object_attack): print(args), the data, the victim, the
    batches, the result file.  make_attacker(classifier) -> the attacker, or None behind a message of its own (status 2);
    name_file(success_rate, rank) -> (directory, file name)."""
    print(args)
    npz = np.load(args.data_root)
    data = load_points(npz, args.num_points)
    label, target = load_labels(npz)
    classifier = open_classifier(args, make_classifier)
    try:
        attacker = make_attacker(classifier)
        if attacker is None:
            return 2
        adv, num = run_batches(attacker, data, target, args.batch_size)
    finally:
        close_classifier(classifier)
    d, name = name_file(float(num) / float(len(data)), 0 if args.local_rank < 0 else args.local_rank)
    save_npz(d, name, adv, label, target)
    return 0
