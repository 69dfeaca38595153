"""Baseline defenses SRS, SOR and DUP-Net on a GPU - MI355X build of baselines/defend_npz.py.

Same flags, defaults and .npz in/out as the reference CLI (baselines/defend_npz.py:13-108):

    python -m ifdefense_amd.defend_npz --data_root=path/to/adv_data.npz [--defense srs|sor|dup] --pu_weight=pu-in_1024-up_4.pth

Output: <dir of input>/<defense>/<defense>_<file name> with test_pc, and test_label / target_label as uint8.  SOR keeps a
different number of points per cloud, so its test_pc is an object array of [N_i, 3] float32 clouds (load it with
allow_pickle=True, as baselines/dataset/ModelNet40.py:10 does); a regular [B, N, 3] float32 array otherwise.

Additions: --seed (the draws are counter-based, keyed by the seed and the cloud's row in the file; the reference is
unseeded) and --pu_weight (the PU-Net checkpoint, .pth or .npz of its arrays; the reference reads config.PU_NET_WEIGHT).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List

import numpy as np

DEFENSES = ("srs", "sor", "dup")
BATCH = 512                      # clouds per call of the defender (the library chunks further)


def build_parser():
    parser = argparse.ArgumentParser(description='Point Cloud Recognition')
    parser.add_argument('--data_root', type=str, default='', help='the npz data to defend')
    parser.add_argument('--defense', type=str, default='', choices=['', 'srs', 'sor', 'dup'],
                        help='Defense method for input processing, apply all if not specified')
    parser.add_argument('--srs_drop_num', type=int, default=500, help='Number of point dropping in SRS')
    parser.add_argument('--sor_k', type=int, default=2, help='KNN in SOR')
    parser.add_argument('--sor_alpha', type=float, default=1.1, help='Threshold = mean + alpha * std')
    parser.add_argument('--seed', type=int, default=0, help='seed of the counter-based random draws')
    parser.add_argument('--pu_weight', type=str, default='', help='PU-Net checkpoint (pu-in_1024-up_4.pth or .npz), needed by dup')
    return parser


def defense_list(defense: str) -> List[str]:
    """'' means all three, in the reference's order (defend_npz.py:85-88)."""
    return list(DEFENSES) if defense == '' else [defense]


def save_path(data_root: str, one_defense: str) -> str:
    """<dir of input>/<defense>/<defense>_<file name> (defend_npz.py:15-21)."""
    folder, name = os.path.split(data_root)
    return os.path.join(folder, one_defense, '{}_{}'.format(one_defense, name))


def input_files(data_root: str) -> List[str]:
    """A directory input means every regular file in it (defend_npz.py:93-100)."""
    if os.path.isdir(data_root):
        return [os.path.join(data_root, f) for f in os.listdir(data_root) if os.path.isfile(os.path.join(data_root, f))]
    return [data_root]


def assemble_test_pc(clouds: List[np.ndarray]) -> np.ndarray:
    """np.array(list of clouds) of the reference (defend_npz.py:69): [B, N, 3] float32 when every cloud has the same
    shape, else a 1-D object array of the clouds (built explicitly: NumPy 2 refuses the ragged np.array call)."""
    clouds = [np.asarray(c, dtype=np.float32) for c in clouds]
    if len({c.shape for c in clouds}) <= 1:
        return np.array(clouds, dtype=np.float32)
    out = np.empty(len(clouds), dtype=object)
    for i, c in enumerate(clouds):
        out[i] = c
    return out


def defend_array(test_pc: np.ndarray, one_defense: str, args, defender) -> np.ndarray:
    """The defended test_pc of one file.  defender: a runtime.DupNet (or anything with its srs / sor / dup methods)."""
    import torch
    out: List[np.ndarray] = []
    for a in range(0, len(test_pc), BATCH):
        pc = torch.from_numpy(np.ascontiguousarray(test_pc[a:a + BATCH][..., :3], dtype=np.float32))
        if one_defense == 'srs':
            r = defender.srs(pc, drop_num=args.srs_drop_num, cloud_index_base=a)
        elif one_defense == 'sor':
            r = defender.sor(pc, k=args.sor_k, alpha=args.sor_alpha)
        else:
            r = defender.dup(pc, k=args.sor_k, alpha=args.sor_alpha, cloud_index_base=a)
        out += [t.detach().cpu().numpy().astype(np.float32) for t in r]
    return assemble_test_pc(out)


def defend(data_root: str, one_defense: str, args, defender) -> str:
    path = save_path(data_root, one_defense)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    npz = np.load(data_root)
    test_pc = defend_array(npz['test_pc'], one_defense, args, defender)
    np.savez(path, test_pc=test_pc, test_label=npz['test_label'].astype(np.uint8),
             target_label=npz['target_label'].astype(np.uint8))
    return path


def main(argv=None, make_defender=None) -> int:
    args = build_parser().parse_args(argv)
    todo = defense_list(args.defense)
    if 'dup' in todo and not args.pu_weight:
        print("defend_npz: the dup defense needs the PU-Net weights: pass --pu_weight=path/to/pu-in_1024-up_4.pth",
              file=sys.stderr)
        return 2
    if make_defender is None:
        def make_defender(weights):
            from .runtime import DupNet
            return DupNet(weights, seed=args.seed)
    weights = None
    if 'dup' in todo:
        from .weights import load_checkpoint
        weights = load_checkpoint(args.pu_weight, "punet")
    defender = make_defender(weights)
    for one_defense in todo:
        print('{} defense'.format(one_defense))
        for f in input_files(args.data_root):
            defend(f, one_defense, args, defender)
    return 0


if __name__ == '__main__':
    sys.exit(main())
