"""Accuracy and attack success rate of a victim model on a (restored) cloud file - MI355X build of baselines/inference.py.

Same flags, rules and printed lines as the reference CLI (baselines/inference.py:86-205):

    python -m ifdefense_amd.inference --data_root=path/to/file.npz --mode=target --model=pointnet --model_path=pointnet.pth

Only the PointNet victim runs here; --model pointnet2 | dgcnn | pointconv (or a path that names one of them) is refused with
a message and a non-zero status (DGCNN and PointNet++ have CLIs of their own, ifdefense_amd.dgcnn_inference and
ifdefense_amd.pointnet2_inference).  --model_path: the victim checkpoint (.pth saved from nn.DataParallel, or an .npz of its
arrays); empty means BEST_WEIGHTS[dataset][1024][model] of baselines/config.py, relative to the working directory.

Differences from the reference: the whole file runs through the classifier in one call (PointNet has no cross-cloud
operation, so --batch_size is accepted and changes nothing), and ragged SOR files - object arrays of [N_i,3] clouds, which the
reference feeds one cloud at a time - are padded into one batch.  Additions: --seed (accepted for symmetry with the other CLIs:
evaluation draws nothing) and --device.
"""
from __future__ import annotations

import argparse
import sys
from typing import Optional

import numpy as np

MODELS = ('dgcnn', 'pointconv', 'pointnet2', 'pointnet')          # the order get_model_name tests them in
DATASETS = ('mn40', 'remesh_mn40', 'opt_mn40', 'conv_opt_mn40')


def str2bool(v) -> bool:
    if isinstance(v, bool):
        return v
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


def build_parser():
    parser = argparse.ArgumentParser(description='Point Cloud Recognition')
    parser.add_argument('--data_root', type=str, default='')
    parser.add_argument('--mode', type=str, default='normal', choices=['normal', 'target'], help='Testing mode')
    parser.add_argument('--model', type=str, default='', metavar='MODEL', choices=['pointnet', 'pointnet2', 'dgcnn', 'pointconv', ''],
                        help='Model to use, [pointnet, pointnet++, dgcnn, pointconv]. If not specified, judge from data_root')
    parser.add_argument('--dataset', type=str, default='mn40', metavar='N', choices=list(DATASETS))
    parser.add_argument('--normalize_pc', type=str2bool, default=False, help='normalize each cloud before the model')
    parser.add_argument('--batch_size', type=int, default=-1, metavar='BS', help='accepted; results do not depend on it')
    parser.add_argument('--num_points', type=int, default=1024, help='num of points to use')
    parser.add_argument('--emb_dims', type=int, default=1024, metavar='N', help='Dimension of embeddings (unused by PointNet)')
    parser.add_argument('--feature_transform', type=str2bool, default=False, help='whether to use STN on features in PointNet')
    parser.add_argument('--k', type=int, default=20, metavar='N', help='Num of nearest neighbors to use (unused by PointNet)')
    parser.add_argument('--model_path', type=str, default='', help='Model weight to load, use config if not specified')
    parser.add_argument('--seed', type=int, default=1, help='accepted; evaluation draws nothing')
    parser.add_argument('--device', type=str, default='cuda:0')
    return parser


def get_model_name(npz_path: str) -> Optional[str]:
    """The victim model named by a file path (inference.py:17-28); None where the reference gives up."""
    low = npz_path.lower()
    for name in MODELS:
        if name in low:
            return name
    return None


def points_to_take(data_root: str, num_points: int) -> int:
    """Rows taken from each cloud (inference.py:126-149): files of the adding attacks hold 512 / 3*32 / 3*64 more points."""
    low = data_root.lower()
    if num_points == 1024:
        if 'add' in low:
            return 1024 + 512
        if 'cluster' in low:
            return 1024 + 3 * 32
        if 'object' in low:
            return 1024 + 3 * 64
    return num_points


def default_weight_path(dataset: str, model: str) -> str:
    """BEST_WEIGHTS[dataset][1024][model] (baselines/config.py:4-41)."""
    return 'pretrain/{}/{}.pth'.format(dataset, model)


def normalize_points_np(points: np.ndarray) -> np.ndarray:
    """Centre on the centroid, scale the farthest point to norm 1 (baselines/util/pointnet_utils.py:107-113), in the
    input's own dtype."""
    points = points - np.mean(points, axis=0)[None, :]
    dist = np.max(np.sqrt(np.sum(points ** 2, axis=1)), 0)
    points = points / dist
    assert np.sum(np.isnan(points)) == 0
    return points


def evaluate_npz(path: str, classifier, mode: str = 'normal', num_points: int = 1024, normalize: bool = False) -> dict:
    """Run every cloud of an .npz (test_pc, test_label and, in target mode, target_label) through ``classifier`` (anything
    with runtime.Classifier's predict).  Each cloud contributes pc[:num_points, :3] (dataset/ModelNet40.py:138).  Returns
    {"n", "accuracy", "success_rate" (None in normal mode), "pred"}; accuracy = correct / n over the whole file, which is the
    reference's size-weighted mean of per-batch accuracies."""
    if mode not in ('normal', 'target'):
        raise ValueError("mode must be 'normal' or 'target'")
    npz = np.load(path, allow_pickle=True)              # SOR files hold an object array of ragged clouds
    if mode == 'target' and 'target_label' not in npz.files:
        raise KeyError("%s has no target_label: target mode needs one" % path)
    data, label = npz['test_pc'], np.asarray(npz['test_label']).astype(np.int64).reshape(-1)
    clouds = [np.asarray(data[i], dtype=np.float32)[:num_points, :3] for i in range(len(data))]
    if len(clouds) != len(label):
        raise ValueError("%s: %d clouds but %d labels" % (path, len(clouds), len(label)))
    if normalize:
        clouds = [normalize_points_np(c) for c in clouds]
    pred = classifier.predict(clouds)
    pred = np.asarray(pred.detach().cpu() if hasattr(pred, "detach") else pred).astype(np.int64).reshape(-1)
    out = {"n": len(label), "accuracy": float((pred == label).sum()) / len(label), "success_rate": None, "pred": pred}
    if mode == 'target':
        target = np.asarray(npz['target_label']).astype(np.int64).reshape(-1)
        out["success_rate"] = float((pred == target).sum()) / len(label)
    return out


def print_result(mode: str, r: dict) -> None:
    """The reference's closing line (baselines/inference.py:198-205) for evaluate_npz's result."""
    if mode == 'normal':
        print('Overall accuracy: {:.4f}'.format(r["accuracy"]))
    else:
        print('Overall accuracy: {:.4f}, '
              'attack success rate: {:.4f}'.
              format(r["accuracy"], r["success_rate"]))


class ClosesClassifier:
    """Base of the CLIs' wrappers around a classifier's predict(): closing the wrapper closes what it wraps."""

    def __init__(self, classifier):
        self.classifier = classifier

    def close(self):
        if hasattr(self.classifier, "close"):
            self.classifier.close()


def run_victim_cli(prog: str, args, classifier, num_points: int, size_error=None) -> int:
    """The tail every victim's CLI shares: evaluate args.data_root with ``classifier``, close it, print the reference's closing
    line.  A file without the labels the mode needs, or (``size_error``: the exception the CLI's wrapper raises) with a cloud
    the victim cannot take, is refused in ``prog``'s name with status 2."""
    try:
        r = evaluate_npz(args.data_root, classifier, args.mode, num_points, args.normalize_pc)
    except KeyError as e:
        print("{}: {}".format(prog, e.args[0] if e.args else e), file=sys.stderr)
        return 2
    except (size_error or ()) as e:
        print("{}: {}: {}".format(prog, args.data_root, e), file=sys.stderr)
        return 2
    finally:
        if hasattr(classifier, "close"):
            classifier.close()
    print_result(args.mode, r)
    return 0


def main(argv=None, make_classifier=None) -> int:
    args = build_parser().parse_args(argv)
    if not args.model:
        args.model = get_model_name(args.data_root)
        if args.model is None:
            print('Victim model not recognized!', file=sys.stderr)
            return 2
    if args.model.lower() != 'pointnet':
        own = {'dgcnn': "`python -m ifdefense_amd.dgcnn_inference`", 'pointnet2': "`python -m ifdefense_amd.pointnet2_inference`"}
        where = own.get(args.model.lower(), "the reference's baselines/inference.py")
        print("inference: the {} victim is not built here (only pointnet is); evaluate it with {}".format(args.model, where),
              file=sys.stderr)
        return 2
    num_points = points_to_take(args.data_root, args.num_points)
    if make_classifier is None:
        def make_classifier(model, feature_transform, model_path):
            from .runtime import Classifier
            from .weights import load_checkpoint
            return Classifier(load_checkpoint(model_path, model, feature_transform), model, feature_transform, device=args.device)
    model_path = args.model_path or default_weight_path(args.dataset, args.model)
    return run_victim_cli("inference", args, make_classifier(args.model, args.feature_transform, model_path), num_points)


if __name__ == '__main__':
    sys.exit(main())
