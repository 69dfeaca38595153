"""Accuracy and attack success rate of the DGCNN victim on a (restored) cloud file - MI355X build of baselines/inference.py
with --model dgcnn.

    python -m ifdefense_amd.dgcnn_inference --data_root=path/to/file-dgcnn-x.npz --mode=target --model_path=dgcnn.pth

The flags, the num-points rules, the evaluation and the printed lines are those of ifdefense_amd.inference (imported, not
repeated); the model comes from --model or from the file's path, and anything but dgcnn is refused with a pointer to
ifdefense_amd.inference (and to ifdefense_amd.pointnet2_inference).  --k is honoured (1 .. 32); --emb_dims other than 1024 is refused.  --model_path: the checkpoint
(.pth saved from nn.DataParallel, or an .npz of its arrays); empty means pretrain/{dataset}/dgcnn.pth.  A file that holds a
cloud of fewer than k points is refused with a message (the reference's topk raises there), as is one of more than 2048.
"""
from __future__ import annotations

import sys

import numpy as np

from .inference import ClosesClassifier, build_parser, default_weight_path, get_model_name, points_to_take, run_victim_cli

MAX_POINTS = 2048


class _CloudSizeError(ValueError):
    pass


class _SizeChecked(ClosesClassifier):
    """predict() of the wrapped classifier behind the check of the clouds' sizes, so that a file the library would refuse is
    refused with the words of this CLI."""

    def __init__(self, classifier, k: int):
        super().__init__(classifier)
        self.k = k

    def predict(self, clouds):
        sizes = np.array([len(c) for c in clouds])
        if (sizes < self.k).any():
            i = int(np.argmax(sizes < self.k))
            raise _CloudSizeError("cloud %d has %d points, fewer than k = %d: DGCNN needs k neighbours for every point"
                                  % (i, int(sizes[i]), self.k))
        if (sizes > MAX_POINTS).any():
            i = int(np.argmax(sizes > MAX_POINTS))
            raise _CloudSizeError("cloud %d has %d points, more than the %d the DGCNN victim takes" % (i, int(sizes[i]), MAX_POINTS))
        return self.classifier.predict(clouds)


def main(argv=None, make_classifier=None) -> int:
    args = build_parser().parse_args(argv)
    if not args.model:
        args.model = get_model_name(args.data_root)
        if args.model is None:
            print('Victim model not recognized!', file=sys.stderr)
            return 2
    if args.model.lower() != 'dgcnn':
        print("dgcnn_inference: only the dgcnn victim runs here, not {}; pointnet is evaluated by "
              "`python -m ifdefense_amd.inference`, pointnet2 by `python -m ifdefense_amd.pointnet2_inference`".format(args.model),
              file=sys.stderr)
        return 2
    if args.emb_dims != 1024:
        print("dgcnn_inference: only --emb_dims 1024 is built, got {}".format(args.emb_dims), file=sys.stderr)
        return 2
    if not 1 <= args.k <= 32:
        print("dgcnn_inference: --k must lie in [1, 32], got {}".format(args.k), file=sys.stderr)
        return 2
    num_points = points_to_take(args.data_root, args.num_points)
    if make_classifier is None:
        def make_classifier(model, k, model_path):
            from .runtime import DgcnnClassifier
            from .weights import load_checkpoint
            return DgcnnClassifier(load_checkpoint(model_path, model), k=k, device=args.device)
    model_path = args.model_path or default_weight_path(args.dataset, 'dgcnn')
    classifier = _SizeChecked(make_classifier('dgcnn', args.k, model_path), args.k)
    return run_victim_cli("dgcnn_inference", args, classifier, num_points, _CloudSizeError)


if __name__ == '__main__':
    sys.exit(main())
