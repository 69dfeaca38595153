"""Comparison logic of the victim classifier's prediction tests, shared by tests/test_gpu_cls_varied.py (which feeds it the
GPU's outputs) and tests/test_cls_varied_cpu.py (which feeds it wrong answers made from the oracle and expects a refusal).

MARGIN_FACTOR: a prediction is compared with the float64 oracle's where the oracle's top-2 margin is at least 8 e_32,
e_32 = max |float32 oracle - float64 oracle| over the logits.  The 8 is derived: the logits are held to |GPU - f64| <= 4 e_32, so
each of the two leading logits may move by 4 e_32 and a margin of 8 e_32 or more cannot change sign."""
import numpy as np
import torch

MARGIN_FACTOR = 8
MAX_EXCLUDED_SHARE = 0.01
MIN_CLASSES = 15


def oracle_logits_pair(sd, x, n_points=None, chunk=4):
    """(float32, float64) logits of pointnet_oracle.forward; x: [B,N,3] (run in chunks) or a list of ragged clouds."""
    import pointnet_oracle as PO
    out = []
    for dt in (torch.float32, torch.float64):
        W = PO.to_torch(sd, dt)
        if isinstance(x, list) or n_points is not None:
            out.append(PO.forward(W, x, n_points, dtype=dt)[0])
        else:
            out.append(torch.cat([PO.forward(W, x[a:a + chunk], dtype=dt)[0] for a in range(0, len(x), chunk)]))
    return out


def e32_of(lo32, lo64):
    return float((lo32.double() - lo64).abs().max())


def top2_margin(lo64):
    top = torch.sort(lo64, dim=1).values
    return (top[:, -1] - top[:, -2]).numpy()


def check_pred_against_f64(pred, lo64, e_32, what=""):
    """pred [B] == argmax of the float64 logits on every cloud whose float64 top-2 margin is >= 8 e_32; at most 1 % of the clouds
    may fall below that margin, and pred must take at least 15 distinct values.  -> (clouds excluded, classes predicted)."""
    pred = np.asarray(pred).astype(np.int64).reshape(-1)
    close = top2_margin(lo64) < MARGIN_FACTOR * e_32
    want = lo64.argmax(1).numpy()
    n_classes = len(set(pred.tolist()))
    print("%s: e_32 %.3e, clouds excluded for a top-2 margin below %d e_32: %d of %d, classes predicted: %d (f64 oracle: %d)"
          % (what, e_32, MARGIN_FACTOR, int(close.sum()), len(pred), n_classes, len(set(want.tolist()))))
    assert len(pred) == len(want)
    assert close.sum() <= MAX_EXCLUDED_SHARE * len(pred), what
    wrong = np.nonzero((pred != want) & ~close)[0]
    assert wrong.size == 0, (what, wrong[:10], pred[wrong[:10]], want[wrong[:10]])
    assert n_classes >= MIN_CLASSES, (what, n_classes)
    return int(close.sum()), n_classes


def check_pred_is_argmax(pred, logits, what=""):
    """pred [B] == torch.argmax of these very logits on the CPU (the lowest class among equals), no exclusions."""
    want = torch.argmax(logits.cpu(), 1)
    got = torch.as_tensor(np.asarray(pred)).long().reshape(-1)
    assert got.shape == want.shape and torch.equal(got, want), (what, torch.nonzero(got != want).reshape(-1)[:10])


def check_same_permutation(logits, pred, perm, logits_p, pred_p, what=""):
    """A run on x[perm] must give logits[perm] and pred[perm], bitwise."""
    perm = torch.as_tensor(np.asarray(perm)).long()
    assert torch.equal(logits_p, logits[perm]), what
    assert torch.equal(torch.as_tensor(np.asarray(pred_p)).long(), torch.as_tensor(np.asarray(pred)).long()[perm]), what


def check_ties(logits, pred, what=""):
    """Under pointnet_oracle.make_tied_weights: classes 20..39 repeat classes 0..19 bit for bit, so the argmax rule alone decides
    between each pair, and it must pick the lower class."""
    logits = logits.cpu()
    assert torch.equal(logits[:, 20:], logits[:, :20]), what
    got = torch.as_tensor(np.asarray(pred)).long().reshape(-1)
    assert bool((got < 20).all()), (what, got[got >= 20][:10])
    check_pred_is_argmax(got, logits, what)
