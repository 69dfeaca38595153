"""Do two builds of libifd.so compute the three victim classifiers bit for bit alike?

    python scripts/ab_victims.py libA.so libB.so

Each library runs in a fresh child process of its own (IFD_LIB): PointNet (with and without feature_transform), DGCNN and
PointNet++ under seeded dense weights, at the sizes where the code they share can go wrong - one cloud, a ragged batch with NaN
beyond the counts, a batch one cloud above a chunk, a second row tile with one valid row, counts of 1.  The child writes logits,
pred and every aux tensor to an .npz; this process compares the raw bytes of the two files, tensor by tensor, and exits 1 on any
difference."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT_S = 120       # a child needs about 20 s, most of it imports and the creation of the contexts


def clouds(rng, B, stride, counts=None):
    """[B,stride,3] in the unit ball's scale, NaN beyond a cloud's count."""
    pc = (rng.standard_normal((B, stride, 3)) * 0.4).astype(np.float32)
    if counts is None:
        return pc, None
    n = np.resize(np.asarray(counts, np.int32), B)
    for b in range(B):
        pc[b, n[b]:] = np.nan
    return pc, n


def flat(prefix, logits, aux, out):
    out[prefix + "/logits"] = logits.cpu().numpy()
    for k, v in aux.items():
        for i, t in enumerate(v if isinstance(v, list) else [v]):
            out["%s/%s%s" % (prefix, k, i if isinstance(v, list) else "")] = t.cpu().numpy()


def child(path):
    sys.path.insert(0, ROOT)
    import torch
    import ifdefense_amd as I
    lib = I._lib.load()
    rng = np.random.default_rng(20)
    dense = lambda n: (rng.standard_normal(int(n)) * 0.03).astype(np.float32)     # noqa: E731
    out = {}
    for ft in (False, True):
        with I.Classifier(dense(lib.ifd_cls_weight_count(I._lib.CLS_POINTNET, int(ft))), feature_transform=ft) as c:
            for B in (1, 17):
                pc, n = clouds(rng, B, 20, [20, 1, 7] if B > 1 else [1])
                flat("pointnet_ft%d/B%d" % (ft, B), *c.logits(pc, torch.from_numpy(n), want_aux=True), out)
    for k in (1, 20):
        with I.DgcnnClassifier(dense(lib.ifd_dgcnn_weight_count()), k=k) as c:
            for B in (1, 17, 129):                                  # 129: one cloud above a chunk
                pc, n = clouds(rng, B, 64, [33, 20, 64])
                flat("dgcnn_k%d/B%d_n64" % (k, B), *c.logits(pc, torch.from_numpy(n), want_aux=True), out)
            for B in (1, 17):                                       # a second row tile with one valid row
                flat("dgcnn_k%d/B%d_n65" % (k, B), *c.logits(clouds(rng, B, 65)[0], want_aux=True), out)
    with I.PointNet2Classifier(dense(lib.ifd_pn2_weight_count())) as c:
        for B in (1, 17, 129):                                      # 129: one cloud above a chunk
            for n in (1, 33, 513, 1025):
                pc, _ = clouds(rng, B, n)
                start = np.stack([rng.integers(0, n, B), rng.integers(1, 512, B)], 1).astype(np.int32)
                flat("pointnet2/B%d_n%d" % (B, n), *c.logits(pc, fps_start=start, want_aux=True), out)
        pc, n = clouds(rng, 17, 40, [40, 1, 33])                    # ragged
        start = np.stack([np.zeros(17), rng.integers(1, 512, 17)], 1).astype(np.int32)
        flat("pointnet2/B17_ragged", *c.logits(pc, torch.from_numpy(n), fps_start=start, want_aux=True), out)
    np.savez(path, **out)


def main(argv):
    if len(argv) == 3 and argv[1] == "--child":
        child(argv[2])
        return 0
    if len(argv) != 3:
        print(__doc__)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        res = []
        for i, lib in enumerate(argv[1:3]):
            path = os.path.join(tmp, "victims_%d.npz" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True, timeout=CHILD_TIMEOUT_S,
                           env=dict(os.environ, IFD_LIB=os.path.abspath(lib)))
            with np.load(path) as z:
                res.append({k: z[k] for k in z.files})
    a, b = res
    different = sorted(set(a) ^ set(b))
    for key in sorted(set(a) & set(b)):
        same = a[key].shape == b[key].shape and a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes()
        if not same:
            different.append(key)
        print("%-36s %-18s %s" % (key, a[key].shape, "equal" if same else "DIFFERENT"))
    print("%d tensors, %d different" % (len(set(a) | set(b)), len(different)))
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
