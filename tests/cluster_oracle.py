"""Test oracle of the CW cluster-adding attack (include/ifd_cluster.h): CWAddClusters.attack (baselines/attack/CW/Add_Cluster.py)
with FarChamferDist(num_add, 'adv2ori', 0.1) (baselines/attack/util/dist_utils.py) restated one cloud at a time, in the reference's
own form: the Chamfer part from add_oracle.pairwise (three bmm's, torch.min, torch.mean), the far part from the ``+ 1e-7`` delta
matrix, torch.norm and the two torch.max, autograd for the distance term's gradient, the real torch.optim.Adam on the CPU with
its state put in from outside, the record and the adjustment of cw_oracle.  The adversarial loss, its gradient and the prediction
come from atk_oracle.run_cloud on the concatenated cloud.  Runs in float32 (the reference's rounding) and float64 (the yardstick).

Also here: DBSCAN by the header's definition in numpy (``dbscan``), the reference's host initialisation (``init_centers``, the
library's attack.init_clusters restated from Add_Cluster.py:98-127 on a RandomState), and the teacher-forced step cases with
their judge.

The near-tie: the ordered pairs (i, j) and (j, i) of a cluster differ only through ``+ 1e-7``, |d + e|^2 - |-d + e|^2 = 4e-7 sum_k d_k,
often within float32 rounding of the norms, so which ORDER the arg-max returns is frequently undecidable at float32, and it moves
the far gradient by about 1e-6 relative.  Hence ``step`` takes an optional forced ordered pair per cluster, and ``judge`` decides
from float64 and the float32 oracle's measured error e of a norm alone: the UNORDERED pair (its norm: the larger of its two orders)
is judged where the two largest differ by more than 8 e, the order inside it only where the two orders differ by more than 8 e;
where the order is not judged, the float64 yardstick of whoever is measured is the oracle's step with THAT one's order forced."""
import numpy as np
import torch

import add_oracle as DO
import atk_oracle as AO
import cw_oracle as CO

fresh_record = CO.fresh_record
adjust = CO.adjust
CHAMFER_WEIGHT = 0.1
NUM_CRI, EPS, MIN_SAMPLES = 128, 0.2, 3
BAND = 4 * 2.0 ** -24                                                  # |d^2 - eps^2| inside which float32 decides for itself


# ---------------------------------------------------------------------------------------------- DBSCAN, the header's definition
def dbscan(points, eps=EPS, min_samples=MIN_SAMPLES):
    """points [n,3] float32 -> (labels [n] int32, number of clusters): include/ifd_cluster.h, term by term in float32."""
    p = np.asarray(points, np.float32)
    n = len(p)
    d = p[:, None, :] - p[None, :, :]
    sq = (d * d).astype(np.float32)
    d2 = ((sq[..., 0] + sq[..., 1]).astype(np.float32) + sq[..., 2]).astype(np.float32)
    eps2 = np.float32(np.float32(eps) * np.float32(eps))
    nb = d2 <= eps2
    core = nb.sum(1) >= min_samples
    lab = np.where(core, np.arange(n), n)
    adj = nb & core[None, :] & core[:, None]
    while True:                                                        # min-label propagation to the fixed point
        new = np.where(core, np.where(adj, lab[None, :], n).min(1, initial=n), n)
        new = np.minimum(lab, new)
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.nonzero(core & (lab == np.arange(n)))[0]
    cid = np.full(n + 1, np.iinfo(np.int32).max, np.int64)
    cid[roots] = np.arange(len(roots))
    out = np.full(n, -1, np.int32)
    out[core] = cid[lab[core]]
    for i in np.nonzero(~core)[0]:
        cn = np.nonzero(nb[i] & core)[0]
        if len(cn):
            out[i] = cid[lab[cn]].min()
    return out, len(roots)


def blob_cloud(rng, n=128):
    """A random cloud of 1 to 7 Gaussian blobs with sigma 0.05 to 0.25: what DBSCAN at eps 0.2 splits into clusters and outliers."""
    k = int(rng.integers(1, 8))
    centre = rng.uniform(-0.6, 0.6, (k, 3))
    sigma = rng.uniform(0.05, 0.25, k)
    which = rng.integers(0, k, n)
    return (centre[which] + sigma[which, None] * rng.standard_normal((n, 3))).astype(np.float32)


def border_cloud():
    """-> (points [9,3], labels under min_samples = 4): two clusters of four cores and a border point (row 5) within eps of one core
    of each.  Row 0 belongs to the second group in space, so that group is cluster 0, and the border point's lowest-INDEX core
    neighbour (row 1) is in cluster 1: it must take the lower LABEL, 0."""
    a = [[0.36, 0, 0], [0.46, 0, 0], [0.41, 0.08, 0], [0.41, -0.08, 0]]
    c = [[0, 0, 0], [-0.1, 0, 0], [-0.05, 0.08, 0], [-0.05, -0.08, 0]]
    return np.array([c[1]] + a + [[0.18, 0, 0], c[0], c[2], c[3]], np.float32), np.array([0, 1, 1, 1, 1, 0, 0, 0, 0], np.int32)


def eps_margin(points, eps=EPS):
    """min over pairs of | |p - q|^2 - eps^2 | in float64: below BAND the neighbour decision is float32's own."""
    p = np.asarray(points, np.float64)
    d2 = ((p[:, None] - p[None]) ** 2).sum(2)
    return float(np.abs(d2 - eps * eps).min())


# ---------------------------------------------------------------------------------------------- the host initialisation
def init_centers(points, labels, num_add, cl_num_p, rng):
    """Add_Cluster.py:103-127 on one cloud with ``rng`` (np.random.RandomState) in place of the global stream -> [num_add,cl_num_p,3].
    The two cases in which the reference raises follow attack.CWAddClusters' docstring."""
    points, result = np.asarray(points), np.asarray(labels)
    keep = result > -0.5
    result = result[keep]
    if keep.any():
        points = points[keep]
    batch = []
    labels, counts = np.unique(result, return_counts=True)
    sel_idx = np.argsort(counts, kind="stable")[-num_add:]
    for one_label in labels[sel_idx]:
        cluster_points = points[result == one_label]
        replace = not (len(cluster_points) > cl_num_p)
        sel = rng.choice(len(cluster_points), cl_num_p, replace=replace)
        batch.append(cluster_points[sel].copy())
    while len(batch) < num_add:
        rand_point = points[rng.choice(len(points), 1)[0]]
        dist_matrix = np.sum((points - rand_point[None, :]) ** 2, axis=1)
        batch.append(points[np.resize(np.argsort(dist_matrix)[:cl_num_p], cl_num_p)].copy())
    return np.array(batch)


# ---------------------------------------------------------------------------------------------- the distance and one step
def far_distance(adv, num_add, forced=None):
    """FarthestDist.forward on one cloud: adv [1,A,3] tensor -> (far [1], far_c [num_add], i* [num_add], j* [num_add] as rows of the
    cloud's added rows, norm [num_add,P,P] with norm[c, i, j] = |(p_j - p_i) + 1e-7|).  forced: [num_add,2] ordered pairs (i, j) as
    such rows, taken in place of the two torch.max."""
    c = adv.view(1, num_add, -1, 3)
    P = c.shape[2]
    delta = c[:, :, None, :, :] - c[:, :, :, None, :] + 1e-7
    norm = torch.norm(delta, p=2, dim=-1)                              # [1, num_add, i, j]
    if forced is None:
        mx, ai = torch.max(norm, dim=2)                                # over i, for every j
        far_c, aj = torch.max(mx, dim=2)                               # over j
        ii = ai.gather(2, aj[:, :, None])[0, :, 0]
        jj = aj[0]
    else:
        f = torch.as_tensor(np.array(forced, np.int64))
        ii, jj = f[:, 0] - torch.arange(num_add) * P, f[:, 1] - torch.arange(num_add) * P
        far_c = norm[0, torch.arange(num_add), ii, jj][None]
    base = torch.arange(num_add) * P
    return torch.sum(far_c, dim=1), far_c[0], (ii + base).numpy(), (jj + base).numpy(), norm[0]


def closed_form_grad(adv, ori, num_add, weight, scale, nn, far_i, far_j):
    """The header's step 4 in float64: c_cd (adv_p - ori_j(p)) + [p == j*] u - [p == i*] u, u = c_far d / |d|, d = (p_j* - p_i*) +
    1e-7, c_far = scale (float)weight, c_cd = c_far 0.1 (2 / A); nothing where i* == j*.  Arrays [A,3]."""
    adv, ori = np.asarray(adv, np.float64), np.asarray(ori, np.float64)
    A = len(adv)
    c_far = scale * float(np.float32(weight))
    g = c_far * CHAMFER_WEIGHT * (2.0 / A) * (adv - ori[np.asarray(nn)])
    for i, j in zip(far_i, far_j):
        if i != j:
            d = adv[j] - adv[i] + 1e-7
            u = c_far * d / np.sqrt((d * d).sum())
            g[j] += u
            g[i] -= u
    return g


def step(grad_adv, pred, target, adv, ori, weight, m, v, t, lr, scale, record, num_add, dtype=torch.float64, forced=None):
    """One iteration (Add_Cluster.py:205-236 behind the forward pass) on one cloud.  adv, grad_adv, m, v: [A,3]; ori [n,3]; t: the
    1-based Adam step; forced: see far_distance.
    -> (adv', m', v', record', dist, dist * weight, diag {min_p, nn, far_i, far_j, far_val, norm, dist_grad})."""
    p = DO._b(adv, dtype).requires_grad_()
    o = DO._b(ori, dtype)
    cd, mins, nn, _ = DO.set_distance(p, o, "chamfer")
    far, far_c, fi, fj, norm = far_distance(p, num_add, forced)
    one = torch.ones(1).float().to(dtype)
    d = (far * one + (cd * one) * CHAMFER_WEIGHT).detach().numpy()[0]  # batch_avg=False, weights None: FarChamferDist.forward
    rec = dict(record)
    if d < rec["bestdist"] and pred == target:                          # Add_Cluster.py:216-222
        rec["bestdist"], rec["bestscore"] = d, int(pred)
    if d < rec["o_bestdist"] and pred == target:
        rec["o_bestdist"], rec["o_bestscore"] = d, int(pred)
        rec["o_bestattack"] = np.array(np.asarray(adv), copy=True)
    w = torch.as_tensor([float(weight)]).float().to(dtype)             # weights.float()
    dl = far * w + (cd * w) * CHAMFER_WEIGHT
    (dl.sum() * scale).backward()
    dg = p.grad.detach().clone()
    g = DO._b(grad_adv, dtype) + dg
    p.grad = None
    opt = torch.optim.Adam([p], lr=lr, weight_decay=0.)                # Add_Cluster.py:173
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": DO._b(m, dtype), "exp_avg_sq": DO._b(v, dtype)}
    p.grad = g.detach()
    opt.step()
    st = opt.state[p]
    diag = {"min_p": mins.detach().numpy(), "nn": nn.numpy(), "far_i": fi, "far_j": fj, "far_val": far_c.detach().numpy(),
            "norm": norm.detach().numpy(), "dist_grad": dg[0].numpy()}
    return p.detach()[0].numpy(), st["exp_avg"][0].numpy(), st["exp_avg_sq"][0].numpy(), rec, d, dl.detach().numpy()[0], diag


def exclusions(adv, ori, e_min, norm64, e_norm):
    """From float64 alone and the float32 oracle's measured errors (e_min of a squared distance to an original, e_norm of a norm):
    (rows_out [A] bool: add_oracle.exclusions' rule, the two nearest originals within 8 e_min;  pair_out [num_add] bool: the two
    largest UNORDERED-pair norms within 8 e_norm;  order_out [num_add] bool: the two orders of the arg-max pair within 8 e_norm)."""
    rows_out, _ = DO.exclusions(adv, ori, e_min, "chamfer")
    norm64 = np.asarray(norm64)
    num_add, P = norm64.shape[:2]
    pair_out, order_out = np.zeros(num_add, bool), np.zeros(num_add, bool)
    iu = np.triu_indices(P)
    for c in range(num_add):
        U = np.maximum(norm64[c], norm64[c].T)[iu]                     # the diagonal is a pair, too
        if len(U) > 1:
            top = np.partition(U, len(U) - 2)[-2:]
            pair_out[c] = top[1] - top[0] <= 8 * e_norm
        k = int(np.argmax(U))
        i, j = iu[0][k], iu[1][k]
        order_out[c] = i != j and abs(norm64[c, i, j] - norm64[c, j, i]) <= 8 * e_norm
    return rows_out, pair_out, order_out


def attack(W, data, target, clusters, noise, num_add, cl_num_p, dtype=torch.float64, binary_step=5, num_iter=500, lr=1e-2,
           init_weight=5., max_weight=30., loss="logits", kappa=0., scale=None):
    """Free-running, cloud by cloud, from the start ``clusters`` [B,A,3].  -> dict: o_bestdist [B], o_bestattack [B,K+A,3], success [B]
    bool (lower > 0), success_num, history [binary_step,B,3] (weight, lower, upper behind every search step)."""
    B, K = np.asarray(data).shape[:2]
    A = int(num_add) * int(cl_num_p)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    scale = 1.0 / B if scale is None else scale
    out = {"o_bestdist": np.full(B, 1e10), "o_bestattack": np.zeros((B, K + A, 3), npdt), "success": np.zeros(B, bool),
           "history": np.zeros((binary_step, B, 3))}
    for b in range(B):
        ori = np.asarray(data[b]).astype(npdt)
        tg = int(target[b])
        start = np.asarray(clusters[b]).astype(npdt)
        weight, lower, upper = float(init_weight), 0., float(max_weight)
        rec = fresh_record(A, npdt)
        for s in range(binary_step):
            adv = start if noise is None else start + np.asarray(noise[s][b]).astype(npdt)
            m, v = np.zeros_like(start), np.zeros_like(start)
            for it in range(num_iter):
                r = AO.run_cloud(W, np.concatenate([ori, adv]), tg, loss, kappa, scale, dtype=dtype)
                pred = int(r["logits"].argmax())
                last = adv
                adv, m, v, rec = step(r["grad"][K:], pred, tg, adv, ori, weight, m, v, it + 1, lr, scale, rec, num_add, dtype)[:4]
            weight, lower, upper, rec = adjust(rec, tg, weight, lower, upper)
            out["history"][s, b] = weight, lower, upper
        out["success"][b] = lower > 0
        out["o_bestdist"][b] = rec["o_bestdist"]
        out["o_bestattack"][b] = np.concatenate([ori, rec["o_bestattack"] if lower > 0 else last])
    out["success_num"] = int(out["success"].sum())
    return out


# ---------------------------------------------------------------------------------------------- teacher-forced step cases
# (name, B, largest n_ori, num_add, cl_num_p): the smallest shapes that reach every code path of cluster_step_kernel
STEP_CASES = (("ref", 17, 64, 3, 32), ("ragged", 5, 300, 7, 11), ("single", 3, 128, 96, 1), ("pairs", 2, 1024, 512, 2),
              ("wide", 1, 2048, 1, 1024))
STEP_LR, STEP_SCALE = 1e-2, 0.25
QUANTITIES = ("adv", "m", "v", "dist", "dist_grad", "far_val")


def make_step_case(name, t, seed=0):
    """Inputs of one teacher-forced step, float32 as the library takes them: the network plays no part (grad, m and positive v are
    random).  Cluster c of a cloud starts from one original (a draw without repeats) + 0.05 randn - never from the reference's 1e-7
    start.  Rows beyond a cloud are NaN: reading them poisons the result."""
    _, B, n_max, num_add, P = next(c for c in STEP_CASES if c[0] == name)
    A = num_add * P
    rng = np.random.default_rng([seed, t, sum(map(ord, name))])
    n_ori = np.full(B, n_max, np.int32)
    stride = n_max + A
    if name == "ragged":
        n_ori = np.array([n_max, 1, 150, n_max - 1, 256], np.int32)
        stride = n_max + A + 3
    cat = np.full((B, stride, 3), np.nan, np.float32)
    grad = np.full((B, stride, 3), np.nan, np.float32)
    for b in range(B):
        n = int(n_ori[b])
        ori = rng.standard_normal((n, 3))
        ori = (ori / np.linalg.norm(ori, axis=1, keepdims=True) * rng.random((n, 1)) ** (1 / 3)).astype(np.float32)
        centre = ori[rng.permutation(max(n, num_add))[:num_add] % n]
        cat[b, :n] = ori
        cat[b, n:n + A] = np.repeat(centre, P, axis=0) + (0.05 * rng.standard_normal((A, 3))).astype(np.float32)
        grad[b, :n + A] = (rng.standard_normal((n + A, 3)) * 10 ** rng.uniform(-4, -1, (n + A, 1))).astype(np.float32)
    m = (rng.standard_normal((B, A, 3)) * 1e-2).astype(np.float32) if t > 1 else np.zeros((B, A, 3), np.float32)
    v = (rng.random((B, A, 3)) * 1e-3 + 1e-8).astype(np.float32) if t > 1 else np.zeros((B, A, 3), np.float32)
    weight = rng.uniform(5. / 8, 30., B)
    target = rng.integers(0, 40, B).astype(np.int32)
    pred = np.where(rng.random(B) < 0.5, target, (target + 1) % 40).astype(np.int32)
    return {"name": name, "t": t, "B": B, "A": A, "num_add": num_add, "cl_num_p": P, "stride": stride, "n_ori": n_ori, "cat": cat,
            "grad": grad, "m": m, "v": v, "weight": weight, "target": target, "pred": pred}


def run_step_case(case, dtype, forced=None):
    """The oracle on every cloud of a case -> list of dicts {adv, m, v, dist, dist_grad, min_p, nn, far_i, far_j, far_val, norm,
    record}.  forced: [B,num_add,2] ordered pairs or None."""
    out = []
    npdt = np.float32 if dtype == torch.float32 else np.float64
    for b in range(case["B"]):
        n, A = int(case["n_ori"][b]), case["A"]
        ori, adv = case["cat"][b, :n].astype(npdt), case["cat"][b, n:n + A].astype(npdt)
        a, m, v, rec, d, _, diag = step(case["grad"][b, n:n + A].astype(npdt), int(case["pred"][b]), int(case["target"][b]), adv, ori,
                                        case["weight"][b], case["m"][b].astype(npdt), case["v"][b].astype(npdt), case["t"], STEP_LR,
                                        STEP_SCALE, fresh_record(A, npdt), case["num_add"], dtype,
                                        None if forced is None else forced[b])
        out.append(dict(diag, adv=a, m=m, v=v, dist=d, record=rec))
    return out


def pairs_of(r):
    """[B,num_add,2]: the ordered pairs (i*, j*) of a run."""
    return np.stack([np.stack([x["far_i"], x["far_j"]], 1) for x in r])


def errors(case, got, yard, free, rows_out):
    """{quantity: max |got - float64|} over the judged rows: adv, m, v, dist_grad against ``yard`` (the float64 step with got's
    order forced), dist and far_val against ``free`` (the float64 arg-max: an undecidable order moves the VALUE by rounding only)."""
    err = {k: 0.0 for k in QUANTITIES}
    for g, y, f, ro in zip(got, yard, free, rows_out):
        for k in ("adv", "m", "v", "dist_grad"):
            err[k] = max(err[k], float(np.abs(np.asarray(g[k], np.float64) - y[k])[~ro].max()))
        err["dist"] = max(err["dist"], abs(float(g["dist"]) - float(f["dist"])))
        err["far_val"] = max(err["far_val"], float(np.abs(np.asarray(g["far_val"], np.float64) - f["far_val"]).max()))
    return err


def check_pairs(case, pairs, r64, pair_out, order_out, who):
    """The decisions that are judged: the unordered pair everywhere (no cluster may be out), the order where it is decidable."""
    for b in range(case["B"]):
        want = np.stack([r64[b]["far_i"], r64[b]["far_j"]], 1)
        assert not pair_out[b].any()
        assert np.array_equal(np.sort(pairs[b], 1), np.sort(want, 1)), "%s: %s takes another pair in cloud %d" % (case["name"], who, b)
        keep = ~order_out[b]
        assert np.array_equal(pairs[b][keep], want[keep]), "%s: %s takes another order in cloud %d" % (case["name"], who, b)


def judge(case, r32, r64):
    """From the two oracles alone -> dict: e_min, e_norm, rows_out / pair_out / order_out (lists over the clouds), share (of rows
    out), undecided (share of clusters whose order is not judged), e32 {quantity: the float32 oracle's largest error over the judged
    rows, against the float64 step with the float32 oracle's order forced}.  Asserts the conditions a parity case must meet: no
    cluster's unordered pair is out, at most 5 % of the rows are out, and the two oracles agree on every judged decision."""
    e_min = max(float(np.abs(a["min_p"].astype(np.float64) - b["min_p"]).max()) for a, b in zip(r32, r64))
    e_norm = max(float(np.abs(a["norm"].astype(np.float64) - b["norm"]).max()) for a, b in zip(r32, r64))
    rows_out, pair_out, order_out = [], [], []
    for b in range(case["B"]):
        n, A = int(case["n_ori"][b]), case["A"]
        ro, po, oo = exclusions(case["cat"][b, n:n + A], case["cat"][b, :n], e_min, r64[b]["norm"], e_norm)
        rows_out.append(ro), pair_out.append(po), order_out.append(oo)
    assert not any(p.any() for p in pair_out), "%s: a cluster's unordered pair is excluded" % case["name"]
    share = sum(int(r.sum()) for r in rows_out) / float(case["B"] * case["A"])
    assert share <= 0.05, "%s: %.1f %% of the rows are excluded" % (case["name"], 100 * share)
    for a, b, ro in zip(r32, r64, rows_out):
        assert np.array_equal(a["nn"][~ro], b["nn"][~ro]), "%s: the oracles disagree on a judged nearest original" % case["name"]
    p32 = pairs_of(r32)
    check_pairs(case, p32, r64, pair_out, order_out, "the float32 oracle")
    yard = r64 if np.array_equal(p32, pairs_of(r64)) else run_step_case(case, torch.float64, p32)
    return {"e_min": e_min, "e_norm": e_norm, "rows_out": rows_out, "pair_out": pair_out, "order_out": order_out, "share": share,
            "undecided": float(np.mean([o.mean() for o in order_out])), "e32": errors(case, r32, yard, r64, rows_out)}
