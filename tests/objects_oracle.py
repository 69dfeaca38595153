"""Test oracle of the CW object-adding attack (include/ifd_object.h): CWAddObjects.attack (baselines/attack/CW/Add_Objects.py) with
L2ChamferDist(num_add, 'adv2ori', 0.2) (baselines/attack/util/dist_utils.py) restated one cloud at a time, in the reference's own
form: the rotation as torch.bmm with the stacked 3 x 3 matrix, the L2 part as sqrt of the sum of squares, the Chamfer part from
add_oracle.pairwise (three bmm's, torch.min, torch.mean), autograd for every gradient, the real torch.optim.Adam over the three
tensors on the CPU with its state put in from outside, ``%`` for the angles, the record and the adjustment of cw_oracle.  The
adversarial loss, its gradient and the prediction come from atk_oracle.run_cloud on the concatenated cloud.  Runs in float32 (the
reference's rounding) and float64 (the yardstick).

Also here: the header's gradients in closed form (``closed_form_grad``), the float32 remainder (``remainder32``), and the
teacher-forced step cases with their judge.  The discrete decision of a step is the nearest original of every world row; where
float32 cannot decide it (add_oracle.exclusions: the two nearest within 8 e_min), the row is not judged on it, and because such a row
feeds its whole object's shift and angle sums, the float64 yardstick of whoever is measured is the step with THAT one's nearest
original forced on exactly those rows."""
import numpy as np
import torch

import add_oracle as DO
import atk_oracle as AO
import cw_oracle as CO

fresh_record = CO.fresh_record
adjust = CO.adjust
CHAMFER_WEIGHT = 0.2
TWO_PI = 2. * np.pi
POSE = ("shift", "angle")
MOMENTS = ("m", "v", "shift_m", "shift_v", "angle_m", "angle_v")


def remainder32(a):
    """torch.remainder(a, (float)(2 pi)) in float32 as the header states it: fmodf, then + b where the result is non-zero and of the
    other sign."""
    a = np.asarray(a, np.float32)
    b = np.float32(TWO_PI)
    r = np.fmod(a, b).astype(np.float32)
    return np.where((r != 0) & (r < 0), (r + b).astype(np.float32), r).astype(np.float32)


def rotate_shift(points, angle, shift):
    """Add_Objects.py:148-185 on one cloud: points [1,num_add,P,3], angle [1,num_add], shift [1,num_add,3] -> [1,num_add,P,3]."""
    num_add, P = points.shape[1], points.shape[2]
    cosval, sinval = torch.cos(angle), torch.sin(angle)
    zeros, ones = torch.zeros_like(cosval).detach(), torch.ones_like(cosval).detach()
    rot_mat = torch.stack([cosval, zeros, sinval, zeros, ones, zeros, -sinval, zeros, cosval], dim=-1).view(num_add, 3, 3)
    rot = torch.bmm(points.view(num_add, P, 3), rot_mat).view(1, num_add, P, 3)
    return rot + shift[:, :, None, :]


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a)).to(dtype)[None].clone()


def step(grad_world, pred, target, obj, shift, angle, objects, ori, weight, mom, t, lr, scale, record, dtype=torch.float64, nn_forced=None):
    """One iteration (Add_Objects.py:259-340 behind the forward pass) on one cloud.  obj [num_add,P,3], shift [num_add,3], angle
    [num_add], objects [num_add,P,3], ori [n,3]; grad_world [A,3]: the added rows of scale * d adv_loss / d cat; mom: dict of the six
    moments (m, v [num_add,P,3]; shift_m, shift_v [num_add,3]; angle_m, angle_v [num_add]); t: the 1-based Adam step; nn_forced [A]:
    the nearest originals to take in place of torch.min.  -> dict: obj, shift, angle, the six moments, world (the placement of the NEW
    state), forwarded (the world rows this step saw), record, dist, dist_loss, l2, cd, min_p, nn, obj_grad, g_shift, g_angle."""
    num_add, P = np.asarray(obj).shape[:2]
    A = num_add * P
    x, s, a = _t(obj, dtype).requires_grad_(), _t(shift, dtype).requires_grad_(), _t(angle, dtype).requires_grad_()
    tmpl, o = _t(objects, dtype), DO._b(ori, dtype)
    world = rotate_shift(x, a, s).view(1, A, 3)
    Pm = DO.pairwise(o, world)                                         # [1, n, A]
    mins, nn = torch.min(Pm, 1)
    if nn_forced is not None:
        nn = torch.as_tensor(np.asarray(nn_forced, np.int64))[None]
        mins = Pm.gather(1, nn[:, None, :])[:, 0]
    cd = torch.mean(mins, dim=1)
    l2 = torch.sqrt(torch.sum((x.view(1, A, 3) - tmpl.view(1, A, 3)) ** 2, dim=[1, 2]))
    one = torch.ones(1).float().to(dtype)
    d = (l2 * one + CHAMFER_WEIGHT * (cd * one)).detach().numpy()[0]   # batch_avg=False, weights None: L2ChamferDist.forward
    fwd = world.detach()[0].numpy().copy()
    rec = dict(record)
    if d < rec["bestdist"] and pred == target:                          # Add_Objects.py:299-305
        rec["bestdist"], rec["bestscore"] = d, int(pred)
    if d < rec["o_bestdist"] and pred == target:
        rec["o_bestdist"], rec["o_bestscore"] = d, int(pred)
        rec["o_bestattack"] = fwd.copy()
    w = torch.as_tensor([float(weight)]).float().to(dtype)             # weights.float()
    l2_loss = l2 * w if float(l2.detach()) > 0 else (l2 * w).detach()           # l2 == 0: no L2 gradient (the header's deviation)
    dl = l2_loss + CHAMFER_WEIGHT * (cd * w)
    ((dl.sum() * scale) + (world * DO._b(grad_world, dtype)).sum()).backward()
    grads = [p.grad.detach().clone() for p in (x, s, a)]
    opt = torch.optim.Adam([x, s, a], lr=lr, weight_decay=0.)          # Add_Objects.py:245
    for p, (km, kv) in zip((x, s, a), (("m", "v"), ("shift_m", "shift_v"), ("angle_m", "angle_v"))):
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": _t(mom[km], dtype), "exp_avg_sq": _t(mom[kv], dtype)}
    opt.step()
    with torch.no_grad():
        a.data = a.data % TWO_PI                                       # Add_Objects.py:340
        new_world = rotate_shift(x, a, s).view(A, 3).numpy().copy()
    out = {"obj": x.detach()[0].numpy(), "shift": s.detach()[0].numpy(), "angle": a.detach()[0].numpy(), "world": new_world,
           "forwarded": fwd, "record": rec, "dist": d, "dist_loss": dl.detach().numpy()[0], "l2": l2.detach().numpy()[0],
           "cd": cd.detach().numpy()[0], "min_p": mins.detach()[0].numpy(), "nn": nn[0].numpy(), "obj_grad": grads[0][0].numpy(),
           "g_shift": grads[1][0].numpy(), "g_angle": grads[2][0].numpy()}
    for p, (km, kv) in zip((x, s, a), (("m", "v"), ("shift_m", "shift_v"), ("angle_m", "angle_v"))):
        out[km], out[kv] = opt.state[p]["exp_avg"][0].numpy(), opt.state[p]["exp_avg_sq"][0].numpy()
    return out


def closed_form_grad(obj, shift, angle, objects, ori, grad_world, weight, scale, nn):
    """The header's step 5 in float64 -> (g_obj [num_add,P,3], g_shift [num_add,3], g_angle [num_add])."""
    obj, objects, ori = np.asarray(obj, np.float64), np.asarray(objects, np.float64), np.asarray(ori, np.float64)
    shift, angle = np.asarray(shift, np.float64), np.asarray(angle, np.float64)
    num_add, P = obj.shape[:2]
    A = num_add * P
    c, s = np.cos(angle)[:, None], np.sin(angle)[:, None]
    r = np.stack([obj[..., 0] * c - obj[..., 2] * s, obj[..., 1], obj[..., 0] * s + obj[..., 2] * c], -1)
    world = r + shift[:, None, :]
    c_w = scale * float(np.float32(weight))
    l2 = np.sqrt(((obj - objects) ** 2).sum())
    gw = c_w * CHAMFER_WEIGHT * (2.0 / A) * (world - ori[np.asarray(nn)].reshape(num_add, P, 3)) + np.asarray(grad_world, np.float64).reshape(num_add, P, 3)
    g_obj = np.stack([gw[..., 0] * c + gw[..., 2] * s, gw[..., 1], -gw[..., 0] * s + gw[..., 2] * c], -1)
    if l2 > 0:
        g_obj = g_obj + (c_w / l2) * (obj - objects)
    return g_obj, gw.sum(1), (gw[..., 2] * r[..., 0] - gw[..., 0] * r[..., 2]).sum(1)


def attack(W, data, target, objects, centers, noise_obj, noise_shift, angles0, dtype=torch.float64, binary_step=5, num_iter=500,
           lr=1e-2, init_weight=5., max_weight=40., loss="logits", kappa=0., scale=None):
    """Free-running, cloud by cloud.  objects [num_add,P,3], centers [B,num_add,3], noise_obj [binary_step,B,A,3] and noise_shift
    [binary_step,B,num_add,3] (or None), angles0 [binary_step,B,num_add].  -> dict: o_bestdist [B], o_bestattack [B,K+A,3], success [B]
    bool (lower > 0), success_num, history [binary_step,B,3] (weight, lower, upper behind every search step)."""
    B, K = np.asarray(data).shape[:2]
    num_add, P = np.asarray(objects).shape[:2]
    A = num_add * P
    npdt = np.float32 if dtype == torch.float32 else np.float64
    scale = 1.0 / B if scale is None else scale
    tmpl = np.asarray(objects).astype(npdt)
    out = {"o_bestdist": np.full(B, 1e10), "o_bestattack": np.zeros((B, K + A, 3), npdt), "success": np.zeros(B, bool),
           "history": np.zeros((binary_step, B, 3))}
    for b in range(B):
        ori = np.asarray(data[b]).astype(npdt)
        tg = int(target[b])
        weight, lower, upper = float(init_weight), 0., float(max_weight)
        rec = fresh_record(A, npdt)
        for s in range(binary_step):
            obj = tmpl if noise_obj is None else tmpl + np.asarray(noise_obj[s][b]).astype(npdt).reshape(num_add, P, 3)
            shift = np.asarray(centers[b]).astype(npdt)
            if noise_shift is not None:
                shift = shift + np.asarray(noise_shift[s][b]).astype(npdt)
            angle = np.asarray(angles0[s][b]).astype(npdt)
            mom = {"m": np.zeros_like(obj), "v": np.zeros_like(obj), "shift_m": np.zeros_like(shift), "shift_v": np.zeros_like(shift),
                   "angle_m": np.zeros_like(angle), "angle_v": np.zeros_like(angle)}
            with torch.no_grad():
                world = rotate_shift(_t(obj, dtype), _t(angle, dtype), _t(shift, dtype)).view(A, 3).numpy()
            for it in range(num_iter):
                r = AO.run_cloud(W, np.concatenate([ori, world]), tg, loss, kappa, scale, dtype=dtype)
                pred = int(r["logits"].argmax())
                last = world
                st = step(r["grad"][K:], pred, tg, obj, shift, angle, tmpl, ori, weight, mom, it + 1, lr, scale, rec, dtype)
                obj, shift, angle, world, rec = st["obj"], st["shift"], st["angle"], st["world"], st["record"]
                mom = {k: st[k] for k in MOMENTS}
            weight, lower, upper, rec = adjust(rec, tg, weight, lower, upper)
            out["history"][s, b] = weight, lower, upper
        out["success"][b] = lower > 0
        out["o_bestdist"][b] = rec["o_bestdist"]
        out["o_bestattack"][b] = np.concatenate([ori, rec["o_bestattack"] if lower > 0 else last])       # Add_Objects.py:355-367
    out["success_num"] = int(out["success"].sum())
    return out


# ---------------------------------------------------------------------------------------------- teacher-forced step cases
# (name, B, largest n_ori, num_add, obj_num_p): the smallest shapes that reach every code path of object_step_kernel
STEP_CASES = (("ref", 17, 64, 3, 64), ("ragged", 5, 300, 7, 11), ("single", 3, 128, 96, 1), ("pairs", 2, 1024, 512, 2),
              ("wide", 1, 2048, 1, 1024))
STEP_LR, STEP_SCALE = 1e-2, 0.25
NEAR = 5e-4                                                            # crafted angles: this far from 0 and from 2 pi
QUANTITIES = ("obj", "shift", "angle") + MOMENTS + ("dist", "l2", "cd", "obj_grad", "g_shift", "g_angle", "world")


def make_step_case(name, t, seed=0):
    """Inputs of one teacher-forced step, float32 as the library takes them: the network plays no part (the gradient and the moments
    are random, v positive).  One template per case, shared by its clouds: num_add objects of P points in a ball of radius 0.3; a
    cloud's obj is the template + 0.05 randn - never the reference's 1e-7 start - its shifts are originals (a draw without repeats) +
    0.02 randn, its angles uniform over [0, 2 pi) with the first one NEAR above 0 and the second (the first, in odd clouds or at t >
    1 where there is one object only) NEAR below 2 pi; at t > 1 their first moments are +- 0.05, so that the step carries them across
    the wrap-around by several NEAR.  Rows beyond a cloud are NaN: reading them poisons the result."""
    _, B, n_max, num_add, P = next(c for c in STEP_CASES if c[0] == name)
    A = num_add * P
    rng = np.random.default_rng([seed, t, sum(map(ord, name))])
    n_ori = np.full(B, n_max, np.int32)
    stride = n_max + A
    if name == "ragged":
        n_ori = np.array([n_max, 1, 150, n_max - 1, 256], np.int32)
        stride = n_max + A + 3
    u = rng.standard_normal((num_add, P, 3))
    objects = (0.3 * u / np.linalg.norm(u, axis=2, keepdims=True) * rng.random((num_add, P, 1)) ** (1 / 3)).astype(np.float32)
    ori = np.full((B, stride - A, 3), np.nan, np.float32)
    grad = np.full((B, stride, 3), np.nan, np.float32)
    obj = (objects[None] + 0.05 * rng.standard_normal((B, num_add, P, 3))).astype(np.float32)
    shift = np.zeros((B, num_add, 3), np.float32)
    angle = rng.uniform(0.01, TWO_PI - 0.01, (B, num_add)).astype(np.float32)
    for b in range(B):
        n = int(n_ori[b])
        o = rng.standard_normal((n, 3))
        ori[b, :n] = (o / np.linalg.norm(o, axis=1, keepdims=True) * rng.random((n, 1)) ** (1 / 3)).astype(np.float32)
        shift[b] = ori[b, rng.permutation(max(n, num_add))[:num_add] % n] + (0.02 * rng.standard_normal((num_add, 3))).astype(np.float32)
        grad[b, :n + A] = (rng.standard_normal((n + A, 3)) * 10 ** rng.uniform(-4, -1, (n + A, 1))).astype(np.float32)
        if num_add > 1:
            angle[b, 0], angle[b, 1] = NEAR, np.float32(TWO_PI) - np.float32(NEAR)
        else:
            angle[b, 0] = NEAR if (b % 2 == 0 and t == 1) else np.float32(TWO_PI) - np.float32(NEAR)
    f = lambda shape, k: ((rng.standard_normal(shape) * 1e-2) if k == "m" else (rng.random(shape) * 1e-3 + 1e-8)).astype(np.float32) \
        if t > 1 else np.zeros(shape, np.float32)                      # noqa: E731
    mom = {"m": f((B, num_add, P, 3), "m"), "v": f((B, num_add, P, 3), "v"), "shift_m": f((B, num_add, 3), "m"),
           "shift_v": f((B, num_add, 3), "v"), "angle_m": f((B, num_add), "m"), "angle_v": f((B, num_add), "v")}
    if t > 1:                                                          # the crafted angles cross the wrap-around by several NEAR
        near_zero = angle < 1e-3
        mom["angle_m"] = np.where(near_zero, 0.05, np.where(angle > TWO_PI - 1e-3, -0.05, mom["angle_m"])).astype(np.float32)
    weight = rng.uniform(5. / 8, 40., B)
    target = rng.integers(0, 40, B).astype(np.int32)
    pred = np.where(rng.random(B) < 0.5, target, (target + 1) % 40).astype(np.int32)
    return dict(mom, name=name, t=t, B=B, A=A, num_add=num_add, obj_num_p=P, stride=stride, n_ori=n_ori, ori=ori, grad=grad,
                objects=objects, obj=obj, shift=shift, angle=angle, weight=weight, target=target, pred=pred)


def run_step_case(case, dtype, nn_forced=None):
    """The oracle on every cloud of a case -> list of ``step``'s dicts.  nn_forced: list of [A] arrays or None."""
    out = []
    npdt = np.float32 if dtype == torch.float32 else np.float64
    for b in range(case["B"]):
        n, A = int(case["n_ori"][b]), case["A"]
        mom = {k: case[k][b].astype(npdt) for k in MOMENTS}
        out.append(step(case["grad"][b, n:n + A].astype(npdt), int(case["pred"][b]), int(case["target"][b]), case["obj"][b].astype(npdt),
                        case["shift"][b].astype(npdt), case["angle"][b].astype(npdt), case["objects"].astype(npdt),
                        case["ori"][b, :n].astype(npdt), case["weight"][b], mom, case["t"], STEP_LR, STEP_SCALE,
                        fresh_record(A, npdt), dtype, None if nn_forced is None else nn_forced[b]))
    return out


def errors(got, yard):
    """{quantity: max |got - float64|} over the clouds; got, yard: lists of dicts with QUANTITIES."""
    err = {k: 0.0 for k in QUANTITIES}
    for g, y in zip(got, yard):
        for k in QUANTITIES:
            err[k] = max(err[k], float(np.abs(np.asarray(g[k], np.float64).reshape(-1) - np.asarray(y[k], np.float64).reshape(-1)).max()))
    return err


def yardstick(case, got_nn, r64, rows_out):
    """The float64 step with the measured side's nearest originals forced on exactly the rows that are not judged."""
    if not any(r.any() for r in rows_out):
        return r64
    return run_step_case(case, torch.float64, [np.where(ro, np.asarray(g), f["nn"]) for g, f, ro in zip(got_nn, r64, rows_out)])


def judge(case, r32, r64):
    """From the two oracles alone -> dict: e_min, rows_out (list over the clouds), share (of rows out), e32 {quantity: the float32
    oracle's largest error against its yardstick}.  Asserts the conditions a parity case must meet: at most 5 % of the rows are out,
    the two oracles agree on every judged nearest original, and no new angle lies within 1e-4 of the wrap-around (where float32
    rounding could put the two sides 2 pi apart)."""
    e_min = max(float(np.abs(a["min_p"].astype(np.float64) - b["min_p"]).max()) for a, b in zip(r32, r64))
    rows_out = [DO.exclusions(b["forwarded"], case["ori"][i, :int(case["n_ori"][i])], e_min, "chamfer")[0] for i, b in enumerate(r64)]
    share = sum(int(r.sum()) for r in rows_out) / float(case["B"] * case["A"])
    assert share <= 0.05, "%s: %.1f %% of the rows are excluded" % (case["name"], 100 * share)
    for a, b, ro in zip(r32, r64, rows_out):
        assert np.array_equal(a["nn"][~ro], b["nn"][~ro]), "%s: the oracles disagree on a judged nearest original" % case["name"]
        assert (np.minimum(b["angle"], TWO_PI - b["angle"]) > 1e-4).all(), "%s: a new angle at the wrap-around" % case["name"]
    yard = yardstick(case, [a["nn"] for a in r32], r64, rows_out)
    return {"e_min": e_min, "rows_out": rows_out, "share": share, "e32": errors(r32, yard)}
