"""The refusals of the point-adding calls (include/ifd_add.h, ifd_cluster.h, ifd_object.h), their texts in full and their order.

Every argument refusal of the ten calls is triggered once through the raw C call, with the argument sets of the three
test_limits_are_refused_one_past_them, and ifd_last_error is compared whole against the table below.  Three calls per attack break
two rules at once: the earlier check must be the one that answers.  All of them return before any kernel is launched, except the
blocking count / target check of the attack calls and of ifd_add_critical_points."""
import ctypes as C

import numpy as np
import pytest
import torch

import pointnet_oracle as PO

pytestmark = pytest.mark.gpu

CW = "m, v, bestdist, bestscore, o_bestdist, o_bestscore, o_bestattack, weight"
ROWS = "num_add < 1, %s < 1 or num_add * %s outside [1, 1024]"


@pytest.fixture(scope="module")
def net():
    import ifdefense_amd as I
    from ifdefense_amd import weights
    with I.Classifier(weights.pack_state_dict(PO.make_weights(0, False), "pointnet"), device="cuda:0") as c:
        yield c


@pytest.fixture(scope="module")
def mem():
    f = lambda *s: torch.zeros(*s, device="cuda")                      # noqa: E731
    i = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")   # noqa: E731
    return {"big": f(1, 10001, 3), "tt": i(2), "cri": f(2, 1025, 3), "idx": i(2, 1025), "o": f(2, 3100, 3), "best": f(2), "ok": i(2),
            "cl": f(2, 1024, 3)}


def counts(*n):
    return torch.tensor(n, dtype=torch.int32).cuda()


class Calls:
    """Runs a call and compares its refusal at once: ifd_last_error holds only the latest."""
    def __init__(self, net, who):
        self.lib, self.ctx, self.who, self.fn = net.lib, net.ctx, who, getattr(net.lib, who)

    def refused(self, text, *args):
        rc = self.fn(self.ctx, *args)
        got = self.lib.ifd_last_error(self.ctx).decode()
        assert rc == -1 and got == self.who + ": " + text, (rc, got, text)


def test_add_select_and_critical_points(net, mem):
    P, T, cri, idx = mem["big"].data_ptr(), mem["tt"].data_ptr(), mem["cri"].data_ptr(), mem["idx"].data_ptr()
    c = Calls(net, "ifd_add_select")
    sel = lambda text, B, stride, num_add, n=None: c.refused(text, P, P, n, B, stride, num_add, cri, idx, None)   # noqa: E731
    sel("bad argument (grad, pc, cri; B >= 1)", 0, 64, 16)
    sel("num_add outside [1, 1024]", 1, 2048, 1025)
    sel("num_add outside [1, 1024]", 1, 2048, 0)
    sel("stride outside [1, 10000]", 1, 10001, 16, T)
    sel("without n_points, stride outside [num_add, 2048]", 1, 2049, 16)
    sel("without n_points, stride outside [num_add, 2048]", 1, 15, 16)
    sel("bad argument (grad, pc, cri; B >= 1)", 0, 10001, 1025)                       # the order: pointers and B, num_add, stride
    sel("num_add outside [1, 1024]", 1, 10001, 1025)
    c = Calls(net, "ifd_add_critical_points")
    crit = lambda text, B, stride, num_add, n=None: c.refused(text, P, n, T, B, stride, num_add, 1.0, cri, None, None)   # noqa: E731
    crit("bad argument (pc, target, cri; B >= 1)", 0, 64, 16)
    crit("num_add outside [1, 1024]", 1, 64, 1025)
    crit("stride outside [1, 10000]", 1, 10001, 16, T)
    crit("without n_points, stride outside [num_add, 2048]", 1, 2049, 16)
    crit("num_add outside [1, 1024]", 1, 10001, 0)
    n = counts(64, 15)
    crit("1 cloud(s) with n_points outside [16, 64]", 2, 64, 16, n.data_ptr())
    assert not mem["cri"].any() and not mem["idx"].any()


def test_step_and_place_calls(net, mem):
    P, T = mem["big"].data_ptr(), mem["tt"].data_ptr()
    from ifdefense_amd import _lib
    st = net.cw_state(2, 1024)
    cw = net._cw_struct(st, 2, 1024)
    S = C.byref(cw)
    no_m = _lib.IfdCwState(None, *[P] * 9)

    c = Calls(net, "ifd_add_step")
    step = lambda text, kind, cat_stride, num_add, n=None, t=1, S=S: c.refused(   # noqa: E731
        text, kind, S, P, T, None, T, P, n, None, None, None, t, 0.01, 1.0, 1, cat_stride, num_add, None)
    step("unknown kind", 2, 64, 16)
    step("state missing (" + CW + ")", 0, 64, 16, S=C.byref(no_m))
    step("state missing (" + CW + ")", 0, 64, 16, S=None)
    step("bad argument (grad, pred, target, cat; t >= 1, B >= 1)", 0, 64, 16, None, 0)
    step("num_add outside [1, 1024]", 0, 4096, 1025)
    step("cat_stride outside [2 num_add, 10000]", 0, 31, 16)
    step("cat_stride outside [2 num_add, 10000]", 0, 10001, 16, T)
    step("without n_ori, cat_stride - num_add > 2048 original rows", 0, 2049 + 16, 16)
    step("unknown kind", 2, 31, 1025, None, 0, C.byref(no_m))                           # the order
    step("bad argument (grad, pred, target, cat; t >= 1, B >= 1)", 0, 31, 1025, None, 0)

    c = Calls(net, "ifd_cluster_step")
    step = lambda text, cat_stride, num_add, P_, n=None, t=1, S=S: c.refused(   # noqa: E731
        text, S, P, T, None, T, P, n, None, None, None, t, 0.01, 1.0, 1, cat_stride, num_add, P_, None)
    rows = ROWS % ("cl_num_p", "cl_num_p")
    step("state missing (" + CW + ")", 200, 3, 32, S=C.byref(no_m))
    step("bad argument (grad, pred, target, cat; t >= 1, B >= 1)", 200, 3, 32, None, 0)
    for cat_stride, num_add, P_ in ((4096, 1025, 1), (4096, 33, 32), (4096, 0, 32), (4096, 3, 0)):
        step(rows, cat_stride, num_add, P_)
    step("cat_stride outside [num_add * cl_num_p + 1, 10000]", 96, 3, 32)
    step("cat_stride outside [num_add * cl_num_p + 1, 10000]", 10001, 3, 32, T)
    step("without n_ori, cat_stride - num_add * cl_num_p > 2048 original rows", 2049 + 96, 3, 32)
    step(rows, 96, 33, 32)                                                              # the order

    c = Calls(net, "ifd_object_place")
    place = lambda text, cat_stride, num_add, P_, n=None, B=1, obj=P: c.refused(text, obj, P, P, P, n, B, cat_stride, num_add, P_, None)   # noqa: E731
    rows = ROWS % ("obj_num_p", "obj_num_p")
    place("bad argument (obj, angle, shift, cat; B >= 1)", 400, 3, 64, None, 0)
    place("bad argument (obj, angle, shift, cat; B >= 1)", 400, 3, 64, None, 1, None)
    place(rows, 4096, 33, 32)
    place("cat_stride outside [num_add * obj_num_p + 1, 10000]", 192, 3, 64)
    place("cat_stride outside [num_add * obj_num_p + 1, 10000]", 10001, 3, 64, T)
    place("without n_ori, cat_stride - num_add * obj_num_p > 2048 original rows", 2049 + 192, 3, 64)
    place(rows, 192, 33, 32)                                                            # the order

    c = Calls(net, "ifd_object_step")
    ost = net.object_state(2, 32, 32)
    OS = C.byref(net._object_struct(ost, 2, 32, 1024))
    no_angle = _lib.IfdObjectState(cw, P, P, None, *[P] * 4)
    step = lambda text, cat_stride, num_add, P_, n=None, t=1, objects=P, S=OS: c.refused(   # noqa: E731
        text, S, objects, P, T, None, T, P, n, None, None, None, t, 0.01, 1.0, 1, cat_stride, num_add, P_, None)
    missing = "state missing (cw: " + CW + "; obj, shift, angle, shift_m, shift_v, angle_m, angle_v)"
    step(missing, 400, 3, 64, S=C.byref(no_angle))
    step(missing, 400, 3, 64, S=C.byref(_lib.IfdObjectState(no_m, *[P] * 7)))
    step("bad argument (objects, grad, pred, target, cat; t >= 1, B >= 1)", 400, 3, 64, None, 0)
    step("bad argument (objects, grad, pred, target, cat; t >= 1, B >= 1)", 400, 3, 64, None, 1, None)
    for cat_stride, num_add, P_ in ((4096, 1025, 1), (4096, 33, 32), (4096, 0, 32), (4096, 3, 0)):
        step(rows, cat_stride, num_add, P_)
    step("cat_stride outside [num_add * obj_num_p + 1, 10000]", 192, 3, 64)
    step("cat_stride outside [num_add * obj_num_p + 1, 10000]", 10001, 3, 64, T)
    step("without n_ori, cat_stride - num_add * obj_num_p > 2048 original rows", 2049 + 192, 3, 64)
    assert not mem["big"].any()


def test_cluster_dbscan(net, mem):
    P, T = mem["big"].data_ptr(), mem["tt"].data_ptr()
    c = Calls(net, "ifd_cluster_dbscan")
    db = lambda text, B, stride, eps=0.2, ms=3, n=None, labels=T: c.refused(text, P, n, B, stride, eps, ms, labels, None, None)   # noqa: E731
    db("bad argument (pts, labels; B >= 1)", 0, 2)
    db("bad argument (pts, labels; B >= 1)", 1, 2, labels=None)
    db("stride outside [1, 10000]", 1, 10001, n=T)
    db("eps must be a finite number above 0", 1, 2, 0.0)
    db("eps must be a finite number above 0", 1, 2, float("nan"))
    db("eps must be a finite number above 0", 1, 2, float("inf"))
    db("min_samples < 1", 1, 2, 0.2, 0)
    db("without n_pts, stride outside [1, 256]", 1, 257)
    db("stride outside [1, 10000]", 1, 10001, 0.0, 0)                                   # the order
    db("eps must be a finite number above 0", 1, 257, 0.0, 0)
    assert not mem["tt"].any()


# what differs between the three attack calls: the params struct with its rows, the pointers between target and B, the texts
def _attacks(mem):
    from ifdefense_amd import _lib
    P, cl = mem["big"].data_ptr(), mem["cl"].data_ptr()
    add = dict(who="ifd_add_attack", rows="num_add outside [1, 1024]", low=16,
               pointers="pc_in, target, pc_out, best_dist, success",
               without="[num_add, min(2048, out_stride - num_add)]",
               params=lambda size, kind, loss, steps, it, rows: _lib.IfdAddParams(size, kind, loss, steps, it, rows[0], 0.0, 0.5, 0.01, 5e3, 4e4),
               size=C.sizeof(_lib.IfdAddParams), good=(16,), bad=((0,), (1025,)), extra=lambda: [None], missing=())
    cluster = dict(who="ifd_cluster_attack", rows=ROWS % ("cl_num_p", "cl_num_p"), low=1,
                   pointers="pc_in, target, clusters, pc_out, best_dist, success",
                   without="[1, min(2048, out_stride - num_add * cl_num_p)]",
                   params=lambda size, kind, loss, steps, it, rows: _lib.IfdClusterParams(size, loss, steps, it, rows[0], rows[1], 0.0, 0.5, 0.01,
                                                                                         5., 30.),
                   size=C.sizeof(_lib.IfdClusterParams), good=(4, 4), bad=((0, 4), (4, 0), (33, 32), (1025, 1)), extra=lambda: [cl, None],
                   missing=([None, None],))
    objects = dict(who="ifd_object_attack", rows=ROWS % ("obj_num_p", "obj_num_p"), low=1,
                   pointers="pc_in, target, objects, centers, angles0, pc_out, best_dist, success",
                   without="[1, min(2048, out_stride - num_add * obj_num_p)]",
                   params=lambda size, kind, loss, steps, it, rows: _lib.IfdObjectParams(size, loss, steps, it, rows[0], rows[1], 0.0, 0.5, 0.01,
                                                                                        5., 40.),
                   size=C.sizeof(_lib.IfdObjectParams), good=(2, 8), bad=((0, 8), (2, 0), (33, 32), (1025, 1)),
                   extra=lambda: [P, P, None, None, P], missing=([None, P, None, None, P], [P, None, None, None, P], [P, P, None, None, None]))
    return {"add": add, "cluster": cluster, "objects": objects}


@pytest.mark.parametrize("name", ["add", "cluster", "objects"])
def test_attack_calls(net, mem, name):
    """B = 2, stride 64, out_stride 80, 16 added rows (Add: 16; Cluster: 4 x 4; Objects: 2 x 8)."""
    a = _attacks(mem)[name]
    P, T = mem["big"].data_ptr(), mem["tt"].data_ptr()
    o, best, ok = mem["o"], mem["best"], mem["ok"]
    c = Calls(net, a["who"])

    def attack(text, stride=64, out_stride=80, rows=a["good"], kind=0, loss=0, steps=1, it=1, size=a["size"], n=None, B=2, out=None,
               extra=None, target=T, best_ptr=best.data_ptr(), params=True):
        prm = a["params"](size, kind, loss, steps, it, rows)
        c.refused(text, C.byref(prm) if params else None, P, None if n is None else n.data_ptr(), target,
                  *(a["extra"]() if extra is None else extra), B, stride, out_stride, o.data_ptr() if out is None else out, best_ptr,
                  ok.data_ptr(), None, None)
    attack("params missing or of another struct_size", size=40)
    attack("params missing or of another struct_size", params=False)
    if name == "add":
        attack("unknown kind", kind=2)
        attack("unknown kind", kind=2, loss=5)                                          # the order
    attack("unknown loss_kind", loss=5)
    attack("binary_step < 1", steps=0)
    attack("num_iter < 1", it=0)
    for rows in a["bad"]:
        attack(a["rows"], rows=rows, out_stride=3100)
    attack("B >= 1 is needed", B=0)
    attack("stride outside [1, 10000]", stride=10001)
    attack("out_stride outside [1, 10000]", out_stride=10001)
    attack("out_stride outside [1, 10000]", out_stride=0)
    missing = "missing pointer (" + a["pointers"] + ")"
    attack(missing, best_ptr=None)
    attack(missing, target=None)
    for extra in a["missing"]:
        attack(missing, extra=extra)
    without = "without n_points, stride outside " + a["without"]
    attack(without, stride=2049, out_stride=3100)
    attack(without, out_stride=79)
    if name == "add":
        attack(without, stride=15)
    attack("pc_out overlaps pc_in", out=P)
    attack("pc_out overlaps pc_in", out=P + 12)
    # two rules broken at once: the earlier check answers
    attack("unknown loss_kind", loss=5, steps=0)
    attack("binary_step < 1", steps=0, it=0)
    attack("num_iter < 1", it=0, rows=a["bad"][0])
    attack(a["rows"], rows=a["bad"][0], B=0)
    attack("B >= 1 is needed", B=0, stride=10001)
    attack("stride outside [1, 10000]", stride=10001, out_stride=10001)
    attack("out_stride outside [1, 10000]", out_stride=10001, best_ptr=None)
    attack(missing, best_ptr=None, out=P)
    attack(missing, best_ptr=None, out_stride=79)
    attack(without, out_stride=79, out=P)
    # the blocking check on the device: counts first, then targets
    lo = a["low"]
    attack("1 cloud(s) with n_points outside [%d, 64]" % lo, n=counts(64, lo - 1))
    attack("2 cloud(s) with n_points outside [%d, 64]" % lo, n=counts(65, lo - 1))
    attack("1 cloud(s) with n_points outside [%d, 54]" % lo, out_stride=70, n=counts(55, 54))
    bad_target = torch.tensor([0, 40], dtype=torch.int32).cuda()
    attack("1 target(s) outside [0, 40)", target=bad_target.data_ptr())
    attack("1 cloud(s) with n_points outside [%d, 64]" % lo, n=counts(65, 64), target=bad_target.data_ptr())
    torch.cuda.synchronize()
    assert not o.any() and not ok.any() and not best.any()
