"""Lifetime of a context's buffers on the GPU (csrc/api.cpp, csrc/ifd_host.h).

Growth: every context buffer that grows on demand and has no stale-workspace test elsewhere (ws_enc, adam_tab and ws, ws_fold,
ws_dup; the classifier, attack and MISE workspaces have theirs) sees a small call, a larger one - the buffer is freed and
allocated again - and the small call again; both small results must equal, bit for bit, the same call on a fresh context.
Create / close: three contexts of each kind, one after the other in one process, each making the smallest call of its kind; the
three outputs must be equal bit for bit.  The DGCNN, PointNet++ and PointConv victims have both tests, on ``logits``.  Seeded weights and inputs throughout.  Nothing here looks at the free
device memory: other processes move it."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _rand(seed, *shape, scale=0.4):
    return torch.from_numpy(np.random.default_rng(seed).uniform(-scale, scale, size=shape).astype(np.float32))


@pytest.fixture(scope="module")
def conv_w():
    import ifdefense_amd as I
    from oracle import convonet_oracle as O
    return I.weights.pack_state_dict(O.make_random_weights(0))


@pytest.fixture(scope="module")
def onet_w():
    import ifdefense_amd as I
    from oracle import onet_oracle as OO
    return I.weights.pack_state_dict(OO.make_random_weights(0), "onet")


@pytest.fixture(scope="module")
def punet_w():
    import ifdefense_amd as I
    import punet_oracle as PO
    return I.weights.pack_state_dict(PO.make_weights(1), "punet")


@pytest.fixture(scope="module")
def cls_w():
    import ifdefense_amd as I
    return I.weights.pack_state_dict(I.weights.pointnet_random_state_dict(1), "pointnet")


def _small_large_small(make, call, sizes):
    """call(ctx, size) on one context at sizes (small, large, small), and at small on a fresh context: all three small results
    are the same bits."""
    small, large = sizes[0], sizes[1]
    assert sizes[2] == small
    fresh = make()
    want = call(fresh, small).cpu()
    fresh.close()
    ctx = make()
    first = call(ctx, small).cpu()
    call(ctx, large)
    again = call(ctx, small).cpu()
    ctx.close()
    assert torch.isfinite(want).all()
    assert torch.equal(first, want), "the first small call differs from a fresh context's"
    assert torch.equal(again, want), "the small call behind a larger one differs from a fresh context's"


def test_encoder_scratch_grows(conv_w):
    import ifdefense_amd as I
    sel = _rand(11, 2, 16, 3)
    _small_large_small(lambda: I.Restorer(conv_w, device=DEV), lambda r, B: r.encode_inputs(sel[:B]), (1, 2, 1))


def test_optimiser_workspace_and_adam_table_grow(conv_w):
    import ifdefense_amd as I
    pre = I.Restorer(conv_w, device=DEV)
    planes = pre.encode_inputs(_rand(12, 2, 16, 3))
    pre.close()
    init = _rand(13, 2, 33, 3)
    _small_large_small(lambda: I.Restorer(conv_w, device=DEV),
                       lambda r, bi: r.optimize_points(init[:bi[0]], planes[:bi[0]], rep_weight=500.0, iterations=bi[1], normalize=False),
                       ((1, 2), (2, 5), (1, 2)))


def test_onet_fold_buffer_grows(onet_w):
    import ifdefense_amd as I
    c, p = _rand(14, 3, 512, scale=1.0), _rand(15, 3, 7, 3)
    _small_large_small(lambda: I.OnetRestorer(onet_w, device=DEV), lambda r, B: r.decode(p[:B], c[:B]), (1, 3, 1))


def test_punet_scratch_grows(punet_w):
    import ifdefense_amd as I
    x = _rand(16, 2, 1024, 3, scale=0.9)
    _small_large_small(lambda: I.DupNet(punet_w, device=DEV, seed=3), lambda d, B: d.pu_net(x[:B]), (1, 2, 1))


def _three_lives(make, call):
    outs = []
    for _ in range(3):
        ctx = make()
        outs.append(call(ctx).cpu())
        ctx.close()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[1], outs[0]) and torch.equal(outs[2], outs[0])


def test_create_call_close_three_times_convonet(conv_w):
    import ifdefense_amd as I
    sel = _rand(21, 1, 16, 3)
    _three_lives(lambda: I.Restorer(conv_w, device=DEV), lambda r: r.encode_inputs(sel))


def test_create_call_close_three_times_onet(onet_w):
    import ifdefense_amd as I
    c, p = _rand(22, 1, 512, scale=1.0), _rand(23, 1, 7, 3)
    _three_lives(lambda: I.OnetRestorer(onet_w, device=DEV), lambda r: r.decode(p, c))


def test_create_call_close_three_times_dup(punet_w):
    import ifdefense_amd as I
    x = _rand(24, 1, 1024, 3, scale=0.9)
    _three_lives(lambda: I.DupNet(punet_w, device=DEV, seed=3), lambda d: d.pu_net(x))


def test_create_call_close_three_times_classifier(cls_w):
    import ifdefense_amd as I
    pc = _rand(25, 1, 1, 3, scale=0.9)                  # one cloud of one point
    _three_lives(lambda: I.Classifier(cls_w, device=DEV), lambda k: k.logits(pc))


# ---- the two later victims: DGCNN (include/ifd_dgcnn.h) and PointNet++ (include/ifd_pn2.h) -------------------------------------
@pytest.fixture(scope="module")
def dgcnn_w():
    import ifdefense_amd as I
    return I.weights.pack_state_dict(I.weights.dgcnn_random_state_dict(1), "dgcnn")


@pytest.fixture(scope="module")
def pn2_w():
    import ifdefense_amd as I
    return I.weights.pack_state_dict(I.weights.pointnet2_random_state_dict(1), "pointnet2")


VICTIM_CALLS = (0, 1, 0)                                # 1 x 64 points, 2 x 2048, 1 x 64: a cloud's workspace grows 32-fold


def _victim_logits(k, which):
    return k.logits(_rand(31 + which, (1, 2)[which], (64, 2048)[which], 3, scale=0.9))


def test_create_call_close_three_times_dgcnn(dgcnn_w):
    import ifdefense_amd as I
    pc = _rand(26, 1, 20, 3, scale=0.9)                 # one cloud of k points
    _three_lives(lambda: I.DgcnnClassifier(dgcnn_w, device=DEV), lambda k: k.logits(pc))


def test_create_call_close_three_times_pointnet2(pn2_w):
    import ifdefense_amd as I
    pc = _rand(27, 1, 1, 3, scale=0.9)                  # one cloud of one point
    _three_lives(lambda: I.PointNet2Classifier(pn2_w, device=DEV), lambda k: k.logits(pc))


def test_dgcnn_workspace_grows(dgcnn_w):
    import ifdefense_amd as I
    _small_large_small(lambda: I.DgcnnClassifier(dgcnn_w, device=DEV), _victim_logits, VICTIM_CALLS)


def test_pointnet2_workspace_grows(pn2_w):
    import ifdefense_amd as I
    _small_large_small(lambda: I.PointNet2Classifier(pn2_w, device=DEV), _victim_logits, VICTIM_CALLS)


# ---- PointConv (include/ifd_pc.h): the largest workspace of the victims, 5.9 MB a cloud, chunks of 32 ------------------------------
@pytest.fixture(scope="module")
def pc_w():
    import ifdefense_amd as I
    return I.weights.pack_state_dict(I.weights.pointconv_random_state_dict(1), "pointconv")


def _pointconv_logits(k, which):                        # 1 x 32 points (the smallest cloud PointConv takes), 2 x 2048, 1 x 32
    return k.logits(_rand(41 + which, (1, 2)[which], (32, 2048)[which], 3, scale=0.9))


def test_create_call_close_three_times_pointconv(pc_w):
    import ifdefense_amd as I
    pc = _rand(28, 1, 32, 3, scale=0.9)                 # one cloud of 32 points
    _three_lives(lambda: I.PointConvClassifier(pc_w, device=DEV), lambda k: k.logits(pc))


def test_pointconv_workspace_grows(pc_w):
    import ifdefense_amd as I
    _small_large_small(lambda: I.PointConvClassifier(pc_w, device=DEV), _pointconv_logits, VICTIM_CALLS)
