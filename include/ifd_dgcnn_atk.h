/*
 * ifd_dgcnn_atk.h - C ABI of the attack primitives on the DGCNN victim in libifd.so: the gradient of an adversarial loss on
 * the DGCNN logits with respect to the input points, and on top of it the FGM family of the reference
 * (baselines/attack/FGM/FGM.py: FGM, I-FGM, MI-FGM, PGD).  Exported from the same library as include/ifd.h and versioned on
 * its own; the conventions of ifd.h hold (int status, device pointers, `stream` = hipStream_t as void*, calls only enqueue
 * work except where noted).  Every call takes a context made by ifd_dgcnn_create (include/ifd_dgcnn.h); the calls of
 * include/ifd_atk.h keep refusing such a context, and these refuse every other.
 *
 * Clouds are point-major, [B][stride][3], cloud b being its first n_points[b] rows, exactly as in ifd_dgcnn_forward:
 * k <= n_points[b] <= stride <= IFD_DGCNN_MAX_POINTS.  The losses, IFD_ATK_LOSS_*, the update kinds, IFD_FGM_*, and
 * ifd_fgm_params are those of include/ifd_atk.h.
 */
#ifndef IFD_DGCNN_ATK_H
#define IFD_DGCNN_ATK_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#include "ifd_dgcnn.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_DGCNN_ATK_ABI_VERSION 1

int ifd_dgcnn_atk_abi_version(void);

/* Optional outputs of ifd_dgcnn_input_grad (each pointer, and each of idx's and win_edge's four, may be NULL):
 *   logits      [B][40]
 *   loss        [B]                     the cloud's own loss (not scaled)
 *   pred        [B]                     argmax of the logits, the lowest class among equals
 *   idx[l]      [B][stride][k]          the neighbour tables, as in ifd_dgcnn_aux
 *   feat        [B][stride][512]        x1 | x2 | x3 | x4
 *   global_feat [B][2048]               max | mean of the conv5 output
 *   win_pool    [B][1024] int32         the point each channel of conv5's max-pool was taken from
 *   win_edge[l] [B][stride][Cout_l]     int32, Cout = 64, 64, 128, 256: the point index j* of the neighbour that holds the
 *                                       maximum of P_j[c] in edge convolution l + 1
 *   act5        [B][stride][32] uint32  bit c % 32 of word c / 32 is set where conv5's pre-activation of channel c is > 0
 * logits, pred, idx, feat and global_feat are bit for bit what ifd_dgcnn_forward returns for the same input.  Rows beyond
 * n_points[b] of idx, feat, win_edge and act5 are left as they were.  The last three are the discrete choices of the backward
 * pass, so that a float64 oracle can be given them. */
typedef struct ifd_dgcnn_grad_out {
    float* logits;
    float* loss;
    int32_t* pred;
    int32_t* idx[4];
    float* feat;
    float* global_feat;
    int32_t* win_pool;
    int32_t* win_edge[4];
    uint32_t* act5;
} ifd_dgcnn_grad_out;

/* grad [B][stride][3] = scale * d loss_b / d pc[b]; rows at or beyond n_points[b] are written as zeros.  The losses are those
 * of ifd_cls_input_grad (ifd_atk.h), with its rules: the hinge at exactly 0 passes the gradient, the first index among equal
 * runner-up logits takes it.  No gradient flows through the neighbour choice (topk's indices are not differentiable in the
 * reference either): this is the gradient of the network with its four neighbour tables held fixed.
 * target: [B] int32 on the device, 0 <= target[b] < 40.  A bad count or target is IFD_ERR_ARG and nothing else is enqueued;
 * they live on the device, so EVERY call blocks the host once, until a checking kernel enqueued on `stream` has run.
 *
 * Forward half: ifd_dgcnn_forward's own kernels on the same numbers.
 * Discrete choices.  LeakyReLU's derivative is 1 where the forward's value is > 0 and 0.2 elsewhere (zero is on the 0.2 side,
 * as in torch): in the head and the edge convolutions from the saved activations, in conv5 from its pre-activations, which are
 * recomputed per 64-point tile in the forward's own order of operations and so are the forward's bits.  conv5's max-pool routes
 * its gradient to the LOWEST point index among equal values.  In an edge convolution, out_i = leaky(max_j P_j + Q_i), the
 * maximum's gradient goes to the neighbour j* with the LOWEST point index among equal P values.
 * Order of every sum:
 *   head        the transposed layers on v_mfma_f32_16x16x4_f32, per output four fused chains over interleaved 16-input groups
 *               added pairwise, (c0 + c1) + (c2 + c3) - the forward's layer arithmetic with a zero bias;
 *   conv5       dY[i][c] = leaky'(y[i][c]) * (g_mean[c] / n + (i == win[c] ? g_max[c] : 0));  dfeat[i][0..512) is ONE chain over
 *               the 1024 channels on the same instruction: chunks of 64 channels ascending, in a chunk the 16-channel groups
 *               ascending, in a group the instruction's four steps e = 0 .. 3, each summing the channels e, 4 + e, 8 + e, 12 + e;
 *   edge conv   dQ_i[c] = s = leaky'(out_i[c]) * dout_i[c];  dP_j[c] = the sum of s over the points i whose j* is j, in
 *               ASCENDING i;  dx = [dP | dQ] . [Wa ; Wb - Wa] as a transposed layer like the head's;  the layers are dense, so
 *               dx is then added to what conv5 left in those columns (conv5's term first);  layer 1: per coordinate one fused chain
 *               over the 64 rows of P, then the 64 of Q.
 * No float atomics anywhere.  A cloud's gradient does not depend on B, on its position in the batch, on stride, on the chunking
 * or on the other clouds, bit for bit.
 * P | Q of each edge convolution are recomputed, not kept.  The batch runs in chunks of up to 128 clouds over context workspace of
 *     7684 * stride + 20 * k * stride + 8192 * ceil(stride / 64) + 31144   bytes per cloud of a chunk (+ 1280),
 * (17.8 MB a cloud at stride 2048 and k = 20, 8.9 MB at 1024), grown on demand: ifd_dgcnn_forward's, the other three neighbour
 * tables, d loss / d feat, one layer's winners and the head's vectors. */
int ifd_dgcnn_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, const int32_t* target,
                         int loss_kind, float kappa, float scale, float* grad, const ifd_dgcnn_grad_out* out, void* stream);

/* ifd_fgm_update (ifd_atk.h) on a DGCNN context: the same kernel, arguments and semantics, with 1 <= stride <= 2048. */
int ifd_dgcnn_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum,
                         float step_size, float budget, float mu, const int32_t* n_points, int B, int stride, void* stream);

/* The whole attack: num_iter x (ifd_dgcnn_input_grad, ifd_dgcnn_fgm_update) on a copy of pc_in, then ifd_dgcnn_forward on the
 * result.  pc_out [B][stride][3] (must not be pc_in), success [B] int32 = (pred == target) of that last forward.  ori_pc IS
 * pc_in; the start noise is the caller's, as in ifd_fgm_attack.  Counts and targets are checked once at the start (the one
 * blocking step); nothing blocks after it.
 * Workspace: ifd_dgcnn_input_grad's, + 24 * stride + 164 bytes per cloud of the WHOLE batch. */
int ifd_dgcnn_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points,
                         const int32_t* target, int B, int stride, float* pc_out, int32_t* success, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_DGCNN_ATK_H */
