/*
 * ifd_pn2_atk.h - C ABI of the attack primitives on the PointNet++ victim in libifd.so: the gradient of an adversarial loss on
 * the PointNet++ logits with respect to the input points, and on top of it the FGM family of the reference
 * (baselines/attack/FGM/FGM.py: FGM, I-FGM, MI-FGM, PGD).  Exported from the same library as include/ifd.h and versioned on
 * its own; the conventions of ifd.h hold (int status, device pointers, `stream` = hipStream_t as void*, calls only enqueue
 * work except where noted).  Every call takes a context made by ifd_pn2_create (include/ifd_pn2.h); the calls of
 * include/ifd_atk.h and include/ifd_dgcnn_atk.h keep refusing such a context, and these refuse every other.
 *
 * Clouds are point-major, [B][stride][3], cloud b being its first n_points[b] rows, and fps_start [B][2] holds the first picks
 * of the two samplings, exactly as in ifd_pn2_forward: 1 <= n_points[b] <= stride <= IFD_PN2_MAX_POINTS.  The losses,
 * IFD_ATK_LOSS_*, the update kinds, IFD_FGM_*, and ifd_fgm_params are those of include/ifd_atk.h.
 */
#ifndef IFD_PN2_ATK_H
#define IFD_PN2_ATK_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#include "ifd_pn2.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_PN2_ATK_ABI_VERSION 1

int ifd_pn2_atk_abi_version(void);

/* Optional outputs of ifd_pn2_input_grad (each pointer may be NULL):
 *   logits      [B][40]
 *   loss        [B]                        the cloud's own loss (not scaled)
 *   pred        [B]                        argmax of the logits, the lowest class among equals
 *   fps1, fps2, ball1, ball2, l1_feat, l2_feat, global_feat      as in ifd_pn2_aux
 *   win1        [B][512][128] int32        the sample position 0 .. 31 that holds the maximum of sa1's group i, channel c
 *   win2        [B][128][256] int32        the sample position 0 .. 63, sa2
 *   win3        [B][1024] int32            the row 0 .. 127, sa3
 *   act1        [B][512][32][4] uint32     per row of sa1: words 0, 1 the first hidden layer's 64 channels, words 2, 3 the second's
 *   act2        [B][128][64][8] uint32     per row of sa2: words 0 .. 3 the first hidden layer's 128 channels, 4 .. 7 the second's
 *   act3        [B][128][24] uint32        per row of sa3: words 0 .. 7 the first layer's 256 channels, 8 .. 23 the second's 512
 * Bit c % 32 of a layer's word c / 32 is set where the pre-activation of its channel c is > 0.  logits, pred, the tables and
 * the features are bit for bit what ifd_pn2_forward returns for the same input.  A winner of -1 would say that no row of the
 * recomputed tile holds the saved maximum; it does not occur.  The win and act arrays are the discrete choices of the backward
 * pass, so that a float64 oracle can be given them. */
typedef struct ifd_pn2_grad_out {
    float* logits;
    float* loss;
    int32_t* pred;
    int32_t* fps1;
    int32_t* fps2;
    int32_t* ball1;
    int32_t* ball2;
    float* l1_feat;
    float* l2_feat;
    float* global_feat;
    int32_t* win1;
    int32_t* win2;
    int32_t* win3;
    uint32_t* act1;
    uint32_t* act2;
    uint32_t* act3;
} ifd_pn2_grad_out;

/* grad [B][stride][3] = scale * d loss_b / d pc[b]; rows at or beyond n_points[b] are written as zeros.  The losses are those
 * of ifd_cls_input_grad (ifd_atk.h), with its rules: the hinge at exactly 0 passes the gradient, the first index among equal
 * runner-up logits takes it.  This is the gradient of the network with its four index tables held fixed - fps1, fps2, ball1,
 * ball2 as the forward computes them from the current pc: farthest_point_sample and query_ball_point return indices, which carry
 * no gradient in the reference either.  The centroids' coordinates do carry gradient, through new_xyz = index_points(xyz, fps)
 * and grouped_xyz - new_xyz.  Clouds of fewer than 512 points repeat centroids and balls are padded with their first member;
 * both are rows like any other.
 * target: [B] int32 on the device, 0 <= target[b] < 40.  A bad count, start or target is IFD_ERR_ARG and nothing else is
 * enqueued; they live on the device, so EVERY call blocks the host once, until two checking kernels enqueued on `stream` have run.
 *
 * Forward half: ifd_pn2_forward's own kernels on the same numbers.
 * Discrete choices.  ReLU's derivative is 1 exactly where the forward's value is > 0 (zero is on the 0 side, as in torch): in
 * the head and in sa3's two hidden layers from the saved activations; in the last layer of every level from the saved feature;
 * in the hidden layers of sa1 and sa2 from the group tile, which the backward kernel recomputes with the forward's own
 * instruction sequence, so that the gates are the forward's bits.  A group maximum routes its gradient to the LOWEST sample
 * position (sa1: of 32, sa2: of 64; sa3: the lowest of the 128 rows) whose recomputed activation equals the saved feature.
 * The gradient of a point is the sum of:
 *   (a) + dd(i, s) for every row (i, s) with ball1[i][s] == p, dd = W1^T dH1 the gradient of the row's difference to its centroid;
 *   (b) d xyz1[i] for every i with fps1[i] == p, where
 *       d xyz1[i] = - sum_s dd(i, s) + sum of de(g, s) over the sa2 rows with ball2[g][s] == i + sum of d xyz2[g] over fps2[g] == i,
 *       d xyz2[g] = - sum_s de(g, s) + the three coordinate columns of sa3's first layer transposed.
 * Order of every sum:
 *   head, sa3's 512 -> 256 and 256 -> [3 | 256], sa2's U -> l1_feat
 *               transposed layers on v_mfma_f32_16x16x4_f32 in the forward's layer arithmetic with a zero bias: the inputs in
 *               blocks of 64, ascending, a block four fused chains from 0 over its 16-input groups added (c0 + c1) + (c2 + c3);
 *   last layers (sa3 1024 -> 512, sa2 256 -> 128, sa1 128 -> 64), sparse: per row and input k ONE fused chain over the channels
 *               c that the row won, in ascending c, of d feat[c] * W[c][k] (channels whose saved feature is not > 0 add zeros);
 *   middle layers of sa2 (128 x 128) and sa1 (64 x 64): dense on the same MFMA, blocks of 64 as above;
 *   first layers per row: a fused chain per quarter of the channels, ascending (sa2: 32 channels, sa1: 16), the quarters added
 *               (q0 + q1) + (q2 + q3);
 *   - sum_s     ((0 - t_0) - t_1) - ... in ascending sample position, then + the term from the level above;
 *   scatters    rows -> level-1 points (dU_j and de), rows -> cloud points (dd), centroids -> points: the receiving point walks
 *               the cloud's rows (g, s) resp. (i, s) in ASCENDING order and adds those that name it, one chain from 0; d xyz1[j]
 *               continues that chain with d xyz2[g] over fps2[g] == j in ascending g, and grad[p] continues its chain with
 *               d xyz1[i] over fps1[i] == p in ascending i.
 * No float atomics anywhere, and no kernel looks at another cloud's rows.  A cloud's gradient does not depend on B, on its
 * position in the batch, on stride, on padding, on the chunking or on the other clouds, bit for bit.
 * sa1's and sa2's tiles are recomputed, not kept.  The batch runs in the forward's chunks of up to 128 clouds over context
 * workspace of
 *     1,172,480 (ifd_pn2_forward's) + 5,668,264 = 6,840,744 bytes per cloud of a chunk (+ 1280),
 * grown on demand, whatever the stride: sa2's first-layer gradient per row (4 MB a cloud) is most of it. */
int ifd_pn2_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride,
                       const int32_t* target, int loss_kind, float kappa, float scale, float* grad, const ifd_pn2_grad_out* out,
                       void* stream);

/* ifd_fgm_update (ifd_atk.h) on a PointNet++ context: the same kernel, arguments and semantics, with 1 <= stride <= 2048. */
int ifd_pn2_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum,
                       float step_size, float budget, float mu, const int32_t* n_points, int B, int stride, void* stream);

/* The whole attack: num_iter x (ifd_pn2_input_grad, ifd_pn2_fgm_update) on a copy of pc_in, then ifd_pn2_forward on the
 * result, all with the same fps_start.  pc_out [B][stride][3] (must not be pc_in), success [B] int32 = (pred == target) of that
 * last forward.  ori_pc IS pc_in; the start noise is the caller's, as in ifd_fgm_attack.  Counts, starts and targets are checked
 * once at the start (the one blocking step); nothing blocks after it.
 * Workspace: ifd_pn2_input_grad's, + 24 * stride + 164 bytes per cloud of the WHOLE batch. */
int ifd_pn2_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points,
                       const int32_t* fps_start, const int32_t* target, int B, int stride, float* pc_out, int32_t* success,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_PN2_ATK_H */
