/*
 * ifd_pc_atk.h - C ABI of the attack primitives on the PointConv victim in libifd.so: the gradient of an adversarial loss on
 * the PointConv logits with respect to the input points, and on top of it the FGM family of the reference
 * (baselines/attack/FGM/FGM.py: FGM, I-FGM, MI-FGM, PGD).  Exported from the same library as include/ifd.h and versioned on
 * its own; the conventions of ifd.h hold (int status, device pointers, `stream` = hipStream_t as void*, calls only enqueue
 * work except where noted).  Every call takes a context made by ifd_pc_create (include/ifd_pc.h); the calls of
 * include/ifd_atk.h, include/ifd_dgcnn_atk.h and include/ifd_pn2_atk.h keep refusing such a context, and these refuse every other.
 *
 * Clouds are point-major, [B][stride][3], cloud b being its first n_points[b] rows, and fps_start [B][2] holds the first picks
 * of the two samplings, exactly as in ifd_pc_forward: 32 <= n_points[b] <= stride <= IFD_PC_MAX_POINTS.  The losses,
 * IFD_ATK_LOSS_*, the update kinds, IFD_FGM_*, and ifd_fgm_params are those of include/ifd_atk.h.
 */
#ifndef IFD_PC_ATK_H
#define IFD_PC_ATK_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#include "ifd_pc.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_PC_ATK_ABI_VERSION 1

int ifd_pc_atk_abi_version(void);

/* Optional outputs of ifd_pc_input_grad (each pointer may be NULL):
 *   logits      [B][40]
 *   loss        [B]                        the cloud's own loss (not scaled)
 *   pred        [B]                        argmax of the logits, the lowest class among equals
 *   fps1, fps2, knn1, knn2, dens1, dens2, dens3, l1_feat, l2_feat, global_feat      as in ifd_pc_aux
 *   dgate1      [B][stride] uint32         DensityNet of every point of the cloud (rows beyond n_points are not written): bits
 *                                          0 .. 7 its first layer's channels, 8 .. 15 the second's, 16 its output
 *   dgate2      [B][512] uint32            ... of the level-1 centroids
 *   dgate3      [B][128] uint32            ... of the level-2 centroids
 *   wgate1      [B][512][32] uint32        WeightNet of every row of sa1: bits 0 .. 7 the first layer, 8 .. 15 the second, 16 .. 31
 *                                          the third
 *   wgate2      [B][128][64] uint32        ... of sa2
 *   wgate3      [B][128] uint32            ... of sa3
 *   mgate1      [B][512][32][8] uint32     the MLP per row of sa1: words 0, 1 the first layer's 64 channels, 2, 3 the second's 64,
 *                                          4 .. 7 the third's 128
 *   mgate2      [B][128][64][16] uint32    sa2: words 0 .. 3 (128 channels), 4 .. 7 (128), 8 .. 15 (256)
 *   mgate3      [B][128][56] uint32        sa3: words 0 .. 7 (256), 8 .. 23 (512), 24 .. 55 (1024)
 * A bit is set where the pre-activation of its channel is > 0: bit c % 32 of a layer's word c / 32.  logits, pred, the tables,
 * the densities and the features are bit for bit what ifd_pc_forward returns for the same input.  The gate arrays are the
 * discrete choices of the backward pass, so that a float64 oracle can be given them. */
typedef struct ifd_pc_grad_out {
    float* logits;
    float* loss;
    int32_t* pred;
    int32_t* fps1;
    int32_t* fps2;
    int32_t* knn1;
    int32_t* knn2;
    float* dens1;
    float* dens2;
    float* dens3;
    float* l1_feat;
    float* l2_feat;
    float* global_feat;
    uint32_t* dgate1;
    uint32_t* dgate2;
    uint32_t* dgate3;
    uint32_t* wgate1;
    uint32_t* wgate2;
    uint32_t* wgate3;
    uint32_t* mgate1;
    uint32_t* mgate2;
    uint32_t* mgate3;
} ifd_pc_grad_out;

/* grad [B][stride][3] = scale * d loss_b / d pc[b]; rows at or beyond n_points[b] are written as zeros.  The losses are those
 * of ifd_cls_input_grad (ifd_atk.h), with its rules: the hinge at exactly 0 passes the gradient, the first index among equal
 * runner-up logits takes it.  This is the gradient of the network of ifd_pc_forward with its four index tables held fixed - fps1,
 * fps2, knn1, knn2 as the forward computes them from the current pc: farthest_point_sample and knn_point return indices, which
 * carry no gradient in the reference either.  Everything else carries gradient, as in the reference's autograd.
 * target: [B] int32 on the device, 0 <= target[b] < 40.  A bad count, start or target is IFD_ERR_ARG and nothing else is
 * enqueued; they live on the device, so EVERY call blocks the host once, until two checking kernels enqueued on `stream` have run.
 *
 * Forward half: ifd_pc_forward's own kernels on the same numbers.
 * A level (sa1: rows (i, k), j = knn1[i][k], the cloud; sa2: j = knn2[i][k], the 512; sa3: one group, j = k, centre the mean)
 * computes, with delta = x_j - c_i:  F = MLP([delta | f_j]),  Wn = WeightNet(delta),  s_j = DensityNet(rho_j),  t = F * s_j,
 * G[c][w] = sum_k t[k][c] Wn[k][w],  Y_i = relu(W_l vec(G) + b_l).  Its backward:
 *     dG = W_l^T (dY where the saved Y > 0),    dt[c] = sum_w dG[c][w] Wn[k][w],    dWn[w] = sum_c dG[c][w] t[k][c],
 *     dF = dt * s_j where F > 0,    ds_j += sum_c dt[c] F[k][c],
 * dF through the MLP's three layers gives d delta from the coordinate columns and, at sa2 and sa3, d f_j; dWn through WeightNet
 * 16 -> 8 -> 8 -> 3 gives a second d delta, and d delta(i, k) is their sum (MLP's + WeightNet's).
 * Discrete choices.  ReLU's derivative is 1 exactly where the forward's value is > 0 (zero is on the 0 side, as in torch): in the
 * head, in sa3's MLP and behind every wide linear from the saved activations; in sa1's and sa2's MLPs, in every WeightNet and
 * DensityNet from values that the backward kernels recompute with the forward's own instruction sequence, so that the gates are the
 * forward's bits.  DensityNet has ReLU after all three layers (ifd_pc.h), so all three gate.
 * The gradient of a point is the sum of:
 *   (a) + d delta(i, k) for every row of sa1 that names it;
 *   (b) - sum_k d delta(i, k) for the centroid it is, through fps1, and through fps2 for the level-2 centroids: centroids repeat on
 *       clouds of fewer than 512 points, and every repeat is a row like any other;
 *   (c) sa3's centre is the mean of the 128 level-2 centroids: xyz2[g] receives d delta(g) - (1/128) sum_g' d delta(g');
 *   (d) the density of every level: ds_j through DensityNet gives d rho_j; with a_j = (d rho_j / (float)n) / c2 and
 *       e_pj = expf(-(d_pj / c1)) point p of the level's n input points receives (2 / c1) * sum_j ((a_p + a_j) * e_pj) * (x_j - x_p);
 *       the self term and bit-identical copies contribute exactly zero;
 *   (e) at sa2 and sa3 all of this lands on xyz1 resp. xyz2 and continues down through (b).
 * Order of every sum:
 *   transposed dense layers (the head; the wide linears W_l^T of 16384, 4096 and 2048 outputs; sa3's 1024 -> 512 -> 256 -> [3 | 256];
 *               sa2's U -> l1_feat) on v_mfma_f32_16x16x4_f32 in the forward's layer arithmetic with a zero bias: the inputs in
 *               blocks of 64, ascending, a block four fused chains from 0 over its 16-input groups added (c0 + c1) + (c2 + c3);
 *   sa1, sa2    per row, the last layer's channels in passes of 64, ascending; in a pass the row's four quarters of 16 channels each
 *               run dt[c] = one fused chain from 0 over w ascending; dWn[w] = fma(dG[c][w], fl(F s_j), dWn[w]) and ds = fma(dt[c],
 *               F, ds) continue ONE chain per quarter over its 16 channels of every pass, and the quarters are added (q0 + q1) + (q2 +
 *               q3); dF = fl(dt * s_j).  The last layer transposed: one 64-input block per pass as above, the passes added in
 *               ascending order from 0.  The middle layer transposed: blocks of 64 as above.  The first layer's coordinate columns:
 *               a fused chain per quarter of the channels, ascending, the quarters added (q0 + q1) + (q2 + q3);
 *   sa3         per row, thread t of 256 takes c = t, t + 256, t + 512, t + 768 with the same chains; the 256 are added in a butterfly
 *               1, 2, ..., 32 within each 64 and the four 64s as (w0 + w1) + (w2 + w3);
 *   WeightNet, DensityNet backward: per layer one fused chain from 0 over the layer's outputs, ascending;
 *   d delta     fl(MLP's + WeightNet's);   - sum_k: ((0 - t_0) - t_1) - ... in the row's order, then + the term from above;
 *   (c)         per axis the 128 d delta = fl(MLP's + WeightNet's) added in ascending g from 0, times 1/128, subtracted;
 *   (d)         per axis lane l of 64 runs acc = fma(fl(fl(a_p + a_j) * e_pj), fl(x_j - x_p), acc) over j = l, l + 64, ... ascending
 *               from 0, the 64 partial sums meet in the butterfly 1, 2, ..., 32 (the forward density's order), times fl(2 / c1),
 *               added to what the point has received otherwise;
 *   scatters    rows -> level-1 points (dU_j, d delta and ds), rows -> cloud points (d delta and ds), centroids -> points: the
 *               receiving point walks the cloud's rows (g, k) resp. (i, k) in ASCENDING order and adds those that name it, one chain
 *               from 0; d xyz1[j] continues that chain with d xyz2[g] over fps2[g] == j in ascending g, then takes the level's
 *               density term; grad[p] continues its chain with d xyz1[i] over fps1[i] == p in ascending i, then the density term.
 * No float atomics anywhere, and no kernel looks at another cloud's rows.  A cloud's gradient does not depend on B, on its
 * position in the batch, on stride, on padding, on the chunking or on the other clouds, bit for bit.
 * sa1's and sa2's tiles are recomputed, not kept; dG of a level lives in the forward's contraction buffer, dead by then.  The batch
 * runs in the forward's chunks of up to 32 clouds over context workspace of
 *     5,903,360 (ifd_pc_forward's) + 6,244,264 = 12,147,624 bytes per cloud of a chunk (+ 1024, rounded up to 256),
 * grown on demand, whatever the stride: sa2's first-layer gradient per row (4 MB a cloud) is most of it. */
int ifd_pc_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride,
                      const int32_t* target, int loss_kind, float kappa, float scale, float* grad, const ifd_pc_grad_out* out,
                      void* stream);

/* ifd_fgm_update (ifd_atk.h) on a PointConv context: the same kernel, arguments and semantics, with 32 <= stride <= 2048. */
int ifd_pc_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum,
                      float step_size, float budget, float mu, const int32_t* n_points, int B, int stride, void* stream);

/* The whole attack: num_iter x (ifd_pc_input_grad, ifd_pc_fgm_update) on a copy of pc_in, then ifd_pc_forward on the
 * result, all with the same fps_start.  pc_out [B][stride][3] (must not be pc_in), success [B] int32 = (pred == target) of that
 * last forward.  ori_pc IS pc_in; the start noise is the caller's, as in ifd_fgm_attack.  Counts, starts and targets are checked
 * once at the start (the one blocking step); nothing blocks after it.
 * Workspace: ifd_pc_input_grad's, + 24 * stride + 164 bytes per cloud of the WHOLE batch. */
int ifd_pc_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points,
                      const int32_t* fps_start, const int32_t* target, int B, int stride, float* pc_out, int32_t* success,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_PC_ATK_H */
