/*
 * ifd_add.h - C ABI of the Carlini-Wagner point-adding attack ("Add", baselines/attack/CW/Add.py CWAdd with ChamferDist('adv2ori') or
 * HausdorffDist('adv2ori'), driven by baselines/attack_scripts/targeted_add_attack.py) on the PointNet victim, in libifd.so.
 * Built on ifd_cls_input_grad (include/ifd_atk.h) and on the state and the weight search of ifd_cw.h, versioned on its own; the
 * conventions of ifd_atk.h hold: int status, device pointers, `stream` = hipStream_t as void*, clouds point-major, contexts made by
 * ifd_cls_create WITHOUT feature_transform (any other is refused with IFD_ERR_ARG).  Every per-cloud reduction runs in one fixed
 * order (a thread's strided partial result, then a fixed tree over the workgroup's 256 threads), no float atomics: a cloud's
 * result does not depend on B, on its position in the batch or on the other clouds, bit for bit.
 *
 * A CONCATENATED cloud is what the victim sees: [B][cat_stride][3], cloud b holding n_ori[b] original rows and behind them num_add
 * added rows - what ifd_cls_input_grad takes with n_points[b] = n_ori[b] + num_add.  num_add is common to the batch.  Limits:
 *   1 <= num_add <= IFD_ADD_MAX_ADD;  num_add <= n_ori[b] <= IFD_ADD_MAX_ORI;  n_ori[b] + num_add <= cat_stride <= 10000
 * (the originals and the added points of one cloud live in a workgroup's static LDS, 36 KB).  Original rows and rows at or beyond
 * n_ori[b] + num_add are never written, rows beyond are never read.
 *
 * DEVIATIONS from the reference, all of rounding or of the caller's freedom, none of them a switch:
 *   - Distances are in difference form, fma(dz, dz, fma(dy, dy, dx * dx)) with d = adv_p - ori_j.  The reference expands
 *     |x|^2 - 2 x.y + |y|^2 from three bmm's: at its start, where every added point sits on an original, that gives min_p in
 *     [-2.4e-7, 2.4e-7], pure rounding, negative values included, so its first Hausdorff arg-max and first recorded distances are
 *     noise.  Here a coincident point has distance exactly 0.
 *   - Ties have an order.  Selection: among equal scores the lowest index comes first (torch.topk promises none, and at 1024
 *     points most clouds select among rows whose gradient is exactly zero).  Nearest original: the lowest index among equal
 *     distances, as torch's CPU min.  Hausdorff: the lowest added point among equal min_p.
 *   - The start noise is the caller's (the reference draws randn * 1e-7 on the GPU from the global stream).
 */
#ifndef IFD_ADD_H
#define IFD_ADD_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#include "ifd_cw.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_ADD_ABI_VERSION 1
#define IFD_ADD_CHAMFER 0            /* dist = sum_p min_p / num_add */
#define IFD_ADD_HAUSDORFF 1          /* dist = max_p min_p */
#define IFD_ADD_MAX_ADD 1024
#define IFD_ADD_MAX_ORI 2048

int ifd_add_abi_version(void);

/* The num_add rows of largest gradient norm (Add.py get_critical_points behind its backward pass); never blocks.
 *   grad, pc  [B][stride][3];  n_points [B] or NULL (then every cloud has `stride` rows);  rows at or beyond n_points[b] are never read
 *   cri  [B][num_add][3]  the selected rows of pc, bit for bit;  idx (may be NULL) [B][num_add] int32 their indices
 * score_p = (gx*gx + gy*gy) + gz*gz in float32, in that order and without contraction.  The output is the num_add rows of largest
 * score in descending score order; among equal scores the lowest index comes first.  That is a total order, so every bit of the
 * output is determined - this library's definition where torch.topk leaves the order among equals open.  (A NaN score is outside
 * the order; the result is then unspecified, but stays inside the arrays.)
 * One workgroup per cloud ranks by counting over the scores in LDS: rank_i = #{j : s_j > s_i or (s_j == s_i and j < i)}, O(n^2).
 * Refused on the host with IFD_ERR_ARG: a missing pointer, B < 1, num_add outside [1, 1024], stride outside [1, 10000], and with
 * n_points == NULL stride < num_add or stride > 2048.  A cloud whose n_points[b] is outside [num_add, min(stride, 2048)] is left
 * untouched (the counts live on the device and the call does not block). */
int ifd_add_select(ifd_ctx* ctx, const float* grad, const float* pc, const int32_t* n_points, int B, int stride, int num_add,
                   float* cri, int32_t* idx, void* stream);

/* get_critical_points whole: ifd_cls_input_grad(pc, target, IFD_ATK_LOSS_CE, kappa 0, scale) - the reference takes the gradient of
 * F.cross_entropy(logits, TARGET), a batch mean: scale = 1 / B_ref - followed by ifd_add_select.  Blocks once, as
 * ifd_cls_input_grad does: there n_points (outside [num_add, min(stride, 2048)]) and target are refused with IFD_ERR_ARG.
 * Workspace, grown on the context: ifd_cls_input_grad's + 12 * stride bytes per cloud of the WHOLE batch, rounded up to 256. */
int ifd_add_critical_points(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* target, int B, int stride,
                            int num_add, float scale, float* cri, int32_t* idx, void* stream);

/* Optional outputs of ifd_add_step, every one may be NULL (and `diag` itself): what lets a test judge the discrete decisions
 * exactly; they cost nothing when NULL. */
typedef struct ifd_add_diag {
    float* dist_grad;        /* [B][num_add][3]  the distance term of step 4, c * (adv_p - ori_j(p)), 0 where a point receives none */
    int32_t* nn_ori;         /* [B][num_add]     j(p), the nearest original */
    int32_t* far;            /* [B]              Hausdorff: the arg-max added point;  Chamfer: -1 */
} ifd_add_diag;

/* One iteration of Add.py:124-177 behind the forward / backward pass on the concatenated cloud; never blocks.
 *   kind   IFD_ADD_CHAMFER | IFD_ADD_HAUSDORFF
 *   state  ifd_cw_state with stride = num_add: m, v, o_bestattack are [B][num_add][3]; a fresh attack starts as ifd_cw.h says
 *   grad   [B][cat_stride][3], pred [B], loss [B] (may be NULL)   as ifd_cls_input_grad wrote them for `cat` with
 *          n_points[b] = n_ori[b] + num_add (grad already carries scale)
 *   cat    [B][cat_stride][3]  the concatenated clouds; the added rows are updated in place
 *   n_ori  [B] or NULL (then every cloud has cat_stride - num_add original rows)
 *   last_input (may be NULL) [B][num_add][3];  info (may be NULL) [B][3]
 *   t      the 1-based number of this Adam step within its search step;  lr  Adam's learning rate;  scale  the reference's 1 / B_ref
 * Per cloud, one workgroup, in this order:
 *   1. For each added point p: min_p = min_j |adv_p - ori_j|^2 in difference form and j(p) its argmin, strict < in ascending j
 *      (the lowest index among equals).
 *   2. dist, float32: Chamfer  (sum_p min_p) / num_add, each thread summing its points p = t, t + 256, ... in ascending order, then
 *      the fixed tree;  Hausdorff  max_p min_p and its arg-max, the lowest p among equals.
 *   3. The two records exactly as ifd_cw_step's step 2 (both comparisons strict, pred == target); o_bestattack and last_input take
 *      the added rows bit for bit, as they were forwarded, BEFORE the update.
 *   4. g_p = fma(c, adv_p - ori_j(p), grad[n_ori + p]) per coordinate, with
 *        Chamfer    c = (scale * (float)weight) * (2 / (float)num_add)      for every p
 *        Hausdorff  c = (scale * (float)weight) * 2                         for the arg-max p; every other p: g_p = grad[n_ori + p]
 *      autograd's gradient of mean_b(dist_b * weight_b) with the argmins held constant.  Where adv_p == ori_j(p) the difference is
 *      exactly zero: the term vanishes and stays finite (no square root is involved).
 *   5. ifd_cw_step's Adam (ifd_cw.h step 5), restated on the added rows only.
 *   info = { loss[b] (0 when loss is NULL), dist * (float)weight, dist }.
 * Refused on the host with IFD_ERR_ARG: an unknown kind, a missing state member or pointer, t < 1, B < 1, num_add outside [1, 1024],
 * cat_stride > 10000, cat_stride < 2 * num_add, and with n_ori == NULL cat_stride - num_add > 2048.  A cloud whose n_ori[b] is
 * outside [num_add, min(2048, cat_stride - num_add)] is left untouched, in every array. */
int ifd_add_step(ifd_ctx* ctx, int kind, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                 const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info, const ifd_add_diag* diag,
                 int t, float lr, float scale, int B, int cat_stride, int num_add, void* stream);

/* The end of a search step is ifd_cw_adjust(ctx, state, target, NULL, B, num_add, stream), as it is. */

typedef struct ifd_add_params {
    int32_t struct_size;     /* sizeof(ifd_add_params) */
    int32_t kind;            /* IFD_ADD_CHAMFER | IFD_ADD_HAUSDORFF */
    int32_t loss_kind;       /* IFD_ATK_LOSS_*, of the loop (the selection always takes cross-entropy) */
    int32_t binary_step;     /* >= 1 */
    int32_t num_iter;        /* >= 1, Adam steps per search step */
    int32_t num_add;         /* 1 .. IFD_ADD_MAX_ADD */
    float kappa, scale, attack_lr, init_weight, max_weight;
} ifd_add_params;

/* The whole attack: cri = ifd_add_critical_points(pc_in);  binary_step x ( added rows = cri + noise[step];  num_iter x
 * (ifd_cls_input_grad on the concatenation, ifd_add_step);  ifd_cw_adjust ), then the ending of Add.py:207-220.
 *   pc_in    [B][stride][3], n_points [B] or NULL (every cloud has `stride` rows)
 *   noise    [binary_step][B][num_add][3], drawn by the caller (the reference: randn * 1e-7); NULL: no noise
 *   pc_out   [B][out_stride][3]: cloud b holds its n_points[b] originals bit for bit, then num_add rows: o_bestattack, or the last
 *            forwarded added rows where lower == 0; rows beyond are left as they were.  Must not overlap pc_in.
 *   best_dist [B]  o_bestdist, 1e10 where no iteration reached the target;  success [B] int32 = lower > 0
 *   bounds   (may be NULL) [3][B] float64: the final weight, lower, upper
 * Counts and targets are checked once at the start (the one blocking step); nothing blocks afterwards.
 * Refused on the host with IFD_ERR_ARG before anything is enqueued: params missing or of another struct_size, an unknown kind or
 * loss_kind, binary_step < 1, num_iter < 1, num_add outside [1, 1024], B < 1, stride or out_stride outside [1, 10000], a missing
 * pointer, pc_out overlapping pc_in, and with n_points == NULL stride outside [num_add, 2048] or stride + num_add > out_stride.  At
 * the blocking check: n_points[b] outside [num_add, min(stride, 2048, out_stride - num_add)], target outside [0, 40).
 * Workspace, grown on the context: ifd_cls_input_grad's at max(stride, out_stride), + 12 * max(stride, out_stride) + 60 * num_add
 * + 52 bytes per cloud of the WHOLE batch (gradient; critical points, m, v, o_bestattack, last_input; the records, weights, pred,
 * loss, the two counts), rounded up to 256. */
int ifd_add_attack(ifd_ctx* ctx, const ifd_add_params* params, const float* pc_in, const int32_t* n_points, const int32_t* target,
                   const float* noise, int B, int stride, int out_stride, float* pc_out, float* best_dist, int32_t* success,
                   double* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_ADD_H */
