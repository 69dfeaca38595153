/*
 * ifd_knn.h - C ABI of the kNN attack ("kNN", baselines/attack/CW/kNN.py CWKNN with ChamferkNNDist('adv2ori', 5, 1.05, 5., 3.) and
 * ProjectInnerClipLinf(0.1), driven by baselines/attack_scripts/targeted_knn_attack.py) on the PointNet victim, in libifd.so.
 * Built on ifd_cls_input_grad (include/ifd_atk.h) and versioned on its own; the conventions of ifd_cw.h hold: int status, device
 * pointers, `stream` = hipStream_t as void*, clouds point-major [B][stride][3] with optional n_points [B] (rows at or beyond a
 * cloud's count are never read or written by the calls below), contexts made by ifd_cls_create WITHOUT feature_transform (any
 * other is refused with IFD_ERR_ARG).  Every per-cloud sum runs in one fixed order (a thread's strided partial sum, then a
 * fixed tree over the workgroup's 256 threads; the neighbour terms a point receives are gathered in ascending order of the
 * sending point), no float atomics: a cloud's result does not depend on B, on its position in the batch or on the other clouds,
 * bit for bit.
 *
 * DEVIATIONS from the reference, all of rounding or of the caller's freedom, none of them a switch:
 *   - Distances are in difference form, fma(dz, dz, fma(dy, dy, dx * dx)), and a point is left out of its own neighbour search by
 *     its INDEX.  The reference expands |x|^2 - 2 x.y + |y|^2 (about 5e-7 of absolute noise at unit scale) and drops column 0 of
 *     its top 6 as "self", whichever point that is.  Ties: the five nearest are the five smallest (distance, index) pairs; the
 *     Chamfer nearest is the lowest index among equal distances, as torch's CPU min is.
 *   - The cross products of the projection are always taken along the coordinate axis.  The reference calls torch.cross(vng,
 *     normal) without `dim`, which takes the FIRST axis of size 3: with a batch of 3 clouds that is the batch axis.
 *   - The start noise is the caller's (the reference draws randn * 1e-7 on the GPU from the global stream).
 *   - k, the number of neighbours, is fixed at 5: it is the kernel's register layout, not a parameter.
 */
#ifndef IFD_KNN_H
#define IFD_KNN_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_KNN_ABI_VERSION 1
#define IFD_KNN_K 5                  /* neighbours of the outlier penalty: fixed */
#define IFD_KNN_MIN_POINTS 6         /* the reference's topk(k + 1) throws below */
#define IFD_KNN_MAX_POINTS 2048      /* a cloud and its original live in one workgroup's 64 KB of LDS */

int ifd_knn_abi_version(void);

typedef struct ifd_knn_params {
    int32_t struct_size;     /* sizeof(ifd_knn_params) */
    int32_t loss_kind;       /* IFD_ATK_LOSS_*                      (ifd_knn_attack only) */
    int32_t num_iter;        /* >= 1, Adam steps                    (ifd_knn_attack only) */
    float kappa, scale, attack_lr;       /* the adversarial loss's margin, 1 / B_ref of the reference's .mean(), Adam's lr (ifd_knn_attack only) */
    float chamfer_weight;    /* w1, the reference: 5 */
    float knn_weight;        /* w2, the reference: 3 */
    float alpha;             /* threshold = mean + alpha * std, the reference: 1.05 */
    float budget;            /* per-point clip of the displacement, the reference: 0.1 */
} ifd_knn_params;

/* Optional outputs of ifd_knn_step, every one may be NULL (and `diag` itself); they are what lets a test judge the discrete
 * decisions exactly, and cost nothing when NULL. */
typedef struct ifd_knn_diag {
    float* info;             /* [B][4]  { loss[b] (0 when loss is NULL), cd, knn, n * (w1 cd + w2 knn) }: the terms of the progress line */
    float* dist_grad;        /* [B][stride][3]  g_dist below, before Adam */
    int32_t* nn_ori;         /* [B][stride]     the Chamfer argmin */
    int32_t* nn5;            /* [B][stride][5]  the five nearest, ascending (distance, index) */
    int32_t* mask;           /* [B][stride]     1 where value > threshold */
} ifd_knn_diag;

/* One iteration of kNN.py:97-116 behind the forward / backward pass; never blocks.  The attack keeps no record, so the step reads
 * neither the prediction nor the target.
 *   params  chamfer_weight, knn_weight, alpha, budget (and struct_size) are read
 *   grad    [B][stride][3], loss [B] (may be NULL)   as ifd_cls_input_grad wrote them for the current `adv`
 *           (grad = scale * d adv_loss_b / d adv[b]: it already carries scale)
 *   adv     [B][stride][3]  updated in place;  ori [B][stride][3];  normal [B][stride][3] or NULL (then step 5 only clips)
 *   m, v    [B][stride][3]  Adam's exp_avg / exp_avg_sq, in place
 *   t       the 1-based number of this Adam step;  lr  Adam's learning rate;  scale  the reference's 1 / B_ref of .mean()
 * Per cloud of n points (n = n_points[b] or stride), one workgroup, the cloud and its original in LDS, in this order:
 *   1. For every point j one scan of ori and one of adv: nn_ori(j) = argmin_i |adv_j - ori_i|^2 and NN5(j), the five nearest
 *      other adversarial points.  value_j = (d_0 + d_1 + d_2 + d_3 + d_4) / 5 over NN5(j)'s squared distances, ascending.
 *   2. mean = sum_j value_j / n;  std = sqrt(sum_j (value_j - mean)^2 / (n - 1))  (torch.std's unbiased default), two passes;
 *      thr = mean + alpha * std;  mask_j = value_j > thr, strict.
 *      cd = sum_j min_i |adv_j - ori_i|^2 / n;  knn = sum_j mask_j value_j / n.
 *   3. g_dist[j] = scale * ( 2 w1 (adv_j - ori_nn(j))
 *                          + (2 w2 / 5) ( mask_j sum_{q in NN5(j)} (adv_j - adv_q)  +  sum_{p masked, j in NN5(p)} (adv_j - adv_p) ) )
 *      autograd's gradient of mean_b(w1 cd_b + w2 knn_b) * K with masks and neighbour sets held constant (the K of `.mean() * K`
 *      cancels the 1 / K of both means; with ragged clouds it is the cloud's own count).  The first sum runs in NN5(j)'s order,
 *      the second over p ascending.  Coincident adversarial points contribute zero difference vectors: the result is finite.
 *   4. torch.optim.Adam's step on g = grad + g_dist, term for term the arithmetic of ifd_cw_step (ifd_cw.h step 5, restated in
 *      csrc/pointnet_knn.hip rather than shared, so that pointnet_cw.hip's object code stays as it is).
 *   5. ifd_knn_project_clip's arithmetic on the updated point.
 * A cloud with n < 6 is left untouched, in every array (the reference's topk(6) throws there; ifd_knn_attack refuses it). */
int ifd_knn_step(ifd_ctx* ctx, const ifd_knn_params* params, const float* grad, const float* loss, float* adv, const float* ori,
                 const float* normal, float* m, float* v, int t, float lr, float scale, const ifd_knn_diag* diag,
                 const int32_t* n_points, int B, int stride, void* stream);

/* ProjectInnerClipLinf(budget) (attack/util/clip_utils.py:79-113, 53-59) in place on adv; never blocks.  Per point, float32, with
 * d = adv - ori and n the point's normal:
 *   d.n < 0:   vng = n x d;  vref = vng x n;  d <- d * vref / (|vref| + 1e-9), an ELEMENT-WISE product as the reference writes it,
 *              kept bug for bug;  d <- 0 where additionally |vng| < 1e-6
 *   then       d <- d * min(budget / (|d| + 1e-9), 1);  adv = ori + d
 * normal == NULL: the clip alone.  1 <= stride <= 10000. */
int ifd_knn_project_clip(ifd_ctx* ctx, float* adv, const float* ori, const float* normal, float budget, const int32_t* n_points,
                         int B, int stride, void* stream);

/* The whole attack: pc_out = pc_in + noise;  num_iter x (ifd_cls_input_grad, ifd_knn_step) on pc_out with m = v = 0 at the
 * start;  then one forward pass.  There is no binary search and there are no records: every cloud's final state is returned.
 *   noise    [B][stride][3], drawn by the caller (the reference: randn * 1e-7); NULL: no noise
 *   normal   [B][stride][3] or NULL (the reference without normals: the clip alone)
 *   pc_out   [B][stride][3]; must not overlap pc_in
 *   pred [B] int32 the final prediction;  success [B] int32 = pred == target
 * Counts and targets are checked once at the start (the one blocking step; a cloud with n_points < 6 is refused there);
 * nothing blocks between iterations.
 * Refused on the host with IFD_ERR_ARG before anything is enqueued: params missing or of another struct_size, num_iter < 1, an
 * unknown loss_kind, B < 1, a missing pointer, pc_out overlapping pc_in, stride < 6, stride > IFD_KNN_MAX_POINTS.
 * Workspace, grown on the context: the larger of ifd_cls_input_grad's and ifd_cls_forward's, + 36 * stride + 168 bytes per cloud
 * of the WHOLE batch (gradient, m, v; the final logits, loss, pred), rounded up to 256. */
int ifd_knn_attack(ifd_ctx* ctx, const ifd_knn_params* params, const float* pc_in, const float* normal, const int32_t* n_points,
                   const int32_t* target, const float* noise, int B, int stride, float* pc_out, int32_t* pred, int32_t* success,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_KNN_H */
