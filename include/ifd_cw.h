/*
 * ifd_cw.h - C ABI of the Carlini-Wagner point-perturbation attack ("Perturb", baselines/attack/CW/Perturb.py CWPerturb with
 * L2Dist, driven by baselines/attack_scripts/targeted_perturb_attack.py) on the PointNet victim, in libifd.so.  Built on
 * ifd_cls_input_grad (include/ifd_atk.h) and versioned on its own; the conventions of ifd_atk.h hold: int status, device
 * pointers, `stream` = hipStream_t as void*, clouds point-major [B][stride][3] with optional n_points [B] (rows at or beyond a
 * cloud's count are never read or written by the calls below), contexts made by ifd_cls_create WITHOUT feature_transform (any
 * other is refused with IFD_ERR_ARG).  Every per-cloud sum runs in one fixed order (a thread's strided partial sum, then a
 * fixed tree over the workgroup's 256 threads), no float atomics: a cloud's result does not depend on B, on its position in
 * the batch or on the other clouds, bit for bit.
 */
#ifndef IFD_CW_H
#define IFD_CW_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_CW_ABI_VERSION 1

int ifd_cw_abi_version(void);

/* The attack's state, all on the device.  A fresh attack starts from bestdist = o_bestdist = 1e10, bestscore = o_bestscore = -1,
 * m = v = 0, lower = 0, upper = max_weight, weight = init_weight (Perturb.py:59-66, 74-76).  The three weights are float64, as the
 * reference's numpy arrays are: the halving (lower + upper) / 2 is then exact for any binary_step that float64 allows, and the
 * distance term takes (float)weight, as L2Dist's weights.float() does. */
typedef struct ifd_cw_state {
    float* m;                /* [B][stride][3]  Adam's exp_avg of the current search step */
    float* v;                /* [B][stride][3]  Adam's exp_avg_sq */
    float* bestdist;         /* [B]  the current search step's record */
    int32_t* bestscore;      /* [B] */
    float* o_bestdist;       /* [B]  the whole attack's record */
    int32_t* o_bestscore;    /* [B] */
    float* o_bestattack;     /* [B][stride][3] */
    double* weight;          /* [B]  current_weight */
    double* lower;           /* [B]  lower_bound */
    double* upper;           /* [B]  upper_bound */
} ifd_cw_state;

/* One iteration of Perturb.py:107-136 behind the forward / backward pass; never blocks.
 *   grad  [B][stride][3], pred [B], loss [B] (may be NULL)   as ifd_cls_input_grad wrote them for the current `adv`
 *         (grad = scale * d adv_loss_b / d adv[b]: it already carries scale)
 *   adv   [B][stride][3]  updated in place;  ori [B][stride][3]
 *   t     the 1-based number of this Adam step within its search step;  lr  Adam's learning rate
 *   scale the reference's 1 / B_ref of .mean()
 * Per cloud, in this order:
 *   1. dist = sqrt(sum (adv - ori)^2) over the cloud's rows, float32.
 *   2. The record (Perturb.py:115-123), both comparisons strict:
 *        dist < bestdist   && pred == target:  bestdist = dist,   bestscore = pred
 *        dist < o_bestdist && pred == target:  o_bestdist = dist, o_bestscore = pred, o_bestattack = adv bit for bit - the
 *        cloud that was forwarded, BEFORE this iteration's update.
 *   3. last_input (may be NULL) = adv, the reference's input_val, also before the update.  The reference overwrites it every
 *      iteration and reads it once, behind its loops (Perturb.py:169-170), so only the copy taken in the last iteration of the
 *      last search step is ever seen: passing NULL everywhere else gives the same attack.
 *   4. g = grad + (scale * (float)weight / dist) * (adv - ori): autograd's gradient of mean(dist * weight).
 *      DEVIATION: where dist == 0 the distance term contributes exactly zero.  The reference's sqrt backward gives 0 / 0 = NaN
 *      there; it never gets there, because it starts every search step from ori + randn * 1e-7.
 *   5. torch.optim.Adam's step (betas 0.9 / 0.999, eps 1e-8, no weight decay, no amsgrad), in the operation order of this
 *      library's optimiser (csrc/optimize.hip, which restates torch/optim/adam.py _single_tensor_adam):
 *        m = m + (1 - b1) (g - m);  v = b2 v + ((1 - b2) g) g;
 *        adv -= (lr / (1 - b1^t)) * (m / (sqrt(v) / sqrt(1 - b2^t) + eps))
 *      with 1 - b1, 1 - b2 and the two bias corrections computed in double on the host and rounded to float, as torch hands its
 *      Python scalars to its float kernels.
 *   info (may be NULL) [B][3] = { loss[b] (0 when loss is NULL), dist * (float)weight, dist }: the two terms the reference's
 *      progress lines average, and the distance. */
int ifd_cw_step(ifd_ctx* ctx, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                const int32_t* target, float* adv, const float* ori, float* last_input, float* info, int t, float lr, float scale,
                const int32_t* n_points, int B, int stride, void* stream);

/* The end of a search step (Perturb.py:154-162), per cloud on the device; never blocks.
 *   success = bestscore == target && bestscore != -1 && bestdist <= o_bestdist        (note the <=)
 *   success: lower = max(lower, weight)   otherwise: upper = min(upper, weight)   both: weight = (lower + upper) / 2
 * Then the reset for the next search step: bestdist = 1e10, bestscore = -1, m = v = 0 (m, v may be NULL). */
int ifd_cw_adjust(ifd_ctx* ctx, const ifd_cw_state* state, const int32_t* target, const int32_t* n_points, int B, int stride,
                  void* stream);

typedef struct ifd_cw_params {
    int32_t struct_size;     /* sizeof(ifd_cw_params) */
    int32_t loss_kind;       /* IFD_ATK_LOSS_* */
    int32_t binary_step;     /* >= 1 */
    int32_t num_iter;        /* >= 1, Adam steps per search step */
    float kappa, scale, attack_lr, init_weight, max_weight;
} ifd_cw_params;

/* The whole attack: binary_step x ( adv = pc_in + noise[step];  num_iter x (ifd_cls_input_grad, ifd_cw_step);  ifd_cw_adjust ),
 * then the ending of Perturb.py:169-175: a cloud whose lower is still 0 gets the last cloud that was forwarded.
 *   noise    [binary_step][B][stride][3], drawn by the caller (the reference: randn * 1e-7); NULL: no noise
 *   pc_out   [B][stride][3]  o_bestattack, or last_input where lower == 0; must not overlap pc_in
 *   best_dist [B]  o_bestdist, 1e10 where no iteration reached the target;  success [B] int32 = lower > 0
 *   bounds   (may be NULL) [3][B] float64: the final weight, lower, upper
 * Counts and targets are checked once at the start (the one blocking step); nothing blocks between iterations or search steps.
 * Refused on the host with IFD_ERR_ARG before anything is enqueued: params missing or of another struct_size, binary_step < 1,
 * num_iter < 1, an unknown loss_kind, stride outside [1, 10000], B < 1, a missing pointer, pc_out overlapping pc_in.
 * Workspace, grown on the context: ifd_cls_input_grad's, + 60 * stride + 64 bytes per cloud of the WHOLE batch
 * (gradient, adv, m, v, last_input; the records, weights, pred, loss), rounded up to 256. */
int ifd_cw_perturb_attack(ifd_ctx* ctx, const ifd_cw_params* params, const float* pc_in, const int32_t* n_points,
                          const int32_t* target, const float* noise, int B, int stride, float* pc_out, float* best_dist,
                          int32_t* success, double* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_CW_H */
