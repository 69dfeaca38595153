/*
 * ifd_atk.h - C ABI of the attack primitives in libifd.so: the gradient of an adversarial loss on the PointNet victim's
 * logits with respect to the input points, and on top of it the FGM family of the reference (baselines/attack/FGM/FGM.py:
 * FGM, I-FGM, MI-FGM, PGD), which writes the adversarial cloud files that the defenses and baselines/inference.py consume.
 * Exported from the same library as include/ifd.h and versioned on its own; the conventions of ifd.h hold (int status,
 * device pointers, `stream` = hipStream_t as void*, calls only enqueue work except where noted).  Every call takes a
 * context made by ifd_cls_create (include/ifd_cls.h) WITHOUT feature_transform: back-propagation through the 64 x 64
 * feature transform is not built, and a context that has one is refused with IFD_ERR_ARG.
 *
 * Clouds are point-major, [B][stride][3], cloud b being its first n_points[b] rows, exactly as in ifd_cls_forward.
 */
#ifndef IFD_ATK_H
#define IFD_ATK_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_cls.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_ATK_ABI_VERSION 1

#define IFD_ATK_LOSS_LOGITS 0        /* LogitsAdvLoss(kappa), baselines/attack/util/adv_utils.py:18-35 */
#define IFD_ATK_LOSS_CE 1            /* CrossEntropyAdvLoss = F.cross_entropy, adv_utils.py:45-53 */

#define IFD_FGM_FGM 0                /* `kind` of ifd_fgm_update / ifd_fgm_params */
#define IFD_FGM_IFGM 1
#define IFD_FGM_MIFGM 2
#define IFD_FGM_PGD 3                /* I-FGM's update; the two differ in the start noise, which the caller draws */

int ifd_atk_abi_version(void);

/* Optional outputs of ifd_cls_input_grad (each pointer may be NULL):
 *   logits      [B][40]
 *   loss        [B]        the cloud's own loss (not scaled)
 *   pred        [B]        argmax of the logits, the lowest class among equals
 *   win_feat    [B][1024]  the point each channel of the trunk's max-pool was taken from; among equal values the LOWEST
 *   win_stn     [B][1024]  index wins, as torch.max does on the CPU.  win_stn: the same of the STN3d's max-pool
 *   global_feat [B][1024]  the max-pooled trunk feature
 * logits, pred and global_feat are bit for bit what ifd_cls_forward returns for the same input. */
typedef struct ifd_atk_out {
    float* logits;
    float* loss;
    int32_t* pred;
    int32_t* win_feat;
    int32_t* win_stn;
    float* global_feat;
} ifd_atk_out;

/* grad [B][stride][3] = scale * d loss_b / d pc[b]; rows at or beyond n_points[b] are written as zeros.
 * What FGM.get_gradient (FGM.py:42-68) computes before its normalisation; the reference's .mean() over a batch of B_ref
 * clouds is scale = 1 / B_ref.
 *   IFD_ATK_LOSS_LOGITS  per cloud: real = logits[target]; other = max over the classes of the logits with the target's
 *                        entry replaced by -10000, the FIRST index among equal maxima taking the gradient;
 *                        loss = max(other - real + kappa, 0).  Where other - real + kappa is exactly 0 the gradient
 *                        PASSES (as if the hinge were open): torch.clamp(min=0)'s backward on the CPU masks with
 *                        x >= min.  Below 0 the gradient is exactly zero in every row.
 *   IFD_ATK_LOSS_CE      loss = logsumexp(logits) - logits[target]  (kappa is ignored)
 * target: [B] int32 on the device, 0 <= target[b] < 40.  pc, n_points, B, stride: as in ifd_cls_forward.  A bad count or
 * target is IFD_ERR_ARG and nothing else is enqueued; they live on the device, so EVERY call blocks the host once, until a
 * checking kernel enqueued on `stream` has run.
 * A cloud's gradient does not depend on B, on its position in the batch, on stride or on the other clouds, bit for bit:
 * every sum runs in a fixed order (over a point's channels ascending; the trunk's contribution to a point first, then the
 * STN3d's) and no float atomics are used.  Both max-pools route their gradient to the recorded winner.  The FC layers' ReLU
 * masks are the forward's saved activations; the point stacks' are recomputed at the winner points by a scalar
 * restatement of the forward's fused chains (that the MFMA sums its four k values in that order is assumed, not measured:
 * a gate within rounding of zero may fall the other way than in the forward).
 * The batch runs in chunks of up to 4096 clouds over context workspace of
 *     8192 * ceil(stride / 256) + 30184   bytes per cloud of a chunk (+ 256), grown on demand. */
int ifd_cls_input_grad(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, const int32_t* target,
                       int loss_kind, float kappa, float scale, float* grad, const ifd_atk_out* out, void* stream);

/* One in-place update of FGM.py on the device; never blocks.  Sums run over a cloud's first n_points[b] rows (all of its
 * `stride` rows when n_points is NULL) in a fixed order: a cloud's result does not depend on the batch, bit for bit.  Rows
 * beyond are not touched.
 *   FGM          pc -= step_size * grad / (||grad||_2 + 1e-9)                                   (FGM.py:66-67, 82-86)
 *   IFGM, PGD    the same, then ClipPointsL2(budget) against ori_pc (clip_utils.py:24-31):
 *                pc = ori_pc + (pc - ori_pc) * min(budget / (||pc - ori_pc||_2 + 1e-9), 1)        (FGM.py:147-152)
 *   MIFGM        g = grad / (||grad||_1 + 1e-9); momentum = mu * momentum + g;
 *                pc -= step_size * momentum / (||momentum||_2 + 1e-9); then the clip             (FGM.py:220-230)
 * ori_pc may be NULL for FGM, momentum [B][stride][3] is needed by MIFGM only (zeros before the first step). */
int ifd_fgm_update(ifd_ctx* ctx, int kind, const float* grad, float* pc, const float* ori_pc, float* momentum,
                   float step_size, float budget, float mu, const int32_t* n_points, int B, int stride, void* stream);

typedef struct ifd_fgm_params {
    int32_t struct_size;     /* sizeof(ifd_fgm_params) */
    int32_t kind;            /* IFD_FGM_* */
    int32_t loss_kind;       /* IFD_ATK_LOSS_* */
    int32_t num_iter;        /* >= 1; FGM is one step of step_size = budget */
    float kappa, scale, step_size, budget, mu;
} ifd_fgm_params;

/* The whole attack: num_iter x (ifd_cls_input_grad, ifd_fgm_update) on a copy of pc_in, then ifd_cls_forward on the
 * result.  pc_out [B][stride][3] (must not overlap pc_in), success [B] int32 = (pred == target) of that last forward.
 * ori_pc IS pc_in, as IFGM.attack defines it (FGM.py:131-134): the start noise (randn * 1e-7 of I-FGM / MI-FGM, PGD's
 * uniform +- budget / sqrt(3 K)) is not drawn here - the caller passes pc_in already perturbed.
 * Counts and targets are checked once at the start (the one blocking step); nothing blocks between the iterations.
 * Workspace: ifd_cls_input_grad's, + 24 * stride bytes per cloud of the WHOLE batch (gradient and momentum). */
int ifd_fgm_attack(ifd_ctx* ctx, const ifd_fgm_params* params, const float* pc_in, const int32_t* n_points,
                   const int32_t* target, int B, int stride, float* pc_out, int32_t* success, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_ATK_H */
