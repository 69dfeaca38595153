/*
 * ifd_victim_atk.h - C ABI of the Perturb, kNN and Drop attacks (include/ifd_cw.h, ifd_knn.h, ifd_drop.h) on ANY of the four
 * victims in libifd.so: PointNet (ifd_cls_create without feature_transform), DGCNN (ifd_dgcnn_create), PointNet++ (ifd_pn2_create)
 * and PointConv (ifd_pc_create).  The calls dispatch on the context's model.  Exported from the same library as include/ifd.h and
 * versioned on its own; the conventions of ifd_atk.h hold: int status, device pointers, `stream` = hipStream_t as void*, clouds
 * point-major [B][stride][3] with n_points [B], calls only enqueue work except for the one check at the start of an attack.
 *
 * The hot path of every loop is the victim's own gradient (ifd_cls_input_grad, ifd_dgcnn_input_grad, ifd_pn2_input_grad,
 * ifd_pc_input_grad) followed by the step kernel of ifd_cw.h / ifd_knn.h / ifd_drop.h, which never touches the network: the
 * arithmetic, the pinned decisions and the deviations of those three headers hold word for word.  No float atomics; a cloud's
 * result does not depend on B, on its position in the batch, on stride, on padding or on the other clouds, bit for bit.  On a
 * PointNet context the calls below give the bits of ifd_cw_perturb_attack, ifd_knn_attack and ifd_drop_attack.
 *
 * fps_start: [B][2] int32 on the device, the first picks of the two samplings as in ifd_pn2_input_grad / ifd_pc_input_grad, for
 * PointNet++ and PointConv contexts (NULL: both 0).  The SAME starts serve every gradient of a call and its final forward.  It
 * must be NULL for PointNet and DGCNN contexts: a non-NULL pointer there is refused with IFD_ERR_ARG.
 *
 * Strides and counts: the victim's own range, min <= n_points[b] <= stride <= max with
 *     PointNet [1, 10000]    DGCNN [k, 2048]    PointNet++ [1, 2048]    PointConv [32, 2048]
 * narrowed by the attack's (kNN: [6, 2048]; Drop: n_points[b] <= 2048).
 */
#ifndef IFD_VICTIM_ATK_H
#define IFD_VICTIM_ATK_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#include "ifd_cw.h"
#include "ifd_drop.h"
#include "ifd_knn.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_VICTIM_ATK_ABI_VERSION 1

int ifd_victim_atk_abi_version(void);

/* ifd_cw_step, ifd_cw_adjust, ifd_knn_step, ifd_knn_project_clip and ifd_drop_step on any victim's context that has a gradient
 * image: the same kernels, arguments, semantics and refusals (a PointNet context with feature_transform keeps its refusal).  The
 * strides are the step kernels' own, whatever the victim.  They never block. */
int ifd_victim_cw_step(ifd_ctx* ctx, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                       const int32_t* target, float* adv, const float* ori, float* last_input, float* info, int t, float lr, float scale,
                       const int32_t* n_points, int B, int stride, void* stream);
int ifd_victim_cw_adjust(ifd_ctx* ctx, const ifd_cw_state* state, const int32_t* target, const int32_t* n_points, int B, int stride,
                         void* stream);
int ifd_victim_knn_step(ifd_ctx* ctx, const ifd_knn_params* params, const float* grad, const float* loss, float* adv, const float* ori,
                        const float* normal, float* m, float* v, int t, float lr, float scale, const ifd_knn_diag* diag,
                        const int32_t* n_points, int B, int stride, void* stream);
int ifd_victim_knn_project_clip(ifd_ctx* ctx, float* adv, const float* ori, const float* normal, float budget, const int32_t* n_points,
                                int B, int stride, void* stream);
int ifd_victim_drop_step(ifd_ctx* ctx, const float* grad, float* pc, int32_t* n_points, int32_t* index, int B, int stride, int k,
                         float alpha, const ifd_drop_out* out, void* stream);

/* ifd_cw_perturb_attack's loop with the context's own gradient: binary_step x ( adv = pc_in + noise[step];  num_iter x (the
 * victim's input gradient with fps_start, ifd_cw_step);  ifd_cw_adjust ), then the reference's ending.  Arguments and outputs are
 * ifd_cw_perturb_attack's.  Counts, starts and targets are checked once at the start (the one blocking step).
 * Refused with IFD_ERR_ARG before anything is enqueued: what ifd_cw_perturb_attack refuses, with the stride held to the victim's
 * range, and a non-NULL fps_start on a victim that does not sample.
 * Workspace, grown on the context: the victim's input gradient's, + 60 * stride + 64 bytes per cloud of the WHOLE batch. */
int ifd_victim_cw_perturb_attack(ifd_ctx* ctx, const ifd_cw_params* params, const float* pc_in, const int32_t* n_points,
                                 const int32_t* fps_start, const int32_t* target, const float* noise, int B, int stride, float* pc_out,
                                 float* best_dist, int32_t* success, double* bounds, void* stream);

/* ifd_knn_attack's loop with the context's own gradient, closed by the victim's forward on the same starts.  Arguments and outputs
 * are ifd_knn_attack's.  Strides and counts lie in [max(6, the victim's minimum), 2048].
 * Workspace: the larger of the victim's gradient's and forward's, + 36 * stride + 168 bytes per cloud of the WHOLE batch. */
int ifd_victim_knn_attack(ifd_ctx* ctx, const ifd_knn_params* params, const float* pc_in, const float* normal, const int32_t* n_points,
                          const int32_t* fps_start, const int32_t* target, const float* noise, int B, int stride, float* pc_out,
                          int32_t* pred, int32_t* success, void* stream);

/* ifd_drop_attack's loop with the context's own gradient, closed by the victim's forward.  Arguments and outputs are
 * ifd_drop_attack's.  The counts shrink on the device while the starts stay fixed: ONE start table serves every round and the
 * final forward, so it must be valid for the cloud that is WRITTEN.  With n = n_points[b] (or stride):
 *     n - num_drop >= the victim's minimum (1 for PointNet and PointNet++, 32 for PointConv, k for DGCNN),  n <= min(stride, 2048),
 *     0 <= fps_start[b][0] < n - num_drop,  0 <= fps_start[b][1] < 512.
 * Both are checked once, at the blocking check, before anything is enqueued: a start at or beyond a shrunken count would seed a
 * sampling from a zeroed row - in bounds, and silently wrong.
 * Workspace: the larger of the victim's gradient's and forward's, + 12 * stride + 164 bytes per cloud of the WHOLE batch. */
int ifd_victim_drop_attack(ifd_ctx* ctx, const ifd_drop_params* params, const float* pc_in, const int32_t* n_points,
                           const int32_t* fps_start, const int32_t* label, int B, int stride, float* pc_out, int32_t* n_out,
                           int32_t* kept, int32_t* correct, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_VICTIM_ATK_H */
