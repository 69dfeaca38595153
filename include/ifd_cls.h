/*
 * ifd_cls.h - C ABI of the victim classifiers in libifd.so: what baselines/inference.py runs on a restored cloud file to
 * measure accuracy and attack success rate.  Exported from the same library as include/ifd.h and versioned on its own;
 * the conventions of ifd.h hold (int status, device pointers, `stream` = hipStream_t as void*, calls only enqueue work
 * except where noted), and the contexts made here are destroyed with ifd_destroy and report through ifd_last_error.
 *
 * Built: PointNetCls(k=40, feature_transform=False|True, use_bn=True) in eval() (baselines/model/pointnet.py).  The other
 * victims of the reference (PointNet++, DGCNN, PointConv) have model ids reserved below and are refused here: each has an ABI
 * of its own (ifd_pn2.h, ifd_dgcnn.h, ifd_pc.h).
 */
#ifndef IFD_CLS_H
#define IFD_CLS_H
#include <stddef.h>
#include <stdint.h>
#include "ifd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_CLS_ABI_VERSION 1
#define IFD_MODEL_CLS 3              /* context kind (beside IFD_MODEL_CONVONET / _ONET / _DUP) */

#define IFD_CLS_POINTNET 0           /* `model` of the calls below */
#define IFD_CLS_POINTNET2 1          /* reserved, not built */
#define IFD_CLS_DGCNN 2              /* reserved, not built */
#define IFD_CLS_POINTCONV 3          /* reserved, not built */

#define IFD_CLS_MAX_POINTS 10000     /* largest stride / n_points of ifd_cls_forward */

int ifd_cls_abi_version(void);

/* Number of floats of a model's weights: 1,606,193 (PointNet) or 3,459,569 (PointNet with feature_transform); 0 for a
 * model that is not built.  Canonical order: every conv / linear layer as {weight [out][in], bias [out]} with its
 * eval-mode BatchNorm (running statistics, eps 1e-5) already folded in,
 *     w' = w * gamma / sqrt(var + eps),    b' = (b - mean) * gamma / sqrt(var + eps) + beta,
 * (layers without a BatchNorm - every fc3 - as they are), in network order:
 *   feat.stn   conv1 [64,3]   conv2 [128,64]  conv3 [1024,128]  fc1 [512,1024]  fc2 [256,512]  fc3 [9,256]
 *   feat       conv1 [64,3]
 *   feat.fstn  conv1 [64,64]  conv2 [128,64]  conv3 [1024,128]  fc1 [512,1024]  fc2 [256,512]  fc3 [4096,256]
 *                                                                            (only with feature_transform)
 *   feat       conv2 [128,64] conv3 [1024,128]
 *   head       fc1 [512,1024] fc2 [256,512] (bn2 folded: dropout is the identity)  fc3 [40,256] */
size_t ifd_cls_weight_count(int model, int feature_transform);

/* A classifier context on `device`.  weights_host is HOST memory in the canonical order.  An unknown model, a
 * model that is not built, n_classes != 40 or a wrong count fail before any HIP call is made: NULL, with the message in
 * ifd_last_error(NULL).
 * Replaces: PointNetCls(k=40, feature_transform=...) + load_state_dict (baselines/inference.py:171-187). */
ifd_ctx* ifd_cls_create(const float* weights_host, size_t n_weights, int model, int feature_transform, int n_classes,
                        int device);

/* Optional outputs of ifd_cls_forward (each pointer may be NULL):
 *   trans       [B][3][3]     STN3d output (identity added)
 *   trans_feat  [B][64][64]   STNkd output (identity added); must be NULL without feature_transform (IFD_ERR_ARG)
 *   global_feat [B][1024]     the max-pooled trunk feature
 *   pred        [B]           argmax of the logits; among equal logits the LOWEST class wins, as torch.argmax does on
 *                             the CPU */
typedef struct ifd_cls_aux {
    float* trans;
    float* trans_feat;
    float* global_feat;
    int32_t* pred;
} ifd_cls_aux;

/* model.eval()(pc.transpose(1, 2)) of baselines/inference.py:43-50: pc [B][stride][3] -> logits [B][n_classes].
 * n_points (optional) [B] int32, device memory: cloud b is its first n_points[b] rows; rows beyond take no part (they may
 * hold anything, NaN included).  NULL means every cloud has `stride` rows.  1 <= stride <= IFD_CLS_MAX_POINTS and
 * 1 <= n_points[b] <= stride, else IFD_ERR_ARG and nothing else is enqueued.  The counts live on the device, so a call WITH
 * n_points blocks the host once, until a checking kernel enqueued on `stream` has run; a call without never blocks.
 * A cloud's result does not depend on B, on its position in the batch, on stride or on the other clouds, bit for bit.
 * The batch runs in chunks of up to 4096 clouds over context workspace of
 *     4096 * ceil(stride / 256) + 7232 (+ 16384 with feature_transform)   bytes per cloud of a chunk (+ 256),
 * grown on demand (see ifd.h); a failed allocation is IFD_ERR_NOMEM.  f32 throughout: every layer of 64 or more input
 * channels runs on v_mfma_f32_16x16x4_f32 - per output the bias, then the inputs in ascending order in one fused chain (the
 * FC layers: four such chains over interleaved 16-input groups, added pairwise) - and the 3-input layers and the 3x3
 * transform are plain fused multiply-adds; both transforms are applied before the layer that follows them, as the
 * reference does, never folded into its weights. */
int ifd_cls_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, float* logits,
                    const ifd_cls_aux* aux, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_CLS_H */
