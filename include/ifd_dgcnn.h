/*
 * ifd_dgcnn.h - C ABI of the DGCNN victim classifier in libifd.so: DGCNN(emb_dims=1024, k, output_channels=40, use_bn=True)
 * in eval() (baselines/model/dgcnn.py), the reference's default victim of the cluster and object attacks and the second
 * column of its result tables.  Exported from the same library as include/ifd.h and versioned on its own; the conventions of
 * ifd_cls.h hold (int status, device pointers, `stream` = hipStream_t as void*, calls only enqueue work except where noted),
 * and the contexts made here are destroyed with ifd_destroy and report through ifd_last_error.
 *
 * DGCNN does not sit behind ifd_cls_*: IFD_CLS_DGCNN stays refused there.
 */
#ifndef IFD_DGCNN_H
#define IFD_DGCNN_H
#include <stddef.h>
#include <stdint.h>
#include "ifd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_DGCNN_ABI_VERSION 1
#define IFD_MODEL_DGCNN 4            /* context kind (beside IFD_MODEL_CONVONET / _ONET / _DUP / _CLS) */

#define IFD_DGCNN_MAX_POINTS 2048    /* largest stride / n_points of ifd_dgcnn_forward */
#define IFD_DGCNN_MAX_K 32           /* largest k of ifd_dgcnn_create */

int ifd_dgcnn_abi_version(void);

/* Number of floats of the weights: 1,807,016.  Canonical order: every layer as {weight [out][in], bias [out]} with its
 * eval-mode BatchNorm (running statistics, eps 1e-5) already folded in, by the formulas of ifd_cls.h,
 *     w' = w * gamma / sqrt(var + eps),    b' = (b - mean) * gamma / sqrt(var + eps) + beta,
 * where a layer without a bias (every one but linear2 and linear3) has b = 0, so that its bias is the BatchNorm's shift;
 * linear3 has no BatchNorm and is stored as it is.  In network order:
 *     conv1 [64,6]  conv2 [64,128]  conv3 [128,128]  conv4 [256,256]  conv5 [1024,512]
 *     linear1 [512,2048]  linear2 [256,512]  linear3 [40,256]
 * Input columns keep the reference's order: of an edge convolution [Cout, 2C] the first C columns multiply x_j - x_i, the last
 * C multiply x_i (get_graph_feature, baselines/model/dgcnn.py:38); of linear1 the first 1024 multiply the max-pooled, the
 * last 1024 the mean-pooled conv5 output. */
size_t ifd_dgcnn_weight_count(void);

/* A DGCNN context on `device`.  weights_host is HOST memory in the canonical order.  1 <= k <= IFD_DGCNN_MAX_K;
 * n_classes == 40; emb_dims is fixed at 1024.  A NULL pointer, a wrong count, k or n_classes fail before any HIP call is
 * made: NULL, with the message in ifd_last_error(NULL).
 * Replaces: DGCNN(args.emb_dims, args.k, output_channels=40) + load_state_dict (baselines/inference.py). */
ifd_ctx* ifd_dgcnn_create(const float* weights_host, size_t n_weights, int k, int n_classes, int device);

/* Optional outputs of ifd_dgcnn_forward (each pointer, and each of idx's four, may be NULL):
 *   idx[l]      [B][stride][k] int32   the neighbours chosen for every point in edge convolution l + 1; the order of a row's
 *                                      k entries is unspecified
 *   feat        [B][stride][512]       x1 | x2 | x3 | x4, the four edge convolutions' outputs (64, 64, 128, 256 channels)
 *   global_feat [B][2048]              max | mean over the points of the conv5 output (after its LeakyReLU)
 *   pred        [B] int32              argmax of the logits; among equal logits the LOWEST class wins
 * Rows of idx and feat beyond n_points[b] are left as they were. */
typedef struct ifd_dgcnn_aux {
    int32_t* idx[4];
    float* feat;
    float* global_feat;
    int32_t* pred;
} ifd_dgcnn_aux;

/* model.eval()(pc.transpose(1, 2)): pc [B][stride][3] -> logits [B][40].
 * n_points (optional) [B] int32, device memory: cloud b is its first n_points[b] rows; rows beyond take no part (they may
 * hold anything, NaN included).  NULL means every cloud has `stride` rows.  k <= n_points[b] <= stride <=
 * IFD_DGCNN_MAX_POINTS, else IFD_ERR_ARG and nothing else is enqueued (the reference's topk raises on a cloud of fewer than k
 * points).  The counts live on the device, so a call WITH n_points blocks the host once, until a checking kernel enqueued
 * on `stream` has run; a call without never blocks.
 * A cloud's outputs do not depend on B, on its position in the batch, on stride or on the other clouds, bit for bit.
 *
 * Neighbour choice.  The input of an edge convolution is x [n][C] in f32 (xyz, then x1, x2, x3: C = 3, 64, 64, 128).  The score
 * of candidate j for point i is
 *     s_ij = 2 <x_i, x_j> - |x_j|^2,
 * the reference's pairwise_distance without its term -|x_i|^2, which is constant along a row.  It is evaluated in f32, the
 * same way for every j: <x_i, x_j> as one fused chain d = fmaf(x_i[c], x_j[c], d) from d = 0 over c = 0 .. C-1 in ascending
 * order, |x_j|^2 as the same chain on (x_j, x_j), and s_ij = fmaf(2, d, -|x_j|^2) - so bit-identical rows j, j' get
 * bit-identical scores.  The k candidates with the largest score are chosen, among equal scores the lowest index; the point
 * itself takes part, as in the reference.  The n x n matrix never exists.
 *
 * Layer form.  All four edge convolutions run in split form: with W = [Wa | Wb] (Wa on x_j - x_i, Wb on x_i),
 *     P = Wa x,   Q = (Wb - Wa) x + b   per point,     out_i = leaky(max_j P_j + Q_i),
 * Wb - Wa rounded to f32 once, at creation.  LeakyReLU(0.2) is monotone, so it commutes with the maximum exactly.
 *
 * Arithmetic.  f32 throughout.  Every layer of 64 or more inputs runs on v_mfma_f32_16x16x4_f32: per output the bias, then
 * four fused chains over interleaved 16-input groups (chain c takes the groups c, c + 4, ...), added pairwise
 * ((c0 + c1) + (c2 + c3)); the 3-input layer is plain fused multiply-adds.
 *
 * Pooling.  The maximum is exact.  The mean is a fixed-order sum divided by n_points[b]: the points are summed in tiles of 64
 * (point 16 t + p of a 32-point half: t = 0, 1 in order, then a butterfly over p; the two halves; then the tiles in ascending
 * order), which depends on nothing but the cloud's own rows and count.  No atomics on floats anywhere.
 *
 * The batch runs in chunks of up to 128 clouds over context workspace of
 *     4100 * stride + 4 * k * stride + 8192 * ceil(stride / 64) + 11264   bytes per cloud of a chunk (+ 1024),
 * (8.8 MB a cloud at stride 2048 and k = 20, 4.4 MB at 1024), grown on demand (see ifd.h); a failed allocation is IFD_ERR_NOMEM. */
int ifd_dgcnn_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, int B, int stride, float* logits,
                      const ifd_dgcnn_aux* aux, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_DGCNN_H */
