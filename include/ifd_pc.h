/*
 * ifd_pc.h - C ABI of the PointConv victim classifier in libifd.so: PointConvDensityClsSsg(num_classes=40) in eval()
 * (baselines/model/pointconv.py), the fourth column of the reference's result tables.  Exported from the same library as
 * include/ifd.h and versioned on its own; the conventions of ifd_cls.h hold (int status, device pointers, `stream` =
 * hipStream_t as void*, calls only enqueue work except where noted), and the contexts made here are destroyed with ifd_destroy
 * and report through ifd_last_error.
 *
 * PointConv does not sit behind ifd_cls_*: IFD_CLS_POINTCONV stays refused there.
 */
#ifndef IFD_PC_H
#define IFD_PC_H
#include <stddef.h>
#include <stdint.h>
#include "ifd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_PC_ABI_VERSION 1
#define IFD_MODEL_PC 6               /* context kind (beside IFD_MODEL_CONVONET / _ONET / _DUP / _CLS / _DGCNN / _PN2) */

#define IFD_PC_MAX_POINTS 2048       /* largest stride / n_points of ifd_pc_forward */
#define IFD_PC_MIN_POINTS 32         /* smallest: sa1 takes the 32 nearest points of a centroid (the reference's topk raises below) */
#define IFD_PC_NPOINT1 512           /* sa1: centroids, 32 nearest neighbours, bandwidth 0.1 */
#define IFD_PC_K1 32
#define IFD_PC_NPOINT2 128           /* sa2: centroids of the 512, 64 nearest neighbours, bandwidth 0.2 */
#define IFD_PC_K2 64                 /* sa3: one group of the 128, bandwidth 0.4 */
#define IFD_PC_CHUNK 32              /* most clouds of one chunk of ifd_pc_forward */

int ifd_pc_abi_version(void);

/* Number of floats of the weights: 19,559,411.  Canonical order: every layer as {weight [out][in], bias [out]} with its
 * eval-mode BatchNorm (running statistics, eps 1e-5) already folded in, by the formulas of ifd_cls.h,
 *     w' = w * gamma / sqrt(var + eps),    b' = (b - mean) * gamma / sqrt(var + eps) + beta
 * (every convolution and linear here has a bias); fc3 has no BatchNorm and is stored as it is.  In network order, per level
 * densitynet x 3, mlp x 3, weightnet x 3, linear:
 *     sa1  [8,1] [8,8] [1,8]   [64,3] [64,64] [128,64]          [8,3] [8,8] [16,8]   [128,2048]       275,353 floats
 *     sa2  [8,1] [8,8] [1,8]   [128,131] [128,128] [256,128]    [8,3] [8,8] [16,8]   [256,4096]     1,115,609
 *     sa3  [8,1] [8,8] [1,8]   [256,259] [512,256] [1024,512]   [8,3] [8,8] [16,8]   [1024,16384]  17,502,041
 *     fc1 [512,1024]  fc2 [256,512]  fc3 [40,256]                                                     666,408
 * Input columns keep the reference's order: of an MLP's first layer the first 3 columns multiply xyz_j - c_i, the others the
 * features of point j; column c * 16 + w of a level's linear multiplies G[c][w] of the contraction below. */
size_t ifd_pc_weight_count(void);

/* A PointConv context on `device`.  weights_host is HOST memory in the canonical order.  n_classes == 40.  A NULL pointer, a
 * wrong count or n_classes fail before any HIP call is made: NULL, with the message in ifd_last_error(NULL).
 * Replaces: PointConvDensityClsSsg(num_classes=40) + load_state_dict (baselines/inference.py). */
ifd_ctx* ifd_pc_create(const float* weights_host, size_t n_weights, int n_classes, int device);

/* Optional outputs of ifd_pc_forward (each pointer may be NULL):
 *   fps1        [B][512] int32       the level-1 centroids, indices into the cloud, in pick order
 *   fps2        [B][128] int32       the level-2 centroids, indices into the 512
 *   knn1        [B][512][32] int32   the nearest neighbours of every level-1 centroid, indices into the cloud
 *   knn2        [B][128][64] int32   the nearest neighbours of every level-2 centroid, indices into the 512
 *   dens1       [B][stride]          DensityNet's output s_j of every point of the cloud (rows beyond n_points are not written)
 *   dens2       [B][512]             ... of the level-1 centroids
 *   dens3       [B][128]             ... of the level-2 centroids
 *   l1_feat     [B][512][128]        sa1's output, centroid-major
 *   l2_feat     [B][128][256]        sa2's output
 *   global_feat [B][1024]            sa3's output
 *   pred        [B] int32            argmax of the logits; among equal logits the LOWEST class wins
 * l1_feat, l2_feat and global_feat are written four floats at a time: like `logits`, they must be 16-byte aligned. */
typedef struct ifd_pc_aux {
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
    int32_t* pred;
} ifd_pc_aux;

/* model.eval()(pc.transpose(1, 2)): pc [B][stride][3] -> logits [B][40] (16-byte aligned: written four floats at a time).
 * n_points (optional) [B] int32, device memory: cloud b is its first n_points[b] rows; rows beyond take no part (they may
 * hold anything, NaN included).  NULL means every cloud has `stride` rows.  32 <= n_points[b] <= stride <= IFD_PC_MAX_POINTS.
 * fps_start (optional) [B][2] int32, device memory: {s1, s2}, the first pick of the level-1 sampling (0 <= s1 < n_points[b]) and
 * of the level-2 sampling (0 <= s2 < 512).  NULL means {0, 0}.  The reference draws them with torch.randint; here they are an
 * input, and the library has no random state.  Anything out of range: IFD_ERR_ARG and nothing else is enqueued.  Counts and
 * starts live on the device, so a call WITH n_points or fps_start blocks the host once, until a checking kernel enqueued on
 * `stream` has run; a call without either never blocks.
 * A cloud's outputs do not depend on B, on its position in the batch, on stride, on the chunks or on the other clouds, bit for
 * bit.
 *
 * Distance (sampling, nearest neighbours and density alike).  Between point j and centre c, in f32,
 *     dx = x_j - x_c,  dy = y_j - y_c,  dz = z_j - z_c,     d = (dx * dx + dy * dy) + dz * dz,
 * every difference, product and sum rounded to f32 on its own, in that order (nothing is fused): the distance of ifd_pn2.h.  The
 * distance of a point to itself, or to a bit-identical copy, is exactly 0.  The reference's knn_point and compute_density use
 * the matrix form (|a|^2 + |b|^2 - 2 <a, b>): a neighbour whose distance lies within that form's rounding of the K-th may be
 * another, and the density loses the matrix form's cancellation error.
 *
 * Farthest point sampling of npoint picks from n points: that of ifd_pn2.h.  The running distance of every point starts at
 * 1e10.  Pick 0 is the start index.  After pick p the running distance of every point j becomes d(j, p) where d(j, p) <
 * running_j (strictly), and the next pick is the point of the largest running distance, among equal ones the LOWEST index.  A
 * cloud of fewer than npoint points therefore repeats points (once every running distance is 0, index 0 is picked again and
 * again), as the reference does.  Level 2 samples the 512 level-1 centroids, repeats included.
 *
 * Nearest neighbours of centroid i over the n points of the level's input (sa1: the cloud, K = 32; sa2: the 512, K = 64): the K
 * points of smallest d, among equal d the LOWER index first, stored in ascending (d, index) order.  The centroid is one of the
 * points, so entry 0 is the lowest index among the centroid's bit-identical copies.  (The reference's topk(sorted=False) leaves
 * the order open; it is fixed here because the contraction sums over the row.)
 *
 * Density of point j among the n points of a level's input (sa1: the cloud; sa2: the 512; sa3: the 128), bandwidth bw = 0.1, 0.2,
 * 0.4: with c1 = (float)(2.0 * bw * bw) and c2 = (float)(2.5 * bw) as the reference's doubles rounded to f32,
 *     e_i = expf(-(d_ij / c1))        (the C library's expf, IEEE division; no fast intrinsic)
 *     rho_j = (sum_i e_i / (float)n) / c2.
 * The sum: 64 partial sums, partial l over i = l, l + 64, l + 128, ... in ascending order from 0, then added pairwise in a
 * butterfly (partials l and l ^ 1, then l ^ 2, ..., l ^ 32; IEEE addition is commutative, so all 64 ends are the same number).  An
 * index beyond n adds nothing.  DensityNet 1 -> 8 -> 8 -> 1 then runs on rho_j with ReLU after ALL THREE layers (the reference's
 * `i == len(self.mlp_convs)` is never true, so its sigmoid never runs): s_j >= 0.
 *
 * sa3's centre is the mean of the 128 level-2 centroids: per axis the coordinates added in ascending index from 0, times 1/128.
 * The xyz columns of sa3's MLP and its WeightNet act on xyz_j - mean (PointNet++ uses raw coordinates there).
 *
 * Layers.  f32 throughout, ReLU after every layer but fc3.  The small layers (DensityNet, WeightNet 3 -> 8 -> 8 -> 16 on
 * xyz_j - c_i, sa1's first layer) are one fused chain from the bias over the inputs in ascending order, fma(w[c], x[c], acc).  A
 * layer of 64 or more inputs runs on v_mfma_f32_16x16x4_f32 exactly as in ifd_pn2.h: inputs in blocks of 64 in ascending order,
 * a block is four fused chains from 0 over its four 16-input groups, added pairwise ((c0 + c1) + (c2 + c3)), and the blocks are
 * added one after the other to the bias - the 2048-, 4096- and 16384-wide linears included (32, 64 and 256 blocks).  Where three
 * coordinate columns stand in front of feature columns (sa2's and sa3's first layers) the feature columns are summed as above,
 * bias included, once per point j, and the coordinates are added to that sum as fma(w2, dz, fma(w1, dy, fma(w0, dx, sum))).
 * Contraction of a group with members k = 0 .. K-1 (the row's order; sa3: the 128 in index order), F the MLP's output:
 *     t[k][c] = F[k][c] * s_k   (rounded),     G[c][w] = fma(t[K-1][c], Wn[K-1][w], ... fma(t[0][c], Wn[0][w], 0)),
 * then the level's linear on G flattened as c * 16 + w.  No atomics on floats anywhere.
 *
 * The batch runs in chunks of up to IFD_PC_CHUNK clouds over context workspace of 5,903,360 bytes per cloud of a chunk
 * (+ 1024), of which the contraction's output takes 4 MB (sa1's [512][2048]; sa2's and sa3's reuse it), grown on demand (see
 * ifd.h); a failed allocation is IFD_ERR_NOMEM. */
int ifd_pc_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride,
                   float* logits, const ifd_pc_aux* aux, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_PC_H */
