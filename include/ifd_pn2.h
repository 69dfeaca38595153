/*
 * ifd_pn2.h - C ABI of the PointNet++ victim classifier in libifd.so: PointNet2ClsSsg(num_classes=40) in eval()
 * (baselines/model/pointnet2.py), the second column of the reference's result tables.  Exported from the same library as
 * include/ifd.h and versioned on its own; the conventions of ifd_cls.h hold (int status, device pointers, `stream` =
 * hipStream_t as void*, calls only enqueue work except where noted), and the contexts made here are destroyed with ifd_destroy
 * and report through ifd_last_error.
 *
 * PointNet++ does not sit behind ifd_cls_*: IFD_CLS_POINTNET2 stays refused there.
 */
#ifndef IFD_PN2_H
#define IFD_PN2_H
#include <stddef.h>
#include <stdint.h>
#include "ifd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_PN2_ABI_VERSION 1
#define IFD_MODEL_PN2 5              /* context kind (beside IFD_MODEL_CONVONET / _ONET / _DUP / _CLS / _DGCNN) */

#define IFD_PN2_MAX_POINTS 2048      /* largest stride / n_points of ifd_pn2_forward */
#define IFD_PN2_NPOINT1 512          /* sa1: centroids, ball r = 0.2, 32 samples */
#define IFD_PN2_NSAMPLE1 32
#define IFD_PN2_NPOINT2 128          /* sa2: centroids of the 512, ball r = 0.4, 64 samples */
#define IFD_PN2_NSAMPLE2 64

int ifd_pn2_abi_version(void);

/* Number of floats of the weights: 1,469,032.  Canonical order: every layer as {weight [out][in], bias [out]} with its
 * eval-mode BatchNorm (running statistics, eps 1e-5) already folded in, by the formulas of ifd_cls.h,
 *     w' = w * gamma / sqrt(var + eps),    b' = (b - mean) * gamma / sqrt(var + eps) + beta
 * (every convolution here has a bias); fc3 has no BatchNorm and is stored as it is.  In network order:
 *     sa1 [64,3] [64,64] [128,64]    sa2 [128,131] [128,128] [256,128]    sa3 [256,259] [512,256] [1024,512]
 *     fc1 [512,1024]  fc2 [256,512]  fc3 [40,256]
 * Input columns keep the reference's order: of sa2's first layer the first 3 columns multiply xyz_j - c_i, the other 128 the
 * level-1 features of point j; of sa3's the first 3 multiply the raw coordinates of the level-2 centroids, the other 256
 * their features (sample_and_group, sample_and_group_all). */
size_t ifd_pn2_weight_count(void);

/* A PointNet++ context on `device`.  weights_host is HOST memory in the canonical order.  n_classes == 40.  A NULL pointer, a
 * wrong count or n_classes fail before any HIP call is made: NULL, with the message in ifd_last_error(NULL).
 * Replaces: PointNet2ClsSsg(num_classes=40) + load_state_dict (baselines/inference.py). */
ifd_ctx* ifd_pn2_create(const float* weights_host, size_t n_weights, int n_classes, int device);

/* Optional outputs of ifd_pn2_forward (each pointer may be NULL):
 *   fps1        [B][512] int32       the level-1 centroids, indices into the cloud, in pick order
 *   fps2        [B][128] int32       the level-2 centroids, indices into the 512
 *   ball1       [B][512][32] int32   the ball of every level-1 centroid, indices into the cloud
 *   ball2       [B][128][64] int32   the ball of every level-2 centroid, indices into the 512
 *   l1_feat     [B][512][128]        sa1's output, centroid-major
 *   l2_feat     [B][128][256]        sa2's output
 *   global_feat [B][1024]            sa3's output
 *   pred        [B] int32            argmax of the logits; among equal logits the LOWEST class wins
 * l1_feat, l2_feat and global_feat are written four floats at a time: like `logits`, they must be 16-byte aligned. */
typedef struct ifd_pn2_aux {
    int32_t* fps1;
    int32_t* fps2;
    int32_t* ball1;
    int32_t* ball2;
    float* l1_feat;
    float* l2_feat;
    float* global_feat;
    int32_t* pred;
} ifd_pn2_aux;

/* model.eval()(pc.transpose(1, 2)): pc [B][stride][3] -> logits [B][40] (16-byte aligned: written four floats at a time).
 * n_points (optional) [B] int32, device memory: cloud b is its first n_points[b] rows; rows beyond take no part (they may
 * hold anything, NaN included).  NULL means every cloud has `stride` rows.  1 <= n_points[b] <= stride <= IFD_PN2_MAX_POINTS.
 * fps_start (optional) [B][2] int32, device memory: {s1, s2}, the first pick of the level-1 sampling (0 <= s1 < n_points[b]) and
 * of the level-2 sampling (0 <= s2 < 512).  NULL means {0, 0}.  The reference draws them with torch.randint; here they are an
 * input, and the library has no random state.  Anything out of range: IFD_ERR_ARG and nothing else is enqueued.  Counts and
 * starts live on the device, so a call WITH n_points or fps_start blocks the host once, until a checking kernel enqueued on
 * `stream` has run; a call without either never blocks.
 * A cloud's outputs do not depend on B, on its position in the batch, on stride, on the chunks or on the other clouds, bit for
 * bit.
 *
 * Distance (sampling and ball query alike).  Between point j and centre c, in f32,
 *     dx = x_j - x_c,  dy = y_j - y_c,  dz = z_j - z_c,     d = (dx * dx + dy * dy) + dz * dz,
 * every difference, product and sum rounded to f32 on its own, in that order (nothing is fused).  The distance of a point to
 * itself, or to a bit-identical copy, is exactly 0.
 *
 * Farthest point sampling of npoint picks from n points.  The running distance of every point starts at 1e10.  Pick 0 is the
 * start index.  After pick p the running distance of every point j becomes d(j, p) where d(j, p) < running_j (strictly), and
 * the next pick is the point of the largest running distance, among equal ones the LOWEST index.  A cloud of fewer than npoint
 * points therefore repeats points (once every running distance is 0, index 0 is picked again and again), as the reference
 * does.  Level 2 samples the 512 level-1 centroids, repeats included.
 *
 * Ball query of centroid i over n points.  j is a member iff !(d_ij > r2), r2 = (float)((double)r * (double)r) with r = 0.2
 * (level 1) or 0.4 (level 2) as doubles.  The row is the first nsample members in ascending index; missing entries are filled
 * with the row's first member.  The centroid is one of the points, so it is a member (d = 0) and the row is never empty.  This
 * is the reference's query_ball_point with its matrix-form distance (|a|^2 + |b|^2 - 2 <a, b>) replaced by the difference form
 * above: a point whose distance lies within rounding of r2 may fall on the other side.
 *
 * Layers.  f32 throughout, ReLU after every layer but fc3.  A layer of 64 or more inputs runs on v_mfma_f32_16x16x4_f32, its
 * inputs in blocks of 64 in ascending order: a block is four fused chains from 0 over its four 16-input groups, added pairwise
 * ((c0 + c1) + (c2 + c3)), and the blocks are added one after the other to the bias.  (fc_kernel's four chains run through the
 * whole input; here they are cut at every block.  Measured with the chains uncut: the global feature of a 1024-point cloud
 * lay at 4.12 times the float32 oracle's own error against float64, 1.9 to 3.7 times at the other sizes, where the bar is 4;
 * with the cut 1.94 at the worst over all sizes, every other tensor below that - DESIGN 7n.)  sa1's first layer is
 * fma(w2, dz, fma(w1, dy, fma(w0, dx, b))) on the differences to the centroid.  Where three coordinate columns stand in front of feature columns (sa2's and sa3's first layers) the feature
 * columns are summed as above, bias included, and the coordinates are added to that sum the same way: fma(w2, z, fma(w1, y,
 * fma(w0, x, sum))), on xyz_j - c_i (formed first, in f32) in sa2 and on the raw coordinates in sa3.  sa2's feature sum
 * depends on j alone and is computed once per level-1 point, not once per group member.  The maximum over a group is exact.
 * No atomics on floats anywhere.
 *
 * The batch runs in chunks of up to 128 clouds over context workspace of 1,172,480 bytes per cloud of a chunk (+ 1024), grown
 * on demand (see ifd.h); a failed allocation is IFD_ERR_NOMEM. */
int ifd_pn2_forward(ifd_ctx* ctx, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B, int stride,
                    float* logits, const ifd_pn2_aux* aux, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_PN2_H */
