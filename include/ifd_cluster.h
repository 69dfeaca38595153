/*
 * ifd_cluster.h - C ABI of the Carlini-Wagner cluster-adding attack ("Add-Cluster", baselines/attack/CW/Add_Cluster.py
 * CWAddClusters with FarChamferDist(num_add, 'adv2ori', 0.1), driven by baselines/attack_scripts/targeted_add_cluster_attack.py)
 * on the PointNet victim, in libifd.so.  Built on ifd_cls_input_grad (ifd_atk.h), on the state and the weight search of ifd_cw.h
 * and on the selection of ifd_add.h, versioned on its own; the conventions of ifd_atk.h / ifd_add.h hold: int status, device
 * pointers, `stream` = hipStream_t as void*, clouds point-major, contexts made by ifd_cls_create WITHOUT feature_transform (any
 * other is refused with IFD_ERR_ARG).  Every per-cloud reduction runs in one fixed order, no float atomics: a cloud's result does
 * not depend on B, on its position in the batch or on the other clouds, bit for bit.
 *
 * The attack adds `num_add` CLUSTERS of `cl_num_p` points each: A = num_add * cl_num_p added rows behind the originals of a
 * concatenated cloud (ifd_add.h), cluster c owning the added rows [c * cl_num_p, (c + 1) * cl_num_p).  Limits:
 *   1 <= A <= IFD_ADD_MAX_ADD;  1 <= n_ori[b] <= IFD_ADD_MAX_ORI;  n_ori[b] + A <= cat_stride <= 10000.
 * Where the clusters start is the caller's: the reference clusters 128 critical points (ifd_add_critical_points with num_add =
 * 128) by DBSCAN and draws from the clusters on the host; ifd_cluster_dbscan is that clustering.
 *
 * DEVIATIONS from the reference, all of rounding or of the caller's freedom, none of them a switch:
 *   - The Chamfer part is ifd_add.h's: difference form, the lowest index among equal distances.
 *   - The far part compares SQUARED norms, fma(dz, dz, fma(dy, dy, dx * dx)), and takes one square root per cluster; the
 *     reference compares torch.norm's rounded roots.  Two pairs whose squares differ but whose rounded roots are equal may
 *     therefore be ranked where torch sees a tie (and takes the lowest j, then i): a rounding-level deviation.
 *   - Ties have an order (below); DBSCAN is this header's definition, not sklearn's text.
 *   - The start clusters and the start noise are the caller's.
 */
#ifndef IFD_CLUSTER_H
#define IFD_CLUSTER_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_add.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_CLUSTER_ABI_VERSION 1
#define IFD_CLUSTER_DBSCAN_MAX_POINTS 256

int ifd_cluster_abi_version(void);

/* DBSCAN of every cloud; never blocks.
 *   pts  [B][stride][3];  n_pts [B] or NULL (then every cloud has `stride` rows);  rows at or beyond n_pts[b] are never read
 *   labels  [B][stride] int32: the first n rows of a cloud are written, rows beyond are left as they were
 *   n_clusters (may be NULL) [B] int32: the number of clusters of every cloud
 * The definition, total - every bit of the output is determined:
 *   - q is a NEIGHBOUR of p iff d2 = (dx*dx + dy*dy) + dz*dz <= eps*eps, d = p - q in float32 difference form, in that order and
 *     without contraction; eps*eps is one float32 product.  p is its own neighbour.  (The relation is symmetric: d2 is.)
 *   - p is CORE iff it has >= min_samples neighbours.
 *   - The CLUSTERS are the connected components of the core points under neighbourhood, numbered 0, 1, ... by ascending lowest
 *     core index.
 *   - A non-core point with at least one core neighbour takes the LOWEST label among its core neighbours' clusters.
 *   - Every other point is -1.
 * sklearn.cluster.DBSCAN(eps, min_samples).fit_predict gives these labels wherever no pair of points lies within float32
 * rounding of eps (it visits the points in index order, so its clusters are numbered by their lowest core point and a border
 * point goes to the first cluster that reaches it - the lowest - too).
 * One workgroup of 256 threads a cloud, thread i owning point i: row i of the adjacency as 256 bits in its owner's registers (no
 * other thread reads it), the labels in LDS, min-label propagation over the core graph with pointer jumping to a fixed point, the
 * roots ranked by counting.  A NaN coordinate is nobody's neighbour, its
 * own included.
 * Refused on the host with IFD_ERR_ARG: a missing pointer (pts, labels), B < 1, stride outside [1, 10000], eps not a finite number
 * above 0, min_samples < 1, and with n_pts == NULL stride > 256.  A cloud whose n_pts[b] is outside [1, min(stride, 256)] is left
 * untouched, in both arrays. */
int ifd_cluster_dbscan(ifd_ctx* ctx, const float* pts, const int32_t* n_pts, int B, int stride, float eps, int min_samples,
                       int32_t* labels, int32_t* n_clusters, void* stream);

/* Optional outputs of ifd_cluster_step, every one may be NULL (and `diag` itself); they cost nothing when NULL. */
typedef struct ifd_cluster_diag {
    float* dist_grad;        /* [B][A][3]        the distance term of step 4 (Chamfer and far part together) */
    int32_t* nn_ori;         /* [B][A]           j(p), the nearest original */
    int32_t* far_i;          /* [B][num_add]     i*_c, as a row of the cloud's added rows (0 .. A - 1) */
    int32_t* far_j;          /* [B][num_add]     j*_c, likewise */
    float* far_val;          /* [B][num_add]     far_c */
} ifd_cluster_diag;

/* One iteration of Add_Cluster.py:183-236 behind the forward / backward pass on the concatenated cloud; never blocks.  The
 * arguments are ifd_add_step's, with num_add clusters of cl_num_p points; `state` has stride A = num_add * cl_num_p.
 * Per cloud, one workgroup, in this order:
 *   1. Chamfer part, ifd_add_step's steps 1 - 2 for IFD_ADD_CHAMFER: min_p, j(p), cd = (sum_p min_p) / A.
 *   2. Far part.  Per cluster c, over the ORDERED pairs (i, j) of its rows: n2(i, j) = fma(dz, dz, fma(dy, dy, dx * dx)) with
 *      d = (p_j - p_i) + 1e-7f per coordinate (i == j included: n2 = 3e-14).  (i*_c, j*_c) is the arg-max; among equal n2 the
 *      lowest j, then the lowest i - the pair torch's CPU max over i and then over j returns.  far_c = sqrtf(n2(i*, j*)), one
 *      root per cluster;  far = sum_c far_c, a serial sum from 0 in ascending c, accumulated in float64 and rounded to float32 once
 *      (with 512 clusters a float32 accumulator loses 1e-5 of a sum of 60, many times the reference's pairwise torch.sum).
 *   3. dist = far + cd * 0.1f (a product, then a sum; no fma).  The two records exactly as ifd_cw_step's step 2; o_bestattack
 *      and last_input take the added rows bit for bit, as they were forwarded, BEFORE the update.
 *   4. g_p = fma(c_cd, adv_p - ori_j(p), grad[n_ori + p]) per coordinate, then, only where s_p = [p == j*_c] - [p == i*_c] is not
 *      zero, g_p += s_p * u_c with u_c = (c_far * d(i*, j*)) / far_c per coordinate, and
 *        c_far = scale * (float)weight;   c_cd = (c_far * 0.1f) * (2 / (float)A)
 *      autograd's gradient of mean_b(dist_b * weight_b) with the argmins and arg-maxes held constant.  Where i* == j* (cl_num_p == 1,
 *      or a cluster of identical rows, whose diagonal is the maximum) the far term is exactly zero: nothing is added.  far_c >=
 *      sqrt(3) * 1e-7 > 0 always, so nothing non-finite appears.
 *   5. ifd_cw_step's Adam (ifd_cw.h step 5) on the added rows only.
 *   info = { loss[b] (0 when loss is NULL), far * w + (cd * w) * 0.1f with w = (float)weight (no fma), dist }.
 * Refused on the host with IFD_ERR_ARG: a missing state member or pointer, t < 1, B < 1, num_add < 1, cl_num_p < 1, A outside
 * [1, 1024], cat_stride > 10000, cat_stride < A + 1, and with n_ori == NULL cat_stride - A > 2048.  A cloud whose n_ori[b] is
 * outside [1, min(2048, cat_stride - A)] is left untouched, in every array. */
int ifd_cluster_step(ifd_ctx* ctx, const ifd_cw_state* state, const float* grad, const int32_t* pred, const float* loss,
                     const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info,
                     const ifd_cluster_diag* diag, int t, float lr, float scale, int B, int cat_stride, int num_add, int cl_num_p,
                     void* stream);

/* The end of a search step is ifd_cw_adjust(ctx, state, target, NULL, B, A, stream), as it is. */

typedef struct ifd_cluster_params {
    int32_t struct_size;     /* sizeof(ifd_cluster_params) */
    int32_t loss_kind;       /* IFD_ATK_LOSS_* */
    int32_t binary_step;     /* >= 1 */
    int32_t num_iter;        /* >= 1, Adam steps per search step */
    int32_t num_add;         /* clusters */
    int32_t cl_num_p;        /* points per cluster; 1 <= num_add * cl_num_p <= IFD_ADD_MAX_ADD */
    float kappa, scale, attack_lr, init_weight, max_weight;
} ifd_cluster_params;

/* The whole attack: binary_step x ( added rows = clusters + noise[step];  num_iter x (ifd_cls_input_grad on the concatenation,
 * ifd_cluster_step);  ifd_cw_adjust ), then the ending of Add_Cluster.py:266-278.
 *   pc_in    [B][stride][3], n_points [B] or NULL (every cloud has `stride` rows)
 *   clusters [B][A][3]  the start of the added rows, made by the caller
 *   noise    [binary_step][B][A][3], drawn by the caller (the reference: randn * 1e-7); NULL: no noise
 *   pc_out, best_dist, success, bounds: exactly as ifd_add_attack's, with A added rows
 * Counts and targets are checked once at the start (the one blocking step); nothing blocks afterwards.
 * Refused on the host with IFD_ERR_ARG before anything is enqueued: params missing or of another struct_size, an unknown loss_kind,
 * binary_step < 1, num_iter < 1, num_add < 1, cl_num_p < 1, A outside [1, 1024], B < 1, stride or out_stride outside [1, 10000], a
 * missing pointer, pc_out overlapping pc_in, and with n_points == NULL stride outside [1, 2048] or stride + A > out_stride.  At the
 * blocking check: n_points[b] outside [1, min(stride, 2048, out_stride - A)], target outside [0, 40).
 * Workspace, grown on the context: ifd_cls_input_grad's at max(stride, out_stride), + 12 * max(stride, out_stride) + 48 * A + 52
 * bytes per cloud of the WHOLE batch (gradient; m, v, o_bestattack, last_input; the records, weights, pred, loss, the two
 * counts), rounded up to 256. */
int ifd_cluster_attack(ifd_ctx* ctx, const ifd_cluster_params* params, const float* pc_in, const int32_t* n_points,
                       const int32_t* target, const float* clusters, const float* noise, int B, int stride, int out_stride,
                       float* pc_out, float* best_dist, int32_t* success, double* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_CLUSTER_H */
