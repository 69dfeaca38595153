/*
 * ifd_object.h - C ABI of the Carlini-Wagner object-adding attack ("Add-Objects", baselines/attack/CW/Add_Objects.py CWAddObjects
 * with L2ChamferDist(num_add, 'adv2ori', 0.2), driven by baselines/attack_scripts/targeted_add_object_attack.py) on the PointNet
 * victim, in libifd.so.  Built on ifd_cls_input_grad (ifd_atk.h), on the state and the weight search of ifd_cw.h and on the
 * concatenated cloud of ifd_add.h, versioned on its own; the conventions of ifd_cluster.h hold: int status, device pointers,
 * `stream` = hipStream_t as void*, clouds point-major, contexts made by ifd_cls_create WITHOUT feature_transform (any other is
 * refused with IFD_ERR_ARG).  Every per-cloud reduction runs in one fixed order, no float atomics: a cloud's result does not depend
 * on B, on its position in the batch or on the other clouds, bit for bit.
 *
 * The attack adds `num_add` OBJECTS of `obj_num_p` points each: A = num_add * obj_num_p added rows behind the originals of a
 * concatenated cloud (ifd_add.h), object c owning the added rows [c * obj_num_p, (c + 1) * obj_num_p).  What is optimised is not the
 * added rows but, per cloud, the object-frame points obj [A][3], one shift [3] and one angle per object; the added ("world") rows
 * the victim sees are
 *     world_p = rotate_shift(obj_p, angle_c, shift_c),   c = p / obj_num_p                                    (THE PLACEMENT)
 *     c = cosf(angle), s = sinf(angle)  (the accurate functions, not the hardware approximations)
 *     r_x = fma(x, c, -(z * s));   r_y = y;   r_z = fma(x, s, z * c)             (r: the rotated row before the shift)
 *     world = (r_x + sx, y + sy, r_z + sz)
 * one product and one fma per rotated coordinate, then one sum, nothing contracted further: the row vector times the reference's
 * matrix [[c, 0, s], [0, 1, 0], [-s, 0, c]] about the y axis.  y' = y + sy is exact at every angle; with angle == 0 (c = 1, s = 0)
 * world = obj + shift bit for bit.  The template `objects` [num_add][obj_num_p][3] the L2 part measures against is ONE array shared
 * by every cloud of the batch, as in the reference.  Limits:
 *   1 <= A <= IFD_ADD_MAX_ADD;  1 <= n_ori[b] <= IFD_ADD_MAX_ORI;  n_ori[b] + A <= cat_stride <= 10000.
 *
 * DEVIATIONS from the reference, all of rounding or of the caller's freedom, none of them a switch:
 *   - The Chamfer part is ifd_add.h's: difference form, the lowest index among equal distances.
 *   - The rotation is the three lines above, not a 3 x 3 torch.bmm (which also adds the exact zeros of the matrix).
 *   - Where l2 == 0 the L2 part contributes exactly zero to the gradient (ifd_cw_step's step 4; autograd gives NaN there, and the
 *     reference's start noise keeps it away).
 *   - The reference's angles are [B][num_add][3]; only component 0 enters its rotation, the other two have zero gradient, never move
 *     and reach no output: one angle per object here.
 *   - Objects, centres, start noise and start angles are the caller's.
 */
#ifndef IFD_OBJECT_H
#define IFD_OBJECT_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_add.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_OBJECT_ABI_VERSION 1

int ifd_object_abi_version(void);

/* The attack's state, all on the device.  `cw` has stride A: m and v are Adam's moments of the object rows, o_bestattack holds WORLD
 * rows, the records and the weights are ifd_cw.h's - ifd_cw_adjust(ctx, &state->cw, target, NULL, B, A, stream) ends a search step as
 * it is (it also zeroes cw.m and cw.v; the pose moments below are the caller's to zero at the start of a search step). */
typedef struct ifd_object_state {
    ifd_cw_state cw;
    float* obj;              /* [B][A][3]        the object-frame points */
    float* shift;            /* [B][num_add][3] */
    float* angle;            /* [B][num_add]     radians about the y axis */
    float* shift_m;          /* [B][num_add][3]  Adam's exp_avg of the shifts */
    float* shift_v;          /* [B][num_add][3]  exp_avg_sq */
    float* angle_m;          /* [B][num_add] */
    float* angle_v;          /* [B][num_add] */
} ifd_object_state;

/* world = THE PLACEMENT of (obj, angle, shift) into the added rows of `cat` [B][cat_stride][3], rows n_ori[b] .. n_ori[b] + A - 1 of
 * cloud b (n_ori NULL: cat_stride - A originals in every cloud); never blocks.  The original rows and the rows beyond are not
 * touched.  Refused on the host with IFD_ERR_ARG: a missing pointer (obj, angle, shift, cat), B < 1, num_add < 1, obj_num_p < 1, A
 * outside [1, 1024], cat_stride > 10000, cat_stride < A + 1, and with n_ori == NULL cat_stride - A > 2048.  A cloud whose n_ori[b] is
 * outside [1, min(2048, cat_stride - A)] is left untouched. */
int ifd_object_place(ifd_ctx* ctx, const float* obj, const float* angle, const float* shift, float* cat, const int32_t* n_ori, int B,
                     int cat_stride, int num_add, int obj_num_p, void* stream);

/* Optional outputs of ifd_object_step, every one may be NULL (and `diag` itself); they cost nothing when NULL. */
typedef struct ifd_object_diag {
    float* obj_grad;         /* [B][A][3]        g_obj of step 5, the whole gradient Adam takes on the object rows */
    int32_t* nn_ori;         /* [B][A]           j(p), the nearest original of world row p */
    float* g_shift;          /* [B][num_add][3] */
    float* g_angle;          /* [B][num_add] */
    float* l2;               /* [B] */
    float* cd;               /* [B] */
} ifd_object_diag;

/* One iteration of Add_Objects.py:256-340 behind the forward / backward pass on the concatenated cloud; never blocks.
 *   objects [num_add][obj_num_p][3]  the template, shared by the batch
 *   grad, pred, loss, target, cat, n_ori, last_input [B][A][3], info [B][3], t, lr, scale: as ifd_add_step takes them.  The added rows
 *   of `cat` must be THE PLACEMENT of the state (ifd_object_place, or this call's own step 8): they are read as they were forwarded.
 * Per cloud, one workgroup of 256 threads, thread t owning the added rows t, t + 256, ..., in this order:
 *   1. Chamfer part, ifd_add_step's steps 1 - 2 for IFD_ADD_CHAMFER on the world rows read from `cat`: d = fma(dz, dz, fma(dy, dy,
 *      dx * dx)) with d. = world_p - ori_j, min_p the smallest over ascending j (the lowest j among equals), j(p) its index,
 *      cd = (sum_p min_p) / A: a thread's sum over its rows in ascending order, then the fixed tree over the 256 threads.
 *   2. l2 = sqrtf(sum over the 3 A coordinates of (obj - objects)^2): ifd_cw_step's sum - thread t takes the coordinates t, t + 256,
 *      ... as a = fma(d, d, a), then the same fixed tree.
 *   3. dist = l2 + cd * 0.2f (a product, then a sum; no fma).
 *   4. The two records exactly as ifd_cw_step's step 2; o_bestattack and last_input (may be NULL) take the forwarded world rows bit
 *      for bit, BEFORE the update.
 *   5. The gradients, with c, s, r of THE PLACEMENT recomputed from the state before the update,
 *        c_w = scale * (float)weight;   c_cd = (c_w * 0.2f) * (2 / (float)A);   c_l2 = l2 > 0 ? c_w / l2 : 0
 *        gw_p    = fma(c_cd, world_p - ori_j(p), grad[n_ori + p])                                 per coordinate
 *        g_obj_p = fma(c_l2, obj_p - objects_p, (fma(gw_x, c, gw_z * s),  gw_y,  fma(gw_z, c, -(gw_x * s))))     per coordinate
 *        ga_p    = fma(gw_z, r_x, -(gw_x * r_z))
 *        g_shift_c = sum of gw_p,  g_angle_c = sum of ga_p  over the object's rows p = c * obj_num_p, ... in ASCENDING p, a serial
 *                    sum from 0 accumulated in float64 and rounded to float32 once (a serial float32 sum of up to 1024 terms carries
 *                    many times the error of the reference's pairwise torch sums: ifd_cluster_step's far sum).
 *      autograd's gradient of mean_b(dist_b * weight_b) + the adversarial term with the argmins held constant.
 *   6. ifd_cw_step's Adam (ifd_cw.h step 5) on the object rows (cw.m, cw.v), on the shifts (shift_m, shift_v) and on the angles
 *      (angle_m, angle_v), all with step t.
 *   7. angle = remainder(angle, (float)(2 pi)) as torch computes it in float32: r = fmodf(angle, b); where r != 0 and r < 0, r += b.
 *   8. The added rows of `cat` = THE PLACEMENT of the new state: what the next forward pass sees.
 *   info = { loss[b] (0 when loss is NULL), l2 * w + (cd * w) * 0.2f with w = (float)weight (no fma), dist }.
 * Refused on the host with IFD_ERR_ARG: a missing state member or pointer (objects, grad, pred, target, cat), t < 1, B < 1, num_add <
 * 1, obj_num_p < 1, A outside [1, 1024], cat_stride > 10000, cat_stride < A + 1, and with n_ori == NULL cat_stride - A > 2048.  A cloud
 * whose n_ori[b] is outside [1, min(2048, cat_stride - A)] is left untouched, in every array. */
int ifd_object_step(ifd_ctx* ctx, const ifd_object_state* state, const float* objects, const float* grad, const int32_t* pred,
                    const float* loss, const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info,
                    const ifd_object_diag* diag, int t, float lr, float scale, int B, int cat_stride, int num_add, int obj_num_p,
                    void* stream);

typedef struct ifd_object_params {
    int32_t struct_size;     /* sizeof(ifd_object_params) */
    int32_t loss_kind;       /* IFD_ATK_LOSS_* */
    int32_t binary_step;     /* >= 1 */
    int32_t num_iter;        /* >= 1, Adam steps per search step */
    int32_t num_add;         /* objects */
    int32_t obj_num_p;       /* points per object; 1 <= num_add * obj_num_p <= IFD_ADD_MAX_ADD */
    float kappa, scale, attack_lr, init_weight, max_weight;
} ifd_object_params;

/* The whole attack: binary_step x ( obj = objects + noise_obj[step], shift = centers + noise_shift[step], angle = angles0[step], every
 * moment 0, THE PLACEMENT;  num_iter x (ifd_cls_input_grad on the concatenation, ifd_object_step);  ifd_cw_adjust ), then the ending of
 * Add_Objects.py:355-367: a cloud whose lower is still 0 gets the last forwarded world rows.
 *   pc_in    [B][stride][3], n_points [B] or NULL (every cloud has `stride` rows)
 *   objects  [num_add][obj_num_p][3], shared;  centers [B][num_add][3], made by the caller
 *   noise_obj   [binary_step][B][A][3], noise_shift [binary_step][B][num_add][3], drawn by the caller (the reference: randn * 1e-7);
 *               either may be NULL: no noise
 *   angles0  [binary_step][B][num_add], drawn by the caller (the reference: rand * pi)
 *   pc_out, best_dist, success, bounds: exactly as ifd_add_attack's, with A added rows
 * Counts and targets are checked once at the start (the one blocking step); nothing blocks afterwards.
 * Refused on the host with IFD_ERR_ARG before anything is enqueued: params missing or of another struct_size, an unknown loss_kind,
 * binary_step < 1, num_iter < 1, num_add < 1, obj_num_p < 1, A outside [1, 1024], B < 1, stride or out_stride outside [1, 10000], a
 * missing pointer (pc_in, target, objects, centers, angles0, pc_out, best_dist, success), pc_out overlapping pc_in, and with n_points
 * == NULL stride outside [1, 2048] or stride + A > out_stride.  At the blocking check: n_points[b] outside [1, min(stride, 2048,
 * out_stride - A)], target outside [0, 40).
 * Workspace, grown on the context: ifd_cls_input_grad's at max(stride, out_stride), + 12 * max(stride, out_stride) + 60 * A + 48 *
 * num_add + 52 bytes per cloud of the WHOLE batch (gradient; m, v, o_bestattack, last_input, obj; shift, angle and their moments; the
 * records, weights, pred, loss, the two counts), rounded up to 256. */
int ifd_object_attack(ifd_ctx* ctx, const ifd_object_params* params, const float* pc_in, const int32_t* n_points,
                      const int32_t* target, const float* objects, const float* centers, const float* noise_obj,
                      const float* noise_shift, const float* angles0, int B, int stride, int out_stride, float* pc_out,
                      float* best_dist, int32_t* success, double* bounds, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_OBJECT_H */
