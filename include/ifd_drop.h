/*
 * ifd_drop.h - C ABI of the saliency point-dropping attack ("Drop", baselines/attack/Saliency/Drop.py SaliencyDrop, driven by
 * baselines/attack_scripts/untargeted_drop_attack.py) on the PointNet victim, in libifd.so.  Built on ifd_cls_input_grad
 * (include/ifd_atk.h), versioned on its own; the conventions of ifd_atk.h hold: int status, device pointers, `stream` = hipStream_t
 * as void*, contexts made by ifd_cls_create WITHOUT feature_transform (any other is refused with IFD_ERR_ARG).  Clouds are
 * point-major, [B][stride][3], cloud b being its first n_points[b] rows.  The counts live on the device and SHRINK there: a whole
 * attack is enqueued without the host looking at anything between its rounds.
 *
 * What this library pins where the reference leaves bits open - decisions, every output bit follows from them:
 *   CENTRE     per coordinate the LOWER median of the cloud's n values: the element of rank (n - 1) / 2 in ascending order, what
 *              torch.median returns on the CPU.  Values compare as floats (-0 == +0; among equal values the lower row comes first,
 *              which only decides the sign of a zero centre).  A NaN is outside the contract.
 *   SALIENCY   d = x - c;  r = sqrtf((dx*dx + dy*dy) + dz*dz);  dot = (dx*gx + dy*gy) + dz*gz;  s = -(r^alpha) * dot, in float32, in
 *              that order, without contraction, with the correctly rounded square root.  alpha == 1 takes r itself, as torch's
 *              pow(x, 1) does: the reference script's setting and the only one held bit for bit.  Any other alpha > 0 goes through
 *              powf and agrees with the reference wherever the k-th and the (k + 1)-th saliency are further apart than rounding.
 *   SELECTION  the k highest saliencies are dropped; among equal values the lowest row goes first.  A total order - torch.topk
 *              promises none among equals, and at 1024 points most rows of a cloud have a gradient of exactly zero.
 *   ORDER      DEVIATION: the survivors KEEP THEIR INPUT ORDER (stable compaction).  The reference returns them in topk's order
 *              (ascending saliency, ties open), which carries no information and cannot be reproduced; every consumer of the file
 *              treats a cloud as a set.
 *   BATCHES    a cloud's result does not depend on B, on its position in the batch, on stride or on the other clouds, bit for bit:
 *              one workgroup a cloud, exact selections, integer counting, no float atomics.
 */
#ifndef IFD_DROP_H
#define IFD_DROP_H
#include <stddef.h>
#include <stdint.h>
#include "ifd_atk.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_DROP_ABI_VERSION 1
#define IFD_DROP_MAX_POINTS 2048     /* a cloud, its saliencies, ranks and indices live in one workgroup's LDS */

int ifd_drop_abi_version(void);

/* Optional outputs of ifd_drop_step, every one may be NULL (and `out` itself); clouds left untouched leave their rows untouched. */
typedef struct ifd_drop_out {
    float* saliency;         /* [B][stride]  over the cloud's first n rows, before the drop */
    float* center;           /* [B][3] */
    int32_t* dropped;        /* [B][k]       rows of the cloud as it was before this call, in drop order (highest saliency first) */
} ifd_drop_out;

/* One round of Drop.py:76-95, in place; never blocks.
 *   grad      [B][stride][3]  as ifd_cls_input_grad wrote it for pc with these counts
 *   pc        [B][stride][3]  in and out
 *   n_points  [B] int32, required, in and out
 *   index     [B][stride] int32 or NULL: compacted with the cloud, so that a caller can carry the rows' original indices through
 *             the rounds
 * Each cloud with k < n <= 2048 and n <= stride (n = n_points[b]) loses the k rows of highest saliency: the survivors move up and
 * keep their order, n_points[b] becomes n - k, rows n - k .. n - 1 are written as zeros (those of index as -1), rows from n on are
 * neither read nor written.  A cloud outside those limits is left wholly untouched, its count included.
 * Refused on the host with IFD_ERR_ARG: a missing pointer (grad, pc, n_points), B < 1, stride outside [1, 10000], k < 1, alpha not
 * a finite number above 0. */
int ifd_drop_step(ifd_ctx* ctx, const float* grad, float* pc, int32_t* n_points, int32_t* index, int B, int stride, int k, float alpha,
                  const ifd_drop_out* out, void* stream);

typedef struct ifd_drop_params {
    int32_t struct_size;     /* sizeof(ifd_drop_params) */
    int32_t num_drop;        /* >= 1, rows every cloud loses */
    int32_t k;               /* >= 1, rows a round drops (the reference's script: 5) */
    float alpha;             /* > 0 (the script: 1) */
    float scale;             /* the reference's loss is F.cross_entropy's mean over a batch of B_ref clouds: 1 / B_ref */
} ifd_drop_params;

/* The whole attack: pc_out = pc_in, then ceil(num_drop / k) rounds of ( ifd_cls_input_grad(pc_out, label, IFD_ATK_LOSS_CE, scale)
 * on the current counts; ifd_drop_step with k' = min(k, num_drop - round * k), Drop.py:65 ), then ifd_cls_forward on the result.
 *   pc_in    [B][stride][3];  n_points [B] or NULL (every cloud has `stride` rows);  label [B] int32, the clouds' true classes
 *   pc_out   [B][stride][3], must not overlap pc_in: cloud b is its first n_out[b] rows; the rows it lost are zeros, rows from
 *            n_points[b] on are pc_in's
 *   n_out    [B] int32 = n - num_drop
 *   kept     [B][stride] int32 or NULL: pc_out[b][i] == pc_in[b][kept[b][i]] for i < n_out[b], -1 beyond
 *   correct  [B] int32 = (pred == label) of the final forward.  The reference calls its sum success_num and its script turns it
 *            into `acc`: the attack is untargeted, "success" counts the clouds that are STILL classified correctly.
 * Counts and labels are checked once at the start (the one blocking step); nothing blocks between the rounds: the launches' grids
 * depend on B and stride only, the shrinking counts are read on the device.
 * Refused on the host with IFD_ERR_ARG before anything is enqueued: params missing or of another struct_size, num_drop < 1, k < 1,
 * alpha not a finite number above 0, B < 1, stride outside [1, 10000], a missing pointer (pc_in, label, pc_out, n_out, correct),
 * pc_out overlapping pc_in, num_drop >= min(stride, 2048), and with n_points == NULL stride above 2048.  At the blocking check: n_points[b]
 * outside [num_drop + 1, min(stride, 2048)], label outside [0, 40).
 * Workspace, grown on the context: ifd_cls_input_grad's (or the final forward's, if larger) + 12 * stride + 164 bytes per cloud of
 * the WHOLE batch (gradient; logits and prediction of the final forward), rounded up to 256. */
int ifd_drop_attack(ifd_ctx* ctx, const ifd_drop_params* params, const float* pc_in, const int32_t* n_points, const int32_t* label,
                    int B, int stride, float* pc_out, int32_t* n_out, int32_t* kept, int32_t* correct, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_DROP_H */
