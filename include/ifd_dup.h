/*
 * ifd_dup.h - C ABI of the baseline defenses in libifd.so: SRS, SOR and DUP-Net (SOR + PU-Net x4 upsampling),
 * the reference's baselines/defend_npz.py.  Exported from the same library as include/ifd.h and versioned on its
 * own; the conventions of ifd.h hold (int status, device pointers, `stream` = hipStream_t as void*, calls only enqueue
 * work except where noted), and the contexts made here are destroyed with ifd_destroy and report through ifd_last_error.
 * SOR itself is ifd.h's ifd_sor, which works on these contexts unchanged.
 *
 * Random draws.  The reference never seeds (np.random.choice, torch.randint).  Here every draw is Philox-4x32-10 of
 * (global cloud index = cloud_index_base + b, draw position, stage), keyed by `seed`, so results do not depend on how a
 * file is batched: stage 16 = SRS, 17 = the DUP fill, 18 + v = the FPS start of SA level v.  A draw below n is
 * floor(r * n / 2^32) of a 32-bit Philox word r; without-replacement choices are a partial Fisher-Yates shuffle over
 * [0, n) in the reference's draw order (the first draw is the first output row).  Every call also accepts explicit
 * draws (parity tests); explicit indices out of range are clamped into it, never read out of bounds.
 */
#ifndef IFD_DUP_H
#define IFD_DUP_H
#include <stddef.h>
#include <stdint.h>
#include "ifd.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IFD_DUP_ABI_VERSION 1
#define IFD_MODEL_DUP 2

int ifd_dup_abi_version(void);

/* Number of floats of the PU-Net weights (814,307) and their canonical order: the state_dict of
 * baselines/defense/DUP_Net/pu-in_1024-up_4.pth, each tensor in its torch layout ([out][in][1][1] weights, then bias):
 *   SA_modules.{0..3}.mlps.0.layer{0,1,2}.conv.{weight,bias}   [32,3] [32,32] [64,32] | [64,67] [64,64] [128,64] |
 *                                                                [128,131] [128,128] [256,128] | [256,259] [256,256] [512,256]
 *   FP_Modules.{0,1,2}.mlp.layer0.conv.{weight,bias}           [64,128] [64,256] [64,512]
 *   FC_Modules.{0..3}.layer{0,1}.conv.{weight,bias}            [256,259] [128,256]
 *   pcd_layer.0.layer0.conv.{weight,bias}  [64,128];   pcd_layer.1.layer0.conv.{weight,bias}  [3,64] */
size_t ifd_punet_weight_count(void);

/* Context of the baseline defenses on `device`.  weights_host (HOST memory, canonical order) may be NULL with n == 0:
 * such a context runs ifd_srs, ifd_sor and ifd_dup_fill but not ifd_punet_forward.  Any other count fails before a
 * HIP call is made (NULL, error in ifd_last_error(NULL)).
 * Replaces: DUPNet(...).pu_net.load_state_dict(torch.load(PU_NET_WEIGHT)) (baselines/defend_npz.py:38-45). */
ifd_ctx* ifd_dup_create(const float* weights_host, size_t n_weights, int device);

/* SRSDefense.random_drop (baselines/defense/drop_points/SRS.py:24-33): out [B, K - drop_num, 3] = rows of pc [B,K,3]
 * in draw order.  idx (optional) [B, K - drop_num] int32: explicit draws (distinct indices in [0, K)).
 * 1 <= K - drop_num, drop_num >= 0, K <= 10000. */
int ifd_srs(ifd_ctx* ctx, const float* pc, int B, int K, int drop_num, uint64_t seed, int64_t cloud_index_base,
            const int32_t* idx, float* out, void* stream);

/* DUPNet.process_data (baselines/defense/DUP_Net/DUP_Net.py:29-62) on SOR's output given as ifd_sor's keep_mask [B,K]:
 * the N kept rows (original order) of each cloud padded or trimmed to npoint rows -> out [B, npoint, 3]:
 *   N > npoint:  the rows of choice(N, npoint, replace=False), in draw order;
 *   N < npoint:  npoint // N whole copies of the kept rows, then the rows of choice(N, npoint - N * (npoint // N));
 *   N == npoint: the kept rows.
 * draws (optional) [B, npoint] int32: explicit choices (indices into the kept rows; the first 0, npoint or
 * npoint - N * (npoint // N) entries are read).  n_kept (optional) [B] int32 = N.  npoint must be 1024
 * (IFD_ERR_UNSUPPORTED otherwise); K <= 10000. */
int ifd_dup_fill(ifd_ctx* ctx, const float* pc, const uint8_t* keep_mask, int B, int K, int npoint, uint64_t seed,
                 int64_t cloud_index_base, const int32_t* draws, float* out, int32_t* n_kept, void* stream);

/* Optional outputs of every discrete decision of ifd_punet_forward (each pointer may be NULL):
 *   fps_idx  [B][1920]          FPS indices of SA levels 0..3 (1024 | 512 | 256 | 128), each into its level's input
 *                               (level 0: the input points; level v: level v-1's centroids in FPS order)
 *   ball_idx [B][1920][32]      ball-query indices of every centroid, same level order and indexing
 *   knn_idx  [B][3][1024][3]    the 3 nearest centroids of SA level f + 1 for each input point, FP module f = 0..2 */
typedef struct ifd_punet_aux {
    int32_t* fps_idx;
    int32_t* ball_idx;
    int32_t* knn_idx;
} ifd_punet_aux;

/* PUNet(npoint=1024, up_ratio=4, use_bn=False, use_res=False).forward (baselines/defense/DUP_Net/pu_net.py:88-132):
 * xyz [B,1024,3] -> out [B,4096,3], output row k * 1024 + i = expansion branch k, point i.  fps_start (optional)
 * [B][4] int32: the start index of each level's FPS (torch.randint(0, N, (B,)) per level, pu_utils.py:68); without it
 * the draws are the library's.  aux (optional) as above.  Only npoint == 1024 and up_ratio == 4 are built
 * (IFD_ERR_UNSUPPORTED otherwise).  The batch runs in chunks of up to 512 clouds over context workspace of
 * 1,398,784 bytes per cloud of a chunk (grown on demand, see ifd.h).  f32 throughout; the FPS, ball-query and 3-NN
 * distances are the reference's float32 expressions in its operation order. */
int ifd_punet_forward(ifd_ctx* ctx, const float* xyz, int B, int npoint, int up_ratio, const int32_t* fps_start,
                      uint64_t seed, int64_t cloud_index_base, float* out, const ifd_punet_aux* aux, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IFD_DUP_H */
