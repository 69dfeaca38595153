// Host-side internal interface between the C ABI (api.cpp) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cmath>
#include "ifd_device.h"

namespace ifd {

struct OptArgs {
    int steps, t0, loss_batch, normalize, knn_scan_every_step, planes_shared;
    float lr, rep_weight, threshold, rep_radius, rep_h, rep_eps;
    DecConst dc;
    unsigned int coop_timeout_ticks;   // bound of a split cloud's cross-CU waits, in ticks of the 100 MHz wall clock (knn_device.h coop_wait)
    int test_drop_member;              // test hook (env IFD_TEST_COOP_DROP): this member of every split cloud never arrives; -1 = off
    int precision;                     // ifd_opt_params.precision: 0 f32 MFMA tiles, 1 bf16x6, 2 bf16x3 (tile_bf.h); the caller passes the matching image
};

// The context's device counter buffer (api.cpp d_counters, unsigned long long): IFD_N_COUNTERS public diagnostics of the last
// optimise call, the wave trace of -DIFD_TRACE builds, then two STICKY status words that no optimise call clears
// (ifd_optimize_status reads and resets them): points whose fixed-point repulsion sums came within a factor two of wrapping,
// and cross-CU waits of split clouds that gave up.
constexpr int DEV_COUNTERS = 16 + 8 * 32;
constexpr int STATUS_OVERFLOW = DEV_COUNTERS;
constexpr int STATUS_TIMEOUT = DEV_COUNTERS + 1;
// ... and the time-out word of the CURRENT optimise call: cleared by every ifd_optimize / ifd_onet_optimize in front of its launches.
// A waiter that gives up raises this word and the sticky one; the other waiters fall out on THIS word only (round-4 advisor: when
// they looked at the sticky word, one time-out made the first wait of every later launch on the context fail too, until the host
// had called ifd_optimize_status).
constexpr int STATUS_TIMEOUT_CUR = DEV_COUNTERS + 2;
constexpr int TRACE2_BASE = DEV_COUNTERS + 3;        // -DIFD_TRACE2 builds: [8 waves][128] stamps inside one decoder tile per wave
constexpr int DEV_COUNTERS_TOTAL = TRACE2_BASE + 8 * 128;

// offsets (floats) of the point-net tensors inside the canonical weight vector (include/ifd.h order)
struct EncPointOffsets {
    int pos_w, pos_b, fc0_w[5], fc0_b[5], fc1_w[5], fc1_b[5], sc_w[5], fcc_w, fcc_b;
};

hipError_t configure_encoder_kernels();
int enc_image_floats();
void build_enc_image(const float* w, const EncPointOffsets& eo, float* img);      // host: aligned point-net weights (encoder.hip)
// zero-fills planes itself
hipError_t launch_encode_points(const float* w, const EncPointOffsets& eo, const float* enc_img, const float* sel,
                                const int* t_per_cloud, int B, int Tmax, float* planes, float* c_out, DecConst dc, hipStream_t s);

// device pointers to the re-packed ([tap][Cin][Cout]) U-Net weights
struct UNetWeights {
    const float *down_w[4][2], *down_b[4][2];
    const float *up_t_w[3], *up_t_b[3], *up_w[3][2], *up_b[3][2];
    const float *fin_w, *fin_b;
    // the 3x3 layers once more in the Winograd F(2x2, 3x3) domain: U = G g G^T, [Cin / 16][16 xi][Cout][16] (unet.hip wino_kernel)
    const float *down_u[4][2], *up_u[3][2];
};
hipError_t configure_unet_kernels();
size_t unet_workspace_floats(int n_img);
hipError_t launch_unet(const UNetWeights& W, const float* x, float* out, float* ws, int n_img, hipStream_t s);

struct PrepArgs {
    int cloud_base;            // global index of cloud 0 of this call (RNG counter)
    int n_sel, n_opt;          // encoder subset size (600), optimised points per cloud (1024)
    float padding_scale, init_sigma;
    uint32_t seed_lo, seed_hi;
    int no_morton;             // measurement hook (IFD_TEST_NO_MORTON with IFD_ENABLE_TEST_HOOKS=1, read at create): the library's own draws keep their draw order
};
constexpr int PREP_MAXK = 10000;     // largest input cloud (points) of ifd_sor / ifd_prepare (prep.hip: LDS of prepare_kernel)
hipError_t configure_prep_kernels();
hipError_t launch_sor(const float* pc, int B, int K, int k_nn, double alpha, uint8_t* keep, double* value, hipStream_t s);
hipError_t launch_prepare(const float* pc, const uint8_t* keep, int B, int K, const PrepArgs& a, const int32_t* sel_idx,
                          const int32_t* init_idx, const float* noise, float* sel, int32_t* t_per_cloud, float* init,
                          int32_t* n_kept, float* proc_out, hipStream_t s);

hipError_t configure_optimize_kernels();
// ws: optimize_ws_bytes(B) of context workspace; split: ifd_opt_params.split; n_cu: compute units of the device
hipError_t launch_optimize(const float* dec_img, const float* planes, float* p, float* m, float* v, float* loss,
                           const int32_t* loss_batch_per_cloud, void* ws, unsigned long long* counters,
                           const float* adam_tab, int B, int K, const OptArgs& a, int split, int n_cu, hipStream_t s);
size_t optimize_ws_bytes(int B);
// ... and its layout: neighbour lists of the B clouds | exchange blocks of split clouds | Adam moments of the split-precision kernels
class Carve;
struct CoopWs;
struct OptWs { uint16_t* knn_lists; CoopWs* coop; f32x4* mv; };
OptWs optimize_ws(Carve& c, int B);
// per-step Adam bias corrections {lr / (1 - beta1^t), sqrt(1 - beta2^t)}, t = t0 + 1 ... t0 + steps -> tab[steps][2]
hipError_t launch_adam_table(float* tab, int t0, int steps, float lr, hipStream_t s);
// bytes of context workspace ifd_optimize needs for B clouds (certified neighbour lists)
size_t knn_list_bytes(int B);
hipError_t launch_decode(const float* dec_img, const float* planes, const float* p, int B, int K, float* logits,
                         float* dlogit_dp, DecConst dc, hipStream_t s);
// ... in a split-precision mode (decode_bf.hip: the optimiser's own tile in MODE_SUM); dec_img_bf = the bf16 piece image
hipError_t configure_decode_bf_kernels();
hipError_t launch_decode_bf(int prec, const float* dec_img_bf, const float* planes, const float* p, int B, int K, float* logits, float* dlogit_dp,
                            DecConst dc, int n_cu, hipStream_t s);
hipError_t launch_repulsion(const float* p, int B, int K, float* loss, float* grad, int32_t* knn_idx, float radius,
                            float h, float eps, hipStream_t s);
hipError_t launch_normalize(float* p, int B, int K, hipStream_t s);
// clouds of MAXK < K <= LARGE_MAXK optimised points: two launches per Adam step (optimize.hip, "large" section)
size_t large_ws_bytes(int B, int K, bool own_moments);
// ... and its layout: [G: B K float4 | own moments (if the caller passes none) | global repulsion accumulators (K > LARGE_LDS_MAXK) |
// certified neighbour lists (K <= LARGE_LDS_MAXK), 16-byte aligned]
struct LargeWs { f32x4* G; float* moments; void *f, *lists; };
LargeWs large_ws(Carve& c, int B, int K, bool own_moments);
// dec_img: the image of a.precision (f32: the optimiser's copy; 1 / 2: the bf16 piece image)
hipError_t launch_large_occupancy(int precision, const float* dec_img, const float* planes, const float* p, int B, int parts, int K,
                                  const int32_t* loss_batch_per_cloud, int loss_batch, float thr, int want_loss, void* G, DecConst dc,
                                  hipStream_t s);
struct LargeLists {
    uint16_t* lists;     // [B][K][LL_M]
    f32x4* cert;         // [B][K]  {position at build time, rho}
    f32x2* dbase;        // [B][K]  {S at build time, alpha: the point's own rho^2 / d5^2 - shrunk when its ball overflowed its list, grown when it
                         //          was half empty, like the persistent kernel's al_f / al_b}
    float* scal;         // [B][4]  S(now) = sum over the call's steps so far of max_j |x_j(s + 1) - x_j(s)|, -, -, -
};
LargeLists large_lists(Carve& c, int B, int K);
size_t large_list_bytes(int B, int K);        // certified neighbour lists of the launch-per-step path (0 beyond LARGE_LDS_MAXK points)
void* large_list_ws(void* ws, int B, int K, bool own_moments);                                      // ... inside ws (nullptr beyond)
size_t large_f_bytes(int B, int K);           // global repulsion accumulators of clouds beyond LARGE_LDS_MAXK points (0 below)
hipError_t large_f_prepare(void* ws, int B, int K, bool own_moments, void** f_ws, hipStream_t s);   // ... at the end of ws, zeroed
hipError_t launch_large_repulsion(const float* p, int B, int K, float* loss, float* grad, int32_t* knn_idx, float radius,
                                  float h, float eps, void* f_ws, hipStream_t s);
// one Adam step from the occupancy gradients G ([B][K] float4: d loss / d xyz, BCE term): exact 5-NN + repulsion + Adam
hipError_t launch_large_step(float* p, float* m, float* v, const void* G, int B, int K, const float* adam_tab, int step,
                             const int32_t* loss_batch_per_cloud, const OptArgs& a, float* loss, void* f_ws, void* list_ws,
                             unsigned long long* counters, hipStream_t s);
hipError_t launch_large_normalize(float* p, int B, int K, hipStream_t s);

// ---- ONet-Opt (onet.hip) --------------------------------------------------------------------------------
// offsets (floats) into the canonical ONet weight vector (include/ifd.h order)
struct OnetEncOffsets {
    int pos_w, pos_b, fc0_w[5], fc0_b[5], fc1_w[5], fc1_b[5], sc_w[5], fcc_w, fcc_b;
};
struct OnetDecOffsets {
    int cbn_gamma_w[11], cbn_gamma_b[11], cbn_beta_w[11], cbn_beta_b[11], cbn_mean[11], cbn_var[11], fc0_b[5];
};
hipError_t configure_onet_kernels();
hipError_t configure_onet_bf_kernels();
// split-precision ONet-Opt launch (onet_bf.hip): img_bf = the bf16 piece image of api.cpp onet_fragment_image_bf, precision 1 | 2
hipError_t launch_onet_optimize_bf(int precision, const float* img_bf, const float* small, const float* ab, float* p, float* m, float* v,
                                   float* loss, const int32_t* loss_batch_per_cloud, uint16_t* knn_lists, unsigned long long* counters,
                                   const float* adam_tab, int B, int K, const OptArgs& a, hipStream_t s);
size_t onet_encode_ws_floats(int B, int Tmax);
int onet_small_floats();
hipError_t launch_onet_encode(const float* w, const OnetEncOffsets& eo, const float* sel, const int* t_per_cloud, int B,
                              int Tmax, float* ws, float* c_out, hipStream_t s);
hipError_t launch_onet_cbn(const float* w, const OnetDecOffsets& od, const float* c, int B, float* gb, float* ab,
                           hipStream_t s);
hipError_t launch_onet_decode(const float* img, const float* small, const float* ab, const float* p, int B, int K,
                              float* logits, float* dlogit_dp, hipStream_t s);
hipError_t launch_onet_large_occupancy_bf(int precision, const float* img_bf, const float* small, const float* ab, const float* p, int B,
                                          int parts, int K, const int32_t* loss_batch_per_cloud, int loss_batch, float thr, void* G,
                                          hipStream_t s);                               // onet_bf.hip
hipError_t launch_onet_decode_bf(int precision, const float* img_bf, const float* small, const float* ab, const float* p, int B, int K,
                                 float* logits, float* dlogit_dp, hipStream_t s);      // onet_bf.hip
// clouds of MAXK < K <= LARGE_MAXK points (ONet/opt_defense.py:27 has no limit): two launches per Adam step, ws as
// large_ws_bytes
hipError_t launch_onet_large_optimize(const float* img, const float* small, const float* ab, float* p, float* m, float* v,
                                      float* loss, const int32_t* loss_batch_per_cloud, void* ws, unsigned long long* counters,
                                      const float* adam_tab, int B, int K, const OptArgs& a, hipStream_t s);
hipError_t launch_onet_optimize(const float* img, const float* small, const float* ab, float* p, float* m, float* v,
                                float* loss, const int32_t* loss_batch_per_cloud, uint16_t* knn_lists,
                                unsigned long long* counters, const float* adam_tab, int B, int K, const OptArgs& a,
                                hipStream_t s);

// ---- ONet-Mesh (mesh.hip) --------------------------------------------------------------------------------
// MISE state of a batch of clouds as dense arrays (per-cloud strides: P3 for val / known, pend_stride for pend,
// sub_total for sub / mix, cap for list)
struct MiseGrid {
    int res0, depth, P, P3, cap, sub_total, sub_off[4];
    size_t pend_stride;
    double threshold;
    float* val;          // [B][P3]   decoder logits at the grid points
    uint8_t* known;      // [B][P3]
    uint8_t* pend;       // [B][pend_stride]  queued for evaluation (byte flags)
    uint8_t* sub;        // [B][sub_total]    voxel of level l subdivided (levels concatenated)
    uint8_t* mix;        // [B][sub_total]    scratch of one update round
    int* list;           // [B][cap]  grid-point indices to evaluate this round
    int* count;          // [B]      queue length of this round (filled by the previous round's mise_apply_kernel)
    int* prev;           // [B]      points evaluated in the round mise_update is closing (0: nothing new is known, the cloud is skipped)
    int* plan;           // [B + 1]  exclusive prefix of the clouds' 128-point decoder passes of this round (grid_plan_kernel)
};
hipError_t launch_mise_init(const MiseGrid& g, int B, hipStream_t s);
hipError_t launch_mise_update(const MiseGrid& g, int B, hipStream_t s);
hipError_t launch_mise_fill(const MiseGrid& g, int B, hipStream_t s);
hipError_t launch_mise_gather(const MiseGrid& g, const float* field, int B, hipStream_t s);
hipError_t launch_onet_grid_eval(const float* img, const float* small, const float* ab, const MiseGrid& g, int B,
                                 int n_blocks, float box, hipStream_t s);
hipError_t launch_onet_grid_eval_bf(int precision, const float* img_bf, const float* small, const float* ab, const MiseGrid& g, int B,
                                    int n_blocks, float box, hipStream_t s);
hipError_t mc_upload_table();
void mc_host_table(int8_t (*tri)[16], uint8_t* ntri);
hipError_t launch_marching_cubes(const float* val, int B, int P, double iso, float box, int* cube_offs, int* ntri_total,
                                 int cap, float* tris, double* area, hipStream_t s);
hipError_t launch_copy_triangles(const float* tris, const double* area, const int* ntri_total, int B, int cap, float* out_tris,
                                 double* out_area, hipStream_t s);
hipError_t launch_sample_surface(const float* tris, const double* cum_area, const int* ntri_total, int B, int cap, int n,
                                 uint64_t seed, int cloud_base, float* out, hipStream_t s);

// ---- baseline defenses: SRS, DUP-Net fill, PU-Net (punet.hip; C ABI in include/ifd_dup.h) ----------------------------
constexpr int DUP_NP = 1024;            // PU-Net input points (npoint)
constexpr int DUP_NS = 1920;            // centroids of the four SA levels per cloud (1024 + 512 + 256 + 128)
constexpr int DUP_NSAMPLE = 32;         // ball-query samples
constexpr int DUP_FEAT_FLOATS = 4 * 65536;   // SA outputs per cloud: [1024][64] | [512][128] | [256][256] | [128][512]
constexpr uint32_t DUP_STAGE_SRS = 16, DUP_STAGE_FILL = 17, DUP_STAGE_FPS = 18;   // Philox counter word 2 (FPS: + level)
__host__ __device__ constexpr int dup_level_off(int v) { return v == 0 ? 0 : (v == 1 ? 1024 : (v == 2 ? 1536 : 1792)); }
__host__ __device__ constexpr size_t dup_feat_off(int v) { return (size_t)v * 65536; }
// radius ** 2 of the reference (a Python double), compared against the float32 distances in float32
__host__ __device__ constexpr float dup_radius2(int v) {
    return v == 0 ? (float)(0.05 * 0.05) : (v == 1 ? (float)(0.1 * 0.1) : (v == 2 ? (float)(0.2 * 0.2) : (float)(0.3 * 0.3)));
}
struct DupDraws { uint32_t cloud_base, seed_lo, seed_hi; };
struct PunetLayer { int w, b; };        // float offsets of a layer's tile image and padded bias inside the PU-Net image
struct PunetHead { PunetLayer fp[3], fc0[4], fc1[4], pcd0, pcd1; };
struct PunetImage { PunetLayer sa[4][3]; PunetHead head; int total; };
struct PunetWs {                        // per-chunk scratch of launch_punet (api.cpp punet_ws_bytes)
    float* nxyz;     // [B][1920][3]  centroids of the four levels
    int32_t* fidx;   // [B][1920]     FPS indices (into the level's input)
    int32_t* bidx;   // [B][1920][32] ball-query indices
    float* feat;     // [B][DUP_FEAT_FLOATS]
    int32_t* kidx;   // [B][3][1024][3]  3-NN of the FP modules
    float* kw;       // [B][3][1024][3]  normalised weights
};
hipError_t configure_punet_kernels();
hipError_t launch_srs(const float* pc, int B, int K, int m, const int32_t* idx, DupDraws d, float* out, hipStream_t s);
hipError_t launch_dup_fill(const float* pc, const uint8_t* keep, int B, int K, const int32_t* draws, DupDraws d, float* out,
                           int32_t* n_kept, hipStream_t s);
hipError_t launch_punet(const float* img, const PunetImage& I, const float* xyz, int B, const int32_t* fps_start, DupDraws d,
                        const PunetWs& w, float* out, hipStream_t s);

// ---- victim classifier: PointNet (pointnet.hip; C ABI in include/ifd_cls.h) ------------------------------------------
constexpr int CLS_TILE = 256;           // points of one workgroup of the fused point-MLP + max kernel
constexpr int CLS_FEAT = 1024;          // width of the max-pooled feature
// One dense layer inside a device image, as float offsets of its weight and bias.  PointNet's FC layers (ClsFc) keep the weight
// as an MFMA tile image (punet.hip layout) with a padded bias; DGCNN's and PointNet++'s keep it row-major [n_out][n_in] with
// bias [n_out] (victim_linear.h).
struct DenseLayer { int w, b, n_out, n_in; };
using ClsFc = DenseLayer;
// One per-point stack ending in the max over points: [3 -> 64] (plain FMAs), optionally [64 -> 64], [64 -> 128], [128 -> 1024].
struct ClsStack { int first, mid_w, mid_b, w2, b2, w3, b3; };      // first: [64][4] = {w0, w1, w2, bias} per output channel
struct ClsImage {
    ClsStack stn, fstn, trunk;          // fstn.first == trunk.first (the STNkd runs on the trunk's conv1 output)
    ClsFc stn_fc[3], fstn_fc[3], head_fc[3];
    int total;
};
struct ClsWs {                          // per-chunk scratch of launch_cls (api.cpp cls_ws_bytes)
    float* part;     // [B][T][1024]  maxima of the 256-point tiles, T = ceil(stride / 256)
    float* gmax;     // [B][1024]
    float* f1;       // [B][512]
    float* f2;       // [B][256]
    float* trans;    // [B][16]      (9 used)
    float* tfeat;    // [B][4096]    (feature_transform only)
};
// bad[0] = number of clouds with n_points (not null) outside [lo, hi]: [1, stride], or [k, stride] for DGCNN
hipError_t launch_count_check(const int32_t* n_points, int B, int lo, int hi, int32_t* bad, hipStream_t s);
// pred[b] = the lowest class among the largest logits of cloud b (torch.argmax on the CPU): the one tie rule of all victims
hipError_t launch_argmax(const float* logits, int B, int n_classes, int32_t* pred, hipStream_t s);
hipError_t launch_cls(const float* img, const ClsImage& I, bool feature_transform, const float* pc, const int32_t* n_points, int B,
                      int stride, const ClsWs& w, float* logits, int n_classes, int32_t* pred, hipStream_t s);


// ---- shared by the victims' attacks (pointnet_grad.hip; C ABI in include/ifd_atk.h) ----------------------------------
// the one check of every attack call: bad[0] = clouds with n_points outside [lo, hi] (n_points may be null), bad[1] = targets
// outside [0, n_classes)
hipError_t launch_atk_check(const int32_t* n_points, const int32_t* target, int B, int lo, int hi, int n_classes, int32_t* bad,
                            hipStream_t s);
// loss [B] and d_out [B][64] = scale * d loss / d logits (zeros behind the classes), the losses of include/ifd_atk.h
hipError_t launch_loss_grad(const float* logits, const int32_t* target, int B, int n_classes, int loss_kind, float kappa, float scale,
                            float* loss, float* d_out, hipStream_t s);
hipError_t launch_fgm_update(int kind, const float* grad, float* pc, const float* ori_pc, float* momentum, float step_size, float budget,
                             float mu, const int32_t* n_points, int B, int stride, hipStream_t s);
hipError_t launch_atk_success(const int32_t* pred, const int32_t* target, int B, int32_t* success, hipStream_t s);
// the counts and starts of an attack loop on a victim that samples (victim_atk.hip): bad[0] = clouds with n_points (may be null:
// hi) outside [lo, hi], bad[1] = clouds with fps_start (may be null) outside [0, n - shrink) x [0, np1)
hipError_t launch_victim_sample_check(const int32_t* n_points, const int32_t* fps_start, int B, int lo, int hi, int shrink, int np1,
                                      int32_t* bad, hipStream_t s);

// ---- PointNet input gradients (pointnet_grad.hip; C ABI in include/ifd_atk.h) ------------------------------------------
// The backward pass's own weight image (api.cpp build_cls_grad_image): the FC layers transposed in the MFMA tile layout
// (a layer [out][in] becomes the layer [in][out padded to 64], zero bias), the point stacks' layers row-major.
struct ClsGradStack { int w1, w2, b2, w3; };     // w1: the forward's [64][4] = {w0, w1, w2, bias}; w2 [128][64]; b2 [128]; w3 [1024][128]
struct ClsGradImage {
    ClsGradStack stn, trunk;
    ClsFc stn_fct[3], head_fct[3];              // fc1^T, fc2^T, fc3^T
    int total;
};
struct ClsGradWs {                              // per-chunk scratch of ifd_cls_input_grad (api.cpp cls_grad_ws)
    float* part;        // [B][T][1024]
    int32_t* part_idx;  // [B][T][1024]
    float *gmax_stn, *gmax;          // [B][1024]
    int32_t *win_stn, *win;          // [B][1024]
    float *f1_stn, *f1;              // [B][512]
    float *f2_stn, *f2;              // [B][256]
    float* trans;       // [B][16]
    float* logits;      // [B][40]
    int32_t* pred;      // [B]
    float* loss;        // [B]
    float* d_out;       // [B][64]   d loss / d logits (40 used), later d loss / d trans (9 used); the rest zero
    float* d2;          // [B][256]
    float* d1;          // [B][512]
    float* g;           // [B][1024] d loss / d (max-pooled feature) of the stack being differentiated
};
hipError_t launch_cls_win(const float* img, const ClsImage& I, const float* pc, const int32_t* n_points, int B, int stride,
                          const ClsGradWs& w, int n_classes, hipStream_t s);
// after launch_cls_win: loss, its gradient through the head, the trunk, the STN head and the STN stack -> grad [B][stride][3]
hipError_t launch_cls_backward(const float* img, const ClsImage& I, const float* gimg, const ClsGradImage& G, const float* pc,
                               const int32_t* n_points, int B, int stride, const int32_t* target, int loss_kind, float kappa, float scale,
                               const ClsGradWs& w, int n_classes, float* grad, hipStream_t s);

// torch.optim.Adam's scalars of step t for the attacks' step kernels (atk_device.h atk_adam): step_size = lr / (1 - b1^t),
// bc2 = sqrt(1 - b2^t), omb1 = 1 - b1, omb2 = 1 - b2.  torch/optim/adam.py: Python doubles, rounded to float where they meet the
// float tensors (optimize.hip adam_table_kernel)
struct AdamStep { float step_size, bc2, omb1, omb2; };
inline AdamStep adam_step_consts(int t, float lr) {
    return AdamStep{(float)((double)lr / (1.0 - std::pow(0.9, (double)t))), (float)std::sqrt(1.0 - std::pow(0.999, (double)t)),
                    (float)(1.0 - 0.9), (float)(1.0 - 0.999)};
}

// ---- the CW point-perturbation attack (pointnet_cw.hip, include/ifd_cw.h) ----
struct CwState {                                // ifd_cw_state, member for member
    float *m, *v;                               // [B][stride][3]
    float* bestdist;                            // [B]
    int32_t* bestscore;
    float* o_bestdist;
    int32_t* o_bestscore;
    float* o_bestattack;                        // [B][stride][3]
    double *weight, *lower, *upper;             // [B]
};
hipError_t launch_cw_start(const float* pc_in, const float* noise, float* adv, const int32_t* n_points, int B, int stride, hipStream_t s);
hipError_t launch_cw_init(const CwState& S, int B, float init_weight, float max_weight, hipStream_t s);
hipError_t launch_cw_step(const CwState& S, const float* grad, const int32_t* pred, const float* loss, const int32_t* target, float* adv,
                          const float* ori, float* last_input, float* info, int t, float lr, float scale, const int32_t* n_points, int B,
                          int stride, hipStream_t s);
hipError_t launch_cw_adjust(const CwState& S, const int32_t* target, const int32_t* n_points, int B, int stride, hipStream_t s);
hipError_t launch_cw_finish(const CwState& S, const float* last_input, float* pc_out, int32_t* success, double* bounds,
                            const int32_t* n_points, int B, int stride, hipStream_t s);

// ---- the kNN attack (pointnet_knn.hip, include/ifd_knn.h) ----
constexpr int KNN_MAX_POINTS = 2048;            // IFD_KNN_MAX_POINTS: adv and ori of one cloud in a workgroup's static LDS
struct KnnDiag {                                // ifd_knn_diag, member for member; every pointer may be null
    float* info;                                // [B][4]
    float* dist_grad;                           // [B][stride][3]
    int32_t* nn_ori;                            // [B][stride]
    int32_t* nn5;                               // [B][stride][5]
    int32_t* mask;                              // [B][stride]
};
// one iteration behind ifd_cls_input_grad, a workgroup a cloud; 6 <= stride <= KNN_MAX_POINTS is the caller's to check
hipError_t launch_knn_step(const float* grad, const float* loss, float* adv, const float* ori, const float* normal, float* m, float* v,
                           const KnnDiag& D, float chamfer_weight, float knn_weight, float alpha, float budget, int t, float lr, float scale,
                           const int32_t* n_points, int B, int stride, hipStream_t s);
hipError_t launch_knn_clip(float* adv, const float* ori, const float* normal, float budget, const int32_t* n_points, int B, int stride,
                           hipStream_t s);

// ---- the CW point-adding attack (pointnet_add.hip, include/ifd_add.h) ----
constexpr int ADD_MAX_ADD = 1024;               // IFD_ADD_MAX_ADD, IFD_ADD_MAX_ORI: the added points and the originals of one cloud
constexpr int ADD_MAX_ORI = 2048;               // in a workgroup's static LDS
constexpr int ADD_CHAMFER = 0, ADD_HAUSDORFF = 1;        // IFD_ADD_CHAMFER, IFD_ADD_HAUSDORFF
struct AddDiag {                                // ifd_add_diag, member for member; every pointer may be null
    float* dist_grad;                           // [B][num_add][3]
    int32_t* nn_ori;                            // [B][num_add]
    int32_t* far;                               // [B]
};
// the limits on stride, num_add and (where n_points is null) the counts are the caller's to check
hipError_t launch_add_select(const float* grad, const float* pc, const int32_t* n_points, int B, int stride, int num_add, float* cri,
                             int32_t* idx, hipStream_t s);
// one iteration behind ifd_cls_input_grad on the concatenated cloud, a workgroup a cloud; S has stride num_add
hipError_t launch_add_step(int kind, const CwState& S, const float* grad, const int32_t* pred, const float* loss, const int32_t* target,
                           float* cat, const int32_t* n_ori, float* last_input, float* info, const AddDiag& D, int t, float lr, float scale,
                           int B, int cat_stride, int num_add, hipStream_t s);
// pc_out[b][0 .. n) = pc_in[b][0 .. n), n_ori[b] = n, n_cat[b] = n + num_add
hipError_t launch_add_begin(const float* pc_in, const int32_t* n_points, int B, int stride, int out_stride, int num_add, float* pc_out,
                            int32_t* n_ori, int32_t* n_cat, hipStream_t s);
hipError_t launch_add_start(const float* cri, const float* noise, const int32_t* n_cat, int B, int out_stride, int num_add, float* pc_out,
                            hipStream_t s);
hipError_t launch_add_finish(const CwState& S, const float* last_input, const int32_t* n_cat, int B, int out_stride, int num_add,
                             float* pc_out, int32_t* success, double* bounds, hipStream_t s);

// ---- the CW cluster-adding attack (pointnet_cluster.hip, include/ifd_cluster.h) ----
constexpr int CLUSTER_DBSCAN_MAX_POINTS = 256;  // IFD_CLUSTER_DBSCAN_MAX_POINTS: a point a thread, the adjacency as bits in LDS
struct ClusterDiag {                            // ifd_cluster_diag, member for member; every pointer may be null
    float* dist_grad;                           // [B][A][3]
    int32_t* nn_ori;                            // [B][A]
    int32_t *far_i, *far_j;                     // [B][num_add]
    float* far_val;                             // [B][num_add]
};
// a workgroup a cloud; the limits on stride, eps, min_samples and (where n_pts is null) the counts are the caller's to check
hipError_t launch_cluster_dbscan(const float* pts, const int32_t* n_pts, int B, int stride, float eps, int min_samples, int32_t* labels,
                                 int32_t* n_clusters, hipStream_t s);
// one iteration behind ifd_cls_input_grad on the concatenated cloud, a workgroup a cloud; S has stride num_add * cl_num_p
hipError_t launch_cluster_step(const CwState& S, const float* grad, const int32_t* pred, const float* loss, const int32_t* target,
                               float* cat, const int32_t* n_ori, float* last_input, float* info, const ClusterDiag& D, int t, float lr,
                               float scale, int B, int cat_stride, int num_add, int cl_num_p, hipStream_t s);

// ---- the CW object-adding attack (pointnet_object.hip, include/ifd_object.h) ----
struct ObjectState {                            // ifd_object_state, member for member
    CwState cw;                                 // stride A = num_add * obj_num_p
    float* obj;                                 // [B][A][3]
    float *shift, *angle;                       // [B][num_add][3], [B][num_add]
    float *shift_m, *shift_v;                   // [B][num_add][3]
    float *angle_m, *angle_v;                   // [B][num_add]
};
struct ObjectDiag {                             // ifd_object_diag, member for member; every pointer may be null
    float* obj_grad;                            // [B][A][3]
    int32_t* nn_ori;                            // [B][A]
    float *g_shift, *g_angle;                   // [B][num_add][3], [B][num_add]
    float *l2, *cd;                             // [B]
};
// the limits on cat_stride, num_add * obj_num_p and (where n_ori is null) the counts are the caller's to check
hipError_t launch_object_place(const float* obj, const float* angle, const float* shift, float* cat, const int32_t* n_ori, int B,
                               int cat_stride, int num_add, int obj_num_p, hipStream_t s);
// one iteration behind ifd_cls_input_grad on the concatenated cloud, a workgroup a cloud
hipError_t launch_object_step(const ObjectState& S, const float* objects, const float* grad, const int32_t* pred, const float* loss,
                              const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info,
                              const ObjectDiag& D, int t, float lr, float scale, int B, int cat_stride, int num_add, int obj_num_p,
                              hipStream_t s);
// the start of a search step of ifd_object_attack: obj, shift, angle from the caller's arrays, the pose moments zeroed, the placement
hipError_t launch_object_start(const ObjectState& S, const float* objects, const float* centers, const float* noise_obj,
                               const float* noise_shift, const float* angles0, const int32_t* n_cat, int B, int out_stride, int num_add,
                               int obj_num_p, float* pc_out, hipStream_t s);

// ---- the saliency Drop attack (pointnet_drop.hip, include/ifd_drop.h) ----
constexpr int DROP_MAX_POINTS = 2048;           // IFD_DROP_MAX_POINTS: a cloud, its saliencies, ranks and indices in a workgroup's LDS
struct DropOut {                                // ifd_drop_out, member for member; every pointer may be null
    float* saliency;                            // [B][stride]
    float* center;                              // [B][3]
    int32_t* dropped;                           // [B][k]
};
// one round, a workgroup a cloud, in place; 1 <= stride, k >= 1 and alpha > 0 are the caller's to check
hipError_t launch_drop_step(const float* grad, float* pc, int32_t* n_points, int32_t* index, int B, int stride, int k, float alpha,
                            const DropOut& D, hipStream_t s);
// n_out[b] = n_points[b] (stride where n_points is null); kept[b][i] = i below that count, -1 beyond (kept may be null)
hipError_t launch_drop_begin(const int32_t* n_points, int B, int stride, int32_t* n_out, int32_t* kept, hipStream_t s);

// ---- victim classifier: DGCNN (dgcnn.hip; C ABI in include/ifd_dgcnn.h) ----------------------------------------------
constexpr int DG_MAX_POINTS = 2048;     // IFD_DGCNN_MAX_POINTS
constexpr int DG_MAX_K = 32;
constexpr int DG_FEAT = 512;            // x1 | x2 | x3 | x4 = 64 + 64 + 128 + 256 channels of a point
constexpr int DG_EMB = 1024;            // conv5's width; the global feature is max | mean = 2 DG_EMB
constexpr int DG_TILE = 64;             // points of one workgroup of the MFMA layers, and of one partial max / sum of conv5
constexpr int DG_KNN_THREADS = 64;      // queries of one workgroup of the kNN kernel, a thread each
constexpr int DG_KNN_PEND = 8;          // candidates a thread queues before the wave updates its lists together
// The device image (api.cpp build_dgcnn_image).  The four edge convolutions are stored in split form: per layer the rows
// P = Wa (no bias) then Q = Wb - Wa (the folded bias), n_out = 2 Cout, n_in = C.  first: the C = 3 layer as [128][4] rows
// {w0, w1, w2, bias}.
struct DgImage {
    int first;
    DenseLayer pq[3];                   // conv2, conv3, conv4
    DenseLayer conv5, fc[3];
    int total;
};
struct DgWs {                           // per-chunk scratch of launch_dgcnn (api.cpp dgcnn_ws)
    float* feat;        // [B][stride][512]
    float* pq;          // [B][stride][512]   P | Q of the current layer (2 Cout <= 512 columns used)
    float* nrm;         // [B][stride]        |x_j|^2 of the current layer's input
    int32_t* idx;       // [B][stride][k]
    float* part_max;    // [B][T][1024], T = ceil(stride / DG_TILE)
    float* part_sum;    // [B][T][1024]
    float* gfeat;       // [B][2048]
    float* f1;          // [B][512]
    float* f2;          // [B][256]
};
struct DgOut {                          // where the caller wants the intermediate results; a null member stays in the scratch
    int32_t* idx[4];
    float* feat;
    float* gfeat;
    int32_t* pred;
};
hipError_t launch_dgcnn(const float* img, const DgImage& I, const float* pc, const int32_t* n_points, int B, int stride, int k,
                        const DgWs& w, const DgOut& out, float* logits, int n_classes, hipStream_t s);

// P | Q of edge convolution l + 1 (l = 0 .. 3) recomputed into w.pq from pc (l = 0) or from feat's columns, by the forward's kernels
hipError_t launch_dg_pq(const float* img, const DgImage& I, int l, const float* pc, const float* feat, const int32_t* n_points, int B,
                        int stride, float* pq, hipStream_t s);

// ---- DGCNN input gradients (dgcnn_grad.hip; C ABI in include/ifd_dgcnn_atk.h) ------------------------------------------
// The backward pass's weight image (api.cpp build_dgcnn_grad_image): every layer transposed, row-major [n_in of the forward][n_out
// of the forward], as a DenseLayer of linear_kernel whose bias is a shared block of zeros.  fct[2] (linear3) has its 40 inputs
// padded to 64 with zero columns.
struct DgGradImage {
    DenseLayer fct[3];                  // linear1^T [2048][512], linear2^T [512][256], linear3^T [256][64]
    DenseLayer pqt[3];                  // conv2 .. conv4: [P ; Q]^T, [C][2 Cout]
    int w5t;                            // conv5^T [512][1024]
    int total;
};
struct DgGradWs {                       // per-chunk scratch of launch_dgcnn_grad (api.cpp dgcnn_grad_ws)
    DgWs f;                             // the forward's
    int32_t* idx[4];    // [B][stride][k] each
    float* logits;      // [B][40]
    int32_t* pred;      // [B]
    float* loss;        // [B]
    float* d_out;       // [B][64]
    float* d2;          // [B][256]
    float* d1;          // [B][512]
    float* g;           // [B][2048]      d loss / d (max | mean)
    int32_t* wtile;     // [B][1024]      the first tile whose maximum is the cloud's
    int32_t* win_pool;  // [B][1024]
    float* dfeat;       // [B][stride][512]
    float* dx;          // [B][stride][128]
    int32_t* win;       // [B][stride][256]
};
struct DgGradOut {                      // ifd_dgcnn_grad_out's members that the kernels write themselves, so that rows beyond a
    int32_t* idx[4];                    // cloud stay as they were; null: not wanted (idx and feat then stay in the scratch)
    float* feat;
    int32_t* win_edge[4];
    uint32_t* act5;
};
hipError_t launch_dgcnn_grad(const float* img, const DgImage& I, const float* gimg, const DgGradImage& G, const float* pc,
                             const int32_t* n_points, int B, int stride, int k, const int32_t* target, int loss_kind, float kappa,
                             float scale, const DgGradWs& w, const DgGradOut& out, int n_classes, float* grad, hipStream_t s);

// ---- victim classifier: PointNet++ (pointnet2.hip; C ABI in include/ifd_pn2.h) ----------------------------------------
constexpr int PN2_MAX_POINTS = 2048;    // IFD_PN2_MAX_POINTS
constexpr int PN2_NP1 = 512, PN2_NS1 = 32;      // sa1: centroids, samples of a ball
constexpr int PN2_NP2 = 128, PN2_NS2 = 64;      // sa2
constexpr int PN2_EMB = 1024;           // width of the global feature
constexpr int PN2_FPS_THREADS = 256;    // a cloud a workgroup of the sampling kernel: thread t owns the points t + 256 k
// radius ** 2 of the reference (a Python double), compared against the float32 distances in float32
__host__ __device__ constexpr float pn2_radius2(int level) { return level == 0 ? (float)(0.2 * 0.2) : (float)(0.4 * 0.4); }
// The device image (api.cpp build_pn2_image).  A layer whose input begins with three coordinate columns is stored as two blocks:
// those columns as [n_out][4] rows {w0, w1, w2, bias or 0} and the feature columns as a plain layer.  sa1_first carries sa1's
// first bias; sa2_u and sa3_u carry theirs, so sa2_xyz and sa3_xyz end in 0.
struct Pn2Image {
    int sa1_first;                      // [64][4]
    DenseLayer sa1[2];                  // 64 -> 64, 64 -> 128
    int sa2_xyz;                        // [128][4]
    DenseLayer sa2_u, sa2[2];           // 128 -> 128 (the feature columns of the first layer); 128 -> 128, 128 -> 256
    int sa3_xyz;                        // [256][4]
    DenseLayer sa3_u, sa3[2];           // 256 -> 256; 256 -> 512, 512 -> 1024
    DenseLayer fc[3];
    int total;
};
struct Pn2Ws {                          // per-chunk scratch of launch_pn2 (api.cpp pn2_ws)
    float* xyz1;        // [B][512][3]   level-1 centroids
    float* xyz2;        // [B][128][3]
    int32_t* fps1;      // [B][512]
    int32_t* fps2;      // [B][128]
    int32_t* ball1;     // [B][512][32]
    int32_t* ball2;     // [B][128][64]
    float* l1_feat;     // [B][512][128]
    float* u2;          // [B][512][128]  b + W_f f of sa2's first layer
    float* l2_feat;     // [B][128][256]
    float* s3a;         // [B][128][256]
    float* s3b;         // [B][128][512]
    float* part_max;    // [B][2][1024]
    float* gfeat;       // [B][1024]
    float* f1;          // [B][512]
    float* f2;          // [B][256]
};
struct Pn2Out {                         // where the caller wants the intermediate results; a null member stays in the scratch
    int32_t *fps1, *fps2, *ball1, *ball2;
    float *l1_feat, *l2_feat, *gfeat;
    int32_t* pred;
};
hipError_t configure_pn2_kernels();
// bad[0] = clouds with n_points outside [1, stride]; bad[1] = clouds (of the others) with a start outside [0, n_points) / [0, 512)
hipError_t launch_pn2_check(const int32_t* n_points, const int32_t* fps_start, int B, int stride, int32_t* bad, hipStream_t s);
hipError_t launch_pn2(const float* img, const Pn2Image& I, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B,
                      int stride, const Pn2Ws& w, const Pn2Out& out, float* logits, int n_classes, hipStream_t s);

// ---- PointNet++ input gradients (pointnet2_grad.hip; C ABI in include/ifd_pn2_atk.h) -----------------------------------
// The backward pass's weight image (api.cpp build_pn2_grad_image): the layers that run dense in the backward pass, transposed as
// DgGradImage's are, all on one block of zeros as their bias.  The sparse last layers read the forward's image.
struct Pn2GradImage {
    DenseLayer fct[3];                  // fc1^T [1024][512], fc2^T [512][256], fc3^T [256][64] (40 inputs padded with zero columns)
    DenseLayer s3t;                     // sa3's middle layer^T [256][512]
    DenseLayer s3ut, s3xt;              // sa3's first layer^T: the feature columns [256][256], the coordinates [4][256] (row 3 zero)
    DenseLayer s2t, s2ut;               // sa2's middle layer^T [128][128], its first layer's feature columns^T [128][128]
    DenseLayer s1t;                     // sa1's middle layer^T [64][64]
    int total;
};
struct Pn2GradWs {                      // per-chunk scratch of launch_pn2_grad (api.cpp pn2_grad_ws)
    Pn2Ws f;                            // the forward's
    float* logits;      // [B][40]
    int32_t* pred;      // [B]
    float* loss;        // [B]
    float* d_out;       // [B][64]
    float* d2;          // [B][256]
    float* d1;          // [B][512]
    float* dg;          // [B][1024]          d loss / d global_feat
    int32_t* win3;      // [B][1024]
    float* ds3b;        // [B][128][512]
    float* ds3a;        // [B][128][256]
    float* dl2;         // [B][128][256]
    float* dx2a;        // [B][128][4]        sa3's coordinate columns transposed
    float* dx2;         // [B][128][4]        d xyz2
    float* dh;          // [B][128][64][128]  sa2's first-layer gradient per row
    float* de;          // [B][128][64][4]    d (xyz1_j - xyz2_g) per row
    float* du;          // [B][512][128]
    float* dx1a;        // [B][512][4]        d xyz1 but for sa1's own term
    float* dl1;         // [B][512][128]
    float* dd;          // [B][512][32][4]    d (x_j - xyz1_i) per row
    float* dx1;         // [B][512][4]        d xyz1
};
struct Pn2GradOut {                     // ifd_pn2_grad_out's members that the kernels write themselves; null: not wanted
    int32_t *fps1, *fps2, *ball1, *ball2;
    float *l1_feat, *l2_feat, *gfeat;
    int32_t *win1, *win2;
    uint32_t *act1, *act2, *act3;
};
hipError_t configure_pn2_grad_kernels();
hipError_t launch_pn2_grad(const float* img, const Pn2Image& I, const float* gimg, const Pn2GradImage& G, const float* pc,
                           const int32_t* n_points, const int32_t* fps_start, int B, int stride, const int32_t* target, int loss_kind,
                           float kappa, float scale, const Pn2GradWs& w, const Pn2GradOut& out, int n_classes, float* grad, hipStream_t s);

// ---- victim classifier: PointConv (pointconv.hip; C ABI in include/ifd_pc.h) ------------------------------------------
constexpr int PC_MAX_POINTS = 2048, PC_MIN_POINTS = 32;   // IFD_PC_MAX_POINTS, IFD_PC_MIN_POINTS
constexpr int PC_NP1 = 512, PC_K1 = 32;         // sa1: centroids, nearest neighbours of each
constexpr int PC_NP2 = 128, PC_K2 = 64;         // sa2; sa3 is one group of the 128
constexpr int PC_WN = 16;                       // WeightNet's outputs
constexpr int PC_EMB = 1024;                    // width of the global feature
constexpr int PC_DN_FLOATS = 97, PC_WN_FLOATS = 248;      // a DensityNet (1 -> 8 -> 8 -> 1) and a WeightNet (3 -> 8 -> 8 -> 16), biases included
// The Gaussian density's two divisors at level 0, 1, 2 (bandwidth 0.1, 0.2, 0.4): the reference's Python doubles, rounded to
// float where they meet the float tensors
__host__ __device__ constexpr float pc_two_bw2(int level) {
    return level == 0 ? (float)(2.0 * 0.1 * 0.1) : (level == 1 ? (float)(2.0 * 0.2 * 0.2) : (float)(2.0 * 0.4 * 0.4));
}
__host__ __device__ constexpr float pc_norm(int level) {
    return level == 0 ? (float)(2.5 * 0.1) : (level == 1 ? (float)(2.5 * 0.2) : (float)(2.5 * 0.4));
}
// One level inside the device image (api.cpp build_pc_image).  dn and wn: the three small layers as they come in the canonical
// vector ({weight [out][in], bias [out]} x 3).  The MLP's first layer as Pn2Image stores it: sa1's as [64][4] rows {w0, w1, w2,
// bias} (first_xyz, u unused); sa2's and sa3's as the coordinate columns [out][4] = {w0, w1, w2, 0} and the feature columns u
// with the bias.  lin: the 16 C -> C linear behind the contraction.
struct PcLevel {
    int dn, wn, first_xyz;
    DenseLayer u, mlp[2], lin;
};
struct PcImage {
    PcLevel sa[3];
    DenseLayer fc[3];
    int total;
};
struct PcWs {                           // per-chunk scratch of launch_pc (api.cpp pc_ws)
    float* xyz1;        // [B][512][3]   level-1 centroids
    float* xyz2;        // [B][128][3]
    float* xyz3;        // [B][128][3]   xyz2 minus its mean
    int32_t* fps1;      // [B][512]
    int32_t* fps2;      // [B][128]
    int32_t* knn1;      // [B][512][32]
    int32_t* knn2;      // [B][128][64]
    float* dens1;       // [B][stride]   DensityNet's output per point of the level's input
    float* dens2;       // [B][512]
    float* dens3;       // [B][128]
    float* g;           // [B][512][2048]  the contraction's output of the level at work: sa1's, then sa2's [128][4096], then sa3's [16384]
    float* l1_feat;     // [B][512][128]
    float* u2;          // [B][512][128]  b + W_f f of sa2's first layer
    float* l2_feat;     // [B][128][256]
    float* s3a;         // [B][128][256]
    float* s3b;         // [B][128][512]
    float* s3c;         // [B][128][1024]
    float* wn3;         // [B][128][16]   WeightNet of sa3's members
    float* gfeat;       // [B][1024]
    float* f1;          // [B][512]
    float* f2;          // [B][256]
};
struct PcOut {                          // where the caller wants the intermediate results; a null member stays in the scratch
    int32_t *fps1, *fps2, *knn1, *knn2;
    float *dens1, *dens2, *dens3;
    float *l1_feat, *l2_feat, *gfeat;
    int32_t* pred;
};
hipError_t configure_pc_kernels();
// bad[0] = clouds with n_points outside [32, stride]; bad[1] = clouds (of the others) with a start outside [0, n_points) / [0, 512)
hipError_t launch_pc_check(const int32_t* n_points, const int32_t* fps_start, int B, int stride, int32_t* bad, hipStream_t s);
hipError_t launch_pc(const float* img, const PcImage& I, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B,
                     int stride, const PcWs& w, const PcOut& out, float* logits, int n_classes, hipStream_t s);


// ---- PointConv input gradients (pointconv_grad.hip; C ABI in include/ifd_pc_atk.h) --------------------------------------
// The backward pass's weight image (api.cpp build_pc_grad_image): every dense layer transposed as Pn2GradImage's are, all on one
// block of zeros as their bias.
struct PcGradLevel {
    DenseLayer lint;                    // the wide linear^T [16 C][C]
    DenseLayer w3t, w2t;                // the MLP's last and middle layers^T
    DenseLayer ut, xt;                  // sa2, sa3: the first layer's feature columns^T; sa3: its coordinate columns^T [4][256] (row 3 zero)
};
struct PcGradImage {
    DenseLayer fct[3];                  // fc1^T [1024][512], fc2^T [512][256], fc3^T [256][64] (40 inputs padded with zero columns)
    PcGradLevel sa[3];
    int total;
};
struct PcGradWs {                       // per-chunk scratch of launch_pc_grad (api.cpp pc_grad_ws)
    PcWs f;                             // the forward's; f.g holds d G of the level at work
    float* logits;      // [B][40]
    int32_t* pred;      // [B]
    float* loss;        // [B]
    float* d_out;       // [B][64]
    float* d2;          // [B][256]
    float* d1;          // [B][512]
    float* dg;          // [B][1024]          d loss / d global_feat
    float* ds3c;        // [B][128][1024]     d F of sa3 under its gate
    float* ds3b;        // [B][128][512]
    float* ds3a;        // [B][128][256]
    float* dl2;         // [B][128][256]
    float* dx3m;        // [B][128][4]        sa3's coordinate columns transposed
    float* dwn3;        // [B][128][4]        sa3's WeightNet term of d (xyz2 - mean)
    float* ds3;         // [B][128]           d s of the level-2 centroids
    float* aj;          // [B][2048]          a_j of the density at work
    float* dx2a;        // [B][128][4]        d xyz2 but for sa2's own term
    float* dx2;         // [B][128][4]        d xyz2
    float* dh;          // [B][128][64][128]  sa2's first-layer gradient per row
    float* de;          // [B][128][64][4]    per row of sa2: d (xyz1_j - xyz2_g), and d s_j in the fourth place
    float* du;          // [B][512][128]
    float* dx1a;        // [B][512][4]        d xyz1 but for sa1's own term
    float* ds2;         // [B][512]           d s of the level-1 centroids
    float* dl1;         // [B][512][128]
    float* dd;          // [B][512][32][4]    per row of sa1: d (x_j - xyz1_i), and d s_j in the fourth place
    float* dx1;         // [B][512][4]        d xyz1
    float* gpre;        // [B][2048][4]       the gradient but for the level-1 density's term
    float* ds1;         // [B][2048]          d s of the cloud's points
};
struct PcGradOut {                      // ifd_pc_grad_out's members that the kernels write themselves; null: not wanted
    PcOut f;
    uint32_t *dgate1, *dgate2, *dgate3, *wgate1, *wgate2, *wgate3, *mgate1, *mgate2, *mgate3;
};
hipError_t configure_pc_grad_kernels();
hipError_t launch_pc_grad(const float* img, const PcImage& I, const float* gimg, const PcGradImage& G, const float* pc,
                          const int32_t* n_points, const int32_t* fps_start, int B, int stride, const int32_t* target, int loss_kind,
                          float kappa, float scale, const PcGradWs& w, const PcGradOut& out, int n_classes, float* grad, hipStream_t s);

}  // namespace ifd
