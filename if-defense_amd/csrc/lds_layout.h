// Layouts: where the blocks of a kernel's dynamic LDS, and of a workspace in global memory, lie.
//
// The rule: a layout is written down ONCE.  An LDS layout is a struct of byte offsets in block order whose last
// member, BYTES, is where the last block ends; the kernel takes every pointer from it (LDS_AT), the launch and the opt-in take the
// size from it (BYTES, opt_in_dynamic_lds).  A layout that depends on a run-time size is a constexpr function of that size
// returning the same kind of struct (int offsets: the kernels index LDS in 32 bits), called by the kernel and by the launcher alike.  A workspace in global memory is one function
// that takes its blocks from a Carve; run on a null base it only counts, and that count is the workspace's size.
//
// Here: the cursor, the opt-in helper, the pieces several layouts share, and the layouts of the kernels that live in .hip files.
// The persistent optimisers' layouts sit with their kernels (OptLds in optimize_kernel.h, OnetDecLds / OnetOptLds in
// onet_kernel.h, their scratch slots - OptScratch - in knn_device.h, whose code reads them).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ifd_device.h"
#include "ifd_internal.h"

namespace ifd {

constexpr size_t LDS_MAX_BYTES = 160 * 1024;         // per workgroup on gfx950

// Cursor over a workspace.  A layout is ONE function that takes its blocks from a Carve in order; on a null base the same
// function gets null pointers and only counts, and that count is the workspace's size: it cannot disagree with the pointers.
class Carve {
    char* base_;
    size_t off_ = 0;

public:
    explicit Carve(void* base) : base_(static_cast<char*>(base)) {}
    template <class T>
    T* take(size_t bytes) {
        T* r = base_ ? reinterpret_cast<T*>(base_ + off_) : nullptr;
        off_ += bytes;
        return r;
    }
    void round_up(size_t to) { off_ = (off_ + to - 1) / to * to; }
    size_t bytes() const { return off_; }
};

// The block of element type T at byte offset `at` (a multiple of sizeof(T)) of a kernel's dynamic LDS.  Macros, stepping in
// elements, because the form of the address reaches the generated code: through a function, even an inlined one, the blocks of
// one array look like separate objects to alias analysis; byte steps, or every block taken from the array's start, changed the
// register allocation of srs_kernel, prepare_kernel, large_repulsion_kernel<true> and the split / split-precision
// optimize_kernel.  Those kernels step each block from the one before it (LDS_NEXT), as their hand-written carves did - the
// steps are differences of the layout's offsets, so the layout still is the only place that states them.
#define LDS_AT(T, smem, at) (reinterpret_cast<T*>(smem) + (int)((at) / sizeof(T)))
// ... and the block at offset `to` stepped from the pointer `prev` of the block at offset `from`, in elements of `prev`
#define LDS_NEXT(T, prev, from, to) reinterpret_cast<T*>((prev) + (int)(((to) - (from)) / (int)sizeof(*(prev))))

// The opt-in to more than 64 KB of dynamic LDS: each configure_*_kernels() is a list of {kernel, its layout's size}.
struct LdsOptIn {
    const void* kernel;
    size_t bytes;
    template <class... A>
    LdsOptIn(void (*k)(A...), size_t b) : kernel(reinterpret_cast<const void*>(k)), bytes(b) {}
};
template <size_t N>
hipError_t opt_in_dynamic_lds(const LdsOptIn (&list)[N]) {
    for (const LdsOptIn& k : list) {
        const hipError_t e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.bytes);
        if (e != hipSuccess) return e;               // the first error wins
    }
    return hipSuccess;
}

// ---- shared pieces ------------------------------------------------------------------------------------------------------------
// the ConvONet decoder's parameter image: f32 (PREC 0) or the bf16 piece image (ifd_device.h)
template <int PREC>
struct DecImageLds {
    static constexpr size_t W = 0, BYTES = PREC == 0 ? (size_t)DEC_FLOATS * 4 : (size_t)BF_IMG_BYTES;
};
static_assert(DecImageLds<0>::BYTES == 67856 && DecImageLds<1>::BYTES == 94736, "the decoder images");

// A cloud of up to MAXK points behind `BASE` bytes of decoder state, as the persistent optimisers keep it: occupancy gradients G,
// points X (+ the far-away dummy X[MAXK]), their sampling coordinates PIX (ConvONet only), the fixed-point repulsion sums F
// (RepAcc, knn_device.h) and the 128-float scratch (OptScratch, knn_device.h).
template <size_t BASE, bool HAS_PIX>
struct CloudLds {
    static constexpr size_t G = BASE;                                      // f32x4 [MAXK]
    static constexpr size_t X = G + MAXK * 16;                             // f32x4 [MAXK + 1]
    static constexpr size_t PIX = X + (MAXK + 1) * 16;                     // f32x4 [MAXK] (HAS_PIX)
    static constexpr size_t F_XY = PIX + (HAS_PIX ? MAXK * 16 : 0);        // long long [MAXK]
    static constexpr size_t F_Z = F_XY + MAXK * 8;                         // int [MAXK]
    static constexpr size_t SCRATCH = F_Z + MAXK * 4;                      // float [128]
    static constexpr size_t END = SCRATCH + 128 * 4;
    static_assert(BASE % 16 == 0, "f32x4 blocks");
};

// ---- the stand-alone entry kernels of optimize.hip ----------------------------------------------------------------------------
struct RepLds {                                      // repulsion_kernel
    static constexpr size_t X = 0;                                         // f32x4 [MAXK]
    static constexpr size_t F = X + MAXK * 16;                             // long long [3 MAXK]
    static constexpr size_t SCRATCH = F + MAXK * 3 * 8;                    // float [16]
    static constexpr size_t BYTES = SCRATCH + 64;
};
struct NrmLds {                                      // normalize_kernel
    static constexpr size_t X = 0;                                         // f32x4 [MAXK]
    static constexpr size_t SCRATCH = X + MAXK * 16;                       // float [16]
    static constexpr size_t BYTES = SCRATCH + 64;
};
static_assert(RepLds::BYTES == 41024 && NrmLds::BYTES == 16448, "LDS of the stand-alone kernels");

// ---- the launch-per-step path (optimize.hip, "large" section) -----------------------------------------------------------------
constexpr int LARGE_THREADS = 1024;
// large_step_kernel<GF> / large_repulsion_kernel<GF>.  GF (K > LARGE_LDS_MAXK): only the K points are in LDS, the repulsion sums
// are in the workspace; otherwise the layout is sized for LARGE_LDS_MAXK points whatever K is.
struct LargeLdsAt { int X, F_XY, F_Z, SCRATCH, BYTES; };
template <bool GF>
__host__ __device__ constexpr LargeLdsAt large_lds_at(int K) {
    LargeLdsAt l{};
    const int n = GF ? K : LARGE_LDS_MAXK;
    l.X = 0;                                                               // f32x4 [n]
    l.F_XY = l.X + n * 16;                                                 // long long [n] (not GF)
    l.F_Z = l.F_XY + (GF ? 0 : n * 8);                                     // int [n] (not GF)
    l.SCRATCH = l.F_Z + (GF ? 0 : n * 4);                                  // float [64]
    l.BYTES = l.SCRATCH + 64 * 4;
    return l;
}
constexpr size_t large_lds_bytes(int K) { return K <= LARGE_LDS_MAXK ? large_lds_at<false>(K).BYTES : large_lds_at<true>(K).BYTES; }
static_assert(large_lds_bytes(LARGE_LDS_MAXK) == 114944 && large_lds_bytes(LARGE_MAXK) == 160256 && large_lds_bytes(LARGE_MAXK) <= LDS_MAX_BYTES,
              "LDS of the brute-force step kernels");

constexpr int LL_BLK = 128;                          // large_step_lists_kernel walks candidates in blocks of 128 consecutive indices, each with a bounding box
struct LargeListsLds {                               // large_step_lists_kernel; N = LARGE_LDS_MAXK
    static constexpr size_t N = LARGE_LDS_MAXK;
    static constexpr size_t X = 0;                                         // f32x4 [N + 1] (the dummy entry)
    static constexpr size_t F_XY = X + (N + 1) * 16;                       // long long [N]
    static constexpr size_t F_Z = F_XY + N * 8;                            // int [N]
    static constexpr size_t RL = F_Z + N * 4;                              // float [N] repulsion loss term of every point
    static constexpr size_t SCRATCH = RL + N * 4;                          // float [64]
    static constexpr size_t QN = SCRATCH + 64 * 4;                         // int: queue length (+ 3 pad)
    static constexpr size_t QD5 = QN + 16;                                 // float [N] upper bound of the queued point's squared 5th distance
    static constexpr size_t QUEUE = QD5 + N * 4;                           // uint16 [N]
    static constexpr size_t BB = QUEUE + N * 2;                            // float [N / LL_BLK][8] bounding boxes {min xyz, -, max xyz, -}
    static constexpr size_t BYTES = BB + (N / LL_BLK) * 8 * 4;
};
static_assert(LargeListsLds::BYTES == 156960 && LargeListsLds::BYTES <= LDS_MAX_BYTES, "LDS of large_step_lists_kernel");

// ---- prep.hip -----------------------------------------------------------------------------------------------------------------
constexpr int PREP_THREADS = 1024;
// PREP_MAXK (ifd_internal.h) = 10,000: the largest input cloud these kernels accept (the LDS of prepare_kernel: 16 bytes per
// point).  Up to SOR_NARROW_MAXK points sor_kernel keeps the cloud in LDS in double (32 bytes per point); above, in float
// with the doubles re-made per pair (12 bytes per point) - same values, see sor_kernel.
constexpr int SOR_NARROW_MAXK = 4096;
constexpr int PREP_SORT_MAX = 4096;      // up to this many optimised points per cloud leave prepare_kernel in Morton order (rank by counting: O(n^2))
// entries of prepare_kernel's key array: the K subset keys, or the n_opt Morton keys of the optimised points if there are more of
// them (rounded so that the doubles behind the array stay 8-byte aligned: 12 K + 4 nkey bytes in front of them)
__host__ __device__ constexpr int prep_nkey(int K, int n_opt_sorted) {
    return n_opt_sorted > K ? n_opt_sorted + ((3 * K + n_opt_sorted) & 1) : K;
}
// sor_kernel<WIDE>: 32 K + 128 B up to SOR_NARROW_MAXK points (131,200 B there, 32,896 B at 1024), 12 K + 128 B above, rounded to
// 8 (120,128 B at 10,000)
struct SorLdsAt { int SCRATCH, X, XX, BYTES; };
template <bool WIDE>
__host__ __device__ constexpr SorLdsAt sor_lds_at(int K) {
    SorLdsAt l{};
    l.SCRATCH = 0;                                                         // double [16]
    l.X = l.SCRATCH + 16 * 8;                                              // narrow: double [K][3]; wide: float [K][3]
    l.XX = l.X + (WIDE ? 12 : 24) * K;                             // narrow: double [K] = |x|^2
    l.BYTES = WIDE ? l.XX + 4 * (K & 1) : l.XX + 8 * K;
    return l;
}
constexpr size_t sor_lds_bytes(int K) { return K <= SOR_NARROW_MAXK ? sor_lds_at<false>(K).BYTES : sor_lds_at<true>(K).BYTES; }
static_assert(sor_lds_bytes(SOR_NARROW_MAXK) == 131200 && sor_lds_bytes(1024) == 32896 && sor_lds_bytes(PREP_MAXK) == 120128, "LDS of sor_kernel");
// prepare_kernel: 16 K + 256 B (160,256 B at 10,000) unless the Morton keys of the optimised points outnumber the subset keys
struct PrepLdsAt { int P, KEY, SCRATCH, BYTES; };
__host__ __device__ constexpr PrepLdsAt prep_lds_at(int K, int nkey) {
    PrepLdsAt l{};
    l.P = 0;                                                               // float [K][3] kept points, then processed
    l.KEY = l.P + 12 * K;                                          // uint32 [nkey] (prep_nkey)
    l.SCRATCH = l.KEY + 4 * nkey;                                  // float [64] (8-byte aligned: holds doubles; PrepScratch)
    l.BYTES = l.SCRATCH + 64 * 4;
    return l;
}
static_assert(prep_lds_at(PREP_MAXK, PREP_MAXK).BYTES == 160256 && prep_lds_at(PREP_MAXK, PREP_MAXK).BYTES <= LDS_MAX_BYTES, "LDS of prepare_kernel");
// slots of prepare_kernel's 64-float scratch: the block reductions' rows (doubles, ints or floats, one per wave) and the kept count
struct PrepScratch {
    static constexpr int REDUCE = 0, REDUCE_FLOATS = 2 * (PREP_THREADS / 64), S_N = 62, FLOATS = 64;
    static_assert(REDUCE + REDUCE_FLOATS <= S_N && S_N < FLOATS, "prepare_kernel's scratch slots");
};

// ---- encoder.hip: LDS by the kernel's thread count (one point per thread) -------------------------------------------------------
constexpr int NET_STRIDE = 33;          // LDS row stride of the [T][32] feature matrix (bank-conflict pad)
constexpr int ENC_NSTR = 36;            // LDS row of the MFMA kernel's [points][32] feature matrix (floats): 16-byte pieces, conflict-free writes
// encode_points_kernel: [threads][33] features + [3][threads] cell rings; the ring construction's scratch (head table int[4096] +
// unordered chains u16[3][threads] = 22,528 B at 1024 threads) aliases the feature matrix, which is first written after it
struct EncLdsAt { size_t NET, RING, BYTES; };
__host__ __device__ constexpr EncLdsAt enc_lds_at(int threads) {
    EncLdsAt l{};
    l.NET = 0;                                                             // float [threads][NET_STRIDE]
    l.RING = l.NET + (size_t)threads * NET_STRIDE * 4;                     // uint16 [3][threads] next point of my cell
    l.BYTES = l.RING + 3 * (size_t)threads * 2;
    return l;
}
struct EncMfmaLdsAt { size_t NET, RING, CELL, BYTES; };                    // encode_points_mfma_kernel
__host__ __device__ constexpr EncMfmaLdsAt enc_mfma_lds_at(int threads) {
    EncMfmaLdsAt l{};
    l.NET = 0;                                                             // float [threads][ENC_NSTR]
    l.RING = l.NET + (size_t)threads * ENC_NSTR * 4;                       // uint16 [3][threads] next point of my cell
    l.CELL = l.RING + 3 * (size_t)threads * 2;                             // uint16 [3][threads] cell of the point per plane
    l.BYTES = l.CELL + 3 * (size_t)threads * 2;
    return l;
}
static_assert(enc_lds_at(1024).BYTES == 141312 && enc_mfma_lds_at(640).BYTES == 99840 && enc_mfma_lds_at(1024).BYTES == 159744 &&
              enc_mfma_lds_at(1024).BYTES <= LDS_MAX_BYTES, "LDS of the encoder kernels");

// ---- unet.hip: wino_kernel<TG, CG> (64 KB at TG = CG = 2, 80 KB at TG = 1, CG = 4) --------------------------------------------
template <int TG, int CG>
struct WinoLds {
    static constexpr size_t V = 0;                                         // float [16 xi][16 TG tiles][16 ch]
    static constexpr size_t U = V + (size_t)16 * (16 * TG) * 16 * 4;       // float [16 xi][16 CG couts][16 ch]
    static constexpr size_t BYTES = U + (size_t)16 * (16 * CG) * 16 * 4;
};
static_assert(WinoLds<2, 2>::BYTES == 65536 && WinoLds<1, 4>::BYTES == 81920, "LDS of wino_kernel");

// ---- mesh.hip: mise_fill_z_kernel, FILLZ_LINES lines of P grid values through LDS ----------------------------------------------
constexpr int FILLZ_LINES = 64;
struct FillzLdsAt { int VAL, KNOWN, BYTES; };
__host__ __device__ constexpr FillzLdsAt fillz_lds_at(int P) {
    FillzLdsAt l{};
    l.VAL = 0;                                                             // float [FILLZ_LINES][P]
    l.KNOWN = l.VAL + FILLZ_LINES * P * 4;                         // uint8 [FILLZ_LINES][P]
    l.BYTES = l.KNOWN + FILLZ_LINES * P;
    return l;
}

// ---- punet.hip: the partial shuffles of srs_kernel (K indices, m draws) and fill_kernel (kept indices, permutation, K draws) ----
struct SrsLdsAt { int PERM, RND, BYTES; };
__host__ __device__ constexpr SrsLdsAt srs_lds_at(int K, int m) {
    SrsLdsAt l{};
    l.PERM = 0;                                                            // int [K]
    l.RND = l.PERM + K * 4;                                                // uint32 [m]
    l.BYTES = l.RND + m * 4;
    return l;
}
struct FillLdsAt { int KEPT, PERM, RND, BYTES; };
__host__ __device__ constexpr FillLdsAt fill_lds_at(int K) {
    FillLdsAt l{};
    l.KEPT = 0;                                                            // int [K] kept indices, original order
    l.PERM = l.KEPT + K * 4;                                       // int [K]
    l.RND = l.PERM + K * 4;                                                // uint32 [K]
    l.BYTES = l.RND + K * 4;
    return l;
}
static_assert(srs_lds_at(PREP_MAXK, PREP_MAXK).BYTES == 80000 && fill_lds_at(PREP_MAXK).BYTES == 120000, "LDS of the DUP-Net sampling kernels");

// ---- pointnet_drop.hip: drop_step_kernel, one cloud of up to DROP_MAX_POINTS points a workgroup of DROP_THREADS threads ----------
constexpr int DROP_THREADS = 256;
struct DropLds {
    static constexpr size_t X = 0;                                         // float [DROP_MAX_POINTS][3] the cloud
    static constexpr size_t S = X + (size_t)DROP_MAX_POINTS * 12;          // float [DROP_MAX_POINTS] saliencies
    static constexpr size_t RANK = S + (size_t)DROP_MAX_POINTS * 4;        // int [DROP_MAX_POINTS] rank in the drop order
    static constexpr size_t INDEX = RANK + (size_t)DROP_MAX_POINTS * 4;    // int [DROP_MAX_POINTS] the caller's index rows
    static constexpr size_t SCAN = INDEX + (size_t)DROP_MAX_POINTS * 4;    // int [DROP_THREADS] prefix count of the survivors
    static constexpr size_t CENTER = SCAN + (size_t)DROP_THREADS * 4;      // float [4]
    static constexpr size_t BYTES = CENTER + 16;
};
static_assert(DropLds::BYTES == 50192 && DropLds::BYTES <= 65536 && DROP_MAX_POINTS % DROP_THREADS == 0, "LDS of drop_step_kernel");

// ---- pointnet_cluster.hip: one cloud a workgroup of CLUSTER_THREADS threads ------------------------------------------------------
constexpr int CLUSTER_THREADS = 256;
struct DbscanLds {                                   // cluster_dbscan_kernel: thread i owns point i
    static constexpr size_t N = CLUSTER_DBSCAN_MAX_POINTS, WORDS = N / 32;
    static constexpr size_t X = 0;                                         // float [N][3] the cloud
    static constexpr size_t CORE = X + N * 12;                             // uint32 [WORDS] the core points, a bit each
    static constexpr size_t LAB = CORE + WORDS * 4;                        // int [2][N] labels, double-buffered
    static constexpr size_t CID = LAB + 2 * N * 4;                         // int [N] a root's cluster number
    static constexpr size_t FLAG = CID + N * 4;                            // int [4] a label changed in this round
    static constexpr size_t BYTES = FLAG + 16;
};
static_assert(DbscanLds::BYTES == 6192 &&CLUSTER_DBSCAN_MAX_POINTS == CLUSTER_THREADS, "LDS of cluster_dbscan_kernel; a point a thread");
struct ClusterStepLds {                              // cluster_step_kernel
    static constexpr size_t O = 0;                                         // float [ADD_MAX_ORI][3] the originals
    static constexpr size_t A = O + (size_t)ADD_MAX_ORI * 12;              // float [ADD_MAX_ADD][3] the added rows
    static constexpr size_t PN = A + (size_t)ADD_MAX_ADD * 12;             // float [ADD_MAX_ADD] row j: max_i n2(i, j)
    static constexpr size_t PI = PN + (size_t)ADD_MAX_ADD * 4;             // int [ADD_MAX_ADD] row j: its arg-max i
    static constexpr size_t CI = PI + (size_t)ADD_MAX_ADD * 4;             // int [ADD_MAX_ADD] cluster c: i*
    static constexpr size_t CJ = CI + (size_t)ADD_MAX_ADD * 4;             // int [ADD_MAX_ADD] cluster c: j*
    static constexpr size_t CF = CJ + (size_t)ADD_MAX_ADD * 4;             // float [ADD_MAX_ADD] cluster c: far_c
    static constexpr size_t SH = CF + (size_t)ADD_MAX_ADD * 4;             // float [CLUSTER_THREADS] the block sum's tree
    static constexpr size_t BYTES = SH + (size_t)CLUSTER_THREADS * 4;
};
static_assert(ClusterStepLds::BYTES == 58368 && ClusterStepLds::BYTES <= 65536 && ADD_MAX_ADD % CLUSTER_THREADS == 0,
              "LDS of cluster_step_kernel");

// ---- pointnet_object.hip: one cloud a workgroup of OBJECT_THREADS threads --------------------------------------------------------
constexpr int OBJECT_THREADS = 256;
struct ObjectStepLds {                               // object_step_kernel
    static constexpr size_t O = 0;                                         // float [ADD_MAX_ORI][3] the originals
    static constexpr size_t W = O + (size_t)ADD_MAX_ORI * 12;              // float [ADD_MAX_ADD][3] the forwarded world rows; behind
                                                                           //   step 5 the new shifts [num_add][3]
    static constexpr size_t G = W + (size_t)ADD_MAX_ADD * 12;              // float [ADD_MAX_ADD][4] row p: gw_x, gw_y, gw_z, ga
    static constexpr size_t CS = G + (size_t)ADD_MAX_ADD * 16;             // float [ADD_MAX_ADD][2] object c: cos, sin of its angle
    static constexpr size_t SH = CS + (size_t)ADD_MAX_ADD * 8;             // float [OBJECT_THREADS] the block sum's tree
    static constexpr size_t BYTES = SH + (size_t)OBJECT_THREADS * 4;
};
static_assert(ObjectStepLds::BYTES == 62464 && ObjectStepLds::BYTES <= 65536 && ADD_MAX_ADD % OBJECT_THREADS == 0,
              "LDS of object_step_kernel");

// ---- dgcnn.hip ----------------------------------------------------------------------------------------------------------------
// dg_knn_kernel: every thread's list of its query's k best (score, index) pairs, entry-major so that the threads of a wave hit 64
// consecutive words
struct DgKnnLdsAt { int SC, IX, PS, PI, BYTES; };
__host__ __device__ constexpr DgKnnLdsAt dg_knn_lds_at(int k) {
    DgKnnLdsAt l{};
    l.SC = 0;                                                              // float [k][DG_KNN_THREADS]
    l.IX = l.SC + k * DG_KNN_THREADS * 4;                                  // int [k][DG_KNN_THREADS]
    l.PS = l.IX + k * DG_KNN_THREADS * 4;                                  // float [DG_KNN_PEND][DG_KNN_THREADS] queued candidates
    l.PI = l.PS + DG_KNN_PEND * DG_KNN_THREADS * 4;                        // int [DG_KNN_PEND][DG_KNN_THREADS]
    l.BYTES = l.PI + DG_KNN_PEND * DG_KNN_THREADS * 4;
    return l;
}
static_assert(dg_knn_lds_at(DG_MAX_K).BYTES == 20480, "LDS of dg_knn_kernel");

// ---- victim_linear.h ----------------------------------------------------------------------------------------------------------
template <bool SUM_TOO>
struct LinearPoolLds {                               // linear_kernel's pool: the two row halves' maxima (and sums) of 64 channels
    static constexpr size_t MAX = 0;                                       // float [2][64]
    static constexpr size_t SUM = MAX + 2 * 64 * 4;                        // float [2][64], only with SUM_TOO
    static constexpr size_t BYTES = SUM + (SUM_TOO ? 2 * 64 * 4 : 0);
};
static_assert(LinearPoolLds<true>::BYTES == 1024 && LinearPoolLds<false>::BYTES == 512, "LDS of linear_kernel's pool");

// ---- pointnet2.hip ------------------------------------------------------------------------------------------------------------
template <int PPT>
struct Pn2FpsLds {                                   // pn2_fps_kernel<PPT>: a cloud of up to PPT * PN2_FPS_THREADS points
    static constexpr size_t X = 0;                                         // float [PPT * PN2_FPS_THREADS][3] the cloud
    static constexpr size_t SLOT_V = X + (size_t)PPT * PN2_FPS_THREADS * 12;   // float [2][waves] a pick's best distance per wave,
    static constexpr size_t SLOT_I = SLOT_V + 2 * (PN2_FPS_THREADS / 64) * 4;  // int [2][waves] ... and its index; by the pick's parity
    static constexpr size_t BYTES = SLOT_I + 2 * (PN2_FPS_THREADS / 64) * 4;
};
static_assert(Pn2FpsLds<8>::BYTES == 24640 && 8 * PN2_FPS_THREADS == PN2_MAX_POINTS && 2 * PN2_FPS_THREADS == PN2_NP1,
              "LDS of pn2_fps_kernel; the largest cloud and the 512 level-1 centroids");
struct Pn2Sa1Lds {                                   // pn2_sa1_kernel: a 64-row tile between its layers
    static constexpr int LD = 64 + 4;                                      // floats of a row (16-byte pieces, bank pad)
    static constexpr size_t A = 0;                                         // float [64][LD] the first layer's output
    static constexpr size_t B = A + (size_t)64 * LD * 4;                   // float [64][LD] the second's
    static constexpr size_t BYTES = B + (size_t)64 * LD * 4;
};
struct Pn2Sa2Lds {                                   // pn2_sa2_kernel
    static constexpr int LD = 128 + 4;
    static constexpr size_t A = 0;                                         // float [64][LD]
    static constexpr size_t B = A + (size_t)64 * LD * 4;                   // float [64][LD]
    static constexpr size_t RED = B + (size_t)64 * LD * 4;                 // float [2][256] the two row halves' maxima
    static constexpr size_t BYTES = RED + 2 * 256 * 4;
};
static_assert(Pn2Sa1Lds::BYTES == 34816 && Pn2Sa2Lds::BYTES == 69632 && Pn2Sa2Lds::BYTES <= LDS_MAX_BYTES, "LDS of the grouped MLPs");

// ---- pointnet2_grad.hip -------------------------------------------------------------------------------------------------------
struct Pn2Sa1BwdLds {                                // pn2_sa1_bwd_kernel: the forward's tile, then the gradients in its place
    static constexpr int LD = Pn2Sa1Lds::LD;
    static constexpr size_t A = 0;                                         // float [64][LD] h1; then d h2
    static constexpr size_t B = A + (size_t)64 * LD * 4;                   // float [64][LD] h2; then d h1 before its gate
    static constexpr size_t WIN = B + (size_t)64 * LD * 4;                 // int [2][128] a group's winner row per channel, -1: none
    static constexpr size_t DG = WIN + 2 * 128 * 4;                        // float [2][128] d l1_feat under the last layer's gate
    static constexpr size_t DD = DG + 2 * 128 * 4;                         // float [64][4] d (x_j - c_i) of the rows
    static constexpr size_t BYTES = DD + 64 * 16;
};
struct Pn2Sa2BwdLds {                                // pn2_sa2_bwd_kernel
    static constexpr int LD = Pn2Sa2Lds::LD;
    static constexpr size_t A = 0;                                         // float [64][LD] a1; then d a2
    static constexpr size_t B = A + (size_t)64 * LD * 4;                   // float [64][LD] a2; then d a1 before its gate
    static constexpr size_t WROW = B + (size_t)64 * LD * 4;                // int [2][256] the two row halves' lowest winner rows
    static constexpr size_t WIN = WROW + 2 * 256 * 4;                      // int [256] the group's winner row per channel, -1: none
    static constexpr size_t DG = WIN + 256 * 4;                            // float [256] d l2_feat under the last layer's gate
    static constexpr size_t DE = DG + 256 * 4;                             // float [64][4] d (xyz1_j - c_g) of the rows
    static constexpr size_t BYTES = DE + 64 * 16;
};
struct Pn2Sa3WinLds {                                // pn2_sa3_win_kernel
    static constexpr size_t WROW = 0;                                      // int [2 tiles][2 row halves][64] lowest winner rows
    static constexpr size_t BYTES = WROW + 4 * 64 * 4;
};
struct Pn2Sa3SparseLds {                             // pn2_sa3_sparse_kernel
    static constexpr size_t WIN = 0;                                       // int [1024]
    static constexpr size_t DG = WIN + (size_t)PN2_EMB * 4;                // float [1024] d global_feat under the last layer's gate
    static constexpr size_t BYTES = DG + (size_t)PN2_EMB * 4;
};
struct Pn2GatherLds {                                // pn2_l1_gather_kernel (8192 rows), pn2_point_gather_kernel (16384 rows)
    static constexpr size_t FPS = 0;                                       // uint16 [512] the centroid table (128 used at level 2)
    static constexpr size_t TAB = FPS + (size_t)PN2_NP1 * 2;               // uint16 [rows] the ball table of the cloud
    static constexpr size_t BYTES = TAB + (size_t)PN2_NP1 * PN2_NS1 * 2;
};
static_assert(Pn2Sa1BwdLds::BYTES == 37888 && Pn2Sa2BwdLds::BYTES == 72704 && Pn2Sa2BwdLds::BYTES <= LDS_MAX_BYTES &&
              Pn2GatherLds::BYTES == 33792 && PN2_NP1 * PN2_NS1 >= PN2_NP2 * PN2_NS2, "LDS of the PointNet++ backward kernels");

// ---- pointconv.hip ------------------------------------------------------------------------------------------------------------
struct PcDensityLds {                                // pc_density_kernel: the level's whole input cloud
    static constexpr size_t X = 0;                                         // float [PC_MAX_POINTS][3]
    static constexpr size_t BYTES = X + (size_t)PC_MAX_POINTS * 12;
};
template <int LD_>
struct PcSaLds {                                     // pc_sa1_kernel (LD 68), pc_sa2_kernel (LD 132): a 64-row tile between its layers
    static constexpr int LD = LD_;                                         // floats of a row (16-byte pieces, bank pad)
    static constexpr size_t A = 0;                                         // float [64][LD] the first layer's output; later 64 scaled channels of the last
    static constexpr size_t B = A + (size_t)64 * LD * 4;                   // float [64][LD] the second's
    static constexpr size_t WN = B + (size_t)64 * LD * 4;                  // float [64][PC_WN] WeightNet of the rows
    static constexpr size_t S = WN + (size_t)64 * PC_WN * 4;               // float [64] the rows' density scales
    static constexpr size_t BYTES = S + 64 * 4;
};
struct PcCentreLds {                                 // pc_centre_kernel
    static constexpr size_t MEAN = 0;                                      // float [3] the mean of the 128 centroids (padded to 16 bytes)
    static constexpr size_t BYTES = MEAN + 16;
};
using PcSa1Lds = PcSaLds<64 + 4>;
using PcSa2Lds = PcSaLds<128 + 4>;
static_assert(PcDensityLds::BYTES == 24576 && PcSa1Lds::BYTES == 39168 && PcSa2Lds::BYTES == 71936 && PcSa2Lds::BYTES <= LDS_MAX_BYTES,
              "LDS of the PointConv kernels");

// ---- pointconv_grad.hip ------------------------------------------------------------------------------------------------------
template <int LD_, int C_>
struct PcSaBwdLds {                                  // pc_sa1_bwd_kernel (LD 68, 2 x 128 channels), pc_sa2_bwd_kernel (LD 132, 256 channels)
    static constexpr int LD = LD_, XLD = 64 + 4;
    static constexpr size_t A = 0;                                         // float [64][LD] the first layer; then [64][XLD] 64 channels of F, then of
                                                                           // d F; at the end d a2 [64][LD]
    static constexpr size_t B = A + (size_t)64 * LD * 4;                   // float [64][LD] the second layer; then d a1 before its gate
    static constexpr size_t DG = B + (size_t)64 * LD * 4;                  // float [C][PC_WN] d G of the tile's group(s)
    static constexpr size_t WN = DG + (size_t)C_ * PC_WN * 4;              // float [64][PC_WN] WeightNet of the rows
    static constexpr size_t S = WN + (size_t)64 * PC_WN * 4;               // float [64] the rows' density scales
    static constexpr size_t DD = S + 64 * 4;                               // float [64][4] d (x_j - c_i) of the rows
    static constexpr size_t BYTES = DD + 64 * 16;
};
using PcSa1BwdLds = PcSaBwdLds<64 + 4, 2 * 128>;
using PcSa2BwdLds = PcSaBwdLds<128 + 4, 256>;
struct PcSa3BwdLds {                                 // pc_sa3_bwd_kernel
    static constexpr size_t RED = 0;                                       // float [4 waves][PC_WN + 1] the waves' sums of d Wn and d s
    static constexpr size_t BYTES = RED + 4 * (PC_WN + 1) * 4;
};
struct PcDensityBwdLds {                             // pc_density_a_kernel, pc_density_nbody_kernel: the level's input cloud and its a_j
    static constexpr size_t X = 0;                                         // float [PC_MAX_POINTS][3]
    static constexpr size_t AJ = X + (size_t)PC_MAX_POINTS * 12;           // float [PC_MAX_POINTS]
    static constexpr size_t BYTES = AJ + (size_t)PC_MAX_POINTS * 4;
};
struct PcGatherLds {                                 // pc_l1_gather_kernel (8192 rows), pc_point_gather_kernel (16384 rows)
    static constexpr size_t FPS = 0;                                       // uint16 [512] the centroid table (128 used at level 2)
    static constexpr size_t TAB = FPS + (size_t)PC_NP1 * 2;                // uint16 [rows] the neighbour table of the cloud
    static constexpr size_t BYTES = TAB + (size_t)PC_NP1 * PC_K1 * 2;
};
static_assert(PcSa1BwdLds::BYTES == 56576 && PcSa2BwdLds::BYTES == 89344 && PcSa2BwdLds::BYTES <= LDS_MAX_BYTES &&
              PcDensityBwdLds::BYTES == 32768 && PcGatherLds::BYTES == 33792 && PC_NP1 * PC_K1 >= PC_NP2 * PC_K2,
              "LDS of the PointConv backward kernels");

// ---- block_sum / block_max / block_sum_d write one value per wave into their scratch ------------------------------------------
static_assert((RepLds::BYTES - RepLds::SCRATCH) / 4 >= OPT_THREADS / 64 && (NrmLds::BYTES - NrmLds::SCRATCH) / 4 >= OPT_THREADS / 64,
              "8 waves: repulsion_kernel, normalize_kernel");
static_assert((large_lds_at<false>(0).BYTES - large_lds_at<false>(0).SCRATCH) / 4 >= LARGE_THREADS / 64 &&
              (large_lds_at<true>(0).BYTES - large_lds_at<true>(0).SCRATCH) / 4 >= LARGE_THREADS / 64 &&
              (LargeListsLds::QN - LargeListsLds::SCRATCH) / 4 >= LARGE_THREADS / 64, "16 waves: the launch-per-step kernels");
static_assert((sor_lds_at<false>(0).X - sor_lds_at<false>(0).SCRATCH) / 8 >= PREP_THREADS / 64, "16 waves of doubles: sor_kernel");

}  // namespace ifd
