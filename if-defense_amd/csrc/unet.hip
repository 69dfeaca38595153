// The encoder's shared 2-D U-Net (ConvONet/src/encoder/unet.py:225-239; depth 4, 32 start filters, concat
// merge, transpose up-conv) as hand-written implicit-GEMM convolutions on v_mfma_f32_32x32x2_f32.
//
//   layout    activations NHWC (channel-last) float32, image index = cloud * 3 + plane; weights re-packed on the
//             host to [tap][Cin][Cout].
//   block     4 waves; one wave = 32 output pixels x 32 output channels (16 accumulator VGPRs).  The block's
//             pixel tile (+1 halo) and the matching weight slab are staged through LDS in chunks of 16 input
//             channels; per chunk a wave issues 9 taps x 8 k-steps = 72 MFMAs.
//   mapping   M = pixel, N = output channel, K = (tap, input channel):  A[m = l&31][k = l>>5] from the LDS pixel
//             tile, B[k = l>>5][n = l&31] from the LDS weight slab, D: lane = channel n, register r = pixel
//             (r&3) + 8(r>>2) + 4(l>>5)  ->  NHWC stores are 128-byte rows, and the 2x2 max-pool partners of a
//             pixel live in the same lane (fused pooling epilogue).
//   fusions   bias + ReLU, max-pool (second output), channel concat of two inputs (skip connections),
//             ConvTranspose2d(k=2, s=2) as four 1x1 convolutions with a strided store.
// Results are independent of the batch size (fixed summation order) - unlike a library convolution whose
// algorithm choice depends on it - which the bitwise sharding-invariance of the whole path relies on.
#include <cstdio>
#include <type_traits>
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"

namespace ifd {

constexpr int CK = 16;               // input channels per LDS chunk
constexpr int CKP = CK + 1;          // padded pixel stride in LDS (floats)
constexpr int UNET_PW = 2;           // 32-pixel sub-tiles per wave of the 3x3 layers at 16^2 ... 64^2

struct ConvArgs {
    const float* in0;      // first input  [N][H][W][C0]
    const float* in1;      // second input [N][H][W][C1] (concat along channels) or nullptr
    const float* w;        // [taps][C0 + C1][Cout]
    const float* bias;     // [Cout]
    float* out;            // [N][H][W][Cout]           (UP: [N][2H][2W][Cout])
    float* pool_out;       // [N][H/2][W/2][Cout] or nullptr
    int H, W, C0, C1, Cout;
    int relu;
    const float* fuse_w;   // FUSE: [Cout][32] weights of a 1x1 convolution applied to this layer's output (conv_final)
    const float* fuse_b;   // FUSE: its bias [32]; a.out then receives the 1x1 convolution's result
};

// TW: tile width in pixels (16 or 8); a wave covers 32/TW rows x TW columns.  PG x CG = 4 waves:
// PG pixel groups (stacked vertically) x CG groups of 32 output channels.  KS: 3 (pad 1) or 1.
// UP: ConvTranspose2d(k=2,s=2): the block computes all 4 (dy,dx) output taps of its input pixels - four accumulators per
// wave on one A operand (the input pixel), the input tile read once (HBM-bound layers: it was read once per tap).
// FUSE (Cout = 32, CG = 1): a following conv1x1 (32 -> 32, bias, no ReLU: conv_final, unet.py:238) is applied to the
// block's activated tile before it leaves the CU - the tile goes through LDS once to turn the accumulator layout
// (lane = channel) into the A-operand layout (lane = pixel), 16 more MFMAs per wave, and the intermediate tensor is
// neither written nor read back (the stand-alone 1x1 kernel was HBM-bound: 1.4 ms at 45 TFLOP/s).  Same MFMA sequence
// over the 32 channels as the stand-alone kernel -> bit-identical results.
// PW: 32-pixel sub-tiles per wave, stacked vertically (1 or 2).  With 2 a wave runs two independent accumulator chains on
// every B operand (weight) it reads from LDS and a block covers twice the pixels per staged weight slab and per barrier.
template <int TW, int PG, int CG, int KS, bool UP, bool FUSE = false, int PW = 1>
__global__ __launch_bounds__(256, (PW == 1 && !UP) ? 5 : 3) void conv_kernel(ConvArgs a) {   // PW 1: <= 96 VGPRs, five blocks (20 waves) per CU
    constexpr int RW = 32 / TW;                 // rows per 32-pixel sub-tile
    constexpr int TH = PG * PW * RW;            // tile height
    constexpr int HALO = KS / 2;
    constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;
    constexpr int TAPS = KS * KS;
    constexpr int WT = UP ? 4 : TAPS;           // weight taps staged per chunk
    constexpr int NACC = UP ? 4 : PW;           // accumulators per wave
    static_assert(!UP || (KS == 1 && PW == 1), "transpose convolution: 1x1 input footprint, one sub-tile");
    constexpr int NCO = 32 * CG;                // output channels per block
    __shared__ __attribute__((aligned(16))) float s_in[LH * LW * CKP];
    __shared__ __attribute__((aligned(16))) float s_w[WT * CK * NCO];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pg = wave % PG, cg = wave / PG;
    const int tiles_x = a.W / TW;
    const int tile = blockIdx.x, ty = tile / tiles_x, tx = tile % tiles_x;
    const int y0 = ty * TH, x0 = tx * TW;
    const int co_blocks = a.Cout / NCO;
    const int cob = (int)blockIdx.y;
    const int co0 = cob * NCO;
    const int n = blockIdx.z;
    const int Cin = a.C0 + a.C1;

    f32x16 acc[NACC];
#pragma unroll
    for (int pw = 0; pw < NACC; ++pw)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[pw][r] = 0.f;

    const int m = lane & 31, kh = lane >> 5;
    const int py = pg * PW * RW + m / TW, px = m % TW;                 // pixel of this lane inside the tile (sub-tile 0)

    // Global -> register -> LDS staging, one chunk ahead: the loads of chunk c+1 are issued before the MFMAs of chunk c
    // and land in registers under them; after the barrier they are written to LDS.  (Round 1 staged inside the chunk,
    // one load per loop iteration with a full vmcnt(0) wait each: ~8 serial L2 round trips per chunk in front of 72 MFMAs.)
    // (Walking several tiles per block with the look-ahead running across the tile boundary was measured too: the
    // longer live ranges cost registers / occupancy, 82.5 ms against 74.0 ms for the whole U-Net.)
    constexpr int IN_N = LH * LW * (CK / 4), IN_IT = (IN_N + 255) / 256;      // f32x4 loads of the pixel tile per thread
    constexpr int W_N = WT * CK * (NCO / 4), W_IT = (W_N + 255) / 256;        // ... of the weight slab
    f32x4 rin[IN_IT], rw[W_IT];
    auto fetch = [&](int c0) {
        const float* src = c0 < a.C0 ? a.in0 : a.in1;
        const int cs = c0 < a.C0 ? a.C0 : a.C1;                        // channel count of the source tensor
        const int cl = c0 < a.C0 ? c0 : c0 - a.C0;                     // channel offset inside it
#pragma unroll
        for (int it = 0; it < IN_IT; ++it) {                           // (TH+2)x(TW+2) pixel tile, 16 channels, zero outside
            const int i = tid + it * 256;
            const int q4 = i % (CK / 4), pix = i / (CK / 4);
            const int ly = pix / LW, lx = pix % LW;
            const int gy = y0 + ly - HALO, gx = x0 + lx - HALO;
            rin[it] = f32x4{0.f, 0.f, 0.f, 0.f};
            if ((IN_N % 256 == 0 || i < IN_N) && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
                rin[it] = *reinterpret_cast<const f32x4*>(src + (((size_t)n * a.H + gy) * a.W + gx) * cs + cl + 4 * q4);
        }
#pragma unroll
        for (int it = 0; it < W_IT; ++it) {                            // weight slab [taps][16][NCO]
            const int i = tid + it * 256;
            const int q4 = i % (NCO / 4), row = i / (NCO / 4);         // row = tap * CK + k
            const int tap = row / CK, k = row % CK;
            if (W_N % 256 == 0 || i < W_N)
                rw[it] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)tap * Cin + c0 + k) * a.Cout + co0 + 4 * q4);
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < Cin; c0 += CK) {
        __syncthreads();                                               // the previous chunk's MFMAs have read the LDS tiles
#pragma unroll
        for (int it = 0; it < IN_IT; ++it) {
            const int i = tid + it * 256;
            if (IN_N % 256 == 0 || i < IN_N) {
                float* d = s_in + (i / (CK / 4)) * CKP + 4 * (i % (CK / 4));
                d[0] = rin[it].x; d[1] = rin[it].y; d[2] = rin[it].z; d[3] = rin[it].w;
            }
        }
#pragma unroll
        for (int it = 0; it < W_IT; ++it) {
            const int i = tid + it * 256;
            if (W_N % 256 == 0 || i < W_N) *reinterpret_cast<f32x4*>(s_w + 4 * i) = rw[it];
        }
        __syncthreads();
        if (c0 + CK < Cin) fetch(c0 + CK);
        if constexpr (UP) {
            const float* ap = s_in + (py * LW + px) * CKP + kh;
            const float* bp = s_w + kh * NCO + cg * 32 + m;
#pragma unroll
            for (int ks = 0; ks < CK / 2; ++ks) {
                const float av = ap[2 * ks];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[(t * CK + 2 * ks) * NCO], acc[t], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const int dy = tap / KS, dx = tap % KS;
                const float* ap = s_in + ((py + dy) * LW + px + dx) * CKP + kh;
                const float* bp = s_w + (tap * CK + kh) * NCO + cg * 32 + m;
#pragma unroll
                for (int ks = 0; ks < CK / 2; ++ks) {
                    const float b = bp[2 * ks * NCO];
#pragma unroll
                    for (int pw = 0; pw < PW; ++pw)
                        acc[pw] = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[pw * RW * LW * CKP + 2 * ks], b, acc[pw], 0, 0, 0);
                }
            }
        }
    }

    // ---- epilogue: bias, ReLU, NHWC store (lane = output channel), optional fused 2x2 max-pool --------------
    const int co = co0 + cg * 32 + m;
    const float bv = a.bias[co];
    if constexpr (FUSE) __syncthreads();                               // every wave is done with the weight slab
#pragma unroll
    for (int pw = 0; pw < NACC; ++pw) {                                // sub-tile (UP: output tap dy * 2 + dx) of this wave
        const int yw = y0 + (UP ? pg : pg * PW + pw) * RW;             // first row of this 32-pixel sub-tile
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            v[r] = acc[pw][r] + bv;
            if (a.relu) v[r] = fmaxf(v[r], 0.f);
        }
        if constexpr (FUSE) {
            static_assert(CG == 1 && !UP && TAPS * CK * NCO >= 128 * 33, "FUSE: one 32-channel group, tile fits the weight slab");
            float* T = s_w + wave * 32 * 33;                           // [32 pixels of this wave][33], wave-private rows
#pragma unroll
            for (int r = 0; r < 16; ++r) T[((r & 3) + 8 * (r >> 2) + 4 * kh) * 33 + m] = v[r];
            f32x16 acc2;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc2[r] = 0.f;
            const float* fw = a.fuse_w + kh * 32 + m;                  // B[k = channel][n = output channel]
            float bw[16];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) bw[ks] = fw[2 * ks * 32];
            const float* tp = T + m * 33 + kh;
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(tp[2 * ks], bw[ks], acc2, 0, 0, 0);
            const float fb = a.fuse_b[m];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = acc2[r] + fb;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = (r & 3) + 8 * (r >> 2) + 4 * kh;           // pixel index inside the sub-tile
            const int oy = yw + mm / TW, ox = x0 + mm % TW;
            if (UP) {
                const int uy = 2 * oy + (pw >> 1), ux = 2 * ox + (pw & 1);
                a.out[(((size_t)n * 2 * a.H + uy) * 2 * a.W + ux) * a.Cout + co] = v[r];
            } else {
                a.out[(((size_t)n * a.H + oy) * a.W + ox) * a.Cout + co] = v[r];
            }
        }
        if (!UP && a.pool_out != nullptr) {
            // partners of pixel mm: mm+1 (register r+1) and mm+TW (TW=16: r+8, TW=8: r+4) - all in this lane
            constexpr int RSTEP = TW == 16 ? 8 : 4;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool top_left = (r & 1) == 0 && ((r / RSTEP) & 1) == 0;
                if (top_left) {
                    const int mm = (r & 3) + 8 * (r >> 2) + 4 * kh;
                    const int oy = yw + mm / TW, ox = x0 + mm % TW;
                    const float pv = fmaxf(fmaxf(v[r], v[r + 1]), fmaxf(v[r + RSTEP], v[r + RSTEP + 1]));
                    a.pool_out[(((size_t)n * (a.H / 2) + oy / 2) * (a.W / 2) + ox / 2) * a.Cout + co] = pv;
                }
            }
        }
    }
}

template <int TW, int PG, int CG, int KS, bool UP, bool FUSE = false, int PW = 1>
static hipError_t launch_conv(const ConvArgs& a, int n_img, hipStream_t s) {
    constexpr int TH = PG * PW * (32 / TW);
    const dim3 grid((a.H / TH) * (a.W / TW), a.Cout / (32 * CG), n_img);
    hipLaunchKernelGGL((conv_kernel<TW, PG, CG, KS, UP, FUSE, PW>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------
// 3x3 convolutions in the Winograd F(2x2, 3x3) domain (round 4): 16 multiplications per 2x2 output tile and channel pair
// instead of 36 - 2.25x fewer MFMA cycles than the implicit GEMM above, for two cheap transforms:
//   V = B^T d B   per 4x4 input patch and input channel   (32 additions; fused into the LDS staging),
//   M_xi = V_xi U_xi, xi = 0 .. 15: sixteen independent [tiles x Cin] . [Cin x Cout] products on v_mfma_f32_16x16x4_f32,
//   Y = A^T M A   per tile and output channel             (24 additions; in registers).
// U = G g G^T is computed on the host in double (api.cpp pack_unet).  F(2x2, 3x3) has the transform matrices of 0, +-1, 1/2
// only.  End to end against a float64 U-Net the kernels' planes are 2e-7 ... 6e-7 of the image maximum away, the float32 CPU
// oracle's direct convolution 3e-7 ... 1e-6 (tests/test_gpu_encoder_f64.py holds every image to 4x the oracle's error).
//
//   block    4 waves = TG tile groups x CG channel groups; a tile group is 16 Winograd tiles = 4 x 4 tiles = 8 x 8 output
//            pixels (groups side by side), a channel group 16 output channels.  Wave (tg, cg) keeps ALL 16 xi accumulators
//            of its 16 tiles x 16 channels (64 VGPRs): the D layout puts the 16 xi of a (tile, channel) pair into one lane,
//            so the output transform, bias, ReLU and the fused 2x2 max-pool (a Winograd tile IS a pooling cell) need no
//            exchange.
//   staging  per chunk of 16 input channels: every thread transforms its share of the patches (tile, 4 channels, TG of the
//            4 xi rows) from registers (loaded one chunk ahead) and writes V as 16-byte pieces [xi][tile][16 ch]; the weight
//            slab [xi][cout][16 ch] is copied as it lies in memory.
//   operands one ds_read_b128 per operand and xi feeds FOUR MFMAs (k-slot (s, kq) <-> channel 4 kq + s on both sides); the
//            16-byte pieces of a row are XOR-swizzled by its index so that the b128 lane groups are conflict-free at a row
//            of 64 bytes (no padding: 64 KB of LDS per block at TG = CG = 2, two blocks per CU).
// Fixed summation order, independent of the batch: the bitwise sharding invariance of the path holds as before.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int wswz(int r) { return (r >> 2) & 2; }        // piece kq of row r sits at kq ^ wswz(r & 15)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t wino_rsrc(const float* p, unsigned int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000);
}

// FUSE (TG = CG = 2, Cout = 32): a following conv1x1 (32 -> 32, bias, no ReLU: conv_final, unet.py:238) is applied to the block's
// activated 16 x 8 pixel tile before it leaves the CU - the tile goes through LDS once (the V buffer is free between an item's
// last MFMA and the next transform) to turn the accumulator layout (lane = channel) into the A-operand layout (lane = pixel),
// 32 more MFMAs per wave, and the intermediate tensor is neither written nor read back.
template <int TG, int CG, bool FUSE = false>
__global__ __launch_bounds__(64 * TG * CG, TG * CG == 4 ? 2 : 1) void wino_kernel(ConvArgs a, int items_per_block, int n_items) {
    static_assert((TG == 1 || TG == 2) && (CG == 2 || CG == 4), "4 or 8 waves");
    static_assert(!FUSE || (TG == 2 && CG == 2), "FUSE: 128 pixels x 32 channels per block");
    constexpr int NT = 16 * TG, NCO = 16 * CG, NTHR = 64 * TG * CG;
    constexpr int RPT = 4 / CG;                  // xi rows per thread in the input transform: NT * 4 * (4 / RPT) = NTHR threads
    constexpr int NROW = RPT + 1;                // patch rows a thread needs for them
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    using L = WinoLds<TG, CG>;
    float* s_v = LDS_AT(float, wsm, L::V);       // [16 xi][NT tiles][16 ch]
    float* s_u = LDS_AT(float, wsm, L::U);       // [16 xi][NCO couts][16 ch]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tg = wave % TG, cg = wave / TG;
    const int regions_x = a.W / (8 * TG), regions = regions_x * (a.H / 8);
    const int co0 = (int)blockIdx.y * NCO;
    const int Cin = a.C0 + a.C1, n_chunks = Cin / 16;
    // A block walks `items_per_block` work items (image, region) and their chunks of 16 input channels as ONE sequence of steps,
    // the global loads of step k + 1 in flight under the MFMAs of step k: the memory latency is paid once per block, not once
    // per region (a 64^2 layer with 32 input channels has two chunks per region).
    const int item0 = (int)blockIdx.x * items_per_block;
    const int n_my = min(items_per_block, n_items - item0);
    const int n_steps = n_my * n_chunks;

    // ---- the thread's share of the input transform: tile ut, channel piece ucq, xi rows [RPT uh, RPT uh + RPT) ----
    // (uh is wave-uniform: 4 NT threads per value)
    const int ucq = tid & 3, ut = (tid >> 2) % NT;
    const int uh = __builtin_amdgcn_readfirstlane(tid / (4 * NT));
    const int utt = ut & 15, uty = utt >> 2, utx = utt & 3;
    const int pyo = 2 * uty - 1, pxo = 8 * (ut >> 4) + 2 * utx - 1;       // top-left of the 4x4 patch inside the region
    // patch rows: RPT 2: uh .. uh + 2; RPT 1: {0 | 1, 2 | 3}
    // Loads are buffer loads (the image is the buffer, 32-bit byte offsets, out-of-image taps get an offset beyond the buffer
    // and come back as the zero padding): no 64-bit address arithmetic, no branches around the loads.
    const int cs = a.C0;                                                   // (both sources of a concat layer have C0 channels: conv())
    const unsigned int img_bytes = (unsigned int)(a.H * a.W * cs) * 4u;
    int yrel[NROW], xrel[4], poff[NROW][4];
#pragma unroll
    for (int k = 0; k < NROW; ++k) yrel[k] = pyo + (RPT == 2 ? uh + k : (k == 0 ? (uh == 0 ? 0 : 1) : (uh == 3 ? 3 : 2)));
#pragma unroll
    for (int x = 0; x < 4; ++x) xrel[x] = pxo + x;
#pragma unroll
    for (int k = 0; k < NROW; ++k)
#pragma unroll
        for (int x = 0; x < 4; ++x) poff[k][x] = ((yrel[k] * a.W + xrel[x]) * cs + 4 * ucq) * 4;
    constexpr int W_IT = (16 * NCO * 4) / NTHR;  // f32x4 pieces of the weight slab per thread
    int woff[W_IT];
#pragma unroll
    for (int it = 0; it < W_IT; ++it) {
        const int i = tid + it * NTHR;
        const int cq = i & 3, nn = (i >> 2) % NCO, xi = i / (4 * NCO);
        woff[it] = ((xi * a.Cout + co0 + nn) * 16 + 4 * cq) * 4;
    }
    const __amdgpu_buffer_rsrc_t wrs = wino_rsrc(a.w, (unsigned int)(16 * Cin * a.Cout) * 4u);
    f32x4 rin[NROW][4], rw[W_IT];
    // (image, region row, region column, chunk) of the step being fetched, advanced by one step per call - no divisions by run-time
    // values inside the loop (each is ~25 dependent instructions in front of the loads, and the MFMAs queue up behind them)
    int f_n = item0 / regions, f_ry = ((item0 % regions) / regions_x) * 8, f_rx = ((item0 % regions) % regions_x) * 8 * TG, f_c0 = 0;
    auto fetch = [&](bool live) {                  // live = false: nothing left to fetch - every tap out of range (the loads return 0)
        const int n = live ? f_n : 0, ry = f_ry, rx = f_rx, c0 = f_c0;
        f_c0 += 16;
        if (f_c0 == Cin) {
            f_c0 = 0;
            f_rx += 8 * TG;
            if (f_rx == a.W) {
                f_rx = 0;
                f_ry += 8;
                if (f_ry == a.H) { f_ry = 0; ++f_n; }
            }
        }
        const float* src = (c0 < a.C0 ? a.in0 : a.in1) + (size_t)n * a.H * a.W * cs;
        const __amdgpu_buffer_rsrc_t irs = wino_rsrc(src, img_bytes);
        const int base = ((ry * a.W + rx) * cs + (c0 < a.C0 ? c0 : c0 - a.C0)) * 4;      // (uniform)
        bool vx[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) vx[x] = (unsigned int)(rx + xrel[x]) < (unsigned int)a.W;
#pragma unroll
        for (int k = 0; k < NROW; ++k) {
            const bool vy = live && (unsigned int)(ry + yrel[k]) < (unsigned int)a.H;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int off = (vy && vx[x]) ? base + poff[k][x] : (int)0x80000000;
                rin[k][x] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(irs, off, 0, 0));
            }
        }
        const int wbase = (c0 / 16) * 16 * a.Cout * 16 * 4;                              // [xi][Cout][16] of this chunk
#pragma unroll
        for (int it = 0; it < W_IT; ++it)
            rw[it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, woff[it], wbase, 0));
    };
    // B^T d B for the thread's xi rows: row combination first, then the columns; one 16-byte store per xi
    float* const vdst = s_v + ut * 16 + 4 * (ucq ^ wswz(utt));
    auto put_row = [&](int xr, const f32x4 (&R)[4]) {
        const f32x4 v0 = R[0] - R[2], v1 = R[1] + R[2], v2 = R[2] - R[1], v3 = R[1] - R[3];
        float* d = vdst + (size_t)(4 * xr) * NT * 16;
        *reinterpret_cast<f32x4*>(d) = v0;
        *reinterpret_cast<f32x4*>(d + NT * 16) = v1;
        *reinterpret_cast<f32x4*>(d + 2 * NT * 16) = v2;
        *reinterpret_cast<f32x4*>(d + 3 * NT * 16) = v3;
    };
    int udst[W_IT];
#pragma unroll
    for (int it = 0; it < W_IT; ++it) {
        const int i = tid + it * NTHR;
        const int cq = i & 3, nn = (i >> 2) % NCO, xi = i / (4 * NCO);
        udst[it] = (xi * NCO + nn) * 16 + 4 * (cq ^ wswz(nn & 15));
    }
    auto transform = [&]() {
        f32x4 R[4];
        if (RPT == 2) {                            // uh 0: xi rows 0, 1 from patch rows 0 1 2; uh 1: xi rows 2, 3 from patch rows 1 2 3
            if (uh == 0) {
#pragma unroll
                for (int x = 0; x < 4; ++x) R[x] = rin[0][x] - rin[2][x];
                put_row(0, R);
#pragma unroll
                for (int x = 0; x < 4; ++x) R[x] = rin[1][x] + rin[2][x];
                put_row(1, R);
            } else {
#pragma unroll
                for (int x = 0; x < 4; ++x) R[x] = rin[1][x] - rin[0][x];
                put_row(2, R);
#pragma unroll
                for (int x = 0; x < 4; ++x) R[x] = rin[0][x] - rin[2][x];
                put_row(3, R);
            }
        } else {                                   // one xi row per thread: patch rows {0, 2}, {1, 2}, {1, 2}, {1, 3}
            if (uh == 1) {
#pragma unroll
                for (int x = 0; x < 4; ++x) R[x] = rin[0][x] + rin[1][x];
            } else if (uh == 2) {
#pragma unroll
                for (int x = 0; x < 4; ++x) R[x] = rin[1][x] - rin[0][x];
            } else {
#pragma unroll
                for (int x = 0; x < 4; ++x) R[x] = rin[0][x] - rin[1][x];
            }
            put_row(uh, R);
        }
#pragma unroll
        for (int it = 0; it < W_IT; ++it) *reinterpret_cast<f32x4*>(s_u + udst[it]) = rw[it];
    };

    f32x4 acc[16];
    const int r = lane & 15, kq = lane >> 4;
    const float* ap = s_v + (tg * 16 + r) * 16 + 4 * (kq ^ wswz(r));
    const float* bp = s_u + (cg * 16 + r) * 16 + 4 * (kq ^ wswz(r));
    const int co = co0 + cg * 16 + r;
    const float bias = a.bias[co];
    const int st_lane = ((2 * kq * a.W + 8 * tg) * a.Cout + co) * 4;               // byte offset of the lane's first output pixel in its region
    const int pl_lane = ((kq * (a.W / 2) + 4 * tg) * a.Cout + co) * 4;             // ... of its first pooled pixel
    const unsigned int out_bytes = (unsigned int)(a.H * a.W * a.Cout) * 4u;

#ifdef IFD_WINO_PROF
    unsigned long long pt[6] = {0, 0, 0, 0, 0, 0}, tl = __builtin_readcyclecounter();
#define WP(i) do { const unsigned long long t_ = __builtin_readcyclecounter(); pt[i] += t_ - tl; tl = t_; } while (0)
#else
#define WP(i)
#endif
    int e_n = f_n, e_ry = f_ry, e_rx = f_rx;       // the item whose chunks are being accumulated: the block's first
    fetch(n_steps > 0);
    int chunk = 0;
#pragma unroll 1
    for (int step = 0; step < n_steps; ++step) {
        WP(5);
        __syncthreads();                                                   // the previous step's MFMAs have read the LDS tiles
        WP(0);
#ifdef IFD_WINO_PROF
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        WP(1);
#endif
        transform();
        WP(2);
        __syncthreads();
        WP(3);
        // 16 xi x 4 k-steps; the operands of xi pair p + 1 are requested before the MFMAs of pair p (two accumulator chains
        // alternate: a dependent 16x16x4 MFMA every other issue).  The first chunk of an item starts its chains from the
        // instruction's zero C operand instead of cleared registers (64 v_mov per item and wave).
        // The global loads of the NEXT step are issued between the MFMAs, two or three per eight: in front of them, as one burst,
        // the 20 x 1 KB requests of the four waves that leave the barrier together queue at the CU's one texture addresser for
        // ~1.3 k cycles, and the in-order wave does not reach its first MFMA before its last load has issued (-DIFD_WINO_PROF:
        // 3.7 k cycles for the 2 k of MFMAs even with the SIMD to itself).
        auto mfma_chunk = [&](auto first_tag) {
            constexpr bool FIRST = decltype(first_tag)::value;
            fetch(step + 1 < n_steps);
            f32x4 av[2][2], bv[2][2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                av[0][e] = *reinterpret_cast<const f32x4*>(ap + e * NT * 16);
                bv[0][e] = *reinterpret_cast<const f32x4*>(bp + e * NCO * 16);
            }
#pragma unroll
            for (int p = 0; p < 8; ++p) {
                const int cur = p & 1, nxt = cur ^ 1;
                if (p + 1 < 8) {
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        av[nxt][e] = *reinterpret_cast<const f32x4*>(ap + (2 * p + 2 + e) * NT * 16);
                        bv[nxt][e] = *reinterpret_cast<const f32x4*>(bp + (2 * p + 2 + e) * NCO * 16);
                    }
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const f32x4 c = (FIRST && s == 0) ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[2 * p + e];
                        acc[2 * p + e] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[cur][e][s], bv[cur][e][s], c, 0, 0, 0);
                    }
                // the next pair's four LDS reads first, then this pair's eight MFMAs: every read has 256 matrix cycles to land
                constexpr int NLD = NROW * 4 + W_IT;                      // global loads of a fetch, spread over the eight pairs
                constexpr int LD_LO = NLD / 8, LD_HI = NLD / 4 - LD_LO;   // 4 LD_HI + 4 LD_LO = NLD
                if (p == 0) __builtin_amdgcn_sched_group_barrier(0x002, 64, 0);      // (the loads' address arithmetic)
                if (p % 2 == 0) __builtin_amdgcn_sched_group_barrier(0x020, LD_HI, 0);
                else __builtin_amdgcn_sched_group_barrier(0x020, LD_LO, 0);
                if (p + 1 < 8) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 8, 0);
            }
        };
        // (The weight slab straight into LDS with `buffer_load ... lds` - no staging registers, half the bytes on the VGPR -> LDS
        // store path that bounds the transform phase, 172 instead of 206 VGPRs - was built and measured: 52.8 against 50.2 ms.
        // The slab can only be requested behind the first barrier of its own step and must have landed before the second: its
        // L2 round trip lies open in the transform phase, while the register-staged form fetches it a whole step ahead.)
        // (Steps of 8 input channels instead of 16 - 32 KB of LDS and 166 VGPRs per block, THREE blocks per CU, 8-byte operand
        // reads - was built and measured: 49.9 against 49.7 ms.  Occupancy is not what holds the kernel at 0.57 of the matrix
        // pipe: 2.4 other vector instructions per MFMA share that pipe, and the staging bytes per MFMA do not change.)
        // (The operands swapped - D rows = output channels, D columns = tiles, so that a lane holds four CHANNELS of one tile, the
        // epilogue is float4 arithmetic and a pixel's four channels leave as one 16-byte store instead of sixteen 4-byte stores per
        // lane - was built and measured: 50.4 against 50.2 ms, nothing; the stores are not what the kernel waits for either.  One
        // thing learnt on the way: `buffer_store_dwordx4 ... offen` with the region's base in the scalar offset operand wrote
        // wrong data in that loop, the same operands with four 4-byte stores, or with the whole offset in the VGPR, did not.)
        // (Wave priorities for the MFMA phase - also a different one for each of the two waves that share a SIMD, so that the
        // two blocks of a CU alternate instead of falling into step - measured nothing: 50.07 against 50.16 ms.)
        if (chunk == 0) mfma_chunk(std::true_type{}); else mfma_chunk(std::false_type{});
        WP(4);
        if (++chunk != n_chunks) continue;
        chunk = 0;
        // ---- Y = A^T M A, bias, ReLU, stores: lane = output channel co, kq = tile row, register = tile column ---------
        const int n = e_n, y0 = e_ry, x0 = e_rx;
        e_rx += 8 * TG;
        if (e_rx == a.W) {
            e_rx = 0;
            e_ry += 8;
            if (e_ry == a.H) { e_ry = 0; ++e_n; }
        }
        const __amdgpu_buffer_rsrc_t ors = wino_rsrc(a.out + (size_t)n * a.H * a.W * a.Cout, out_bytes);
        const __amdgpu_buffer_rsrc_t prs = wino_rsrc(a.pool_out != nullptr ? a.pool_out + (size_t)n * (a.H / 2) * (a.W / 2) * a.Cout : a.out, out_bytes / 4u);
        const int st_reg = (y0 * a.W + x0) * a.Cout * 4, pl_reg = ((y0 / 2) * (a.W / 2) + x0 / 2) * a.Cout * 4;
        constexpr int TRS = 36;                                            // row of the activated tile T[128 pixels][32 ch] (floats)
        // (Sending EVERY layer's tile through LDS - T[pixel][32 ch], then 16-byte stores of whole 128-byte pixel rows instead of 20
        // four-byte stores per lane from the accumulator layout - was measured: 53.3 against 50.0 ms for the U-Net, the two extra
        // barriers per item cost more than the address unit saves.  Only the fused layer's tile goes through LDS.)
        if (FUSE) __syncthreads();                                      // every wave's MFMAs have read s_v: it becomes T
#pragma unroll
        for (int tx = 0; tx < 4; ++tx) {
            float t0[4], t1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                t0[j] = acc[j][tx] + acc[4 + j][tx] + acc[8 + j][tx];
                t1[j] = acc[4 + j][tx] - acc[8 + j][tx] - acc[12 + j][tx];
            }
            float y[2][2];
            y[0][0] = t0[0] + t0[1] + t0[2]; y[0][1] = t0[1] - t0[2] - t0[3];
            y[1][0] = t1[0] + t1[1] + t1[2]; y[1][1] = t1[1] - t1[2] - t1[3];
#pragma unroll
            for (int ya = 0; ya < 2; ++ya)
#pragma unroll
                for (int xb = 0; xb < 2; ++xb) {
                    float v = y[ya][xb] + bias;
                    if (a.relu) v = fmaxf(v, 0.f);
                    y[ya][xb] = v;
                    if (FUSE) s_v[((2 * kq + ya) * 16 + 8 * tg + 2 * tx + xb) * TRS + cg * 16 + r] = v;
                    else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ors, st_lane, st_reg + ((ya * a.W + 2 * tx + xb) * a.Cout) * 4, 0);
                }
            if (a.pool_out != nullptr) {
                const float pv = fmaxf(fmaxf(y[0][0], y[0][1]), fmaxf(y[1][0], y[1][1]));
                if (FUSE) s_v[(128 + kq * 8 + 4 * tg + tx) * TRS + cg * 16 + r] = pv;
                else __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(pv), prs, pl_lane, pl_reg + tx * a.Cout * 4, 0);
            }
        }
        if constexpr (FUSE) {
            // out[px][co2] = fuse_b[co2] + sum_c T[px][c] fuse_w[c][co2]: wave w takes the pixel rows 2 w, 2 w + 1 of the tile (16
            // pixels each) and both groups of 16 output channels; k-slot (s, kq) <-> channel 8 kq + s on both operands
            __syncthreads();
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                float bw[8];
#pragma unroll
                for (int k8 = 0; k8 < 8; ++k8) bw[k8] = a.fuse_w[(8 * kq + k8) * 32 + 16 * c2 + r];
                const float fb = a.fuse_b[16 * c2 + r];
#pragma unroll
                for (int pg = 0; pg < 2; ++pg) {
                    const int ly = 2 * wave + pg;
                    const float* tp = s_v + (ly * 16 + r) * TRS + 8 * kq;
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(tp), a1 = *reinterpret_cast<const f32x4*>(tp + 4);
                    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k8 = 0; k8 < 8; ++k8) o = __builtin_amdgcn_mfma_f32_16x16x4f32(k8 < 4 ? a0[k8] : a1[k8 - 4], bw[k8], o, 0, 0, 0);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr)       // D: lane (co2 = 16 c2 + r, kq), register rr <-> pixel column 4 kq + rr of row ly
                        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o[rr] + fb), ors, (16 * c2 + r) * 4,
                                                              st_reg + ((ly * a.W + 4 * kq + rr) * a.Cout) * 4, 0);
                }
            }
        }
    }
#ifdef IFD_WINO_PROF
    if (!FUSE && lane == 0 && a.fuse_b != nullptr) {
        unsigned long long* o = reinterpret_cast<unsigned long long*>(const_cast<float*>(a.fuse_b));
        for (int i = 0; i < 6; ++i) atomicAdd(o + i, pt[i]);
        atomicAdd(o + 6, (unsigned long long)n_steps);
    }
#endif
}

constexpr int WINO_ITEMS = 16;       // (image, region) work items per block
template <int TG, int CG, bool FUSE = false>
static hipError_t launch_wino(const ConvArgs& a, int n_img, hipStream_t s) {
    constexpr size_t LDS = WinoLds<TG, CG>::BYTES;
    const int n_items = n_img * (a.H / 8) * (a.W / (8 * TG));
    // up to WINO_ITEMS items per block, fewer where that would leave less than ~12 blocks per block slot of the chip
    const int gy = a.Cout / (16 * CG);
    const int per = max(1, min(WINO_ITEMS, (int)((long long)n_items * gy / 6144)));
    const dim3 grid((n_items + per - 1) / per, gy, 1);
#ifdef IFD_WINO_PROF
    if (FUSE) {
        hipLaunchKernelGGL((wino_kernel<TG, CG, FUSE>), grid, dim3(64 * TG * CG), LDS, s, a, per, n_items);
        return hipGetLastError();
    }
    static unsigned long long* dbg = nullptr;
    if (dbg == nullptr) (void)hipMalloc(reinterpret_cast<void**>(&dbg), 64);
    (void)hipMemsetAsync(dbg, 0, 64, s);
    ConvArgs b = a;
    b.fuse_b = reinterpret_cast<const float*>(dbg);
    hipLaunchKernelGGL((wino_kernel<TG, CG, FUSE>), grid, dim3(64 * TG * CG), LDS, s, b, per, n_items);
    unsigned long long h[8];
    (void)hipMemcpyAsync(h, dbg, 56, hipMemcpyDeviceToHost, s);
    (void)hipStreamSynchronize(s);
    const double ws = (double)h[6];     // wave-steps
    fprintf(stderr, "wino<%d,%d> HW %d Cin %d Cout %d: per wave-step cycles: barrier1 %.0f | vmcnt %.0f | transform %.0f | barrier2 %.0f | fetch+mfma %.0f | tail(epilogue,loop) %.0f\n",
            TG, CG, a.H, a.C0 + a.C1, a.Cout, h[0] / ws, h[1] / ws, h[2] / ws, h[3] / ws, h[4] / ws, h[5] / ws);
    return hipGetLastError();
#else
    hipLaunchKernelGGL((wino_kernel<TG, CG, FUSE>), grid, dim3(64 * TG * CG), LDS, s, a, per, n_items);
    return hipGetLastError();
#endif
}

hipError_t configure_unet_kernels() {
    return opt_in_dynamic_lds({{wino_kernel<2, 2>, WinoLds<2, 2>::BYTES}, {wino_kernel<1, 4>, WinoLds<1, 4>::BYTES},
                               {wino_kernel<2, 2, true>, WinoLds<2, 2>::BYTES}});
}

// env IFD_UNET_DIRECT=1: every 3x3 layer on the implicit-GEMM kernel (A/B and validation of the Winograd path)
static bool unet_direct() {
    static const bool d = [] { const char* e = getenv("IFD_UNET_DIRECT"); return e != nullptr && e[0] == '1'; }();
    return d;
}

// conv3x3 / conv1x1 / transpose-conv dispatch on the image size (64/32/16 -> 8x16 pixel tiles, 8 -> 8x8 tiles)
static hipError_t conv(const float* in0, int C0, const float* in1, int C1, const float* w, const float* b, float* out,
                       float* pool_out, int HW, int Cout, int ks, bool up, bool relu, int n_img, hipStream_t s,
                       const float* fuse_w = nullptr, const float* fuse_b = nullptr, const float* wu = nullptr) {
    ConvArgs a{in0, in1, w, b, out, pool_out, HW, HW, C0, C1, Cout, relu ? 1 : 0, fuse_w, fuse_b};
    if (wu != nullptr && ks == 3 && !up && (C1 == 0 || C1 == C0) && !unet_direct()) {     // Winograd-domain weights given: F(2x2, 3x3)
        a.w = wu;
        if (fuse_w != nullptr) {
            if (HW < 16 || Cout != 32) return hipErrorInvalidValue;
            return launch_wino<2, 2, true>(a, n_img, s);
        }
        // (8-wave blocks of 32 tiles x 64 channels - the input transform shared by twice the MFMAs - measured 51.3 against 50.1 ms)
        if (HW >= 16) return launch_wino<2, 2>(a, n_img, s);
        return launch_wino<1, 4>(a, n_img, s);
    }
    if (fuse_w != nullptr) {
        if (HW < 16 || ks != 3 || up || Cout != 32) return hipErrorInvalidValue;
        return launch_conv<16, 4, 1, 3, false, true, UNET_PW>(a, n_img, s);
    }
    if (HW >= 16) {
        if (up) return launch_conv<16, 4, 1, 1, true>(a, n_img, s);
        if (ks == 3) return launch_conv<16, 4, 1, 3, false, false, UNET_PW>(a, n_img, s);
        return launch_conv<16, 4, 1, 1, false>(a, n_img, s);
    }
    if (up) return launch_conv<8, 2, 2, 1, true>(a, n_img, s);
    if (ks == 3) return launch_conv<8, 2, 2, 3, false>(a, n_img, s);
    return launch_conv<8, 2, 2, 1, false>(a, n_img, s);
}

size_t unet_workspace_floats(int n_img) {
    // d0a d0 u2up u2a u2 (64^2x32) | d1a d1 u1up u1a u1 (32^2x64) | p1 (32^2x32) | d2a d2 u0up u0a u0 (16^2x128)
    // | p2 (16^2x64) | d3a d3 (8^2x256) | p3 (8^2x128)
    return (size_t)n_img * (5 * 131072 + 5 * 65536 + 32768 + 5 * 32768 + 16384 + 2 * 16384 + 8192);
}

// x [n_img][64][64][32] -> out [n_img][64][64][32]; wd = device copy of the re-packed U-Net weights.
hipError_t launch_unet(const UNetWeights& W, const float* x, float* out, float* ws, int n_img, hipStream_t s) {
    size_t o = 0;
    auto take = [&](size_t per_img) { float* p = ws + o; o += per_img * (size_t)n_img; return p; };
    float *d0a = take(131072), *d0 = take(131072), *u2up = take(131072), *u2a = take(131072), *u2 = take(131072);
    float *d1a = take(65536), *d1 = take(65536), *u1up = take(65536), *u1a = take(65536), *u1 = take(65536);
    float* p1 = take(32768);
    float *d2a = take(32768), *d2 = take(32768), *u0up = take(32768), *u0a = take(32768), *u0 = take(32768);
    float* p2 = take(16384);
    float *d3a = take(16384), *d3 = take(16384);
    float* p3 = take(8192);
    (void)u2;                                // conv_final is fused into the layer that produced u2; the slot stays in the layout
    hipError_t e;
#define IFD_TRY(x) do { e = (x); if (e != hipSuccess) return e; } while (0)
    // encoder pathway (DownConv, unet.py:66-72): conv-relu, conv-relu, pool (not on the last level)
    IFD_TRY(conv(x, 32, nullptr, 0, W.down_w[0][0], W.down_b[0][0], d0a, nullptr, 64, 32, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[0][0]));
    IFD_TRY(conv(d0a, 32, nullptr, 0, W.down_w[0][1], W.down_b[0][1], d0, p1, 64, 32, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[0][1]));
    IFD_TRY(conv(p1, 32, nullptr, 0, W.down_w[1][0], W.down_b[1][0], d1a, nullptr, 32, 64, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[1][0]));
    IFD_TRY(conv(d1a, 64, nullptr, 0, W.down_w[1][1], W.down_b[1][1], d1, p2, 32, 64, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[1][1]));
    IFD_TRY(conv(p2, 64, nullptr, 0, W.down_w[2][0], W.down_b[2][0], d2a, nullptr, 16, 128, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[2][0]));
    IFD_TRY(conv(d2a, 128, nullptr, 0, W.down_w[2][1], W.down_b[2][1], d2, p3, 16, 128, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[2][1]));
    IFD_TRY(conv(p3, 128, nullptr, 0, W.down_w[3][0], W.down_b[3][0], d3a, nullptr, 8, 256, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[3][0]));
    IFD_TRY(conv(d3a, 256, nullptr, 0, W.down_w[3][1], W.down_b[3][1], d3, nullptr, 8, 256, 3, false, true, n_img, s, nullptr, nullptr, W.down_u[3][1]));
    // decoder pathway (UpConv, unet.py:101-114): upconv, cat(up, skip), conv-relu, conv-relu
    IFD_TRY(conv(d3, 256, nullptr, 0, W.up_t_w[0], W.up_t_b[0], u0up, nullptr, 8, 128, 1, true, false, n_img, s));
    IFD_TRY(conv(u0up, 128, d2, 128, W.up_w[0][0], W.up_b[0][0], u0a, nullptr, 16, 128, 3, false, true, n_img, s, nullptr, nullptr, W.up_u[0][0]));
    IFD_TRY(conv(u0a, 128, nullptr, 0, W.up_w[0][1], W.up_b[0][1], u0, nullptr, 16, 128, 3, false, true, n_img, s, nullptr, nullptr, W.up_u[0][1]));
    IFD_TRY(conv(u0, 128, nullptr, 0, W.up_t_w[1], W.up_t_b[1], u1up, nullptr, 16, 64, 1, true, false, n_img, s));
    IFD_TRY(conv(u1up, 64, d1, 64, W.up_w[1][0], W.up_b[1][0], u1a, nullptr, 32, 64, 3, false, true, n_img, s, nullptr, nullptr, W.up_u[1][0]));
    IFD_TRY(conv(u1a, 64, nullptr, 0, W.up_w[1][1], W.up_b[1][1], u1, nullptr, 32, 64, 3, false, true, n_img, s, nullptr, nullptr, W.up_u[1][1]));
    IFD_TRY(conv(u1, 64, nullptr, 0, W.up_t_w[2], W.up_t_b[2], u2up, nullptr, 32, 32, 1, true, false, n_img, s));
    IFD_TRY(conv(u2up, 32, d0, 32, W.up_w[2][0], W.up_b[2][0], u2a, nullptr, 64, 32, 3, false, true, n_img, s, nullptr, nullptr, W.up_u[2][0]));
    // last conv-relu with conv_final (conv1x1, unet.py:238) fused into its epilogue
    IFD_TRY(conv(u2a, 32, nullptr, 0, W.up_w[2][1], W.up_b[2][1], out, nullptr, 64, 32, 3, false, true, n_img, s, W.fin_w,
                 W.fin_b, W.up_u[2][1]));
#undef IFD_TRY
    return hipSuccess;
}

}  // namespace ifd
