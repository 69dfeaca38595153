// Shared device-side definitions for libifd (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ifd {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int RES = 64;              // plane resolution
constexpr int CH = 32;               // c_dim == hidden
constexpr int NBLK = 5;
constexpr int PLANE_FLOATS = RES * RES * CH;        // one plane, channel-last
constexpr int CLOUD_PLANE_FLOATS = 3 * PLANE_FLOATS; // 1.5 MiB / cloud

// ---- decoder parameter image (identical in global memory and in LDS) -------------
// W[15][32][34]: layer L = 3*i + j (j: 0 fc_c[i], 1 blocks[i].fc_0, 2 blocks[i].fc_1), row = out
// channel o, column = wperm(in channel c), row stride 34 floats.  The 16x16x4 MFMA operand mapping of optimize.hip
// (lane = (n, q), A[m = n][k = q]) reads the A operands with ds_read(2)_b32: 32 banks, the lanes 0-31 (q = 0, 1) and
// 32-63 (q = 2, 3) are served together.
//   forward  gather W[16 mt + n][16 mt' + 4 q + r']:  bank (2 n + wperm(4 q) + const) mod 32 - wperm(4 q) = 0, 1, 16, 17:
//            the two q of a group differ in parity, 2 n covers the even banks: conflict-free;
//   backward gather W[16 mt' + 4 q + r'][16 mt + n]:  bank (8 q + wperm(n) + const) mod 32 - wperm maps the columns
//            0-15 onto {0-7, 16-23} (16-31 onto {8-15, 24-31}), a set disjoint from itself shifted by 8: conflict-free.
// (Rounds 1-2 kept the columns of a 16-block together, wperm(c) = (c & 16) + 4 (c & 3) + ((c >> 2) & 3): the backward gather
// was then 2-way - banks 8 q + [0, 16) - and owned 72 % of the kernel's SQ_LDS_BANK_CONFLICT cycles, 488 per 32-point tile;
// scripts/pmc_lds_attrib.sh.)
constexpr int W_STRIDE = 34;
constexpr int W_LAYER = 32 * W_STRIDE;               // 1088
__host__ __device__ constexpr int wperm(int c) { return 8 * ((c >> 4) & 1) + ((c >> 2) & 1) + 2 * (c & 3) + 16 * ((c >> 3) & 1); }
constexpr int DEC_OFF_W = 0;
constexpr int DEC_OFF_BIAS = 15 * W_LAYER;           // 16320: [15][32]
constexpr int DEC_OFF_WP = DEC_OFF_BIAS + 15 * 32;   // [32][4] = {Wp[ch][0..2], bp[ch]}
constexpr int DEC_OFF_WOUT = DEC_OFF_WP + 32 * 4;    // [32]
constexpr int DEC_OFF_BOUT = DEC_OFF_WOUT + 32;      // [1] (+3 pad)
constexpr int DEC_FLOATS = DEC_OFF_BOUT + 4;         // 16964 floats = 67,856 B

// ---- decoder parameter image of the split-precision tiles (tile_bf.h) --------------------------------------
// The 15 layers as bf16 PIECES in the operand order of v_mfma_f32_16x16x32_bf16: w = w1 + w2 + w3 with w1 = bf16(w),
// w2 = bf16(w - w1), w3 = bf16(w - w1 - w2) (round to nearest even; the three pieces carry the 24 mantissa bits exactly).
//   [layer 15][piece 3][M-tile 2][lane 64][8 bf16]: lane (m = lane & 15, g = lane >> 4) of M-tile mt holds, for j = 0 ... 7,
//   W[16 mt + m][bf_chan(g, j)] - one ds_read_b128 per A operand; element j of the B operand of lane group g is the accumulator
//   register j of the layer before (channel bf_chan(g, j)): activations never leave registers, like in the f32 tile.
// The transposed operand of the backward pass comes out of the SAME image through ds_read_b64_tr_b16 (tile_bf.h load_wfrag_bf).
// Behind the layers, in f32: the biases [15][32] (fc_c's folded like in the f32 image), fc_p [32][4], fc_out [32], {fc_out's bias, 1 / B}.
__host__ __device__ constexpr int bf_chan(int g, int j) { return 16 * (j >> 2) + 4 * g + (j & 3); }
constexpr int BF_ENTRY_BYTES = 16;
constexpr int BF_PIECE_BYTES = 2 * 64 * BF_ENTRY_BYTES;           // 2048: both M-tiles of one piece
constexpr int BF_LAYER_BYTES = 3 * BF_PIECE_BYTES;               // 6144
constexpr int BF_OFF_BIAS = 15 * BF_LAYER_BYTES;                 // 92,160: float [15][32]
constexpr int BF_OFF_WP = BF_OFF_BIAS + 15 * 32 * 4;             // float [32][4]
constexpr int BF_OFF_WOUT = BF_OFF_WP + 32 * 4 * 4;              // float [32]
constexpr int BF_OFF_BOUT = BF_OFF_WOUT + 32 * 4;                // float [4]: fc_out's bias, 1 / B (written by the kernel), pad
constexpr int BF_IMG_BYTES = BF_OFF_BOUT + 16;                   // 94,736 B

constexpr int MAXK = 1024;           // points per cloud held in LDS (persistent optimiser kernel)
constexpr int LARGE_MAXK = 10000;    // largest cloud of the launch-per-step path (optimize.hip, "large" section)
constexpr int LARGE_LDS_MAXK = 4096; // ... up to here its repulsion accumulators sit in LDS, above in global memory
constexpr int OPT_THREADS = 512;     // 8 waves: 2 per SIMD (256 VGPRs each), two points per thread
constexpr float FIX_SCALE = 1099511627776.0f;        // 2^40: fixed-point scale of the neighbour scatter
constexpr float FIX_INV = 1.0f / 1099511627776.0f;

// ---- ONet-Opt variant (onet.hip): shipped config ONet/configs/onet_mn40.yaml ------------------------------
constexpr int ONET_H = 256;          // decoder hidden size (onet/models/decoder.py:89)
constexpr int ONET_C = 512;          // latent code (onet_mn40.yaml:18)
constexpr int ONET_ENC_H = 512;      // encoder hidden size (onet_mn40.yaml:16-17)
constexpr int ONET_NCBN = 11;        // bn_0 / bn_1 of 5 blocks + the final bn

// x + (x of lane ^ 16) and x + (x of lane ^ 32) through gfx950's row / half swaps (v_permlane16_swap, v_permlane32_swap:
// one vector instruction, no LDS crossbar round trip like the ds_bpermute behind __shfl_xor).  Same pairs, and the float
// sum commutes: bit-identical to the shuffle form.
// [pcsamp:tile.lane_reduce]
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float add_lane_xor16(float x) {
    const u32x2_t r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float add_lane_xor32(float x) {
    const u32x2_t r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}

struct DecConst {
    float sdiv;      // (float)(1 + padding + 10e-6)           common.py:250
    float uclamp;    // (float)(1 - 10e-6)                     common.py:255
};

// ---- Philox-4x32-10 (Salmon et al., SC'11) ---------------------------------------------------------
struct U4 { uint32_t x, y, z, w; };
__device__ __forceinline__ U4 philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return U4{c0, c1, c2, c3};
}
__device__ __forceinline__ float u01(uint32_t r) { return ((float)(r >> 8) + 0.5f) * (1.0f / 16777216.0f); }   // (0,1)


}  // namespace ifd
