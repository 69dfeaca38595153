// Input gradients of the PointNet++ victim (include/ifd_pn2_atk.h): d loss / d points for the two adversarial losses of
// include/ifd_atk.h, with the four index tables (fps1, fps2, ball1, ball2) held fixed: farthest_point_sample and query_ball_point
// return indices, which carry no gradient in the reference either.  The centroids' coordinates do carry gradient.
// The forward half is launch_pn2 itself (pointnet2.hip), so logits, pred, the tables and the features are its bits; it leaves
// xyz1, xyz2, the tables, l1_feat, u2, l2_feat, s3a, s3b, the tiles' maxima, gfeat, f1 and f2 behind.  The backward half, in launch order:
//
//   launch_head_backward      (victim_linear.h) loss_grad_kernel: logits, target -> loss, scale * d loss / d logits; the three FC
//                             layers transposed (Pn2GradImage.fct, zero bias, no activation), a cloud a row; act_gate_kernel between
//                             them: times ReLU's derivative at the saved activation, 1 where it is > 0, else 0
//   pn2_sa3_win_kernel        sa3's last layer again per 64-row tile, by linear_kernel<Pn2Sa3Last>'s own instruction sequence: per
//                             channel the lowest row whose activation equals the saved global feature
//   pn2_sa3_sparse_kernel     the last layer transposed in its sparse form: a workgroup a row g, one chain over the channels c it
//                             won, ascending: d s3b[g][k] += d gfeat[c] W[c][k], then the gate s3b > 0
//   linear_kernel<Pn2Linear>  512 -> 256 transposed, act_gate_kernel (s3a), 256 -> 256 transposed (d l2_feat) and 256 -> 3 (xyz2's
//                             columns of sa3's first layer)
//   pn2_sa2_bwd_kernel        a workgroup a group of 64 rows: the forward's tile again (same instruction sequence), winners of the
//                             256 channels, the last layer transposed in its sparse form (one row per channel), the 128 x 128 middle
//                             layer transposed on v_mfma_f32_16x16x4_f32, the first layer's gate; per row d U and d e = Wxyz^T d a1
//                             go to global memory, d xyz2[g] = -sum_s d e + sa3's term
//   pn2_l1_gather_kernel      rows -> level-1 points without atomics: a wave owns a level-1 point j and walks the cloud's 8192 rows in
//                             ascending order, adding the rows whose ball2 entry is j; then the groups g with fps2[g] == j, ascending
//   linear_kernel<Pn2Linear>  d l1_feat = Wf^T d U
//   pn2_sa1_bwd_kernel        a workgroup two groups of 32 rows, as pn2_sa2_bwd_kernel: d d = W1^T d h1 per row to global memory,
//                             d xyz1[i] = -sum_s d d + what pn2_l1_gather_kernel left
//   pn2_point_gather_kernel   rows -> cloud points: a thread owns a point and walks the cloud's 16384 rows in ascending order, then
//                             the 512 centroids in ascending order; writes grad, zeros in the rows beyond the cloud.
// Every sum has a fixed order, nothing here uses float atomics, and every kernel works on one cloud's rows alone.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "victim_linear.h"

namespace ifd {

namespace {

constexpr int P2G_NONE = 0x7fffffff;
constexpr int PN2_ROWS1 = PN2_NP1 * PN2_NS1, PN2_ROWS2 = PN2_NP2 * PN2_NS2;
static_assert(PN2_NP1 == 512 && PN2_NS1 == 32 && PN2_NP2 == 128 && PN2_NS2 == 64 && PN2_EMB == 1024 && LINEAR_TILE == 64,
              "the tilings of the backward kernels");

// act3 [B][128][24]: word w < 8 of a row: s3a's channels 32 w .. 32 w + 31; w >= 8: s3b's channels 32 (w - 8) ..
__global__ __launch_bounds__(256) void pn2_act3_kernel(const float* __restrict__ s3a, const float* __restrict__ s3b, int B,
                                                       uint32_t* __restrict__ act3) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * PN2_NP2 * 24) return;
    const int w = i % 24;
    const size_t row = (size_t)(i / 24);
    const float* x = w < 8 ? s3a + row * 256 + 32 * w : s3b + row * 512 + 32 * (w - 8);
    uint32_t bits = 0;
    for (int e = 0; e < 32; ++e)
        if (x[e] > 0.f) bits |= 1u << e;
    act3[i] = bits;
}

// W [1024][512], bias [1024]: sa3's last layer.  win3 [B][1024]: the lowest row g of s3b [B][128][512] with
// relu(bias + W s3b[g]) == gfeat, -1 where no row has it (which would be a bug: the sums are linear_kernel<Pn2Sa3Last>'s).
__global__ __launch_bounds__(256) void pn2_sa3_win_kernel(const float* __restrict__ W, const float* __restrict__ bias,
                                                          const float* __restrict__ s3b, const float* __restrict__ gfeat,
                                                          int32_t* __restrict__ win3) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[Pn2Sa3WinLds::BYTES];
    int* wrow = LDS_AT(int, smem, Pn2Sa3WinLds::WROW);
    const int b = blockIdx.y;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int obase = blockIdx.x * 64 + 32 * (wv >> 1);
    const float* Gf = gfeat + (size_t)b * PN2_EMB;
#pragma unroll 1
    for (int tile = 0; tile < PN2_NP2 / LINEAR_TILE; ++tile) {
        const int rbase = tile * LINEAR_TILE + 32 * (wv & 1);
        const float* xr[2];
        const float* wr[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            xr[t] = s3b + ((size_t)b * PN2_NP2 + rbase + 16 * t + p) * 512 + 4 * q;
            wr[t] = W + (size_t)(obase + 16 * t + p) * 512 + 4 * q;
        }
        f32x4 sum[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + obase + 16 * m + 4 * q);
#pragma unroll
            for (int t = 0; t < 2; ++t) sum[t][m] = bv;
        }
        for (int g = 0; g < 512; g += 64) linear_block64(xr, wr, g, sum);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const f32x4 gm = *reinterpret_cast<const f32x4*>(Gf + obase + 16 * m + 4 * q);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int cand = P2G_NONE;
#pragma unroll
                for (int t = 1; t >= 0; --t)
                    if (fmaxf(sum[t][m][r], 0.f) == gm[r]) cand = rbase + 16 * t + p;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) cand = min(cand, __shfl_xor(cand, d));
                if (p == 0) wrow[(tile * 2 + (wv & 1)) * 64 + 32 * (wv >> 1) + 16 * m + 4 * q + r] = cand;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int c = threadIdx.x;
        const int w = min(min(wrow[c], wrow[64 + c]), min(wrow[128 + c], wrow[192 + c]));
        win3[(size_t)b * PN2_EMB + blockIdx.x * 64 + c] = w == P2G_NONE ? -1 : w;
    }
}

// A workgroup a row g of a cloud: d s3b[g][k] = (s3b[g][k] > 0) * sum over the channels c with win3[c] == g and gfeat[c] > 0,
// ascending, of dg[c] W[c][k]; one fused chain per k.  W [1024][512].
__global__ __launch_bounds__(256) void pn2_sa3_sparse_kernel(const float* __restrict__ W, const int32_t* __restrict__ win3,
                                                             const float* __restrict__ gfeat, const float* __restrict__ dg,
                                                             const float* __restrict__ s3b, float* __restrict__ ds3b) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[Pn2Sa3SparseLds::BYTES];
    int* win = LDS_AT(int, smem, Pn2Sa3SparseLds::WIN);
    float* dgs = LDS_AT(float, smem, Pn2Sa3SparseLds::DG);
    const int g = blockIdx.x, b = blockIdx.y;
    for (int c = threadIdx.x; c < PN2_EMB; c += 256) {
        win[c] = win3[(size_t)b * PN2_EMB + c];
        dgs[c] = gfeat[(size_t)b * PN2_EMB + c] > 0.f ? dg[(size_t)b * PN2_EMB + c] : 0.f;
    }
    __syncthreads();
    float a0 = 0.f, a1 = 0.f;
    for (int c = 0; c < PN2_EMB; ++c) {
        if (win[c] != g) continue;                                     // the whole workgroup
        const float d = dgs[c];
        a0 = fmaf(d, W[(size_t)c * 512 + threadIdx.x], a0);
        a1 = fmaf(d, W[(size_t)c * 512 + 256 + threadIdx.x], a1);
    }
    const size_t at = ((size_t)b * PN2_NP2 + g) * 512 + threadIdx.x;
    ds3b[at] = s3b[at] > 0.f ? a0 : 0.f;
    ds3b[at + 256] = s3b[at + 256] > 0.f ? a1 : 0.f;
}

// the lowest of the wave's rows 16 t + p (+ base) whose v equals the saved maximum, for channel (m, r) of every lane's q
__device__ __forceinline__ int tile_winner(const f32x4 (&v)[2][2], int m, int r, float saved, int base, int p) {
    int cand = P2G_NONE;
#pragma unroll
    for (int t = 1; t >= 0; --t)
        if (v[t][m][r] == saved) cand = base + 16 * t + p;
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) cand = min(cand, __shfl_xor(cand, d));
    return cand;
}

// sa2 backward.  The forward's arguments (pn2_sa2_kernel), W2T [128][128] the middle layer transposed, l2 the saved l2_feat,
// dl2 its gradient, dx2a [B][128][4] sa3's term of d xyz2.  Out: dh [B][128][64][128], de [B][128][64][4], dx2 [B][128][4];
// win2 [B][128][256] and act2 [B][128][64][8] where wanted.
__global__ __launch_bounds__(256, 2) void pn2_sa2_bwd_kernel(const float* __restrict__ U, const float* __restrict__ wx, const float* __restrict__ W2,
                                                          const float* __restrict__ b2, const float* __restrict__ W3, const float* __restrict__ b3,
                                                          const float* __restrict__ W2T, const int32_t* __restrict__ ball,
                                                          const float* __restrict__ xyz1, const float* __restrict__ cen,
                                                          const float* __restrict__ l2, const float* __restrict__ dl2,
                                                          const float* __restrict__ dx2a, float* __restrict__ dh, float* __restrict__ de,
                                                          float* __restrict__ dx2, int32_t* __restrict__ win2, uint32_t* __restrict__ act2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using L = Pn2Sa2BwdLds;
    float* A = LDS_AT(float, smem, L::A);
    float* Bm = LDS_AT(float, smem, L::B);
    int* wrow = LDS_AT(int, smem, L::WROW);
    int* win = LDS_AT(int, smem, L::WIN);
    float* dgs = LDS_AT(float, smem, L::DG);
    float* des = LDS_AT(float, smem, L::DE);
    constexpr int LD = L::LD;
    const int b = blockIdx.y, g = blockIdx.x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int row = threadIdx.x >> 2, o0 = (threadIdx.x & 3) * 32;       // the elementwise passes: a thread = a row x 32 channels
    const size_t grow = ((size_t)b * PN2_NP2 + g) * PN2_NS2 + row;      // this row among the cloud's
    uint32_t gate1 = 0;                                                // a1 > 0 of the thread's 32 channels
    {                                                                  // pn2_sa2_kernel's first layer
        const int j = min(max(ball[grow], 0), PN2_NP1 - 1);
        const float* x = xyz1 + ((size_t)b * PN2_NP1 + j) * 3;
        const float* c = cen + ((size_t)b * PN2_NP2 + g) * 3;
        const float dx = x[0] - c[0], dy = x[1] - c[1], dz = x[2] - c[2];
        const float* u = U + ((size_t)b * PN2_NP1 + j) * 128 + o0;
#pragma unroll
        for (int e = 0; e < 32; e += 4) {
            f32x4 v = *reinterpret_cast<const f32x4*>(u + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(wx + (o0 + e + r) * 4);
                v[r] = fmaxf(fmaf(w[2], dz, fmaf(w[1], dy, fmaf(w[0], dx, v[r]))), 0.f);
                if (v[r] > 0.f) gate1 |= 1u << (e + r);
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = v;
        }
    }
    if (act2) act2[grow * 8 + (threadIdx.x & 3)] = gate1;
    __syncthreads();
    f32x4 v[2][2];
#pragma unroll
    for (int ob = 0; ob < 128; ob += 64) {
        const int obase = ob + 32 * (wv >> 1);
        tile_layer<128, LD>(A, W2, b2, obase, wv, q, p, v);
        tile_store<LD>(Bm, obase, wv, q, p, v);
    }
    __syncthreads();
    // the last layer again: per channel the lowest row that holds the saved maximum
    const float* Lg = l2 + ((size_t)b * PN2_NP2 + g) * 256;
#pragma unroll 1
    for (int ob = 0; ob < 256; ob += 64) {
        const int obase = ob + 32 * (wv >> 1);
        tile_layer<128, LD>(Bm, W3, b3, obase, wv, q, p, v);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const f32x4 sv = *reinterpret_cast<const f32x4*>(Lg + obase + 16 * m + 4 * q);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int cand = tile_winner(v, m, r, sv[r], 32 * (wv & 1), p);
                if (p == 0) wrow[(wv & 1) * 256 + obase + 16 * m + 4 * q + r] = cand;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 32; e += 4) *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = f32x4{0.f, 0.f, 0.f, 0.f};   // a1 is in gate1 now
    __syncthreads();
    {
        const int c = threadIdx.x;
        const int w = min(wrow[c], wrow[256 + c]);
        win[c] = w == P2G_NONE ? -1 : w;
        dgs[c] = Lg[c] > 0.f ? dl2[((size_t)b * PN2_NP2 + g) * 256 + c] : 0.f;
        if (win2) win2[((size_t)b * PN2_NP2 + g) * 256 + c] = win[c];
    }
    __syncthreads();
    // d a2[s][k] = sum over the channels c won by row s, ascending, of dgs[c] W3[c][k]: the even rows by waves 0 and 1, the odd by 2 and 3
    {
        const int k = threadIdx.x & 127, par = threadIdx.x >> 7;
#pragma unroll 4
        for (int c = 0; c < 256; ++c) {
            const float w = W3[c * 128 + k];
            const int s = win[c];
            if (s >= 0 && (s & 1) == par) A[s * LD + k] = fmaf(dgs[c], w, A[s * LD + k]);
        }
    }
    __syncthreads();
    {                                                                  // the middle layer's gate
        uint32_t gate2 = 0;
#pragma unroll
        for (int e = 0; e < 32; e += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(Bm + row * LD + o0 + e);
            f32x4 d = *reinterpret_cast<const f32x4*>(A + row * LD + o0 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (a[r] > 0.f) gate2 |= 1u << (e + r);
                else d[r] = 0.f;
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = d;
        }
        if (act2) act2[grow * 8 + 4 + (threadIdx.x & 3)] = gate2;
    }
    __syncthreads();
#pragma unroll
    for (int ob = 0; ob < 128; ob += 64) tile_layer_t<128, LD>(A, W2T, Bm, ob + 32 * (wv >> 1), wv, q, p);
    __syncthreads();
    {                                                                  // the first layer's gate; d U of the row; d e = Wxyz^T d a1
        float px = 0.f, py = 0.f, pz = 0.f;
        float* H = dh + grow * 128 + o0;
#pragma unroll
        for (int e = 0; e < 32; e += 4) {
            f32x4 d = *reinterpret_cast<const f32x4*>(Bm + row * LD + o0 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!((gate1 >> (e + r)) & 1u)) d[r] = 0.f;
                const f32x4 w = *reinterpret_cast<const f32x4*>(wx + (o0 + e + r) * 4);
                px = fmaf(d[r], w[0], px);
                py = fmaf(d[r], w[1], py);
                pz = fmaf(d[r], w[2], pz);
            }
            *reinterpret_cast<f32x4*>(H + e) = d;
        }
        // the four 32-channel chains of a row: (c0 + c1) + (c2 + c3), every lane the same tree
        px += __shfl_xor(px, 1); py += __shfl_xor(py, 1); pz += __shfl_xor(pz, 1);
        px += __shfl_xor(px, 2); py += __shfl_xor(py, 2); pz += __shfl_xor(pz, 2);
        if ((threadIdx.x & 3) == 0) {
            const f32x4 d = f32x4{px, py, pz, 0.f};
            *reinterpret_cast<f32x4*>(de + grow * 4) = d;
            *reinterpret_cast<f32x4*>(des + row * 4) = d;
        }
    }
    __syncthreads();
    if (threadIdx.x < 4) {                                             // d xyz2[g] = (0 - d e_0 - d e_1 ...) + sa3's term
        const size_t at = ((size_t)b * PN2_NP2 + g) * 4 + threadIdx.x;
        float acc = 0.f;
        for (int s = 0; s < PN2_NS2; ++s) acc -= des[s * 4 + threadIdx.x];
        dx2[at] = threadIdx.x < 3 ? acc + dx2a[at] : 0.f;
    }
}

// A wave = a level-1 point j of a cloud.  du[j] = the sum over the rows (g, s) with ball2[g][s] == j, ascending, of dh[g][s];
// dx1a[j] = the sum over the same rows of de[g][s], then over the groups g with fps2[g] == j, ascending, of dx2[g].
__global__ __launch_bounds__(256) void pn2_l1_gather_kernel(const int32_t* __restrict__ ball2, const int32_t* __restrict__ fps2,
                                                            const float* __restrict__ dh, const float* __restrict__ de,
                                                            const float* __restrict__ dx2, float* __restrict__ du, float* __restrict__ dx1a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[Pn2GatherLds::BYTES];
    uint16_t* fps = LDS_AT(uint16_t, smem, Pn2GatherLds::FPS);
    uint16_t* tab = LDS_AT(uint16_t, smem, Pn2GatherLds::TAB);
    const int b = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < PN2_ROWS2; e += 256) tab[e] = (uint16_t)min(max(ball2[(size_t)b * PN2_ROWS2 + e], 0), PN2_NP1 - 1);
    if (threadIdx.x < PN2_NP2) fps[threadIdx.x] = (uint16_t)min(max(fps2[(size_t)b * PN2_NP2 + threadIdx.x], 0), PN2_NP1 - 1);
    __syncthreads();
    const float* H = dh + (size_t)b * PN2_ROWS2 * 128 + 2 * lane;
    const float* E = de + (size_t)b * PN2_ROWS2 * 4 + (lane & 3);
#pragma unroll 1
    for (int jj = 0; jj < 2; ++jj) {
        const int j = blockIdx.x * 8 + wv * 2 + jj;
        float a0 = 0.f, a1 = 0.f, ex = 0.f;
        for (int r0 = 0; r0 < PN2_ROWS2; r0 += 64) {
            unsigned long long m = __ballot(tab[r0 + lane] == j);
            while (m) {                                                // wave-uniform
                const int r = r0 + __builtin_ctzll(m);
                m &= m - 1;
                const float2 h = *reinterpret_cast<const float2*>(H + (size_t)r * 128);
                a0 += h.x; a1 += h.y;
                if (lane < 4) ex += E[(size_t)r * 4];
            }
        }
        for (int g = 0; g < PN2_NP2; ++g)
            if (fps[g] == j && lane < 4) ex += dx2[((size_t)b * PN2_NP2 + g) * 4 + lane];
        *reinterpret_cast<float2*>(du + ((size_t)b * PN2_NP1 + j) * 128 + 2 * lane) = float2{a0, a1};
        if (lane < 4) dx1a[((size_t)b * PN2_NP1 + j) * 4 + lane] = ex;
    }
}

// sa1 backward, two groups a workgroup.  The forward's arguments (pn2_sa1_kernel), W2T [64][64] the middle layer transposed, l1 the
// saved l1_feat, dl1 its gradient, dx1a what pn2_l1_gather_kernel left.  Out: dd [B][512][32][4], dx1 [B][512][4]; win1
// [B][512][128] and act1 [B][512][32][4] where wanted.
__global__ __launch_bounds__(256) void pn2_sa1_bwd_kernel(const float* __restrict__ first, const float* __restrict__ W2, const float* __restrict__ b2,
                                                          const float* __restrict__ W3, const float* __restrict__ b3,
                                                          const float* __restrict__ W2T, const float* __restrict__ pc,
                                                          const int32_t* __restrict__ n_points, int stride, const int32_t* __restrict__ ball,
                                                          const float* __restrict__ cen, const float* __restrict__ l1,
                                                          const float* __restrict__ dl1, const float* __restrict__ dx1a,
                                                          float* __restrict__ dd, float* __restrict__ dx1, int32_t* __restrict__ win1,
                                                          uint32_t* __restrict__ act1) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[Pn2Sa1BwdLds::BYTES];
    using L = Pn2Sa1BwdLds;
    float* A = LDS_AT(float, smem, L::A);
    float* Bm = LDS_AT(float, smem, L::B);
    int* win = LDS_AT(int, smem, L::WIN);
    float* dgs = LDS_AT(float, smem, L::DG);
    float* dds = LDS_AT(float, smem, L::DD);
    constexpr int LD = L::LD;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int n = cloud_points(n_points, b, stride);
    const int row = threadIdx.x >> 2, o0 = (threadIdx.x & 3) * 16;       // the elementwise passes: a thread = a row x 16 channels
    const size_t grow = ((size_t)b * PN2_NP1 + tile * 2) * PN2_NS1 + row;   // this row among the cloud's
    uint32_t gate1 = 0;                                                // h1 > 0 of the thread's 16 channels
    {                                                                  // pn2_sa1_kernel's first layer
        const int g = tile * 2 + (row >> 5);
        const int j = min(max(ball[grow], 0), n - 1);
        const float* x = pc + ((size_t)b * stride + j) * 3;
        const float* c = cen + ((size_t)b * PN2_NP1 + g) * 3;
        const float dx = x[0] - c[0], dy = x[1] - c[1], dz = x[2] - c[2];
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(first + (o0 + e + r) * 4);
                v[r] = fmaxf(fmaf(w[2], dz, fmaf(w[1], dy, fmaf(w[0], dx, w[3]))), 0.f);
                if (v[r] > 0.f) gate1 |= 1u << (e + r);
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = v;
        }
    }
    if (act1) {                                                        // wave-uniform
        uint32_t word = gate1 << (16 * (threadIdx.x & 1));
        word |= __shfl_xor(word, 1);
        if ((threadIdx.x & 1) == 0) act1[grow * 4 + ((threadIdx.x & 3) >> 1)] = word;
    }
    __syncthreads();
    f32x4 v[2][2];
    tile_layer<64, LD>(A, W2, b2, 32 * (wv >> 1), wv, q, p, v);
    tile_store<LD>(Bm, 32 * (wv >> 1), wv, q, p, v);
    __syncthreads();
    // the last layer again: the wave's 32 rows are one group; per channel its lowest row that holds the saved maximum
    {
        const int grp = wv & 1;
        const size_t gat = ((size_t)b * PN2_NP1 + tile * 2 + grp) * 128;
#pragma unroll
        for (int ob = 0; ob < 128; ob += 64) {
            const int obase = ob + 32 * (wv >> 1);
            tile_layer<64, LD>(Bm, W3, b3, obase, wv, q, p, v);
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int ch = obase + 16 * m + 4 * q;
                const f32x4 sv = *reinterpret_cast<const f32x4*>(l1 + gat + ch);
                const f32x4 dv = *reinterpret_cast<const f32x4*>(dl1 + gat + ch);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int cand = tile_winner(v, m, r, sv[r], 0, p);
                    if (p == 0) {
                        const int w = cand == P2G_NONE ? -1 : cand;
                        win[grp * 128 + ch + r] = w;
                        dgs[grp * 128 + ch + r] = sv[r] > 0.f ? dv[r] : 0.f;
                        if (win1) win1[gat + ch + r] = w;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; e += 4) *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = f32x4{0.f, 0.f, 0.f, 0.f};   // h1 is in gate1 now
    __syncthreads();
    // d h2[s][k] = sum over the channels c won by row s of the group, ascending, of dgs[c] W3[c][k]: a wave = a group's even or odd rows
    {
        const int grp = threadIdx.x >> 7, par = (threadIdx.x >> 6) & 1, k = threadIdx.x & 63;
#pragma unroll 4
        for (int c = 0; c < 128; ++c) {
            const float w = W3[c * 64 + k];
            const int s = win[grp * 128 + c];
            if (s >= 0 && (s & 1) == par) A[(32 * grp + s) * LD + k] = fmaf(dgs[grp * 128 + c], w, A[(32 * grp + s) * LD + k]);
        }
    }
    __syncthreads();
    {                                                                  // the middle layer's gate
        uint32_t gate2 = 0;
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(Bm + row * LD + o0 + e);
            f32x4 d = *reinterpret_cast<const f32x4*>(A + row * LD + o0 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (a[r] > 0.f) gate2 |= 1u << (e + r);
                else d[r] = 0.f;
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = d;
        }
        if (act1) {                                                    // wave-uniform
            uint32_t word = gate2 << (16 * (threadIdx.x & 1));
            word |= __shfl_xor(word, 1);
            if ((threadIdx.x & 1) == 0) act1[grow * 4 + 2 + ((threadIdx.x & 3) >> 1)] = word;
        }
    }
    __syncthreads();
    tile_layer_t<64, LD>(A, W2T, Bm, 32 * (wv >> 1), wv, q, p);
    __syncthreads();
    {                                                                  // the first layer's gate; d d = W1^T d h1
        float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(Bm + row * LD + o0 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float dv = ((gate1 >> (e + r)) & 1u) ? d[r] : 0.f;
                const f32x4 w = *reinterpret_cast<const f32x4*>(first + (o0 + e + r) * 4);
                px = fmaf(dv, w[0], px);
                py = fmaf(dv, w[1], py);
                pz = fmaf(dv, w[2], pz);
            }
        }
        // the four 16-channel chains of a row: (c0 + c1) + (c2 + c3), every lane the same tree
        px += __shfl_xor(px, 1); py += __shfl_xor(py, 1); pz += __shfl_xor(pz, 1);
        px += __shfl_xor(px, 2); py += __shfl_xor(py, 2); pz += __shfl_xor(pz, 2);
        if ((threadIdx.x & 3) == 0) {
            const f32x4 d = f32x4{px, py, pz, 0.f};
            *reinterpret_cast<f32x4*>(dd + grow * 4) = d;
            *reinterpret_cast<f32x4*>(dds + row * 4) = d;
        }
    }
    __syncthreads();
    if (threadIdx.x < 8) {                                             // d xyz1[i] = (0 - d d_0 - d d_1 ...) + the level above's term
        const int grp = threadIdx.x >> 2, a = threadIdx.x & 3;
        const size_t at = ((size_t)b * PN2_NP1 + tile * 2 + grp) * 4 + a;
        float acc = 0.f;
        for (int s = 0; s < PN2_NS1; ++s) acc -= dds[(32 * grp + s) * 4 + a];
        dx1[at] = a < 3 ? acc + dx1a[at] : 0.f;
    }
}

// A thread = a point p of a cloud: grad[p] = the sum over the rows (i, s) with ball1[i][s] == p, ascending, of dd[i][s], then over
// the centroids i with fps1[i] == p, ascending, of dx1[i]; one chain.  Zeros in the rows beyond the cloud.
__global__ __launch_bounds__(256) void pn2_point_gather_kernel(const int32_t* __restrict__ ball1, const int32_t* __restrict__ fps1,
                                                               const float* __restrict__ dd, const float* __restrict__ dx1,
                                                               const int32_t* __restrict__ n_points, int stride, float* __restrict__ grad) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[Pn2GatherLds::BYTES];
    uint16_t* fps = LDS_AT(uint16_t, smem, Pn2GatherLds::FPS);
    uint16_t* tab = LDS_AT(uint16_t, smem, Pn2GatherLds::TAB);
    const int b = blockIdx.y, pt = blockIdx.x * 256 + threadIdx.x;
    const int n = cloud_points(n_points, b, stride);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (blockIdx.x * 256 < n) {                                        // the whole workgroup
        for (int e = threadIdx.x; e < PN2_ROWS1; e += 256) tab[e] = (uint16_t)min(max(ball1[(size_t)b * PN2_ROWS1 + e], 0), n - 1);
        for (int e = threadIdx.x; e < PN2_NP1; e += 256) fps[e] = (uint16_t)min(max(fps1[(size_t)b * PN2_NP1 + e], 0), n - 1);
        __syncthreads();
        const float* D = dd + (size_t)b * PN2_ROWS1 * 4;
        for (int r0 = 0; r0 < PN2_ROWS1; r0 += 8) {
            const uint4 t = *reinterpret_cast<const uint4*>(tab + r0);
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = (int)((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                if (j == pt) {
                    const f32x4 d = *reinterpret_cast<const f32x4*>(D + (size_t)(r0 + e) * 4);
                    gx += d[0]; gy += d[1]; gz += d[2];
                }
            }
        }
        const float* X = dx1 + (size_t)b * PN2_NP1 * 4;
        for (int i = 0; i < PN2_NP1; ++i)
            if (fps[i] == pt) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(X + (size_t)i * 4);
                gx += d[0]; gy += d[1]; gz += d[2];
            }
    }
    if (pt < stride) {
        float* o = grad + ((size_t)b * stride + pt) * 3;
        const bool in = pt < n;
        o[0] = in ? gx : 0.f; o[1] = in ? gy : 0.f; o[2] = in ? gz : 0.f;
    }
}

}  // namespace

hipError_t configure_pn2_grad_kernels() { return opt_in_dynamic_lds({{pn2_sa2_bwd_kernel, Pn2Sa2BwdLds::BYTES}}); }

hipError_t launch_pn2_grad(const float* img, const Pn2Image& I, const float* gimg, const Pn2GradImage& G, const float* pc,
                           const int32_t* n_points, const int32_t* fps_start, int B, int stride, const int32_t* target, int loss_kind,
                           float kappa, float scale, const Pn2GradWs& w, const Pn2GradOut& out, int n_classes, float* grad, hipStream_t s) {
    const dim3 block(256);
    Pn2Out o{};
    o.fps1 = out.fps1; o.fps2 = out.fps2; o.ball1 = out.ball1; o.ball2 = out.ball2;
    o.l1_feat = out.l1_feat; o.l2_feat = out.l2_feat; o.gfeat = out.gfeat;
    o.pred = w.pred;
    hipError_t e = launch_pn2(img, I, pc, n_points, fps_start, B, stride, w.f, o, w.logits, n_classes, s);
    if (e != hipSuccess) return e;
    const int32_t* fps1 = out.fps1 ? out.fps1 : w.f.fps1;
    const int32_t* fps2 = out.fps2 ? out.fps2 : w.f.fps2;
    const int32_t* ball1 = out.ball1 ? out.ball1 : w.f.ball1;
    const int32_t* ball2 = out.ball2 ? out.ball2 : w.f.ball2;
    const float* l1 = out.l1_feat ? out.l1_feat : w.f.l1_feat;
    const float* l2 = out.l2_feat ? out.l2_feat : w.f.l2_feat;
    const float* gfeat = out.gfeat ? out.gfeat : w.f.gfeat;
    e = launch_head_backward<Pn2Linear>(gimg, G.fct, w, target, B, n_classes, loss_kind, kappa, scale, w.dg, PN2_EMB, s);
    if (e != hipSuccess) return e;
    // sa3
    hipLaunchKernelGGL(pn2_sa3_win_kernel, dim3(PN2_EMB / 64, B), block, 0, s, img + I.sa3[1].w, img + I.sa3[1].b, (const float*)w.f.s3b, gfeat,
                       w.win3);
    hipLaunchKernelGGL(pn2_sa3_sparse_kernel, dim3(PN2_NP2, B), block, 0, s, img + I.sa3[1].w, (const int32_t*)w.win3, gfeat,
                       (const float*)w.dg, (const float*)w.f.s3b, w.ds3b);
    launch_linear<Pn2Linear>(gimg, G.s3t, w.ds3b, 512, (size_t)PN2_NP2 * 512, nullptr, B, PN2_NP2, w.ds3a, 256, (size_t)PN2_NP2 * 256, 0, s);
    launch_act_gate<Pn2Linear>(w.ds3a, w.f.s3a, B * PN2_NP2 * 256, s);
    launch_linear<Pn2Linear>(gimg, G.s3ut, w.ds3a, 256, (size_t)PN2_NP2 * 256, nullptr, B, PN2_NP2, w.dl2, 256, (size_t)PN2_NP2 * 256, 0, s);
    launch_linear<Pn2Linear>(gimg, G.s3xt, w.ds3a, 256, (size_t)PN2_NP2 * 256, nullptr, B, PN2_NP2, w.dx2a, 4, (size_t)PN2_NP2 * 4, 0, s);
    if (out.act3)
        hipLaunchKernelGGL(pn2_act3_kernel, dim3((B * PN2_NP2 * 24 + 255) / 256), block, 0, s, (const float*)w.f.s3a, (const float*)w.f.s3b, B,
                           out.act3);
    // sa2
    hipLaunchKernelGGL(pn2_sa2_bwd_kernel, dim3(PN2_NP2, B), block, (size_t)Pn2Sa2BwdLds::BYTES, s, (const float*)w.f.u2, img + I.sa2_xyz,
                       img + I.sa2[0].w, img + I.sa2[0].b, img + I.sa2[1].w, img + I.sa2[1].b, gimg + G.s2t.w, ball2, (const float*)w.f.xyz1,
                       (const float*)w.f.xyz2, l2, (const float*)w.dl2, (const float*)w.dx2a, w.dh, w.de, w.dx2, out.win2, out.act2);
    hipLaunchKernelGGL(pn2_l1_gather_kernel, dim3(PN2_NP1 / 8, B), block, 0, s, ball2, fps2, (const float*)w.dh, (const float*)w.de,
                       (const float*)w.dx2, w.du, w.dx1a);
    launch_linear<Pn2Linear>(gimg, G.s2ut, w.du, 128, (size_t)PN2_NP1 * 128, nullptr, B, PN2_NP1, w.dl1, 128, (size_t)PN2_NP1 * 128, 0, s);
    // sa1
    hipLaunchKernelGGL(pn2_sa1_bwd_kernel, dim3(PN2_NP1 / 2, B), block, 0, s, img + I.sa1_first, img + I.sa1[0].w, img + I.sa1[0].b,
                       img + I.sa1[1].w, img + I.sa1[1].b, gimg + G.s1t.w, pc, n_points, stride, ball1, (const float*)w.f.xyz1, l1,
                       (const float*)w.dl1, (const float*)w.dx1a, w.dd, w.dx1, out.win1, out.act1);
    hipLaunchKernelGGL(pn2_point_gather_kernel, dim3((stride + 255) / 256, B), block, 0, s, ball1, fps1, (const float*)w.dd, (const float*)w.dx1,
                       n_points, stride, grad);
    return hipGetLastError();
}

}  // namespace ifd
