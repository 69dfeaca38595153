// The PointConv victim classifier of the reference (baselines/model/pointconv.py: PointConvDensityClsSsg(num_classes=40) in eval
// mode; include/ifd_pc.h states every definition used here).  Eval-mode BatchNorm is folded into the weights on the host.  The
// [B, C, K, npoint] tensors of the reference never exist: a level gathers a tile of 64 grouped rows into LDS, runs its MLP and its
// WeightNet on the tile, and writes only the contraction G[c][w] = sum_k s_k F[k][c] Wn[k][w] of every group, on which the level's
// wide linear then runs as one linear_kernel launch.
//
//   pc_check_kernel       the counts and the starts of a call, on the device.
//   pc_density_kernel     a wave a point j: lane l adds expf(-d_ij / c1) over i = l, l + 64, ..., the 64 partial sums meet in a
//                         butterfly, DensityNet 1 -> 8 -> 8 -> 1 runs on the result.  The level's input cloud sits in LDS.
//   pn2_fps_kernel<PPT>   farthest point sampling (victim_fps.h, PointNet++'s).
//   pc_knn_kernel<PPT, K> a wave a centroid: lane l keeps the candidates l + 64 k as 64-bit keys (distance bits | index) in
//                         registers; K times the wave's smallest key is found by a butterfly and struck out by its owner.  Keys are
//                         unique and order like (d, index), so the row comes out in ascending (d, index) order.
//   pc_sa1_kernel         64 rows = two 32-neighbour groups: 3 -> 64 by plain FMAs into LDS, 64 -> 64 and 64 -> 128 on MFMA
//                         (tile_layer), WeightNet of every row by plain FMAs; the last layer comes 64 channels at a time, scaled by
//                         s_j, back into LDS, where 8 outputs a thread contract it with the rows' WeightNet.
//   pc_sa2_kernel         64 rows = one 64-neighbour group.  The first layer in split form, as pn2_sa2_kernel: U_j = b + W_f f_j
//                         per level-1 point (linear_kernel), then relu(U_j + W_xyz (xyz_j - c_i)) per row; 128 -> 128 and
//                         128 -> 256 on MFMA; the contraction as in sa1, 4 outputs a thread.
//   pc_centre_kernel      sa3: the mean of the 128 level-2 centroids, xyz_j - mean, WeightNet of the 128 rows.
//   pc_contract3_kernel   sa3: G[c][w] over the 128 rows of linear_kernel's [128][1024] output.
//   linear_kernel         victim_linear.h <Pn2Linear>: sa2's U, sa3's three MLP layers (the first with its xyz columns), the three
//                         wide linears behind the contractions (2048, 4096 and 16384 inputs) and the head.
//
// Columns of an MFMA never mix, and no kernel looks at another cloud: a cloud's result depends on nothing but its own rows.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "pc_device.h"
#include "victim_fps.h"
#include "victim_linear.h"

namespace ifd {

namespace {

__global__ __launch_bounds__(256) void pc_check_kernel(const int32_t* __restrict__ n_points, const int32_t* __restrict__ fps_start, int B,
                                                       int stride, int32_t* __restrict__ bad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int n = stride;
    if (n_points) {
        n = n_points[b];
        if (n < PC_MIN_POINTS || n > stride) { atomicAdd(bad, 1); return; }
    }
    if (fps_start) {
        const int s1 = fps_start[2 * b], s2 = fps_start[2 * b + 1];
        if (s1 < 0 || s1 >= n || s2 < 0 || s2 >= PC_NP1) atomicAdd(bad + 1, 1);
    }
}

// dens[b][j] = DensityNet(rho_j), rho_j the Gaussian density of point j among the n points of cloud b (include/ifd_pc.h).
// X: rows of 3 floats, a cloud's from X + b * xb.  dn: {[8][1], [8], [8][8], [8], [1][8], [1]}.  A workgroup: 32 points, 8 a wave.
__global__ __launch_bounds__(256) void pc_density_kernel(const float* __restrict__ X, size_t xb, const int32_t* __restrict__ n_points,
                                                         int n_fixed, const float* __restrict__ dn, float c1, float c2,
                                                         float* __restrict__ dens, int ldd) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcDensityLds::BYTES];
    float* sx = LDS_AT(float, smem, PcDensityLds::X);
    const int b = blockIdx.y, wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int n = cloud_points(n_points, b, n_fixed);
    if (blockIdx.x * 32 >= n) return;                                  // the whole workgroup
    const float* Xb = X + (size_t)b * xb;
    for (int e = threadIdx.x; e < 3 * n; e += 256) sx[e] = Xb[e];
    __syncthreads();
    const float nf = (float)n;
    for (int jj = 0; jj < 8; ++jj) {
        const int j = blockIdx.x * 32 + jj * 4 + wv;
        if (j >= n) continue;                                          // the whole wave
        const float xj = sx[3 * j], yj = sx[3 * j + 1], zj = sx[3 * j + 2];
        float acc = 0.f;
        for (int i = l; i < n; i += 64) acc += expf(-(pn2_dist(sx[3 * i], sx[3 * i + 1], sx[3 * i + 2], xj, yj, zj) / c1));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
        const float rho[1] = {(acc / nf) / c2};
        float h1[8], h2[8], out[1];
        small_layer<8, 1>(dn, dn + 8, rho, h1);
        small_layer<8, 8>(dn + 16, dn + 80, h1, h2);
        small_layer<1, 8>(dn + 88, dn + 96, h2, out);
        if (l == 0) dens[(size_t)b * ldd + j] = out[0];
    }
}

// out[b][i][0 .. K): the K points j < n of smallest d(x_j, c_i), the lower index first among equal d, in ascending (d, index)
// order.  n <= 64 PPT, K <= 64, K <= n (the host's to see to).
template <int PPT, int K>
__global__ __launch_bounds__(256) void pc_knn_kernel(const float* __restrict__ X, size_t xb, const int32_t* __restrict__ n_points, int n_fixed,
                                                     const float* __restrict__ cen, int npoint, int32_t* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (i >= npoint) return;                                           // the whole wave
    const int n = cloud_points(n_points, b, n_fixed);
    const float* Xb = X + (size_t)b * xb;
    const float* c = cen + ((size_t)b * npoint + i) * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    unsigned long long key[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int j = l + 64 * k;
        key[k] = ~0ull;                                                // rows beyond the cloud: above every key, never chosen
        if (j < n) {                                                   // d >= +0, so its bits order as it does
            const float d = pn2_dist(Xb[3 * j], Xb[3 * j + 1], Xb[3 * j + 2], cx, cy, cz);
            key[k] = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
        }
    }
    int mine = 0;
    for (int r = 0; r < K; ++r) {
        unsigned long long m = key[0];
#pragma unroll
        for (int k = 1; k < PPT; ++k) m = key[k] < m ? key[k] : m;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned hi = __shfl_xor((unsigned)(m >> 32), off), lo = __shfl_xor((unsigned)m, off);
            const unsigned long long o = ((unsigned long long)hi << 32) | lo;
            m = o < m ? o : m;
        }
#pragma unroll
        for (int k = 0; k < PPT; ++k)
            if (key[k] == m) key[k] = ~0ull;                           // its owner strikes it out: the index makes every key unique
        if (l == r) mine = (int)(unsigned)m;
    }
    if (l < K) out[((size_t)b * npoint + i) * K + l] = min(mine, n - 1);
}

// Rows 32 g2 .. of the tile in A (64 channels, already scaled by s_k) against the rows' WeightNet: N outputs w0 .. w0 + N - 1 of
// channel c over KN members, one fused chain from 0 in the row's order.
template <int N, int KN, int LD>
__device__ __forceinline__ void contract(const float* __restrict__ A, const float* __restrict__ WN, int row0, int c, int w0, float* __restrict__ g) {
    float acc[N];
#pragma unroll
    for (int e = 0; e < N; ++e) acc[e] = 0.f;
    for (int k = 0; k < KN; ++k) {
        const float f = A[(row0 + k) * LD + c];
        const float* wn = WN + (row0 + k) * PC_WN + w0;
#pragma unroll
        for (int e = 0; e < N; ++e) acc[e] = fmaf(f, wn[e], acc[e]);
    }
#pragma unroll
    for (int e = 0; e < N; e += 4) *reinterpret_cast<f32x4*>(g + e) = f32x4{acc[e], acc[e + 1], acc[e + 2], acc[e + 3]};
}

// v[t][m] of a wave's 32 rows times the rows' density scale
__device__ __forceinline__ void tile_scale(const float* __restrict__ S, int wv, int p, f32x4 (&v)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float s = S[32 * (wv & 1) + 16 * t + p];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[t][m][r] *= s;
    }
}

// sa1.  first: [64][4] = {w0, w1, w2, bias}; wn: WeightNet.  knn [B][512][32] into the cloud, cen [B][512][3], dens [B][ldd].
// G [B][512][2048] from G + b * gb.
__global__ __launch_bounds__(256) void pc_sa1_kernel(const float* __restrict__ first, const float* __restrict__ W2, const float* __restrict__ b2,
                                                     const float* __restrict__ W3, const float* __restrict__ b3, const float* __restrict__ wn,
                                                     const float* __restrict__ pc, const int32_t* __restrict__ n_points, int stride,
                                                     const int32_t* __restrict__ knn, const float* __restrict__ cen,
                                                     const float* __restrict__ dens, int ldd, float* __restrict__ G, size_t gb) {
    using L = PcSa1Lds;
    __shared__ __attribute__((aligned(16))) unsigned char smem[L::BYTES];
    float* A = LDS_AT(float, smem, L::A);
    float* Bm = LDS_AT(float, smem, L::B);
    float* WN = LDS_AT(float, smem, L::WN);
    float* S = LDS_AT(float, smem, L::S);
    constexpr int LD = L::LD;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int n = cloud_points(n_points, b, stride);
    {
        const int row = threadIdx.x >> 2, part = threadIdx.x & 3, o0 = part * 16;
        const int g = tile * 2 + (row >> 5);
        const int j = min(max(knn[((size_t)b * PC_NP1 + g) * PC_K1 + (row & 31)], 0), n - 1);
        const float* x = pc + ((size_t)b * stride + j) * 3;
        const float* c = cen + ((size_t)b * PC_NP1 + g) * 3;
        const float dx = x[0] - c[0], dy = x[1] - c[1], dz = x[2] - c[2];
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(first + (o0 + e + r) * 4);
                v[r] = fmaxf(fmaf(w[2], dz, fmaf(w[1], dy, fmaf(w[0], dx, w[3]))), 0.f);
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = v;
        }
        float w4[4];
        weight_net<4>(wn, dx, dy, dz, part * 4, w4);
        *reinterpret_cast<f32x4*>(WN + row * PC_WN + part * 4) = f32x4{w4[0], w4[1], w4[2], w4[3]};
        if (part == 0) S[row] = dens[(size_t)b * ldd + j];
    }
    __syncthreads();
    f32x4 v[2][2];
    tile_layer<64, LD>(A, W2, b2, 32 * (wv >> 1), wv, q, p, v);
    tile_store<LD>(Bm, 32 * (wv >> 1), wv, q, p, v);
    __syncthreads();
    const int g2 = threadIdx.x >> 7, c = threadIdx.x & 63, w0 = ((threadIdx.x >> 6) & 1) * 8;
    float* Gg = G + (size_t)b * gb + (size_t)(tile * 2 + g2) * (128 * PC_WN);
#pragma unroll 1
    for (int ob = 0; ob < 128; ob += 64) {
        tile_layer<64, LD>(Bm, W3, b3, ob + 32 * (wv >> 1), wv, q, p, v);
        tile_scale(S, wv, p, v);
        tile_store<LD>(A, 32 * (wv >> 1), wv, q, p, v);                // channels ob .. ob + 63 at columns 0 .. 63
        __syncthreads();
        contract<8, PC_K1, LD>(A, WN, 32 * g2, c, w0, Gg + (ob + c) * PC_WN + w0);
        __syncthreads();
    }
}

// sa2.  U [B][512][128] = b + W_f f_j; wx: [128][4] = {w0, w1, w2, -}.  knn [B][128][64] into the 512, xyz1 [B][512][3],
// cen [B][128][3], dens [B][512].  G [B][128][4096] from G + b * gb.
__global__ __launch_bounds__(256) void pc_sa2_kernel(const float* __restrict__ U, const float* __restrict__ wx, const float* __restrict__ W2,
                                                     const float* __restrict__ b2, const float* __restrict__ W3, const float* __restrict__ b3,
                                                     const float* __restrict__ wn, const int32_t* __restrict__ knn,
                                                     const float* __restrict__ xyz1, const float* __restrict__ cen,
                                                     const float* __restrict__ dens, float* __restrict__ G, size_t gb) {
    using L = PcSa2Lds;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* A = LDS_AT(float, smem, L::A);
    float* Bm = LDS_AT(float, smem, L::B);
    float* WN = LDS_AT(float, smem, L::WN);
    float* S = LDS_AT(float, smem, L::S);
    constexpr int LD = L::LD;
    const int b = blockIdx.y, g = blockIdx.x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    {
        const int row = threadIdx.x >> 2, part = threadIdx.x & 3, o0 = part * 32;
        const int j = min(max(knn[((size_t)b * PC_NP2 + g) * PC_K2 + row], 0), PC_NP1 - 1);
        const float* x = xyz1 + ((size_t)b * PC_NP1 + j) * 3;
        const float* c = cen + ((size_t)b * PC_NP2 + g) * 3;
        const float dx = x[0] - c[0], dy = x[1] - c[1], dz = x[2] - c[2];
        const float* u = U + ((size_t)b * PC_NP1 + j) * 128 + o0;
#pragma unroll
        for (int e = 0; e < 32; e += 4) {
            f32x4 v = *reinterpret_cast<const f32x4*>(u + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(wx + (o0 + e + r) * 4);
                v[r] = fmaxf(fmaf(w[2], dz, fmaf(w[1], dy, fmaf(w[0], dx, v[r]))), 0.f);
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = v;
        }
        float w4[4];
        weight_net<4>(wn, dx, dy, dz, part * 4, w4);
        *reinterpret_cast<f32x4*>(WN + row * PC_WN + part * 4) = f32x4{w4[0], w4[1], w4[2], w4[3]};
        if (part == 0) S[row] = dens[(size_t)b * PC_NP1 + j];
    }
    __syncthreads();
    f32x4 v[2][2];
#pragma unroll
    for (int ob = 0; ob < 128; ob += 64) {
        const int obase = ob + 32 * (wv >> 1);
        tile_layer<128, LD>(A, W2, b2, obase, wv, q, p, v);
        tile_store<LD>(Bm, obase, wv, q, p, v);
    }
    __syncthreads();
    const int c = threadIdx.x & 63, w0 = (threadIdx.x >> 6) * 4;
    float* Gg = G + (size_t)b * gb + (size_t)g * (256 * PC_WN);
#pragma unroll 1
    for (int ob = 0; ob < 256; ob += 64) {
        tile_layer<128, LD>(Bm, W3, b3, ob + 32 * (wv >> 1), wv, q, p, v);
        tile_scale(S, wv, p, v);
        tile_store<LD>(A, 32 * (wv >> 1), wv, q, p, v);                // channels ob .. ob + 63 at columns 0 .. 63
        __syncthreads();
        contract<4, PC_K2, LD>(A, WN, 0, c, w0, Gg + (ob + c) * PC_WN + w0);
        __syncthreads();
    }
}

// sa3's centre.  xyz2 [B][128][3] -> xyz3 = xyz2 - mean, wn3 [B][128][16] = WeightNet(xyz3).  A workgroup of 128 threads a cloud.
__global__ __launch_bounds__(PC_NP2) void pc_centre_kernel(const float* __restrict__ xyz2, const float* __restrict__ wn, float* __restrict__ xyz3,
                                                           float* __restrict__ wn3) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcCentreLds::BYTES];
    float* mean = LDS_AT(float, smem, PcCentreLds::MEAN);
    const int b = blockIdx.x, k = threadIdx.x;
    const float* X = xyz2 + (size_t)b * PC_NP2 * 3;
    if (k < 3) {
        float sum = 0.f;
        for (int j = 0; j < PC_NP2; ++j) sum += X[3 * j + k];          // ascending, from 0
        mean[k] = sum * (1.f / PC_NP2);
    }
    __syncthreads();
    const float dx = X[3 * k] - mean[0], dy = X[3 * k + 1] - mean[1], dz = X[3 * k + 2] - mean[2];
    float* o = xyz3 + ((size_t)b * PC_NP2 + k) * 3;
    o[0] = dx; o[1] = dy; o[2] = dz;
    float w[PC_WN];
    weight_net<PC_WN>(wn, dx, dy, dz, 0, w);
    float* wo = wn3 + ((size_t)b * PC_NP2 + k) * PC_WN;
#pragma unroll
    for (int e = 0; e < PC_WN; e += 4) *reinterpret_cast<f32x4*>(wo + e) = f32x4{w[e], w[e + 1], w[e + 2], w[e + 3]};
}

// sa3's contraction.  F [B][128][1024], dens [B][128], wn3 [B][128][16] -> G [16384] at G + b * gb: 64 channels a workgroup, 4
// outputs a thread.
__global__ __launch_bounds__(256) void pc_contract3_kernel(const float* __restrict__ F, const float* __restrict__ dens,
                                                           const float* __restrict__ wn3, float* __restrict__ G, size_t gb) {
    const int b = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), w0 = (threadIdx.x >> 6) * 4;
    const float* Fb = F + (size_t)b * PC_NP2 * PC_EMB + c;
    const float* Sb = dens + (size_t)b * PC_NP2;
    const float* Wb = wn3 + (size_t)b * PC_NP2 * PC_WN + w0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < PC_NP2; ++k) {
        const float f = Fb[(size_t)k * PC_EMB] * Sb[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(f, Wb[k * PC_WN + e], acc[e]);
    }
    *reinterpret_cast<f32x4*>(G + (size_t)b * gb + c * PC_WN + w0) = f32x4{acc[0], acc[1], acc[2], acc[3]};
}

template <int K>
void launch_knn(const float* X, int stride, const int32_t* n_points, const float* cen, int npoint, int B, int32_t* out, hipStream_t s) {
    const dim3 grid(npoint / 4, B), block(256);
    if (stride <= 512)
        hipLaunchKernelGGL((pc_knn_kernel<8, K>), grid, block, 0, s, X, (size_t)stride * 3, n_points, stride, cen, npoint, out);
    else if (stride <= 1024)
        hipLaunchKernelGGL((pc_knn_kernel<16, K>), grid, block, 0, s, X, (size_t)stride * 3, n_points, stride, cen, npoint, out);
    else
        hipLaunchKernelGGL((pc_knn_kernel<32, K>), grid, block, 0, s, X, (size_t)stride * 3, n_points, stride, cen, npoint, out);
}

void launch_density(const float* img, const PcImage& I, int level, const float* X, int stride, const int32_t* n_points, int B, float* dens,
                    int ldd, hipStream_t s) {
    hipLaunchKernelGGL(pc_density_kernel, dim3((stride + 31) / 32, B), dim3(256), 0, s, X, (size_t)stride * 3, n_points, stride,
                       img + I.sa[level].dn, pc_two_bw2(level), pc_norm(level), dens, ldd);
}

}  // namespace

hipError_t configure_pc_kernels() { return opt_in_dynamic_lds({{pc_sa2_kernel, PcSa2Lds::BYTES}}); }

hipError_t launch_pc_check(const int32_t* n_points, const int32_t* fps_start, int B, int stride, int32_t* bad, hipStream_t s) {
    hipError_t e = hipMemsetAsync(bad, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pc_check_kernel, dim3((B + 255) / 256), dim3(256), 0, s, n_points, fps_start, B, stride, bad);
    return hipGetLastError();
}

hipError_t launch_pc(const float* img, const PcImage& I, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B,
                     int stride, const PcWs& w, const PcOut& out, float* logits, int n_classes, hipStream_t s) {
    int32_t* fps1 = out.fps1 ? out.fps1 : w.fps1;
    int32_t* fps2 = out.fps2 ? out.fps2 : w.fps2;
    int32_t* knn1 = out.knn1 ? out.knn1 : w.knn1;
    int32_t* knn2 = out.knn2 ? out.knn2 : w.knn2;
    float* dens1 = out.dens1 ? out.dens1 : w.dens1;
    const int ldd1 = out.dens1 ? stride : PC_MAX_POINTS;
    float* dens2 = out.dens2 ? out.dens2 : w.dens2;
    float* dens3 = out.dens3 ? out.dens3 : w.dens3;
    float* l1 = out.l1_feat ? out.l1_feat : w.l1_feat;
    float* l2 = out.l2_feat ? out.l2_feat : w.l2_feat;
    float* gfeat = out.gfeat ? out.gfeat : w.gfeat;
    const PcLevel &S1 = I.sa[0], &S2 = I.sa[1], &S3 = I.sa[2];
    const dim3 block(256);
    constexpr size_t GB = (size_t)PC_NP1 * 128 * PC_WN;                // floats of a cloud's contraction buffer
    // level 1: the cloud's density scales, 512 centroids, their 32 nearest neighbours, the grouped MLP and contraction, the linear
    launch_density(img, I, 0, pc, stride, n_points, B, dens1, ldd1, s);
    launch_fps(pc, stride, n_points, fps_start, 0, PC_NP1, B, fps1, w.xyz1, s);
    launch_knn<PC_K1>(pc, stride, n_points, w.xyz1, PC_NP1, B, knn1, s);
    hipLaunchKernelGGL(pc_sa1_kernel, dim3(PC_NP1 / 2, B), block, 0, s, img + S1.first_xyz, img + S1.mlp[0].w, img + S1.mlp[0].b,
                       img + S1.mlp[1].w, img + S1.mlp[1].b, img + S1.wn, pc, n_points, stride, (const int32_t*)knn1, (const float*)w.xyz1,
                       (const float*)dens1, ldd1, w.g, GB);
    launch_linear<Pn2Linear>(img, S1.lin, w.g, 128 * PC_WN, GB, nullptr, B, PC_NP1, l1, 128, (size_t)PC_NP1 * 128, 1, s);
    // level 2: the same on the 512, with U = b + W_f f per level-1 point
    launch_density(img, I, 1, w.xyz1, PC_NP1, nullptr, B, dens2, PC_NP1, s);
    launch_fps(w.xyz1, PC_NP1, nullptr, fps_start, 1, PC_NP2, B, fps2, w.xyz2, s);
    launch_knn<PC_K2>(w.xyz1, PC_NP1, nullptr, w.xyz2, PC_NP2, B, knn2, s);
    launch_linear<Pn2Linear>(img, S2.u, l1, 128, (size_t)PC_NP1 * 128, nullptr, B, PC_NP1, w.u2, 128, (size_t)PC_NP1 * 128, 0, s);
    hipLaunchKernelGGL(pc_sa2_kernel, dim3(PC_NP2, B), block, (size_t)PcSa2Lds::BYTES, s, (const float*)w.u2, img + S2.first_xyz,
                       img + S2.mlp[0].w, img + S2.mlp[0].b, img + S2.mlp[1].w, img + S2.mlp[1].b, img + S2.wn, (const int32_t*)knn2,
                       (const float*)w.xyz1, (const float*)w.xyz2, (const float*)dens2, w.g, GB);
    launch_linear<Pn2Linear>(img, S2.lin, w.g, 256 * PC_WN, GB, nullptr, B, PC_NP2, l2, 256, (size_t)PC_NP2 * 256, 1, s);
    // level 3: one group of the 128 rows [xyz - mean | 256 features]
    launch_density(img, I, 2, w.xyz2, PC_NP2, nullptr, B, dens3, PC_NP2, s);
    hipLaunchKernelGGL(pc_centre_kernel, dim3(B), dim3(PC_NP2), 0, s, (const float*)w.xyz2, img + S3.wn, w.xyz3, w.wn3);
    launch_linear<Pn2Linear>(img, S3.u, l2, 256, (size_t)PC_NP2 * 256, nullptr, B, PC_NP2, w.s3a, 256, (size_t)PC_NP2 * 256, 1, s,
                             img + S3.first_xyz, w.xyz3);
    launch_linear<Pn2Linear>(img, S3.mlp[0], w.s3a, 256, (size_t)PC_NP2 * 256, nullptr, B, PC_NP2, w.s3b, 512, (size_t)PC_NP2 * 512, 1, s);
    launch_linear<Pn2Linear>(img, S3.mlp[1], w.s3b, 512, (size_t)PC_NP2 * 512, nullptr, B, PC_NP2, w.s3c, PC_EMB, (size_t)PC_NP2 * PC_EMB, 1, s);
    hipLaunchKernelGGL(pc_contract3_kernel, dim3(PC_EMB / 64, B), block, 0, s, (const float*)w.s3c, (const float*)dens3, (const float*)w.wn3,
                       w.g, GB);
    // the 16384-wide linear and the head, a cloud a row
    launch_linear<Pn2Linear>(img, S3.lin, w.g, (int)GB, 0, nullptr, 1, B, gfeat, PC_EMB, 0, 1, s);
    launch_linear<Pn2Linear>(img, I.fc[0], gfeat, PC_EMB, 0, nullptr, 1, B, w.f1, 512, 0, 1, s);
    launch_linear<Pn2Linear>(img, I.fc[1], w.f1, 512, 0, nullptr, 1, B, w.f2, 256, 0, 1, s);
    launch_linear<Pn2Linear>(img, I.fc[2], w.f2, 256, 0, nullptr, 1, B, logits, n_classes, 0, 0, s);
    return out.pred ? launch_argmax(logits, B, n_classes, out.pred, s) : hipGetLastError();
}

}  // namespace ifd
