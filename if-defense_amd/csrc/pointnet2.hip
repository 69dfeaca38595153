// The PointNet++ victim classifier of the reference (baselines/model/pointnet2.py: PointNet2ClsSsg(num_classes=40) in eval mode).
// Eval-mode BatchNorm is folded into the weights on the host.  The [B, C, nsample, npoint] tensor of the reference never exists:
// a set-abstraction level gathers a tile of 64 grouped rows into LDS, runs its layers on the tile and writes only the maximum
// of every group.
//
//   pn2_fps_kernel<PPT>   farthest point sampling (victim_fps.h, shared with the PointConv victim), with the distance both use.
//   pn2_ball_kernel       a wave a centroid: the cloud is walked in index order 64 candidates at a time; a ballot and the count
//                         of the member lanes below a lane keep the order; the walk stops at nsample members.
//   pn2_sa1_kernel        64 rows = two 32-sample groups: 3 -> 64 by plain FMAs into LDS, 64 -> 64 and 64 -> 128 on MFMA, the
//                         maximum over each group's rows.  A wave's 32 rows are one group, so the maximum never leaves the wave.
//   pn2_sa2_kernel        64 rows = one 64-sample group.  The first layer in split form: U_j = b + W_f f_j per level-1 point
//                         (linear_kernel, 512 rows instead of 8192), then relu(U_j + W_xyz (xyz_j - c_i)) per row with the
//                         difference formed first, as the reference forms it; 128 -> 128 and 128 -> 256 on MFMA, the maximum.
//   linear_kernel         victim_linear.h: Y = relu(W X + b [+ W_xyz xyz]) in blocks of 64 inputs.  <Pn2Linear>: sa2's U, the
//                         first two layers of sa3, the head; <Pn2Sa3Last>: sa3's last layer, reduced to the maxima of its two
//                         64-row tiles.  The grouped MLPs' tile_layer runs the same 64-input block (linear_block64) from LDS.
//   pn2_pool_kernel       a cloud's two tiles -> its [1024] feature.  The prediction is launch_argmax's (pointnet.hip).
//
// Columns of an MFMA never mix, and no kernel looks at another cloud: a cloud's result depends on nothing but its own rows.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "victim_fps.h"
#include "victim_linear.h"

namespace ifd {

namespace {

__global__ __launch_bounds__(256) void pn2_check_kernel(const int32_t* __restrict__ n_points, const int32_t* __restrict__ fps_start, int B,
                                                        int stride, int32_t* __restrict__ bad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int n = stride;
    if (n_points) {
        n = n_points[b];
        if (n < 1 || n > stride) { atomicAdd(bad, 1); return; }
    }
    if (fps_start) {
        const int s1 = fps_start[2 * b], s2 = fps_start[2 * b + 1];
        if (s1 < 0 || s1 >= n || s2 < 0 || s2 >= PN2_NP1) atomicAdd(bad + 1, 1);
    }
}

// out[b][i][0 .. nsample): the first nsample j < n (ascending) with !(d(x_j, c_i) > r2), the rest filled with the first.
__global__ __launch_bounds__(256) void pn2_ball_kernel(const float* __restrict__ X, size_t xb, const int32_t* __restrict__ n_points, int n_fixed,
                                                       const float* __restrict__ cen, int npoint, int nsample, float r2,
                                                       int32_t* __restrict__ out) {
    const int b = blockIdx.y, i = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    if (i >= npoint) return;                                           // the whole wave
    const int n = cloud_points(n_points, b, n_fixed);
    const float* Xb = X + (size_t)b * xb;
    const float* c = cen + ((size_t)b * npoint + i) * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    int32_t* o = out + ((size_t)b * npoint + i) * nsample;
    int count = 0, first = 0;
    for (int j0 = 0; j0 < n && count < nsample; j0 += 64) {            // wave-uniform
        const int j = j0 + l;
        bool in = false;
        if (j < n) in = !(pn2_dist(Xb[3 * j], Xb[3 * j + 1], Xb[3 * j + 2], cx, cy, cz) > r2);
        const unsigned long long m = __ballot(in);
        if (m == 0) continue;
        if (count == 0) first = j0 + __builtin_ctzll(m);
        const int at = count + __builtin_popcountll(m & ((1ull << l) - 1ull));
        if (in && at < nsample) o[at] = j;
        count += __builtin_popcountll(m);
    }
    for (int e = count + l; e < nsample; e += 64) o[e] = first;
}

// the maximum over the wave's 32 rows: v[0][m] of every lane = max over t and p
__device__ __forceinline__ void tile_rowmax(f32x4 (&v)[2][2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float x = fmaxf(v[0][m][r], v[1][m][r]);
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) x = fmaxf(x, __shfl_xor(x, d));
            v[0][m][r] = x;
        }
}

// sa1.  first: [64][4] = {w0, w1, w2, bias}.  ball [B][512][32] into the cloud, cen [B][512][3].  feat [B][512][128].
__global__ __launch_bounds__(256) void pn2_sa1_kernel(const float* __restrict__ first, const float* __restrict__ W2, const float* __restrict__ b2,
                                                      const float* __restrict__ W3, const float* __restrict__ b3, const float* __restrict__ pc,
                                                      const int32_t* __restrict__ n_points, int stride, const int32_t* __restrict__ ball,
                                                      const float* __restrict__ cen, float* __restrict__ feat) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[Pn2Sa1Lds::BYTES];
    float* A = LDS_AT(float, smem, Pn2Sa1Lds::A);
    float* Bm = LDS_AT(float, smem, Pn2Sa1Lds::B);
    constexpr int LD = Pn2Sa1Lds::LD;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int n = cloud_points(n_points, b, stride);
    {
        const int row = threadIdx.x >> 2, o0 = (threadIdx.x & 3) * 16;
        const int g = tile * 2 + (row >> 5);
        const int j = min(max(ball[((size_t)b * PN2_NP1 + g) * PN2_NS1 + (row & 31)], 0), n - 1);
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
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = v;
        }
    }
    __syncthreads();
    f32x4 v[2][2];
    tile_layer<64, LD>(A, W2, b2, 32 * (wv >> 1), wv, q, p, v);
    tile_store<LD>(Bm, 32 * (wv >> 1), wv, q, p, v);
    __syncthreads();
    const int g = tile * 2 + (wv & 1);                                 // the wave's 32 rows are this group
    float* F = feat + ((size_t)b * PN2_NP1 + g) * 128;
#pragma unroll
    for (int ob = 0; ob < 128; ob += 64) {
        const int obase = ob + 32 * (wv >> 1);
        tile_layer<64, LD>(Bm, W3, b3, obase, wv, q, p, v);
        tile_rowmax(v);
        if (p == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m) *reinterpret_cast<f32x4*>(F + obase + 16 * m + 4 * q) = v[0][m];
        }
    }
}

// sa2.  U [B][512][128] = b + W_f f_j; wx: [128][4] = {w0, w1, w2, -}.  ball [B][128][64] into the 512, xyz1 [B][512][3],
// cen [B][128][3].  feat [B][128][256].
__global__ __launch_bounds__(256) void pn2_sa2_kernel(const float* __restrict__ U, const float* __restrict__ wx, const float* __restrict__ W2,
                                                      const float* __restrict__ b2, const float* __restrict__ W3, const float* __restrict__ b3,
                                                      const int32_t* __restrict__ ball, const float* __restrict__ xyz1,
                                                      const float* __restrict__ cen, float* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* A = LDS_AT(float, smem, Pn2Sa2Lds::A);
    float* Bm = LDS_AT(float, smem, Pn2Sa2Lds::B);
    float* red = LDS_AT(float, smem, Pn2Sa2Lds::RED);
    constexpr int LD = Pn2Sa2Lds::LD;
    const int b = blockIdx.y, g = blockIdx.x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    {
        const int row = threadIdx.x >> 2, o0 = (threadIdx.x & 3) * 32;
        const int j = min(max(ball[((size_t)b * PN2_NP2 + g) * PN2_NS2 + row], 0), PN2_NP1 - 1);
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
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = v;
        }
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
#pragma unroll 1
    for (int ob = 0; ob < 256; ob += 64) {
        const int obase = ob + 32 * (wv >> 1);
        tile_layer<128, LD>(Bm, W3, b3, obase, wv, q, p, v);
        tile_rowmax(v);
        if (p == 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m) *reinterpret_cast<f32x4*>(red + (wv & 1) * 256 + obase + 16 * m + 4 * q) = v[0][m];
        }
    }
    __syncthreads();
    feat[((size_t)b * PN2_NP2 + g) * 256 + threadIdx.x] = fmaxf(red[threadIdx.x], red[256 + threadIdx.x]);
}

__global__ __launch_bounds__(256) void pn2_pool_kernel(const float* __restrict__ part_max, int T, float* __restrict__ gfeat) {
    const int b = blockIdx.x, c = threadIdx.x * 4;
    const float* P = part_max + (size_t)b * T * PN2_EMB + c;
    f32x4 m = *reinterpret_cast<const f32x4*>(P);
    for (int t = 1; t < T; ++t) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(P + (size_t)t * PN2_EMB);
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = fmaxf(m[r], v[r]);
    }
    *reinterpret_cast<f32x4*>(gfeat + (size_t)b * PN2_EMB + c) = m;
}

}  // namespace

hipError_t configure_pn2_kernels() { return opt_in_dynamic_lds({{pn2_sa2_kernel, Pn2Sa2Lds::BYTES}}); }

hipError_t launch_pn2_check(const int32_t* n_points, const int32_t* fps_start, int B, int stride, int32_t* bad, hipStream_t s) {
    hipError_t e = hipMemsetAsync(bad, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pn2_check_kernel, dim3((B + 255) / 256), dim3(256), 0, s, n_points, fps_start, B, stride, bad);
    return hipGetLastError();
}

hipError_t launch_pn2(const float* img, const Pn2Image& I, const float* pc, const int32_t* n_points, const int32_t* fps_start, int B,
                      int stride, const Pn2Ws& w, const Pn2Out& out, float* logits, int n_classes, hipStream_t s) {
    int32_t* fps1 = out.fps1 ? out.fps1 : w.fps1;
    int32_t* fps2 = out.fps2 ? out.fps2 : w.fps2;
    int32_t* ball1 = out.ball1 ? out.ball1 : w.ball1;
    int32_t* ball2 = out.ball2 ? out.ball2 : w.ball2;
    float* l1 = out.l1_feat ? out.l1_feat : w.l1_feat;
    float* l2 = out.l2_feat ? out.l2_feat : w.l2_feat;
    float* gfeat = out.gfeat ? out.gfeat : w.gfeat;
    const dim3 block(256);
    // level 1: 512 centroids of the cloud, their balls, the grouped MLP
    launch_fps(pc, stride, n_points, fps_start, 0, PN2_NP1, B, fps1, w.xyz1, s);
    hipLaunchKernelGGL(pn2_ball_kernel, dim3(PN2_NP1 / 4, B), block, 0, s, pc, (size_t)stride * 3, n_points, stride, (const float*)w.xyz1,
                       PN2_NP1, PN2_NS1, pn2_radius2(0), ball1);
    hipLaunchKernelGGL(pn2_sa1_kernel, dim3(PN2_NP1 / 2, B), block, 0, s, img + I.sa1_first, img + I.sa1[0].w, img + I.sa1[0].b,
                       img + I.sa1[1].w, img + I.sa1[1].b, pc, n_points, stride, (const int32_t*)ball1, (const float*)w.xyz1, l1);
    // level 2: 128 centroids of the 512, their balls, U = b + W_f f per level-1 point, the grouped MLP
    launch_fps(w.xyz1, PN2_NP1, nullptr, fps_start, 1, PN2_NP2, B, fps2, w.xyz2, s);
    hipLaunchKernelGGL(pn2_ball_kernel, dim3(PN2_NP2 / 4, B), block, 0, s, (const float*)w.xyz1, (size_t)PN2_NP1 * 3, (const int32_t*)nullptr,
                       PN2_NP1, (const float*)w.xyz2, PN2_NP2, PN2_NS2, pn2_radius2(1), ball2);
    launch_linear<Pn2Linear>(img, I.sa2_u, l1, 128, (size_t)PN2_NP1 * 128, nullptr, B, PN2_NP1, w.u2, 128, (size_t)PN2_NP1 * 128, 0, s);
    hipLaunchKernelGGL(pn2_sa2_kernel, dim3(PN2_NP2, B), block, (size_t)Pn2Sa2Lds::BYTES, s, (const float*)w.u2, img + I.sa2_xyz,
                       img + I.sa2[0].w, img + I.sa2[0].b, img + I.sa2[1].w, img + I.sa2[1].b, (const int32_t*)ball2, (const float*)w.xyz1,
                       (const float*)w.xyz2, l2);
    // level 3: one group of the 128 rows [xyz | 256 features]
    launch_linear<Pn2Linear>(img, I.sa3_u, l2, 256, (size_t)PN2_NP2 * 256, nullptr, B, PN2_NP2, w.s3a, 256, (size_t)PN2_NP2 * 256, 1, s,
                             img + I.sa3_xyz, w.xyz2);
    launch_linear<Pn2Linear>(img, I.sa3[0], w.s3a, 256, (size_t)PN2_NP2 * 256, nullptr, B, PN2_NP2, w.s3b, 512, (size_t)PN2_NP2 * 512, 1, s);
    constexpr int T = PN2_NP2 / LINEAR_TILE;                           // the tiles linear_kernel<Pn2Sa3Last> writes
    launch_linear<Pn2Sa3Last>(img, I.sa3[1], w.s3b, 512, (size_t)PN2_NP2 * 512, nullptr, B, PN2_NP2, nullptr, 0, 0, 1, s, nullptr, nullptr,
                              w.part_max);
    hipLaunchKernelGGL(pn2_pool_kernel, dim3(B), block, 0, s, (const float*)w.part_max, T, gfeat);
    // the head, a cloud a row
    launch_linear<Pn2Linear>(img, I.fc[0], gfeat, PN2_EMB, 0, nullptr, 1, B, w.f1, 512, 0, 1, s);
    launch_linear<Pn2Linear>(img, I.fc[1], w.f1, 512, 0, nullptr, 1, B, w.f2, 256, 0, 1, s);
    launch_linear<Pn2Linear>(img, I.fc[2], w.f2, 256, 0, nullptr, 1, B, logits, n_classes, 0, 0, s);
    return out.pred ? launch_argmax(logits, B, n_classes, out.pred, s) : hipGetLastError();
}

}  // namespace ifd
