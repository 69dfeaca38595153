// The difference-form distance and the farthest point sampling that the PointNet++ and the PointConv victims share
// (include/ifd_pn2.h and include/ifd_pc.h define both word for word alike).  Device code only.
//
//   pn2_fps_kernel<PPT>   farthest point sampling, a workgroup of 256 threads a cloud.  Thread t keeps the points t + 256 k
//                         (k < PPT) and their running distances in registers; a pick is a scan of its own PPT points, a
//                         butterfly of (distance, index) pairs over the wave, ONE exchange of the four waves' pairs through LDS
//                         and ONE barrier (the slots are double-buffered by the pick's parity).  The picked point's coordinates
//                         come from the cloud's copy in LDS and are written as the picks are made, so that the grouping reads
//                         centroids, not indices.
#pragma once
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "victim_device.h"

namespace ifd {

// d = (dx dx + dy dy) + dz dz, every product and sum rounded on its own (include/ifd_pn2.h).  hipcc contracts by default, and
// __fmul_rn / __fadd_rn are plain operators to it, so the contraction is switched off for exactly this function.
__device__ __forceinline__ float pn2_dist(float x, float y, float z, float cx, float cy, float cz) {
#pragma clang fp contract(off)
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

// X: rows of 3 floats, a cloud's from X + b * xb; its first n_points[b] (n_fixed where null) rows are the cloud, n <= 256 PPT.
// fps_start [B][2] (null: 0), column `level`.  idx [B][npoint], xyz [B][npoint][3].
template <int PPT>
__global__ __launch_bounds__(PN2_FPS_THREADS) void pn2_fps_kernel(const float* __restrict__ X, size_t xb, const int32_t* __restrict__ n_points,
                                                                  int n_fixed, const int32_t* __restrict__ fps_start, int level, int npoint,
                                                                  int32_t* __restrict__ idx, float* __restrict__ xyz) {
    using L = Pn2FpsLds<PPT>;
    __shared__ __attribute__((aligned(16))) unsigned char smem[L::BYTES];
    float* sx = LDS_AT(float, smem, L::X);
    float* sv = LDS_AT(float, smem, L::SLOT_V);
    int* si = LDS_AT(int, smem, L::SLOT_I);
    const int b = blockIdx.x, t = threadIdx.x, wv = t >> 6;
    const int n = cloud_points(n_points, b, n_fixed);
    const float* Xb = X + (size_t)b * xb;
    float x[PPT], y[PPT], z[PPT], d[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int j = t + PN2_FPS_THREADS * k;
        x[k] = y[k] = z[k] = 0.f;
        d[k] = -1.f;                                                   // rows beyond the cloud: below every distance, never picked
        if (j < n) {
            x[k] = Xb[3 * j]; y[k] = Xb[3 * j + 1]; z[k] = Xb[3 * j + 2];
            d[k] = 1e10f;
            sx[3 * j] = x[k]; sx[3 * j + 1] = y[k]; sx[3 * j + 2] = z[k];
        }
    }
    __syncthreads();
    int far = fps_start ? fps_start[2 * b + level] : 0;
    far = min(max(far, 0), n - 1);                                     // starts outside are refused by the host
    int32_t* I = idx + (size_t)b * npoint;
    float* O = xyz + (size_t)b * npoint * 3;
    for (int i = 0; i < npoint; ++i) {
        const float cx = sx[3 * far], cy = sx[3 * far + 1], cz = sx[3 * far + 2];
        if (t == 0) { I[i] = far; O[3 * i] = cx; O[3 * i + 1] = cy; O[3 * i + 2] = cz; }
        float best = -2.f;
        int bi = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const float dist = pn2_dist(x[k], y[k], z[k], cx, cy, cz);
            if (dist < d[k]) d[k] = dist;
            if (d[k] > best) { best = d[k]; bi = t + PN2_FPS_THREADS * k; }      // strictly: the lowest index of a thread's equals
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ob = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        const int par = (i & 1) * 4;
        if ((t & 63) == 0) { sv[par + wv] = best; si[par + wv] = bi; }
        __syncthreads();
        best = sv[par]; bi = si[par];
#pragma unroll
        for (int w = 1; w < PN2_FPS_THREADS / 64; ++w) {
            const float ob = sv[par + w];
            const int oi = si[par + w];
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        far = bi;
    }
}

// npoint picks of every cloud of the batch; the points a thread keeps follow from the stride (<= PN2_MAX_POINTS rows)
inline void launch_fps(const float* X, int stride, const int32_t* n_points, const int32_t* fps_start, int level, int npoint, int B,
                       int32_t* idx, float* xyz, hipStream_t s) {
    if (stride <= 512)
        hipLaunchKernelGGL((pn2_fps_kernel<2>), dim3(B), dim3(PN2_FPS_THREADS), 0, s, X, (size_t)stride * 3, n_points, stride, fps_start, level,
                           npoint, idx, xyz);
    else if (stride <= 1024)
        hipLaunchKernelGGL((pn2_fps_kernel<4>), dim3(B), dim3(PN2_FPS_THREADS), 0, s, X, (size_t)stride * 3, n_points, stride, fps_start, level,
                           npoint, idx, xyz);
    else
        hipLaunchKernelGGL((pn2_fps_kernel<8>), dim3(B), dim3(PN2_FPS_THREADS), 0, s, X, (size_t)stride * 3, n_points, stride, fps_start, level,
                           npoint, idx, xyz);
}

}  // namespace ifd
