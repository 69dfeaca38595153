// Device helpers shared by the victim classifiers (pointnet.hip, dgcnn.hip, pointnet2.hip), the PointNet backward pass
// (pointnet_grad.hip) and PU-Net (punet.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ifd_device.h"

namespace ifd {

// c + A B of one 16-input group on v_mfma_f32_16x16x4_f32: four dependent MFMAs, inputs 4 q + 0 .. 3 in ascending order
__device__ __forceinline__ f32x4 mfma4(const f32x4 a, const f32x4 b, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], b[3], c, 0, 0, 0);
    return c;
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    return f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
}
__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : 0.2f * v; }
__device__ __forceinline__ f32x4 leaky4(f32x4 v) { return f32x4{leaky(v[0]), leaky(v[1]), leaky(v[2]), leaky(v[3])}; }

// The rows of cloud b: n_points[b], or stride where n_points is null.  The clamp only keeps a kernel inside the cloud's buffer
// whatever the count says; the lower bound proper is enforced by the host, which refuses counts outside [1, stride] (PointNet,
// PointNet++) or [k, stride] (DGCNN) before any kernel that uses them runs.
__device__ __forceinline__ int cloud_points(const int32_t* __restrict__ n_points, int b, int stride) {
    const int n = n_points ? n_points[b] : stride;
    return min(max(n, 1), stride);
}

}  // namespace ifd
