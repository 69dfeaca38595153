// Device-side pieces shared by the attacks on the PointNet victim: pointnet_grad.hip, pointnet_cw.hip, pointnet_knn.hip and
// pointnet_add.hip.  Everything here is __forceinline__ and works on values the caller holds: the callers' loads and stores
// stay where they are, in their order, so the kernels compile to the code they had with their own copies.
#pragma once
#include "ifd_device.h"
#include "ifd_internal.h"

namespace ifd {

// sum over the workgroup (256 threads) of v, every thread's contribution already summed in its own fixed order: a fixed tree
__device__ __forceinline__ float atk_block_sum(float v, float* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) sh[tid] += sh[tid + w];
        __syncthreads();
    }
    return sh[0];
}

// the rows of cloud b that are its own: n_points[b] (stride where n_points is null), clamped to [0, stride]
__device__ __forceinline__ int atk_rows(const int32_t* n_points, int b, int stride) {
    const int n = n_points ? n_points[b] : stride;
    return min(max(n, 0), stride);
}

// torch.optim.Adam's step on one element (torch/optim/adam.py _single_tensor_adam, csrc/optimize.hip's Adam phase, term by
// term): gradient g, moments mr and vr updated in place, the new x returned.  step_size, bc2, omb1, omb2: adam_step_consts
// (ifd_internal.h).  On register values only: M, V and the cloud are loaded and stored by the caller.  knn_step_kernel spells
// these lines out itself: calling this there changed its register allocation.
__device__ __forceinline__ float atk_adam(float x, float g, float& mr, float& vr, float step_size, float bc2, float omb1, float omb2) {
    mr = __builtin_fmaf(g - mr, omb1, mr);
    vr = __builtin_fmaf(omb2 * g, g, vr * 0.999f);
    const float denom = sqrtf(vr) / bc2 + 1e-8f;
    return __builtin_fmaf(-step_size, mr / denom, x);
}

// Not here: the record / info block that cw_step_kernel and add_step_kernel share (add_step_kernel's writes D.far as well).  As a helper (out-parameters,
// a returned struct, state by value or by reference) it compiled both kernels to other instructions, so each keeps its copy.

// thread 0 of the two finish kernels: success = lower > 0, bounds [3][B] = {weight, lower, upper} where asked for
__device__ __forceinline__ void atk_cw_report(const CwState& S, int b, int B, double lo, int32_t* __restrict__ success,
                                              double* __restrict__ bounds) {
    success[b] = lo > 0.0 ? 1 : 0;
    if (bounds) {
        bounds[b] = S.weight[b];
        bounds[(size_t)B + b] = lo;
        bounds[2 * (size_t)B + b] = S.upper[b];
    }
}

}  // namespace ifd
