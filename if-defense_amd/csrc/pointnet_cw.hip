// The Carlini-Wagner point-perturbation attack on the PointNet victim (include/ifd_cw.h; the reference's
// baselines/attack/CW/Perturb.py with L2Dist) behind ifd_cls_input_grad's forward / backward pass (pointnet_grad.hip).
//
//   cw_start_kernel    adv = pc_in + noise of a search step, the cloud's own rows only.
//   cw_step_kernel     one workgroup a cloud: the L2 distance to the original (a strided per-thread sum and a fixed tree, like
//                      fgm_update_kernel), the two records, then ONE elementwise pass that copies the pre-update cloud where a
//                      record or last_input wants it, adds the distance term's gradient and takes torch.optim.Adam's step.
//                      Bandwidth work: reads adv, ori, grad, m, v, writes adv, m, v (12 KB each at 1024 points).
//   cw_adjust_kernel   the binary search on the weight and the reset for the next search step.
//   cw_finish_kernel   the fallback to the last forwarded cloud, success = lower > 0.
//
// The weights are float64 (the reference's numpy arrays): thread 0 alone touches them, nothing on the hot path is double.
#include "atk_device.h"

namespace ifd {

namespace {

__global__ __launch_bounds__(256) void cw_start_kernel(const float* __restrict__ pc_in, const float* __restrict__ noise,
                                                       float* __restrict__ adv, const int32_t* __restrict__ n_points, int stride) {
    const int b = blockIdx.x, E = atk_rows(n_points, b, stride) * 3;
    const size_t off = (size_t)b * stride * 3;
    for (int i = threadIdx.x; i < E; i += 256) adv[off + i] = noise ? pc_in[off + i] + noise[off + i] : pc_in[off + i];
}

// step_size, bc2, omb1, omb2: adam_step_consts (ifd_internal.h)
__global__ __launch_bounds__(256) void cw_step_kernel(CwState S, const float* __restrict__ grad, const int32_t* __restrict__ pred,
                                                      const float* __restrict__ loss, const int32_t* __restrict__ target,
                                                      float* __restrict__ adv, const float* __restrict__ ori,
                                                      float* __restrict__ last_input, float* __restrict__ info, float step_size,
                                                      float bc2, float omb1, float omb2, float scale,
                                                      const int32_t* __restrict__ n_points, int stride) {
    __shared__ float sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int E = atk_rows(n_points, b, stride) * 3;
    const size_t off = (size_t)b * stride * 3;
    float* A = adv + off;
    const float* O = ori + off;
    const float* G = grad + off;
    float* M = S.m + off;
    float* V = S.v + off;
    float a = 0.f;
    for (int i = tid; i < E; i += 256) { const float d = A[i] - O[i]; a = fmaf(d, d, a); }
    const float dist = sqrtf(atk_block_sum(a, sh));
    const bool hit = pred[b] == target[b];
    const bool rec = hit && dist < S.bestdist[b], orec = hit && dist < S.o_bestdist[b];
    const float w = (float)S.weight[b];
    __syncthreads();
    if (tid == 0) {
        if (rec) { S.bestdist[b] = dist; S.bestscore[b] = pred[b]; }
        if (orec) { S.o_bestdist[b] = dist; S.o_bestscore[b] = pred[b]; }
        if (info) {
            info[(size_t)b * 3] = loss ? loss[b] : 0.f;
            info[(size_t)b * 3 + 1] = dist * w;
            info[(size_t)b * 3 + 2] = dist;
        }
    }
    float* OB = S.o_bestattack + off;
    float* LI = last_input ? last_input + off : nullptr;
    const float c = dist > 0.f ? (scale * w) / dist : 0.f;             // dist == 0: no distance term (the header's deviation)
    for (int i = tid; i < E; i += 256) {
        const float x = A[i];
        if (orec) OB[i] = x;
        if (LI) LI[i] = x;
        const float g = G[i] + c * (x - O[i]);
        float mr = M[i], vr = V[i];
        A[i] = atk_adam(x, g, mr, vr, step_size, bc2, omb1, omb2);
        M[i] = mr;
        V[i] = vr;
    }
}

__global__ __launch_bounds__(256) void cw_adjust_kernel(CwState S, const int32_t* __restrict__ target,
                                                        const int32_t* __restrict__ n_points, int stride) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int E = atk_rows(n_points, b, stride) * 3;
    const size_t off = (size_t)b * stride * 3;
    if (tid == 0) {
        const int bs = S.bestscore[b];
        const double w = S.weight[b];
        double lo = S.lower[b], up = S.upper[b];
        if (bs == target[b] && bs != -1 && S.bestdist[b] <= S.o_bestdist[b]) lo = fmax(lo, w);
        else up = fmin(up, w);
        S.lower[b] = lo;
        S.upper[b] = up;
        S.weight[b] = (lo + up) / 2.0;
        S.bestdist[b] = 1e10f;
        S.bestscore[b] = -1;
    }
    if (S.m)
        for (int i = tid; i < E; i += 256) S.m[off + i] = 0.f;
    if (S.v)
        for (int i = tid; i < E; i += 256) S.v[off + i] = 0.f;
}

__global__ __launch_bounds__(256) void cw_init_kernel(CwState S, int B, float init_weight, float max_weight) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    S.bestdist[b] = 1e10f;
    S.bestscore[b] = -1;
    S.o_bestdist[b] = 1e10f;
    S.o_bestscore[b] = -1;
    S.weight[b] = (double)init_weight;
    S.lower[b] = 0.0;
    S.upper[b] = (double)max_weight;
}

__global__ __launch_bounds__(256) void cw_finish_kernel(CwState S, const float* __restrict__ last_input, float* __restrict__ pc_out,
                                                        int32_t* __restrict__ success, double* __restrict__ bounds, int B,
                                                        const int32_t* __restrict__ n_points, int stride) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int E = atk_rows(n_points, b, stride) * 3;
    const size_t off = (size_t)b * stride * 3;
    const double lo = S.lower[b];
    if (lo == 0.0)
        for (int i = tid; i < E; i += 256) pc_out[off + i] = last_input[off + i];
    if (tid == 0) atk_cw_report(S, b, B, lo, success, bounds);
}

}  // namespace

hipError_t launch_cw_start(const float* pc_in, const float* noise, float* adv, const int32_t* n_points, int B, int stride, hipStream_t s) {
    hipLaunchKernelGGL(cw_start_kernel, dim3(B), dim3(256), 0, s, pc_in, noise, adv, n_points, stride);
    return hipGetLastError();
}

hipError_t launch_cw_init(const CwState& S, int B, float init_weight, float max_weight, hipStream_t s) {
    hipLaunchKernelGGL(cw_init_kernel, dim3((B + 255) / 256), dim3(256), 0, s, S, B, init_weight, max_weight);
    return hipGetLastError();
}

hipError_t launch_cw_step(const CwState& S, const float* grad, const int32_t* pred, const float* loss, const int32_t* target, float* adv,
                          const float* ori, float* last_input, float* info, int t, float lr, float scale, const int32_t* n_points, int B,
                          int stride, hipStream_t s) {
    const AdamStep a = adam_step_consts(t, lr);
    hipLaunchKernelGGL(cw_step_kernel, dim3(B), dim3(256), 0, s, S, grad, pred, loss, target, adv, ori, last_input, info, a.step_size, a.bc2,
                       a.omb1, a.omb2, scale, n_points, stride);
    return hipGetLastError();
}

hipError_t launch_cw_adjust(const CwState& S, const int32_t* target, const int32_t* n_points, int B, int stride, hipStream_t s) {
    hipLaunchKernelGGL(cw_adjust_kernel, dim3(B), dim3(256), 0, s, S, target, n_points, stride);
    return hipGetLastError();
}

hipError_t launch_cw_finish(const CwState& S, const float* last_input, float* pc_out, int32_t* success, double* bounds,
                            const int32_t* n_points, int B, int stride, hipStream_t s) {
    hipLaunchKernelGGL(cw_finish_kernel, dim3(B), dim3(256), 0, s, S, last_input, pc_out, success, bounds, B, n_points, stride);
    return hipGetLastError();
}

}  // namespace ifd
