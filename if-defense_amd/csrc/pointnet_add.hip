// The CW point-adding attack on the PointNet victim (include/ifd_add.h; the reference's baselines/attack/CW/Add.py with
// ChamferDist('adv2ori') or HausdorffDist('adv2ori')) behind ifd_cls_input_grad's forward / backward pass (pointnet_grad.hip).
//
//   add_select_kernel   one workgroup of 256 threads a cloud: the per-point scores in LDS (8 KB at 2048 points), a point's rank by
//                       counting the points in front of it in the total order (score descending, index ascending).  O(n^2) compares,
//                       4.2 M at 2048 points, once per attack.
//   add_step_kernel     one workgroup of 256 threads a cloud, the originals and the added points in LDS (12 bytes a point: 24 KB +
//                       12 KB at 2048 + 1024 points).  Thread t owns the added points t, t + 256, ...: ONE pass over the originals
//                       serves all of them (each LDS read of an original is a broadcast used up to four times) and finds each one's
//                       nearest original in difference form.  Then the set distance (a fixed-tree sum, or a fixed-tree arg-max on
//                       (value, index) pairs), the two records, the distance term's gradient and Adam on the added rows.
//                       Work per cloud: num_add * n_ori distances (2.1 M at 1024 x 2048, 0.5 M at 512 x 1024) - VALU-bound; global
//                       traffic is the cloud once and four arrays of 12 num_add bytes.
//   add_begin_kernel    the originals into the concatenated cloud, n_ori and n_ori + num_add (the counts the victim sees).
//   add_start_kernel    added rows = critical points + noise of a search step.
//   add_finish_kernel   the best added rows or, where lower == 0, the last forwarded ones; success = lower > 0.
#include <climits>

#include "atk_device.h"

namespace ifd {

namespace {

constexpr int ADD_PPT = ADD_MAX_ADD / 256;           // added points a thread owns at the most
constexpr int ADD_SPT = ADD_MAX_ORI / 256;           // scores a thread ranks at the most
static_assert(ADD_MAX_ADD % 256 == 0 && ADD_MAX_ORI % 256 == 0, "whole rows of 256 threads");
static_assert((ADD_MAX_ORI + ADD_MAX_ADD) * 12 + 256 * 8 <= 65536, "static LDS of add_step_kernel");

// the largest (value, index) pair of the workgroup, the lowest index among equal values: a fixed tree; -> sh[0], shi[0]
__device__ __forceinline__ void add_block_argmax(float v, int i, float* sh, int* shi) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    shi[tid] = i;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            const float ov = sh[tid + w];
            const int oi = shi[tid + w];
            if (ov > sh[tid] || (ov == sh[tid] && oi < shi[tid])) { sh[tid] = ov; shi[tid] = oi; }
        }
        __syncthreads();
    }
}

// the cloud's original rows, or -1 where the cloud is outside the header's limits (block-uniform)
__device__ __forceinline__ int add_rows(const int32_t* n_ori, int b, int cat_stride, int num_add) {
    const int n = n_ori ? n_ori[b] : cat_stride - num_add;
    return (n < num_add || n > ADD_MAX_ORI || n > cat_stride - num_add) ? -1 : n;
}

__global__ __launch_bounds__(256) void add_select_kernel(const float* __restrict__ grad, const float* __restrict__ pc,
                                                         const int32_t* __restrict__ n_points, int stride, int num_add,
                                                         float* __restrict__ cri, int32_t* __restrict__ idx) {
    __shared__ float sS[ADD_MAX_ORI];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = n_points ? n_points[b] : stride;
    if (n < num_add || n > ADD_MAX_ORI || n > stride) return;  // the header: left untouched (block-uniform)
    const size_t off = (size_t)b * stride * 3;
    for (int i = tid; i < n; i += 256) {
#pragma clang fp contract(off)
        const float gx = grad[off + 3 * i], gy = grad[off + 3 * i + 1], gz = grad[off + 3 * i + 2];
        const float xx = gx * gx, yy = gy * gy, zz = gz * gz;
        const float xy = xx + yy;
        sS[i] = xy + zz;
    }
    __syncthreads();
    float s[ADD_SPT];
    int rank[ADD_SPT];
#pragma unroll
    for (int r = 0; r < ADD_SPT; ++r) {
        const int i = r * 256 + tid;
        s[r] = i < n ? sS[i] : 0.f;
        rank[r] = 0;
    }
    for (int j = 0; j < n; ++j) {
        const float sj = sS[j];                                 // broadcast read
#pragma unroll
        for (int r = 0; r < ADD_SPT; ++r) rank[r] += (sj > s[r] || (sj == s[r] && j < r * 256 + tid)) ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < ADD_SPT; ++r) {
        const int i = r * 256 + tid;
        if (i < n && rank[r] < num_add) {                       // a NaN score ranks 0 and may collide: still inside the arrays
            const size_t o = ((size_t)b * num_add + rank[r]) * 3;
            cri[o] = pc[off + 3 * i];
            cri[o + 1] = pc[off + 3 * i + 1];
            cri[o + 2] = pc[off + 3 * i + 2];
            if (idx) idx[(size_t)b * num_add + rank[r]] = i;
        }
    }
}

// step_size, bc2, omb1, omb2: adam_step_consts (ifd_internal.h)
__global__ __launch_bounds__(256) void add_step_kernel(int kind, CwState S, const float* __restrict__ grad, const int32_t* __restrict__ pred,
                                                       const float* __restrict__ loss, const int32_t* __restrict__ target,
                                                       float* __restrict__ cat, const int32_t* __restrict__ n_ori,
                                                       float* __restrict__ last_input, float* __restrict__ info, AddDiag D,
                                                       float step_size, float bc2, float omb1, float omb2, float scale, int cat_stride,
                                                       int num_add) {
    __shared__ float sO[ADD_MAX_ORI * 3];
    __shared__ float sA[ADD_MAX_ADD * 3];
    __shared__ float sh[256];
    __shared__ int shi[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = add_rows(n_ori, b, cat_stride, num_add);
    if (n < 0) return;                                          // the header: left untouched (block-uniform)
    const size_t coff = (size_t)b * cat_stride * 3, aoff = (size_t)b * num_add * 3;
    float* X = cat + coff + (size_t)n * 3;                      // the added rows
    for (int i = tid; i < n * 3; i += 256) sO[i] = cat[coff + i];
    for (int i = tid; i < num_add * 3; i += 256) sA[i] = X[i];
    __syncthreads();

    // ---- 1. the nearest original of every owned added point, one pass over the originals ----
    float ax[ADD_PPT], ay[ADD_PPT], az[ADD_PPT], best[ADD_PPT];
    int bi[ADD_PPT];
#pragma unroll
    for (int r = 0; r < ADD_PPT; ++r) {
        const int p = min(r * 256 + tid, num_add - 1);          // a slot beyond num_add repeats the last point; never used
        ax[r] = sA[3 * p]; ay[r] = sA[3 * p + 1]; az[r] = sA[3 * p + 2];
        best[r] = INFINITY;
        bi[r] = 0;
    }
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
        const float ox = sO[3 * j], oy = sO[3 * j + 1], oz = sO[3 * j + 2];
#pragma unroll
        for (int r = 0; r < ADD_PPT; ++r) {
            const float dx = ax[r] - ox, dy = ay[r] - oy, dz = az[r] - oz;
            const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (d < best[r]) { best[r] = d; bi[r] = j; }        // strict: the lowest index among equal distances
        }
    }

    // ---- 2. the set distance ----
    float dist;
    int far = -1;
    if (kind == ADD_CHAMFER) {
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < ADD_PPT; ++r) part += (r * 256 + tid < num_add) ? best[r] : 0.f;
        dist = atk_block_sum(part, sh) / (float)num_add;
    } else {
        float mv = -INFINITY;
        int mi = INT_MAX;
#pragma unroll
        for (int r = 0; r < ADD_PPT; ++r)
            if (r * 256 + tid < num_add && best[r] > mv) { mv = best[r]; mi = r * 256 + tid; }
        add_block_argmax(mv, mi, sh, shi);
        dist = sh[0];
        far = shi[0];
    }

    // ---- 3. the records: every thread reads the old values, thread 0 writes the new ones behind a barrier ----
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
        if (D.far) D.far[b] = far;
    }

    // ---- 4, 5. the gradient and Adam, per owned added point ----
    const float coef = kind == ADD_CHAMFER ? (scale * w) * (2.f / (float)num_add) : (scale * w) * 2.f;
    const float* G = grad + coff + (size_t)n * 3;
    float* M = S.m + aoff;
    float* V = S.v + aoff;
    float* OB = S.o_bestattack + aoff;
    float* LI = last_input ? last_input + aoff : nullptr;
#pragma unroll
    for (int r = 0; r < ADD_PPT; ++r) {
        const int p = r * 256 + tid;
        if (p >= num_add) continue;
        const bool active = kind == ADD_CHAMFER || p == far;
        if (D.nn_ori) D.nn_ori[(size_t)b * num_add + p] = bi[r];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int i = 3 * p + c;
            const float x = sA[i];
            if (orec) OB[i] = x;
            if (LI) LI[i] = x;
            const float d = x - sO[3 * bi[r] + c];
            if (D.dist_grad) D.dist_grad[aoff + i] = active ? coef * d : 0.f;
            const float g = active ? __builtin_fmaf(coef, d, G[i]) : G[i];
            float mr = M[i], vr = V[i];
            X[i] = atk_adam(x, g, mr, vr, step_size, bc2, omb1, omb2);
            M[i] = mr;
            V[i] = vr;
        }
    }
}

__global__ __launch_bounds__(256) void add_begin_kernel(const float* __restrict__ pc_in, const int32_t* __restrict__ n_points, int stride,
                                                        int out_stride, int num_add, float* __restrict__ pc_out,
                                                        int32_t* __restrict__ n_ori, int32_t* __restrict__ n_cat) {
    const int b = blockIdx.x, n = n_points ? n_points[b] : stride;
    const size_t in = (size_t)b * stride * 3, out = (size_t)b * out_stride * 3;
    for (int i = threadIdx.x; i < n * 3; i += 256) pc_out[out + i] = pc_in[in + i];
    if (threadIdx.x == 0) { n_ori[b] = n; n_cat[b] = n + num_add; }
}

__global__ __launch_bounds__(256) void add_start_kernel(const float* __restrict__ cri, const float* __restrict__ noise,
                                                        const int32_t* __restrict__ n_cat, int out_stride, int num_add,
                                                        float* __restrict__ pc_out) {
    const int b = blockIdx.x;
    const size_t a = (size_t)b * num_add * 3, out = ((size_t)b * out_stride + (n_cat[b] - num_add)) * 3;
    for (int i = threadIdx.x; i < num_add * 3; i += 256) pc_out[out + i] = noise ? cri[a + i] + noise[a + i] : cri[a + i];
}

__global__ __launch_bounds__(256) void add_finish_kernel(CwState S, const float* __restrict__ last_input, const int32_t* __restrict__ n_cat,
                                                         int out_stride, int num_add, float* __restrict__ pc_out,
                                                         int32_t* __restrict__ success, double* __restrict__ bounds, int B) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t a = (size_t)b * num_add * 3, out = ((size_t)b * out_stride + (n_cat[b] - num_add)) * 3;
    const double lo = S.lower[b];
    const float* src = lo == 0.0 ? last_input : S.o_bestattack;
    for (int i = tid; i < num_add * 3; i += 256) pc_out[out + i] = src[a + i];
    if (tid == 0) atk_cw_report(S, b, B, lo, success, bounds);
}

}  // namespace

hipError_t launch_add_select(const float* grad, const float* pc, const int32_t* n_points, int B, int stride, int num_add, float* cri,
                             int32_t* idx, hipStream_t s) {
    hipLaunchKernelGGL(add_select_kernel, dim3(B), dim3(256), 0, s, grad, pc, n_points, stride, num_add, cri, idx);
    return hipGetLastError();
}

hipError_t launch_add_step(int kind, const CwState& S, const float* grad, const int32_t* pred, const float* loss, const int32_t* target,
                           float* cat, const int32_t* n_ori, float* last_input, float* info, const AddDiag& D, int t, float lr, float scale,
                           int B, int cat_stride, int num_add, hipStream_t s) {
    const AdamStep a = adam_step_consts(t, lr);
    hipLaunchKernelGGL(add_step_kernel, dim3(B), dim3(256), 0, s, kind, S, grad, pred, loss, target, cat, n_ori, last_input, info, D,
                       a.step_size, a.bc2, a.omb1, a.omb2, scale, cat_stride, num_add);
    return hipGetLastError();
}

hipError_t launch_add_begin(const float* pc_in, const int32_t* n_points, int B, int stride, int out_stride, int num_add, float* pc_out,
                            int32_t* n_ori, int32_t* n_cat, hipStream_t s) {
    hipLaunchKernelGGL(add_begin_kernel, dim3(B), dim3(256), 0, s, pc_in, n_points, stride, out_stride, num_add, pc_out, n_ori, n_cat);
    return hipGetLastError();
}

hipError_t launch_add_start(const float* cri, const float* noise, const int32_t* n_cat, int B, int out_stride, int num_add, float* pc_out,
                            hipStream_t s) {
    hipLaunchKernelGGL(add_start_kernel, dim3(B), dim3(256), 0, s, cri, noise, n_cat, out_stride, num_add, pc_out);
    return hipGetLastError();
}

hipError_t launch_add_finish(const CwState& S, const float* last_input, const int32_t* n_cat, int B, int out_stride, int num_add,
                             float* pc_out, int32_t* success, double* bounds, hipStream_t s) {
    hipLaunchKernelGGL(add_finish_kernel, dim3(B), dim3(256), 0, s, S, last_input, n_cat, out_stride, num_add, pc_out, success, bounds, B);
    return hipGetLastError();
}

}  // namespace ifd
