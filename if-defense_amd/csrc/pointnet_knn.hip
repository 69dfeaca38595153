// The kNN attack on the PointNet victim (include/ifd_knn.h; the reference's baselines/attack/CW/kNN.py with ChamferkNNDist and
// ProjectInnerClipLinf) behind ifd_cls_input_grad's forward / backward pass (pointnet_grad.hip).
//
//   knn_step_kernel     one workgroup of 256 threads a cloud, the cloud and its original in LDS (12 bytes a point: 48 KB at 2048
//                       points).  Thread t owns the points t, t + 256, ...: for each of them ONE brute-force pass over all points finds
//                       the nearest original and the five nearest other adversarial points (difference form, knn_device.h Top5).  Then
//                       mean and unbiased std of the per-point values (two fixed-tree sums), the mask, the gradient, Adam, project and
//                       clip.  The neighbour terms a point RECEIVES (index_points' backward, a scatter in autograd) are a gather: the
//                       masked points and their five indices are compacted into LDS in index order - a ballot per wave and row, a
//                       prefix over the at most 32 (row, wave) counts - and the owner of j walks that list.  A list longer than the LDS
//                       room for it is walked in chunks, in the same order.  No atomics, no float sum whose order could vary.
//                       Work per cloud: 2 n^2 distances (8.4 M at 2048 points) - VALU-bound; global traffic is 8 arrays of 12 n bytes.
//   knn_clip_kernel     the projection and the clip alone, the step's device function.
#include "atk_device.h"
#include "knn_device.h"

namespace ifd {

namespace {

constexpr int KNN_PPT = KNN_MAX_POINTS / 256;        // points a thread owns at the most
constexpr int KNN_LIST_CAP = 1024;                   // masked points per chunk of the gather list (3 words each: 12 KB)
static_assert(KNN_MAX_POINTS % 256 == 0 && KNN_MAX_POINTS <= 65536, "the gather list holds 16-bit indices");
static_assert(2 * KNN_MAX_POINTS * 12 + KNN_LIST_CAP * 12 + 256 * 4 + KNN_PPT * 4 * 4 <= 65536, "static LDS of knn_step_kernel");

// ProjectInnerClipLinf on one point (clip_utils.py:83-112, 54-59): p the point, o its original, nrm its normal or nullptr
__device__ __forceinline__ void knn_project_clip_point(float (&p)[3], const float (&o)[3], const float* __restrict__ nrm, float budget) {
    float dx = p[0] - o[0], dy = p[1] - o[1], dz = p[2] - o[2];
    if (nrm) {
        const float nx = nrm[0], ny = nrm[1], nz = nrm[2];
        const float dn = dx * nx + dy * ny + dz * nz;
        if (dn < 0.f) {
            const float vx = ny * dz - nz * dy, vy = nz * dx - nx * dz, vz = nx * dy - ny * dx;        // vng = n x d
            const float rx = vy * nz - vz * ny, ry = vz * nx - vx * nz, rz = vx * ny - vy * nx;        // vref = vng x n
            const float vn = sqrtf(vx * vx + vy * vy + vz * vz);
            const float rn = sqrtf(rx * rx + ry * ry + rz * rz) + 1e-9f;
            const bool opposite = vn < 1e-6f;
            dx = opposite ? 0.f : dx * rx / rn;                                                       // element-wise, as the reference
            dy = opposite ? 0.f : dy * ry / rn;
            dz = opposite ? 0.f : dz * rz / rn;
        }
    }
    const float norm = sqrtf(dx * dx + dy * dy + dz * dz);
    const float sf = fminf(budget / (norm + 1e-9f), 1.f);
    p[0] = o[0] + dx * sf;
    p[1] = o[1] + dy * sf;
    p[2] = o[2] + dz * sf;
}

struct KnnHyper {
    float c_cd, c_knn;       // 2 w1, 2 w2 / 5: the gradient's two factors
    float w1, w2, alpha, budget;
};

// step_size, bc2, omb1, omb2: adam_step_consts (ifd_internal.h)
__global__ __launch_bounds__(256) void knn_step_kernel(const float* __restrict__ grad, const float* __restrict__ loss, float* __restrict__ adv,
                                                       const float* __restrict__ ori, const float* __restrict__ normal,
                                                       float* __restrict__ m, float* __restrict__ v, KnnDiag D, KnnHyper H, float step_size,
                                                       float bc2, float omb1, float omb2, float scale,
                                                       const int32_t* __restrict__ n_points, int stride) {
    __shared__ float sA[KNN_MAX_POINTS * 3];
    __shared__ float sO[KNN_MAX_POINTS * 3];
    __shared__ unsigned int sList[KNN_LIST_CAP * 3];          // { p | i0 << 16, i1 | i2 << 16, i3 | i4 << 16 } of a masked point
    __shared__ float sh[256];
    __shared__ int sCnt[KNN_PPT * 4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = atk_rows(n_points, b, stride);
    if (n < 6) return;                                          // the header: left untouched (block-uniform)
    const size_t off = (size_t)b * stride * 3;
    float* A = adv + off;
    const float* O = ori + off;
    for (int i = tid; i < n * 3; i += 256) { sA[i] = A[i]; sO[i] = O[i]; }
    __syncthreads();

    // ---- 1. the two scans of every owned point, in one pass over j ----
    int nno[KNN_PPT];                                           // the Chamfer argmin
    unsigned int ia[KNN_PPT], ib[KNN_PPT], ic[KNN_PPT];         // NN5, packed 16 bits each: i0 | i1 << 16, i2 | i3 << 16, i4
    float val[KNN_PPT], cdm[KNN_PPT];
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) {
        const int p = r * 256 + tid;
        nno[r] = 0; ia[r] = ib[r] = ic[r] = 0u; val[r] = 0.f; cdm[r] = 0.f;
        if (p < n) {
            const float ax = sA[3 * p], ay = sA[3 * p + 1], az = sA[3 * p + 2];
            float best = INFINITY;
            int bi = 0;
            Top5 t;
            top5_init(t);
#pragma unroll 4
            for (int j = 0; j < n; ++j) {
                const float ox = ax - sO[3 * j], oy = ay - sO[3 * j + 1], oz = az - sO[3 * j + 2];
                const float ex = sA[3 * j] - ax, ey = sA[3 * j + 1] - ay, ez = sA[3 * j + 2] - az;
                const float dc = fmaf(oz, oz, fmaf(oy, oy, ox * ox));
                float da = fmaf(ez, ez, fmaf(ey, ey, ex * ex));
                da = (j == p) ? INFINITY : da;
                if (dc < best) { best = dc; bi = j; }          // strict: the lowest index among equal distances
                top5_insert(t, da, j);
            }
            nno[r] = bi;
            cdm[r] = best;
            ia[r] = (unsigned int)t.i0 | ((unsigned int)t.i1 << 16);
            ib[r] = (unsigned int)t.i2 | ((unsigned int)t.i3 << 16);
            ic[r] = (unsigned int)t.i4;
            val[r] = ((((t.d0 + t.d1) + t.d2) + t.d3) + t.d4) / 5.f;
        }
    }

    // ---- 2. mean, unbiased std, threshold, mask ----
    float part = 0.f;
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) part += (r * 256 + tid < n) ? val[r] : 0.f;
    const float mean = atk_block_sum(part, sh) / (float)n;
    part = 0.f;
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) {
        const float c = val[r] - mean;
        part += (r * 256 + tid < n) ? c * c : 0.f;
    }
    const float sd = sqrtf(atk_block_sum(part, sh) / (float)(n - 1));
    const float thr = mean + H.alpha * sd;
    unsigned int mbits = 0u;
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) mbits |= ((r * 256 + tid < n) && val[r] > thr) ? (1u << r) : 0u;

    if (D.info) {                                               // block-uniform
        float pc = 0.f, pk = 0.f;
#pragma unroll
        for (int r = 0; r < KNN_PPT; ++r) {
            pc += (r * 256 + tid < n) ? cdm[r] : 0.f;
            pk += ((mbits >> r) & 1u) ? val[r] : 0.f;
        }
        const float cd = atk_block_sum(pc, sh) / (float)n;
        const float kn = atk_block_sum(pk, sh) / (float)n;
        if (tid == 0) {
            float* I = D.info + (size_t)b * 4;
            I[0] = loss ? loss[b] : 0.f;
            I[1] = cd;
            I[2] = kn;
            I[3] = (float)n * (H.w1 * cd + H.w2 * kn);
        }
    }

    // ---- 3a. the masked points' place in the gather list: index order = (row, wave, lane) ----
    int pos[KNN_PPT];
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) {
        const unsigned long long bal = __ballot((mbits >> r) & 1u);
        pos[r] = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) sCnt[r * 4 + wave] = __popcll(bal);
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w == wave) pos[r] += total;
            total += sCnt[r * 4 + w];
        }
    }

    // ---- 3b. what every owned point receives from the masked points that count it among their five ----
    float acc[KNN_PPT][3];
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;
    for (int base = 0; base < total; base += KNN_LIST_CAP) {   // block-uniform trip count
        __syncthreads();
#pragma unroll
        for (int r = 0; r < KNN_PPT; ++r) {
            const int e = pos[r] - base;
            if (((mbits >> r) & 1u) && e >= 0 && e < KNN_LIST_CAP) {
                sList[3 * e] = (unsigned int)(r * 256 + tid) | ((ia[r] & 0xffffu) << 16);
                sList[3 * e + 1] = (ia[r] >> 16) | ((ib[r] & 0xffffu) << 16);
                sList[3 * e + 2] = (ib[r] >> 16) | (ic[r] << 16);
            }
        }
        __syncthreads();
        const int cnt = min(KNN_LIST_CAP, total - base);
        for (int e = 0; e < cnt; ++e) {
            const unsigned int w0 = sList[3 * e], w1 = sList[3 * e + 1], w2 = sList[3 * e + 2];       // broadcast reads
            const int pp = (int)(w0 & 0xffffu);
            const int q0 = (int)(w0 >> 16), q1 = (int)(w1 & 0xffffu), q2 = (int)(w1 >> 16), q3 = (int)(w2 & 0xffffu), q4 = (int)(w2 >> 16);
            const float px = sA[3 * pp], py = sA[3 * pp + 1], pz = sA[3 * pp + 2];
#pragma unroll
            for (int r = 0; r < KNN_PPT; ++r) {
                const int j = r * 256 + tid;                    // j >= n matches nothing: the list holds indices below n
                if (j == q0 || j == q1 || j == q2 || j == q3 || j == q4) {
                    acc[r][0] += sA[3 * j] - px;
                    acc[r][1] += sA[3 * j + 1] - py;
                    acc[r][2] += sA[3 * j + 2] - pz;
                }
            }
        }
    }

    // ---- 3c - 5. the gradient, Adam, project and clip, per owned point ----
    const float* G = grad + off;
    float* M = m + off;
    float* V = v + off;
#pragma unroll
    for (int r = 0; r < KNN_PPT; ++r) {
        const int j = r * 256 + tid;
        if (j >= n) continue;
        const bool mk = (mbits >> r) & 1u;
        const int q[5] = {(int)(ia[r] & 0xffffu), (int)(ia[r] >> 16), (int)(ib[r] & 0xffffu), (int)(ib[r] >> 16), (int)ic[r]};
        float x[3], o[3], gd[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            x[c] = sA[3 * j + c];
            o[c] = sO[3 * j + c];
            float own = 0.f;
            if (mk) {
#pragma unroll
                for (int k = 0; k < 5; ++k) own += x[c] - sA[3 * q[k] + c];
            }
            gd[c] = scale * (H.c_cd * (x[c] - sO[3 * nno[r] + c]) + H.c_knn * (own + acc[r][c]));
        }
        if (D.dist_grad) {
#pragma unroll
            for (int c = 0; c < 3; ++c) D.dist_grad[off + 3 * j + c] = gd[c];
        }
        if (D.nn_ori) D.nn_ori[(size_t)b * stride + j] = nno[r];
        if (D.mask) D.mask[(size_t)b * stride + j] = mk ? 1 : 0;
        if (D.nn5) {
#pragma unroll
            for (int k = 0; k < 5; ++k) D.nn5[((size_t)b * stride + j) * 5 + k] = q[k];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int i = 3 * j + c;
            const float g = G[i] + gd[c];
            // atk_adam (atk_device.h) term by term: calling it here compiles this kernel to other register numbers
            float mr = M[i], vr = V[i];
            mr = __builtin_fmaf(g - mr, omb1, mr);
            vr = __builtin_fmaf(omb2 * g, g, vr * 0.999f);
            const float denom = sqrtf(vr) / bc2 + 1e-8f;
            x[c] = __builtin_fmaf(-step_size, mr / denom, x[c]);
            M[i] = mr;
            V[i] = vr;
        }
        knn_project_clip_point(x, o, normal ? normal + off + 3 * j : nullptr, H.budget);
#pragma unroll
        for (int c = 0; c < 3; ++c) A[3 * j + c] = x[c];
    }
}

__global__ __launch_bounds__(256) void knn_clip_kernel(float* __restrict__ adv, const float* __restrict__ ori, const float* __restrict__ normal,
                                                       float budget, const int32_t* __restrict__ n_points, int stride) {
    const int b = blockIdx.x, n = atk_rows(n_points, b, stride);
    const size_t off = (size_t)b * stride * 3;
    for (int j = threadIdx.x; j < n; j += 256) {
        float x[3], o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { x[c] = adv[off + 3 * j + c]; o[c] = ori[off + 3 * j + c]; }
        knn_project_clip_point(x, o, normal ? normal + off + 3 * j : nullptr, budget);
#pragma unroll
        for (int c = 0; c < 3; ++c) adv[off + 3 * j + c] = x[c];
    }
}

}  // namespace

hipError_t launch_knn_step(const float* grad, const float* loss, float* adv, const float* ori, const float* normal, float* m, float* v,
                           const KnnDiag& D, float chamfer_weight, float knn_weight, float alpha, float budget, int t, float lr, float scale,
                           const int32_t* n_points, int B, int stride, hipStream_t s) {
    const AdamStep a = adam_step_consts(t, lr);
    const KnnHyper H{2.f * chamfer_weight, 2.f * knn_weight / 5.f, chamfer_weight, knn_weight, alpha, budget};
    hipLaunchKernelGGL(knn_step_kernel, dim3(B), dim3(256), 0, s, grad, loss, adv, ori, normal, m, v, D, H, a.step_size, a.bc2,
                       a.omb1, a.omb2, scale, n_points, stride);
    return hipGetLastError();
}

hipError_t launch_knn_clip(float* adv, const float* ori, const float* normal, float budget, const int32_t* n_points, int B, int stride,
                           hipStream_t s) {
    hipLaunchKernelGGL(knn_clip_kernel, dim3(B), dim3(256), 0, s, adv, ori, normal, budget, n_points, stride);
    return hipGetLastError();
}

}  // namespace ifd
