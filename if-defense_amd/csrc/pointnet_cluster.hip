// The CW cluster-adding attack on the PointNet victim (include/ifd_cluster.h; the reference's baselines/attack/CW/Add_Cluster.py with
// FarChamferDist(num_add, 'adv2ori', 0.1)) behind ifd_cls_input_grad's forward / backward pass (pointnet_grad.hip).  The start and
// the end of the whole attack are pointnet_add.hip's add_begin / add_start / add_finish kernels.
//
//   cluster_dbscan_kernel   one workgroup of 256 threads a cloud of up to 256 points, thread i owning point i (DbscanLds, 6 KB).
//                           1. Row i of the adjacency as 256 bits in the owner's registers - no other thread reads it - and the
//                              neighbour count; the core points as a bit mask in LDS; the row is then cut down to core neighbours.
//                           2. Min-label propagation over the core graph, double-buffered in LDS, with one pointer jump a round
//                              (label = L[min over core neighbours]); a round that changes nothing ends it.  Labels only fall and
//                              stay indices of core points of the own component, so the fixed point is the component's lowest
//                              core index whatever the number of rounds.
//                           3. The roots (label == own index) ranked by counting the roots in front of them: the cluster numbers.
//                           4. Core points take their root's number, border points the lowest number among their core neighbours.
//   cluster_step_kernel     one workgroup of 256 threads a cloud, the originals and the added rows in LDS (ClusterStepLds, 57 KB).
//                           Thread t owns the added rows t, t + 256, ...  The Chamfer part is add_step_kernel's, line for line.
//                           The far part: every owned row j walks the rows i of its cluster in ascending order (cl_num_p LDS
//                           reads serve up to four owned rows) and keeps max n2 and the lowest arg-max i; the cluster's arg-max
//                           over j is one thread's ascending scan of those cl_num_p results; far is every thread's serial sum of
//                           the clusters' roots, kept in float64 and rounded once.  Work per cloud: A * n_ori + A * cl_num_p
//                           distances - 3 x 32^2 beside 96 x 1024 at the reference's sizes.
#include <climits>

#include "atk_device.h"
#include "lds_layout.h"

namespace ifd {

namespace {

constexpr int CL_PPT = ADD_MAX_ADD / CLUSTER_THREADS;       // added rows a thread owns at the most
constexpr int DB_WORDS = (int)DbscanLds::WORDS;

// the header's d2, term by term
__device__ __forceinline__ float dbscan_d2(float x, float y, float z, float qx, float qy, float qz) {
#pragma clang fp contract(off)
    const float dx = x - qx, dy = y - qy, dz = z - qz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    return xy + zz;
}

__global__ __launch_bounds__(CLUSTER_THREADS) void cluster_dbscan_kernel(const float* __restrict__ pts, const int32_t* __restrict__ n_pts,
                                                                         int stride, float eps2, int min_samples,
                                                                         int32_t* __restrict__ labels, int32_t* __restrict__ n_clusters) {
    extern __shared__ float lds_f[];
    float* sX = LDS_AT(float, lds_f, DbscanLds::X);
    unsigned* sCore = LDS_AT(unsigned, lds_f, DbscanLds::CORE);
    int* sLab = LDS_AT(int, lds_f, DbscanLds::LAB);
    int* sCid = LDS_AT(int, lds_f, DbscanLds::CID);
    int* sFlag = LDS_AT(int, lds_f, DbscanLds::FLAG);
    constexpr int N = (int)DbscanLds::N;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = n_pts ? n_pts[b] : stride;
    if (n < 1 || n > N || n > stride) return;                   // the header: left untouched (block-uniform)
    const size_t off = (size_t)b * stride * 3;
    for (int i = tid; i < n * 3; i += CLUSTER_THREADS) sX[i] = pts[off + i];
    if (tid < DB_WORDS) sCore[tid] = 0u;
    __syncthreads();

    // ---- 1. my neighbours, the core points ----
    const bool in = tid < n;
    const int me = in ? tid : 0;
    const float x = sX[3 * me], y = sX[3 * me + 1], z = sX[3 * me + 2];
    unsigned row[DB_WORDS];
    int count = 0;
#pragma unroll
    for (int w = 0; w < DB_WORDS; ++w) {
        unsigned word = 0u;
        const int hi = min(32, n - 32 * w);
        for (int k = 0; k < hi; ++k) {
            const int j = 32 * w + k;
            if (dbscan_d2(x, y, z, sX[3 * j], sX[3 * j + 1], sX[3 * j + 2]) <= eps2) word |= 1u << k;      // broadcast reads
        }
        row[w] = in ? word : 0u;
        count += __popc(row[w]);
    }
    const bool core = in && count >= min_samples;
    if (core) atomicOr(&sCore[tid >> 5], 1u << (tid & 31));     // integer: the order does not matter
    __syncthreads();
#pragma unroll
    for (int w = 0; w < DB_WORDS; ++w) row[w] &= sCore[w];      // core neighbours only, from here on

    // ---- 2. min-label propagation over the core graph ----
    int lab = core ? tid : INT_MAX;
    sLab[tid] = lab;
    int cur = 0;
    for (;;) {
        __syncthreads();                                        // buffer `cur` is written, last round's flag is read
        if (tid == 0) sFlag[0] = 0;
        __syncthreads();
        const int* L = sLab + cur * N;
        int best = lab;
        if (core) {
#pragma unroll
            for (int w = 0; w < DB_WORDS; ++w) {
                unsigned word = row[w];
                while (word) {
                    const int k = __ffs((int)word) - 1;
                    word &= word - 1u;
                    best = min(best, L[32 * w + k]);
                }
            }
            best = min(best, L[best]);                          // a core point of my component: its label is one, too
        }
        if (best < lab) sFlag[0] = 1;
        lab = best;
        sLab[(cur ^ 1) * N + tid] = lab;
        __syncthreads();
        if (!sFlag[0]) break;                                   // block-uniform: both buffers now hold the fixed point
        cur ^= 1;
    }

    // ---- 3. the roots in index order are the clusters 0, 1, ... ----
    const int* L = sLab + (cur ^ 1) * N;
    int* sRoot = sLab + cur * N;                                // equal to L and no longer needed
    __syncthreads();
    sRoot[tid] = (core && lab == tid) ? 1 : 0;
    __syncthreads();
    int before = 0;
    for (int j = 0; j < tid; ++j) before += sRoot[j];
    sCid[tid] = before;
    if (tid == CLUSTER_THREADS - 1 && n_clusters) n_clusters[b] = before + sRoot[tid];
    __syncthreads();

    // ---- 4. the labels ----
    if (!in) return;
    int out;
    if (core) {
        out = sCid[lab];
    } else {
        out = INT_MAX;
#pragma unroll
        for (int w = 0; w < DB_WORDS; ++w) {
            unsigned word = row[w];
            while (word) {
                const int k = __ffs((int)word) - 1;
                word &= word - 1u;
                out = min(out, sCid[L[32 * w + k]]);
            }
        }
        if (out == INT_MAX) out = -1;
    }
    labels[(size_t)b * stride + tid] = out;
}

// the header's dist and info[1], term by term
__device__ __forceinline__ float cluster_dist(float far, float cd) {
#pragma clang fp contract(off)
    const float c = cd * 0.1f;
    return far + c;
}
__device__ __forceinline__ float cluster_dist_loss(float far, float cd, float w) {
#pragma clang fp contract(off)
    const float f = far * w, c = cd * w;
    const float c1 = c * 0.1f;
    return f + c1;
}

// step_size, bc2, omb1, omb2: adam_step_consts (ifd_internal.h)
__global__ __launch_bounds__(CLUSTER_THREADS) void cluster_step_kernel(CwState S, const float* __restrict__ grad, const int32_t* __restrict__ pred,
                                                                       const float* __restrict__ loss, const int32_t* __restrict__ target,
                                                                       float* __restrict__ cat, const int32_t* __restrict__ n_ori,
                                                                       float* __restrict__ last_input, float* __restrict__ info, ClusterDiag D,
                                                                       float step_size, float bc2, float omb1, float omb2, float scale,
                                                                       int cat_stride, int num_add, int P) {
    extern __shared__ float lds_f[];
    float* sO = LDS_AT(float, lds_f, ClusterStepLds::O);
    float* sA = LDS_AT(float, lds_f, ClusterStepLds::A);
    float* sPN = LDS_AT(float, lds_f, ClusterStepLds::PN);
    int* sPI = LDS_AT(int, lds_f, ClusterStepLds::PI);
    int* sCI = LDS_AT(int, lds_f, ClusterStepLds::CI);
    int* sCJ = LDS_AT(int, lds_f, ClusterStepLds::CJ);
    float* sCF = LDS_AT(float, lds_f, ClusterStepLds::CF);
    float* sh = LDS_AT(float, lds_f, ClusterStepLds::SH);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int A = num_add * P;
    const int n = n_ori ? n_ori[b] : cat_stride - A;
    if (n < 1 || n > ADD_MAX_ORI || n > cat_stride - A) return; // the header: left untouched (block-uniform)
    const size_t coff = (size_t)b * cat_stride * 3, aoff = (size_t)b * A * 3;
    float* X = cat + coff + (size_t)n * 3;                      // the added rows
    for (int i = tid; i < n * 3; i += CLUSTER_THREADS) sO[i] = cat[coff + i];
    for (int i = tid; i < A * 3; i += CLUSTER_THREADS) sA[i] = X[i];
    __syncthreads();

    // ---- 1. the nearest original of every owned added row, one pass over the originals (add_step_kernel's) ----
    float ax[CL_PPT], ay[CL_PPT], az[CL_PPT], best[CL_PPT];
    int bi[CL_PPT], base[CL_PPT];
#pragma unroll
    for (int r = 0; r < CL_PPT; ++r) {
        const int p = min(r * CLUSTER_THREADS + tid, A - 1);    // a slot beyond A repeats the last row; never used
        ax[r] = sA[3 * p]; ay[r] = sA[3 * p + 1]; az[r] = sA[3 * p + 2];
        best[r] = INFINITY;
        bi[r] = 0;
        base[r] = (p / P) * P;                                  // the first row of p's cluster
    }
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
        const float ox = sO[3 * j], oy = sO[3 * j + 1], oz = sO[3 * j + 2];
#pragma unroll
        for (int r = 0; r < CL_PPT; ++r) {
            const float dx = ax[r] - ox, dy = ay[r] - oy, dz = az[r] - oz;
            const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (d < best[r]) { best[r] = d; bi[r] = j; }        // strict: the lowest index among equal distances
        }
    }
    float part = 0.f;
#pragma unroll
    for (int r = 0; r < CL_PPT; ++r) part += (r * CLUSTER_THREADS + tid < A) ? best[r] : 0.f;
    const float cd = atk_block_sum(part, sh) / (float)A;

    // ---- 2. the far part: row j against the rows i of its cluster, ascending i, strict > (the lowest i among equals) ----
    float fn[CL_PPT];
    int fi[CL_PPT];
#pragma unroll
    for (int r = 0; r < CL_PPT; ++r) { fn[r] = -INFINITY; fi[r] = base[r]; }
    for (int ii = 0; ii < P; ++ii) {
#pragma unroll
        for (int r = 0; r < CL_PPT; ++r) {
            const int i = base[r] + ii;
            const float dx = (ax[r] - sA[3 * i]) + 1e-7f, dy = (ay[r] - sA[3 * i + 1]) + 1e-7f, dz = (az[r] - sA[3 * i + 2]) + 1e-7f;
            const float n2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (n2 > fn[r]) { fn[r] = n2; fi[r] = i; }
        }
    }
#pragma unroll
    for (int r = 0; r < CL_PPT; ++r) {
        const int p = r * CLUSTER_THREADS + tid;
        if (p < A) { sPN[p] = fn[r]; sPI[p] = fi[r]; }
    }
    __syncthreads();
    for (int c = tid; c < num_add; c += CLUSTER_THREADS) {      // ascending j, strict >: the lowest j among equals
        float mv = -INFINITY;
        int mj = c * P;
        for (int j = c * P; j < (c + 1) * P; ++j) {
            const float v = sPN[j];
            if (v > mv) { mv = v; mj = j; }
        }
        const float f = sqrtf(mv);
        sCI[c] = sPI[mj];
        sCJ[c] = mj;
        sCF[c] = f;
        if (D.far_i) D.far_i[(size_t)b * num_add + c] = sPI[mj];
        if (D.far_j) D.far_j[(size_t)b * num_add + c] = mj;
        if (D.far_val) D.far_val[(size_t)b * num_add + c] = f;
    }
    __syncthreads();
    double fsum = 0.0;                                          // in float64: 512 roots summed serially in float32 lose 1e-5 of 60
    for (int c = 0; c < num_add; ++c) fsum += (double)sCF[c];   // every thread the same serial sum (broadcast reads)
    const float far = (float)fsum;
    const float dist = cluster_dist(far, cd);

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
            info[(size_t)b * 3 + 1] = cluster_dist_loss(far, cd, w);
            info[(size_t)b * 3 + 2] = dist;
        }
    }

    // ---- 4, 5. the gradient and Adam, per owned added row ----
    const float c_far = scale * w;
    const float c_cd = (c_far * 0.1f) * (2.f / (float)A);
    const float* G = grad + coff + (size_t)n * 3;
    float* M = S.m + aoff;
    float* V = S.v + aoff;
    float* OB = S.o_bestattack + aoff;
    float* LI = last_input ? last_input + aoff : nullptr;
#pragma unroll
    for (int r = 0; r < CL_PPT; ++r) {
        const int p = r * CLUSTER_THREADS + tid;
        if (p >= A) continue;
        const int c = base[r] / P, is = sCI[c], js = sCJ[c];
        const int sgn = (p == js ? 1 : 0) - (p == is ? 1 : 0);  // 0 where i* == j*: the far term is exactly zero
        const float fc = sCF[c];
        if (D.nn_ori) D.nn_ori[(size_t)b * A + p] = bi[r];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * p + k;
            const float x = sA[i];
            if (orec) OB[i] = x;
            if (LI) LI[i] = x;
            const float d = x - sO[3 * bi[r] + k];
            float g = __builtin_fmaf(c_cd, d, G[i]);
            float dg = c_cd * d;
            if (sgn != 0) {
                const float delta = (sA[3 * js + k] - sA[3 * is + k]) + 1e-7f;
                const float u = (c_far * delta) / fc;
                g = sgn > 0 ? g + u : g - u;
                dg = sgn > 0 ? dg + u : dg - u;
            }
            if (D.dist_grad) D.dist_grad[aoff + i] = dg;
            float mr = M[i], vr = V[i];
            X[i] = atk_adam(x, g, mr, vr, step_size, bc2, omb1, omb2);
            M[i] = mr;
            V[i] = vr;
        }
    }
}

}  // namespace

hipError_t launch_cluster_dbscan(const float* pts, const int32_t* n_pts, int B, int stride, float eps, int min_samples, int32_t* labels,
                                 int32_t* n_clusters, hipStream_t s) {
    hipLaunchKernelGGL(cluster_dbscan_kernel, dim3(B), dim3(CLUSTER_THREADS), DbscanLds::BYTES, s, pts, n_pts, stride, eps * eps,
                       min_samples, labels, n_clusters);
    return hipGetLastError();
}

hipError_t launch_cluster_step(const CwState& S, const float* grad, const int32_t* pred, const float* loss, const int32_t* target,
                               float* cat, const int32_t* n_ori, float* last_input, float* info, const ClusterDiag& D, int t, float lr,
                               float scale, int B, int cat_stride, int num_add, int cl_num_p, hipStream_t s) {
    const AdamStep a = adam_step_consts(t, lr);
    hipLaunchKernelGGL(cluster_step_kernel, dim3(B), dim3(CLUSTER_THREADS), ClusterStepLds::BYTES, s, S, grad, pred, loss, target, cat,
                       n_ori, last_input, info, D, a.step_size, a.bc2, a.omb1, a.omb2, scale, cat_stride, num_add, cl_num_p);
    return hipGetLastError();
}

}  // namespace ifd
