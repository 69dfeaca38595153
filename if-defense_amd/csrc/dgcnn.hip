// The DGCNN victim classifier of the reference (baselines/model/dgcnn.py: DGCNN(emb_dims=1024, k, use_bn) in eval mode).
// Eval-mode BatchNorm is folded into the weights on the host.  The [B, 2C, N, k] edge tensor of the reference never exists:
// every edge convolution runs in split form,
//     W [x_j - x_i; x_i] + b = Wa x_j + (Wb - Wa) x_i + b = P_j + Q_i,        out_i = leaky(max_j P_j + Q_i)
// (LeakyReLU is monotone, so it commutes with the maximum over the neighbours exactly), which costs one per-point layer of
// 2 Cout outputs and a gather over the neighbour graph instead of k per-edge layers.
//
//   dg_norm_kernel      |x_j|^2 of a layer's input, one fused chain over the channels in ascending order
//   dg_knn_kernel<C>    a thread owns one query point, a workgroup 64 of them.  The candidates j = 0 .. n-1 are walked in
//                       ascending order by the whole wave together, so a candidate's row is wave-uniform and comes through
//                       the scalar cache; the score s_ij = 2 <x_i, x_j> - |x_j|^2 is one fused chain over the channels in
//                       ascending order, then fmaf(2, dot, -|x_j|^2).  Each thread keeps its k best (score, index) pairs in
//                       LDS, unsorted, behind a threshold (the worst of them): a candidate replaces the worst entry only where
//                       it beats it strictly, so among equal scores the lowest index stays; the new worst entry is found by
//                       one scan of the k entries.  Such an update is rare for one thread and near certain for one of 64, so
//                       a thread only queues what beats its threshold and the wave works all queues off together.  The n x n
//                       matrix never exists.
//   dg_first_kernel     P | Q of the C = 3 layer, plain fused multiply-adds
//   linear_kernel       victim_linear.h: Y = leaky(W X + b), per output the bias, then four chains across all inputs, added
//                       pairwise.  <DgLinear>: P | Q of conv2 .. conv4 and the FC head; <DgConv5>: conv5, whose [points, 1024]
//                       output is reduced to the maximum and the sum of each 64-point tile at once.
//   dg_gather_kernel    out_i = leaky(max_j P_j + Q_i) over the k neighbours of idx, written into its columns of feat
//   dg_pool_kernel      a cloud's tiles -> max | mean [2048]; the sum runs over the tiles in ascending order, and a tile's sum is
//                       a fixed tree, so the mean depends on nothing but the cloud's own rows and count.  No atomics.
// The prediction is launch_argmax's (pointnet.hip): the lowest class among equal logits.
//
// Columns of an MFMA never mix: a point's (a cloud's) result depends on nothing but its own row, whatever shares its wave.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "victim_linear.h"

namespace ifd {

namespace {

static_assert(DG_TILE == LINEAR_TILE, "dg_pool_kernel walks the tiles linear_kernel<DgConv5> wrote");

// X: rows of ldx floats, C of them used; a cloud's rows start at X + b * xb
template <int C>
__global__ __launch_bounds__(256) void dg_norm_kernel(const float* __restrict__ X, int ldx, size_t xb, const int32_t* __restrict__ n_points,
                                                      int stride, float* __restrict__ nrm) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int n = cloud_points(n_points, b, stride);
    if (i >= n) return;
    const float* x = X + (size_t)b * xb + (size_t)i * ldx;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s = fmaf(x[c], x[c], s);
    nrm[(size_t)b * stride + i] = s;
}

template <int C>
__global__ __launch_bounds__(DG_KNN_THREADS) void dg_knn_kernel(const float* __restrict__ X, int ldx, size_t xb, const float* __restrict__ nrm,
                                                                const int32_t* __restrict__ n_points, int stride, int k,
                                                                int32_t* __restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const DgKnnLdsAt L = dg_knn_lds_at(k);
    float* sc = LDS_AT(float, smem, L.SC) + threadIdx.x;
    int* ix = LDS_AT(int, smem, L.IX) + threadIdx.x;
    const int b = blockIdx.y;
    const int n = cloud_points(n_points, b, stride);
    if ((int)blockIdx.x * DG_KNN_THREADS >= n) return;                 // the whole workgroup
    const int i = blockIdx.x * DG_KNN_THREADS + threadIdx.x;
    const float* Xb = X + (size_t)b * xb;
    const float* Nb = nrm + (size_t)b * stride;
    float xq[C];
    {
        const float* x = Xb + (size_t)min(i, n - 1) * ldx;             // threads beyond the cloud walk along with its last row
#pragma unroll
        for (int c = 0; c < C; ++c) xq[c] = x[c];
    }
    float* ps = LDS_AT(float, smem, L.PS) + threadIdx.x;
    int* pi = LDS_AT(int, smem, L.PI) + threadIdx.x;
    const int kk = min(k, n);
    float thr = 0.f;                                                   // the worst entry of the list: its score, and where it lies
    int tpos = 0;
    // the new worst entry: the lowest score, of equals the highest index
    auto rescan = [&]() {
        float m = sc[0];
        int mi = ix[0], mp = 0;
#pragma unroll 4
        for (int e = 1; e < kk; ++e) {
            const float se = sc[e * DG_KNN_THREADS];
            const int ie = ix[e * DG_KNN_THREADS];
            if (se < m || (se == m && ie > mi)) { m = se; mi = ie; mp = e; }
        }
        thr = m;
        tpos = mp;
    };
    // A candidate that beats the threshold is only queued; the queues of all the wave's threads are worked off together once one
    // of them is full, so that the list updates of 64 queries run side by side instead of one thread's at a time.  The threshold
    // a candidate was queued under may be stale (too low), never too high: every queued candidate meets the current one again.
    int pending = 0;
    auto flush = [&]() {
        for (int t = 0; t < DG_KNN_PEND; ++t) {
            if (t < pending) {
                const float s = ps[t * DG_KNN_THREADS];
                if (s > thr) {                                         // strictly: among equal scores the lower index, which came first, stays
                    sc[tpos * DG_KNN_THREADS] = s;
                    ix[tpos * DG_KNN_THREADS] = pi[t * DG_KNN_THREADS];
                    rescan();
                }
            }
        }
        pending = 0;
    };
    for (int j = 0; j < n; ++j) {
        const float* xj = Xb + (size_t)j * ldx;                        // wave-uniform
        float d = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) d = fmaf(xq[c], xj[c], d);
        const float s = fmaf(2.f, d, -Nb[j]);
        if (j < kk) {                                                  // the first k always, whatever their values
            sc[j * DG_KNN_THREADS] = s;
            ix[j * DG_KNN_THREADS] = j;
            if (j == kk - 1) rescan();
        } else {
            if (s > thr) {
                ps[pending * DG_KNN_THREADS] = s;
                pi[pending * DG_KNN_THREADS] = j;
                ++pending;
            }
            if (__ballot(pending == DG_KNN_PEND) != 0) flush();        // wave-uniform
        }
    }
    flush();
    if (i < n) {
        int32_t* o = idx + ((size_t)b * stride + i) * k;
        for (int e = 0; e < kk; ++e) o[e] = ix[e * DG_KNN_THREADS];
    }
}

// first: [128][4] = {w0, w1, w2, bias}; pq[b][i][o] for o < 128.  A thread = one point x four outputs.
__global__ __launch_bounds__(256) void dg_first_kernel(const float* __restrict__ first, const float* __restrict__ pc,
                                                       const int32_t* __restrict__ n_points, int stride, float* __restrict__ pq) {
    const int b = blockIdx.y, i = blockIdx.x * 8 + (threadIdx.x >> 5), o = (threadIdx.x & 31) * 4;
    const int n = cloud_points(n_points, b, stride);
    if (i >= n) return;
    const float* p = pc + ((size_t)b * stride + i) * 3;
    const float x = p[0], y = p[1], z = p[2];
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(first + (o + r) * 4);
        v[r] = fmaf(w[2], z, fmaf(w[1], y, fmaf(w[0], x, w[3])));
    }
    *reinterpret_cast<f32x4*>(pq + ((size_t)b * stride + i) * DG_FEAT + o) = v;
}

// pq rows of DG_FEAT floats: P in [0, cout), Q in [cout, 2 cout).  feat[b][i][col + c] = leaky(max_j P[idx[i][j]][c] + Q[i][c]).
// A thread = one point x four channels; a workgroup = 1024 / cout points.
__global__ __launch_bounds__(256) void dg_gather_kernel(const float* __restrict__ pq, const int32_t* __restrict__ idx,
                                                        const int32_t* __restrict__ n_points, int stride, int k, int cout, int col,
                                                        float* __restrict__ feat) {
    const int per = cout >> 2, b = blockIdx.y;
    const int i = blockIdx.x * (256 / per) + threadIdx.x / per, c = (threadIdx.x % per) * 4;
    const int n = cloud_points(n_points, b, stride);
    if (i >= n) return;
    const float* Pb = pq + (size_t)b * stride * DG_FEAT;
    const int32_t* nb = idx + ((size_t)b * stride + i) * k;
    const int kk = min(k, n);
    f32x4 m = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int e = 0; e < kk; ++e) {
        const int j = min(max(nb[e], 0), n - 1);
        const f32x4 v = *reinterpret_cast<const f32x4*>(Pb + (size_t)j * DG_FEAT + c);
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = fmaxf(m[r], v[r]);
    }
    const f32x4 qv = *reinterpret_cast<const f32x4*>(Pb + (size_t)i * DG_FEAT + cout + c);
    *reinterpret_cast<f32x4*>(feat + ((size_t)b * stride + i) * DG_FEAT + col + c) = leaky4(m + qv);
}

__global__ __launch_bounds__(256) void dg_pool_kernel(const float* __restrict__ part_max, const float* __restrict__ part_sum,
                                                      const int32_t* __restrict__ n_points, int stride, int T, float* __restrict__ gfeat) {
    const int b = blockIdx.x, c = threadIdx.x * 4;
    const int n = cloud_points(n_points, b, stride);
    const int tiles = (n + DG_TILE - 1) / DG_TILE;
    const float* Pm = part_max + (size_t)b * T * DG_EMB + c;
    const float* Ps = part_sum + (size_t)b * T * DG_EMB + c;
    f32x4 m = *reinterpret_cast<const f32x4*>(Pm), s = *reinterpret_cast<const f32x4*>(Ps);
    for (int t = 1; t < tiles; ++t) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(Pm + (size_t)t * DG_EMB);
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = fmaxf(m[r], v[r]);
        s += *reinterpret_cast<const f32x4*>(Ps + (size_t)t * DG_EMB);
    }
    const float fn = (float)n;
    *reinterpret_cast<f32x4*>(gfeat + (size_t)b * 2 * DG_EMB + c) = m;
    *reinterpret_cast<f32x4*>(gfeat + (size_t)b * 2 * DG_EMB + DG_EMB + c) = f32x4{s[0] / fn, s[1] / fn, s[2] / fn, s[3] / fn};
}

template <int C>
void launch_knn(const float* X, int ldx, size_t xb, const int32_t* n_points, int B, int stride, int k, float* nrm, int32_t* idx,
                hipStream_t s) {
    hipLaunchKernelGGL((dg_norm_kernel<C>), dim3((stride + 255) / 256, B), dim3(256), 0, s, X, ldx, xb, n_points, stride, nrm);
    hipLaunchKernelGGL((dg_knn_kernel<C>), dim3((stride + DG_KNN_THREADS - 1) / DG_KNN_THREADS, B), dim3(DG_KNN_THREADS),
                       (size_t)dg_knn_lds_at(k).BYTES, s, X, ldx, xb, (const float*)nrm, n_points, stride, k, idx);
}

}  // namespace

hipError_t launch_dg_pq(const float* img, const DgImage& I, int l, const float* pc, const float* feat, const int32_t* n_points, int B,
                        int stride, float* pq, hipStream_t s) {
    const size_t fb = (size_t)stride * DG_FEAT;
    const int col_in[4] = {0, 0, 64, 128};
    if (l == 0) hipLaunchKernelGGL(dg_first_kernel, dim3((stride + 7) / 8, B), dim3(256), 0, s, img + I.first, pc, n_points, stride, pq);
    else launch_linear<DgLinear>(img, I.pq[l - 1], feat + col_in[l], DG_FEAT, fb, n_points, B, stride, pq, DG_FEAT, fb, 0, s);
    return hipGetLastError();
}

hipError_t launch_dgcnn(const float* img, const DgImage& I, const float* pc, const int32_t* n_points, int B, int stride, int k,
                        const DgWs& w, const DgOut& out, float* logits, int n_classes, hipStream_t s) {
    float* feat = out.feat ? out.feat : w.feat;
    float* gfeat = out.gfeat ? out.gfeat : w.gfeat;
    const size_t fb = (size_t)stride * DG_FEAT;
    const dim3 block(256);
    // layer 1: kNN on xyz, P | Q by plain FMAs
    int32_t* idx = out.idx[0] ? out.idx[0] : w.idx;
    launch_knn<3>(pc, 3, (size_t)stride * 3, n_points, B, stride, k, w.nrm, idx, s);
    hipLaunchKernelGGL(dg_first_kernel, dim3((stride + 7) / 8, B), block, 0, s, img + I.first, pc, n_points, stride, w.pq);
    hipLaunchKernelGGL(dg_gather_kernel, dim3((stride + 15) / 16, B), block, 0, s, (const float*)w.pq, (const int32_t*)idx, n_points,
                       stride, k, 64, 0, feat);
    // layers 2 .. 4 on x1, x2, x3 = columns [0, 64), [64, 128), [128, 256) of feat
    const int cin[3] = {64, 64, 128}, col_in[3] = {0, 64, 128}, cout[3] = {64, 128, 256}, col_out[3] = {64, 128, 256};
    for (int l = 0; l < 3; ++l) {
        idx = out.idx[l + 1] ? out.idx[l + 1] : w.idx;
        if (cin[l] == 64) launch_knn<64>(feat + col_in[l], DG_FEAT, fb, n_points, B, stride, k, w.nrm, idx, s);
        else launch_knn<128>(feat + col_in[l], DG_FEAT, fb, n_points, B, stride, k, w.nrm, idx, s);
        launch_linear<DgLinear>(img, I.pq[l], feat + col_in[l], DG_FEAT, fb, n_points, B, stride, w.pq, DG_FEAT, fb, 0, s);
        const int ppb = 1024 / cout[l];
        hipLaunchKernelGGL(dg_gather_kernel, dim3((stride + ppb - 1) / ppb, B), block, 0, s, (const float*)w.pq, (const int32_t*)idx,
                           n_points, stride, k, cout[l], col_out[l], feat);
    }
    // conv5 + LeakyReLU -> max | mean over the points
    const int T = (stride + DG_TILE - 1) / DG_TILE;
    launch_linear<DgConv5>(img, I.conv5, feat, DG_FEAT, fb, n_points, B, stride, nullptr, 0, 0, 1, s, nullptr, nullptr, w.part_max, w.part_sum);
    hipLaunchKernelGGL(dg_pool_kernel, dim3(B), block, 0, s, (const float*)w.part_max, (const float*)w.part_sum, n_points, stride, T, gfeat);
    // the head, a cloud a row
    launch_linear<DgLinear>(img, I.fc[0], gfeat, 2 * DG_EMB, 0, nullptr, 1, B, w.f1, 512, 0, 1, s);
    launch_linear<DgLinear>(img, I.fc[1], w.f1, 512, 0, nullptr, 1, B, w.f2, 256, 0, 1, s);
    launch_linear<DgLinear>(img, I.fc[2], w.f2, 256, 0, nullptr, 1, B, logits, n_classes, 0, 0, s);
    return out.pred ? launch_argmax(logits, B, n_classes, out.pred, s) : hipGetLastError();
}

}  // namespace ifd
