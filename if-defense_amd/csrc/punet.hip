// Baseline defenses of the reference (baselines/defend_npz.py): SRS, the DUP-Net input fill, and the PU-Net forward
// (baselines/defense/DUP_Net/pu_net.py, pu_modules.py, pu_utils.py) with npoint = 1024, up_ratio = 4, no BN, no residual.
//
//   srs_kernel    SRSDefense.random_drop (drop_points/SRS.py:24-33): K - drop rows of each cloud in draw order.
//   fill_kernel   DUPNet.process_data (DUP_Net.py:29-62): SOR's kept points padded / trimmed to 1024 rows.
//   fps_kernel    farthest_point_sample (pu_utils.py:55-74) of all four SA levels in one launch: one wave per cloud.
//   ball_kernel   query_ball_point (pu_utils.py:77-98): the 32 smallest member indices in the expanded-form distance.
//   sa_kernel     QueryAndGroup + SharedMLP + max_pool2d (pu_modules.py:22-60) of one SA level: grouped rows live in
//                 registers only (gather -> three 1x1 convs on v_mfma_f32_16x16x4_f32 -> max over the 32 samples).
//   knn3_kernel   the 3-NN search and weights of the three PointnetFPModule (pu_modules.py:157-171).
//   head_kernel   FP interpolation + MLPs, the 259-channel concatenation (pu_net.py:118-122), the four expansion
//                 branches and the reconstruction (:124-132), per 16-point tile of one wave.
//
// Matrix layout of every 1x1 conv: a wave holds 16 points (lane l: point l & 15, quarter q = l >> 4).  An activation tile t
// (16 channels) is one f32x4 per lane: register r = channel 16 t + 4 q + r.  A layer is C = W X with A = W (rows = output
// channels) and B = X^T: k-step 4 g + j takes channel 16 g + 4 q + j on both operands, so the accumulator of one layer IS the
// B operand of the next and features never leave registers between layers.  The weight image (api.cpp punet image) stores,
// per (output tile m, input group g), the 64 lanes' f32x4 of W[16 m + (l & 15)][16 g + 4 (l >> 4) + 0..3], zero-padded to
// whole tiles.  Summation per output: bias, then the inputs in ascending k in an fmaf chain (the MFMA's numerics).
//
// The distance arithmetic reproduces the reference's float32 operation order exactly, so the discrete decisions (FPS indices,
// ball members, 3-NN) are the reference's own wherever the inputs are: no contraction anywhere in this file, and the one
// fused multiply-add that torch's CPU matmul does use (3-term dot products: fma(z, z', fma(y, y', x x'))) is written out.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "victim_device.h"

#pragma clang fp contract(off)

namespace ifd {

namespace {

// acc[m] = bias + W X for the MT output tiles of a layer with SG input groups; in(g) yields the lane's f32x4 of group g.
template <int SG, int MT, class In>
__device__ __forceinline__ void dense(const float* __restrict__ img, const float* __restrict__ bias, In in, f32x4 (&acc)[MT]) {
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = *reinterpret_cast<const f32x4*>(bias + 16 * m + 4 * (l >> 4));
#pragma unroll
    for (int g = 0; g < SG; ++g) {
        const f32x4 b = in(g);
#pragma unroll
        for (int m = 0; m < MT; ++m)
            acc[m] = mfma4(*reinterpret_cast<const f32x4*>(img + ((size_t)(m * SG + g) * 64 + l) * 4), b, acc[m]);
    }
}

template <int T>
__device__ __forceinline__ void relu_all(f32x4 (&a)[T]) {
#pragma unroll
    for (int t = 0; t < T; ++t) a[t] = relu4(a[t]);
}

// squared distance in the reference's expanded form (pu_utils.py:24-27): (-2 * (s . d) + |s|^2) + |d|^2, float32
__device__ __forceinline__ float sq3(float x, float y, float z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ float expanded(float sx, float sy, float sz, float ss, float dx, float dy, float dz, float dd) {
    const float dot = fmaf(sz, dz, fmaf(sy, dy, sx * dx));
    return (-2.f * dot + ss) + dd;
}

__device__ __forceinline__ uint32_t draw_below(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

// Partial Fisher-Yates over [0, n) for `m` positions in LDS: perm[0..m) is a uniformly random ordered m-subset.  The draws
// are Philox(cloud, position, stage) so they do not depend on the batch split.
__device__ void partial_shuffle(int* perm, uint32_t* rnd, int n, int m, uint32_t gcloud, uint32_t stage, uint32_t s_lo, uint32_t s_hi) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) perm[i] = i;
    for (int j = threadIdx.x; j < m; j += blockDim.x) rnd[j] = philox(gcloud, (uint32_t)j, stage, 0u, s_lo, s_hi).x;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 0; j < m; ++j) {
            const int r = j + (int)draw_below(rnd[j], (uint32_t)(n - j));
            const int t = perm[j]; perm[j] = perm[r]; perm[r] = t;
        }
    }
    __syncthreads();
}

constexpr int DUP_THREADS = 256;

__global__ __launch_bounds__(DUP_THREADS) void srs_kernel(const float* __restrict__ pc, int K, int m, const int32_t* __restrict__ idx,
                                                          DupDraws d, float* __restrict__ out) {
    extern __shared__ int lds_i[];
    const int b = blockIdx.x;
    const float* P = pc + (size_t)b * K * 3;
    float* O = out + (size_t)b * m * 3;
    const int* perm;
    if (idx) {
        perm = idx + (size_t)b * m;
    } else {
        const SrsLdsAt at = srs_lds_at(K, m);
        int* shuffled = LDS_AT(int, lds_i, at.PERM);
        partial_shuffle(shuffled, LDS_AT(uint32_t, lds_i, at.RND), K, m, (uint32_t)(d.cloud_base + b), DUP_STAGE_SRS, d.seed_lo, d.seed_hi);
        perm = shuffled;
    }
    for (int t = threadIdx.x; t < m * 3; t += blockDim.x) {
        const int j = t / 3, c = t - 3 * j;
        const int src = min(max(perm[j], 0), K - 1);
        O[t] = P[src * 3 + c];
    }
}

__global__ __launch_bounds__(DUP_THREADS) void fill_kernel(const float* __restrict__ pc, const uint8_t* __restrict__ keep, int K,
                                                           const int32_t* __restrict__ draws, DupDraws d, float* __restrict__ out,
                                                           int32_t* __restrict__ n_kept) {
    extern __shared__ int lds_i[];
    __shared__ int part[DUP_THREADS + 1];
    const FillLdsAt at = fill_lds_at(K);
    int* L = LDS_AT(int, lds_i, at.KEPT);             // [K] kept indices, original order
    int* perm = LDS_AT(int, lds_i, at.PERM);          // [K]
    uint32_t* rnd = LDS_AT(uint32_t, lds_i, at.RND);
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint8_t* M = keep + (size_t)b * K;
    const int per = (K + DUP_THREADS - 1) / DUP_THREADS, lo = min(tid * per, K), hi = min(lo + per, K);
    int c = 0;
    for (int i = lo; i < hi; ++i) c += M[i] != 0;
    part[tid + 1] = c;
    __syncthreads();
    if (tid == 0) { part[0] = 0; for (int i = 1; i <= DUP_THREADS; ++i) part[i] += part[i - 1]; }
    __syncthreads();
    int o = part[tid];
    for (int i = lo; i < hi; ++i) if (M[i]) L[o++] = i;
    const int N = part[DUP_THREADS];
    if (tid == 0 && n_kept) n_kept[b] = N;
    float* O = out + (size_t)b * DUP_NP * 3;
    const float* P = pc + (size_t)b * K * 3;
    if (N == 0) {                                     // cannot come out of ifd_sor (the smallest value is always kept)
        for (int t = tid; t < DUP_NP * 3; t += DUP_THREADS) O[t] = 0.f;
        return;
    }
    const int q = N >= DUP_NP ? 0 : DUP_NP / N;
    const int nd = N > DUP_NP ? DUP_NP : (N < DUP_NP ? DUP_NP - q * N : 0);
    const int* pr = perm;
    if (nd > 0) {
        if (draws) pr = draws + (size_t)b * DUP_NP;
        else partial_shuffle(perm, rnd, N, nd, (uint32_t)(d.cloud_base + b), DUP_STAGE_FILL, d.seed_lo, d.seed_hi);
    }
    __syncthreads();
    for (int t = tid; t < DUP_NP * 3; t += DUP_THREADS) {
        const int j = t / 3, cc = t - 3 * j;
        int k;
        if (N == DUP_NP) k = j;
        else if (N > DUP_NP) k = pr[j];
        else k = j < q * N ? j % N : pr[j - q * N];
        k = min(max(k, 0), N - 1);
        O[t] = P[L[k] * 3 + cc];
    }
}

// ---- FPS ------------------------------------------------------------------------------------------------------------
// One wave per cloud.  Level v samples S_v points from the N_v points of level v - 1's output (level 0: the input); lane l
// holds points l + 64 j.  Arg-max: largest distance, first index among equals (torch.max on CPU).
__global__ __launch_bounds__(64) void fps_kernel(const float* __restrict__ xyz, const int32_t* __restrict__ start, DupDraws d,
                                                 int32_t* __restrict__ fidx, float* __restrict__ nxyz) {
    __shared__ float buf[2][DUP_NP * 3];
    const int b = blockIdx.x, l = threadIdx.x;
    const float* X = xyz + (size_t)b * DUP_NP * 3;
    for (int t = l; t < DUP_NP * 3; t += 64) buf[0][t] = X[t];
    __syncthreads();
    for (int v = 0; v < 4; ++v) {
        const int N = v == 0 ? DUP_NP : (DUP_NP >> (v - 1)), S = DUP_NP >> v, P = N / 64;
        const float* in = buf[v & 1];
        float* ou = buf[(v + 1) & 1];
        int far;
        if (start) far = min(max(start[b * 4 + v], 0), N - 1);
        else far = (int)draw_below(philox((uint32_t)(d.cloud_base + b), 0u, DUP_STAGE_FPS + v, 0u, d.seed_lo, d.seed_hi).x, (uint32_t)N);
        float dist[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) dist[j] = 1e10f;
        int32_t* FI = fidx + (size_t)b * DUP_NS + dup_level_off(v);
        float* NX = nxyz + ((size_t)b * DUP_NS + dup_level_off(v)) * 3;
        for (int i = 0; i < S; ++i) {
            const float cx = in[far * 3], cy = in[far * 3 + 1], cz = in[far * 3 + 2];
            if (l == 0) {
                FI[i] = far;
                NX[i * 3] = cx; NX[i * 3 + 1] = cy; NX[i * 3 + 2] = cz;
                ou[i * 3] = cx; ou[i * 3 + 1] = cy; ou[i * 3 + 2] = cz;
            }
            float bv = -1.f;
            int bi = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j < P) {
                    const int p = l + 64 * j;
                    const float dx = in[p * 3] - cx, dy = in[p * 3 + 1] - cy, dz = in[p * 3 + 2] - cz;
                    const float dd = (dx * dx + dy * dy) + dz * dz;
                    if (dd < dist[j]) dist[j] = dd;
                    if (dist[j] > bv) { bv = dist[j]; bi = p; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o);
                const int oi = __shfl_xor(bi, o);
                if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            }
            far = bi;
        }
        __syncthreads();
    }
}

// ---- ball query -----------------------------------------------------------------------------------------------------
// One wave per centroid of any level (grid over the 1,920 centroids of every cloud); index order scan, 64 points a step.
__global__ __launch_bounds__(256) void ball_kernel(const float* __restrict__ xyz, const float* __restrict__ nxyz, int32_t* __restrict__ bidx) {
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6), l = threadIdx.x & 63;
    const int b = blockIdx.y;
    if (w >= DUP_NS) return;
    const int v = w < 1024 ? 0 : (w < 1536 ? 1 : (w < 1792 ? 2 : 3));
    const int N = v == 0 ? DUP_NP : (DUP_NP >> (v - 1));
    const float* pts = v == 0 ? xyz + (size_t)b * DUP_NP * 3 : nxyz + ((size_t)b * DUP_NS + dup_level_off(v - 1)) * 3;
    const float* c = nxyz + ((size_t)b * DUP_NS + w) * 3;
    const float sx = c[0], sy = c[1], sz = c[2], ss = sq3(sx, sy, sz);
    const float r2 = dup_radius2(v);
    int32_t* O = bidx + ((size_t)b * DUP_NS + w) * DUP_NSAMPLE;
    int cnt = 0, first = 0;
    for (int base = 0; base < N && cnt < DUP_NSAMPLE; base += 64) {
        const int j = base + l;
        bool hit = false;
        if (j < N) {
            const float dx = pts[j * 3], dy = pts[j * 3 + 1], dz = pts[j * 3 + 2];
            hit = !(expanded(sx, sy, sz, ss, dx, dy, dz, sq3(dx, dy, dz)) > r2);
        }
        const uint64_t mask = __ballot(hit);
        if (mask == 0) continue;
        if (cnt == 0) first = base + __ffsll((unsigned long long)mask) - 1;
        const int pos = cnt + __popcll(mask & ((1ull << l) - 1ull));
        if (hit && pos < DUP_NSAMPLE) O[pos] = j;
        cnt += __popcll(mask);
    }
    for (int p = cnt + l; p < DUP_NSAMPLE; p += 64) O[p] = first;
}

// ---- SA levels --------------------------------------------------------------------------------------------------------
template <int V> struct Sa;
template <> struct Sa<0> { static constexpr int C = 0, G0 = 1, M1 = 2, M2 = 2, M3 = 4; };
template <> struct Sa<1> { static constexpr int C = 64, G0 = 5, M1 = 4, M2 = 4, M3 = 8; };
template <> struct Sa<2> { static constexpr int C = 128, G0 = 9, M1 = 8, M2 = 8, M3 = 16; };
template <> struct Sa<3> { static constexpr int C = 256, G0 = 17, M1 = 16, M2 = 16, M3 = 32; };

// Four waves = two centroids; each wave takes 16 of a centroid's 32 samples.  Input channel order of the first layer:
// [features (C), dx, dy, dz, 0...] (the weight image permutes W's columns to match).
template <int V>
__global__ __launch_bounds__(256) void sa_kernel(const float* __restrict__ img, PunetLayer L1, PunetLayer L2, PunetLayer L3,
                                                 const float* __restrict__ xyz, const float* __restrict__ nxyz,
                                                 const int32_t* __restrict__ bidx, float* __restrict__ feats) {
    using CF = Sa<V>;
    constexpr int N = V == 0 ? DUP_NP : (DUP_NP >> (V - 1)), COUT = 16 * CF::M3;
    __shared__ float red[4][COUT];
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int b = blockIdx.y, cen = blockIdx.x * 2 + (wv >> 1);
    const float* c = nxyz + ((size_t)b * DUP_NS + dup_level_off(V) + cen) * 3;
    const float cx = c[0], cy = c[1], cz = c[2];
    int j = bidx[((size_t)b * DUP_NS + dup_level_off(V) + cen) * DUP_NSAMPLE + 16 * (wv & 1) + p];
    j = min(max(j, 0), N - 1);
    const float* pts = V == 0 ? xyz + (size_t)b * DUP_NP * 3 : nxyz + ((size_t)b * DUP_NS + dup_level_off(V - 1)) * 3;
    const float* frow = feats + (size_t)b * DUP_FEAT_FLOATS + (V > 0 ? dup_feat_off(V - 1) + (size_t)j * CF::C : 0);
    auto gather = [&](int g) -> f32x4 {
        if (16 * g < CF::C) return *reinterpret_cast<const f32x4*>(frow + 16 * g + 4 * q);
        if (q == 0) return f32x4{pts[j * 3] - cx, pts[j * 3 + 1] - cy, pts[j * 3 + 2] - cz, 0.f};
        return f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x4 a1[CF::M1];
    dense<CF::G0, CF::M1>(img + L1.w, img + L1.b, gather, a1);
    relu_all(a1);
    f32x4 a2[CF::M2];
    dense<CF::M1, CF::M2>(img + L2.w, img + L2.b, [&](int g) { return a1[g]; }, a2);
    relu_all(a2);
#pragma unroll 1
    for (int m = 0; m < CF::M3; ++m) {
        f32x4 o[1];
        dense<CF::M2, 1>(img + L3.w + (size_t)m * CF::M2 * 256, img + L3.b + 16 * m, [&](int g) { return a2[g]; }, o);
        f32x4 r = relu4(o[0]);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float x = r[k];
            x = fmaxf(x, __shfl_xor(x, 1)); x = fmaxf(x, __shfl_xor(x, 2));
            x = fmaxf(x, __shfl_xor(x, 4)); x = fmaxf(x, __shfl_xor(x, 8));
            r[k] = x;
        }
        if (p == 0) *reinterpret_cast<f32x4*>(&red[wv][16 * m + 4 * q]) = r;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * COUT; t += 256) {
        const int pr = t / COUT, ch = t - pr * COUT;
        feats[(size_t)b * DUP_FEAT_FLOATS + dup_feat_off(V) + (size_t)(blockIdx.x * 2 + pr) * COUT + ch] = fmaxf(red[2 * pr][ch], red[2 * pr + 1][ch]);
    }
}

// ---- FP 3-NN --------------------------------------------------------------------------------------------------------
// Query = the 1024 input points (input order), known = the centroids of SA level f + 1 (f = FP module 0..2).
__global__ __launch_bounds__(256) void knn3_kernel(const float* __restrict__ xyz, const float* __restrict__ nxyz,
                                                   int32_t* __restrict__ kidx, float* __restrict__ kw) {
    __shared__ float kn[512 * 4];
    const int f = blockIdx.y, b = blockIdx.z, M = DUP_NP >> (f + 1);
    const float* K = nxyz + ((size_t)b * DUP_NS + dup_level_off(f + 1)) * 3;
    for (int t = threadIdx.x; t < M; t += 256) {
        const float x = K[t * 3], y = K[t * 3 + 1], z = K[t * 3 + 2];
        kn[t * 4] = x; kn[t * 4 + 1] = y; kn[t * 4 + 2] = z; kn[t * 4 + 3] = sq3(x, y, z);
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const float* Q = xyz + ((size_t)b * DUP_NP + i) * 3;
    const float sx = Q[0], sy = Q[1], sz = Q[2], ss = sq3(sx, sy, sz);
    float d0 = INFINITY, d1 = INFINITY, d2 = INFINITY;
    int i0 = 0, i1 = 0, i2 = 0;
    for (int t = 0; t < M; ++t) {
        const float dd = expanded(sx, sy, sz, ss, kn[t * 4], kn[t * 4 + 1], kn[t * 4 + 2], kn[t * 4 + 3]);
        if (dd < d2) {
            if (dd < d1) {
                d2 = d1; i2 = i1;
                if (dd < d0) { d1 = d0; i1 = i0; d0 = dd; i0 = t; }
                else { d1 = dd; i1 = t; }
            } else { d2 = dd; i2 = t; }
        }
    }
    // weight = 1 / (d + 1e-8), normalised (pu_modules.py:168-170); no guard: a coinciding point's noise is reproduced
    const float w0 = 1.f / (d0 + 1e-8f), w1 = 1.f / (d1 + 1e-8f), w2 = 1.f / (d2 + 1e-8f);
    const float s = (w0 + w1) + w2;
    const size_t o = (((size_t)b * 3 + f) * DUP_NP + i) * 3;
    kidx[o] = i0; kidx[o + 1] = i1; kidx[o + 2] = i2;
    kw[o] = w0 / s; kw[o + 1] = w1 / s; kw[o + 2] = w2 / s;
}

// ---- head ---------------------------------------------------------------------------------------------------------
// One wave per 16 input points.  The concatenation is held as 17 tiles in the order [l_feats[1] row i (64), up0, up1, up2
// (64 each), x, y, z, 0...]; the weight image of the expansion layers permutes W's columns to it.  Row i of l_feats[1] is
// SA-1's i-th centroid while xyz and up* are point i (the reference's pairing, pu_net.py:118-122).
template <int C>
__device__ __forceinline__ void fp_module(const float* __restrict__ img, PunetLayer Lf, const float* __restrict__ feat,
                                          const int32_t* __restrict__ ki, const float* __restrict__ kwt, f32x4 (&up)[4]) {
    const int q = (threadIdx.x & 63) >> 4;
    const int n0 = ki[0], n1 = ki[1], n2 = ki[2];
    const float w0 = kwt[0], w1 = kwt[1], w2 = kwt[2];
    const float *r0 = feat + (size_t)n0 * C + 4 * q, *r1 = feat + (size_t)n1 * C + 4 * q, *r2 = feat + (size_t)n2 * C + 4 * q;
    auto interp = [&](int g) -> f32x4 {
        const f32x4 a = *reinterpret_cast<const f32x4*>(r0 + 16 * g), bb = *reinterpret_cast<const f32x4*>(r1 + 16 * g),
                    c = *reinterpret_cast<const f32x4*>(r2 + 16 * g);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (a[k] * w0 + bb[k] * w1) + c[k] * w2;
        return o;
    };
    dense<C / 16, 4>(img + Lf.w, img + Lf.b, interp, up);
    relu_all(up);
}

__global__ __launch_bounds__(256) void head_kernel(const float* __restrict__ img, PunetHead H, const float* __restrict__ xyz,
                                                   const float* __restrict__ feats, const int32_t* __restrict__ kidx,
                                                   const float* __restrict__ kw, float* __restrict__ out) {
    const int l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int b = blockIdx.y, i = blockIdx.x * 64 + (threadIdx.x >> 6) * 16 + p;
    const float* F = feats + (size_t)b * DUP_FEAT_FLOATS;
    f32x4 cat[17];
    {
        const float* r = F + (size_t)i * 64 + 4 * q;                  // l_feats[1] (SA-1 output, FPS order) row i
#pragma unroll
        for (int t = 0; t < 4; ++t) cat[t] = *reinterpret_cast<const f32x4*>(r + 16 * t);
    }
    const size_t ko = ((size_t)b * 3 * DUP_NP + i) * 3;
    {
        f32x4 u[4];
        fp_module<128>(img, H.fp[0], F + dup_feat_off(1), kidx + ko, kw + ko, u);
#pragma unroll
        for (int t = 0; t < 4; ++t) cat[4 + t] = u[t];
        fp_module<256>(img, H.fp[1], F + dup_feat_off(2), kidx + ko + DUP_NP * 3, kw + ko + DUP_NP * 3, u);
#pragma unroll
        for (int t = 0; t < 4; ++t) cat[8 + t] = u[t];
        fp_module<512>(img, H.fp[2], F + dup_feat_off(3), kidx + ko + 2 * DUP_NP * 3, kw + ko + 2 * DUP_NP * 3, u);
#pragma unroll
        for (int t = 0; t < 4; ++t) cat[12 + t] = u[t];
    }
    {
        const float* X = xyz + ((size_t)b * DUP_NP + i) * 3;
        cat[16] = q == 0 ? f32x4{X[0], X[1], X[2], 0.f} : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        f32x4 h1[16];
        dense<17, 16>(img + H.fc0[k].w, img + H.fc0[k].b, [&](int g) { return cat[g]; }, h1);
        relu_all(h1);
        f32x4 h2[8];
        dense<16, 8>(img + H.fc1[k].w, img + H.fc1[k].b, [&](int g) { return h1[g]; }, h2);
        relu_all(h2);
        f32x4 h3[4];
        dense<8, 4>(img + H.pcd0.w, img + H.pcd0.b, [&](int g) { return h2[g]; }, h3);
        relu_all(h3);
        f32x4 o[1];
        dense<4, 1>(img + H.pcd1.w, img + H.pcd1.b, [&](int g) { return h3[g]; }, o);
        if (q == 0) {
            float* O = out + ((size_t)b * DUP_NP * 4 + (size_t)k * DUP_NP + i) * 3;     // branch-major rows (pu_net.py:128)
            O[0] = o[0][0]; O[1] = o[0][1]; O[2] = o[0][2];
        }
    }
}

}  // namespace

hipError_t configure_punet_kernels() {
    return opt_in_dynamic_lds({{srs_kernel, srs_lds_at(PREP_MAXK, PREP_MAXK).BYTES}, {fill_kernel, fill_lds_at(PREP_MAXK).BYTES}});
}

hipError_t launch_srs(const float* pc, int B, int K, int m, const int32_t* idx, DupDraws d, float* out, hipStream_t s) {
    const size_t lds = idx ? 0 : srs_lds_at(K, m).BYTES;
    hipLaunchKernelGGL(srs_kernel, dim3(B), dim3(DUP_THREADS), lds, s, pc, K, m, idx, d, out);
    return hipGetLastError();
}

hipError_t launch_dup_fill(const float* pc, const uint8_t* keep, int B, int K, const int32_t* draws, DupDraws d, float* out,
                           int32_t* n_kept, hipStream_t s) {
    hipLaunchKernelGGL(fill_kernel, dim3(B), dim3(DUP_THREADS), fill_lds_at(K).BYTES, s, pc, keep, K, draws, d, out, n_kept);
    return hipGetLastError();
}

hipError_t launch_punet(const float* img, const PunetImage& I, const float* xyz, int B, const int32_t* fps_start, DupDraws d,
                        const PunetWs& w, float* out, hipStream_t s) {
    hipLaunchKernelGGL(fps_kernel, dim3(B), dim3(64), 0, s, xyz, fps_start, d, w.fidx, w.nxyz);
    hipLaunchKernelGGL(ball_kernel, dim3(DUP_NS / 4, B), dim3(256), 0, s, xyz, w.nxyz, w.bidx);
    hipLaunchKernelGGL(sa_kernel<0>, dim3(512, B), dim3(256), 0, s, img, I.sa[0][0], I.sa[0][1], I.sa[0][2], xyz, w.nxyz, w.bidx,
                       w.feat);
    hipLaunchKernelGGL(sa_kernel<1>, dim3(256, B), dim3(256), 0, s, img, I.sa[1][0], I.sa[1][1], I.sa[1][2], xyz, w.nxyz, w.bidx,
                       w.feat);
    hipLaunchKernelGGL(sa_kernel<2>, dim3(128, B), dim3(256), 0, s, img, I.sa[2][0], I.sa[2][1], I.sa[2][2], xyz, w.nxyz, w.bidx,
                       w.feat);
    hipLaunchKernelGGL(sa_kernel<3>, dim3(64, B), dim3(256), 0, s, img, I.sa[3][0], I.sa[3][1], I.sa[3][2], xyz, w.nxyz, w.bidx,
                       w.feat);
    hipLaunchKernelGGL(knn3_kernel, dim3(DUP_NP / 256, 3, B), dim3(256), 0, s, xyz, w.nxyz, w.kidx, w.kw);
    hipLaunchKernelGGL(head_kernel, dim3(DUP_NP / 64, B), dim3(256), 0, s, img, I.head, xyz, (const float*)w.feat, w.kidx, w.kw, out);
    return hipGetLastError();
}

}  // namespace ifd
