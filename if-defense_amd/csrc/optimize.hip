// Host launchers and the stand-alone / large-cloud kernels of the ConvONet-Opt optimiser; the persistent kernel itself is in
// optimize_kernel.h.
#include "optimize_kernel.h"

namespace ifd {

// ---------------------------------------------------------------------------------------------
// [pcsamp:other_kernels]
// stand-alone entry kernels (same device functions; used by ifd_decode / ifd_repulsion and tests)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS, 2) void decode_kernel(const float* __restrict__ dec_img,
                                                                 const float* __restrict__ planes,
                                                                 const float* __restrict__ p, int K,
                                                                 float* __restrict__ logits,
                                                                 float* __restrict__ dlogit_dp, DecConst dc) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* W = LDS_AT(float, smem, DecImageLds<0>::W);
    const int cloud = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    load_dec_image(W, dec_img);
    __syncthreads();
    const float* pl = planes + (size_t)cloud * CLOUD_PLANE_FLOATS;
    const float* pc = p + (size_t)cloud * K * 3;
    const int ntiles = (K + 15) >> 4;
    for (int tile = wave; tile < ntiles; tile += (int)(blockDim.x >> 6)) {
        const int tp = min(tile * 16 + (lane & 15), K - 1);
        const float x0 = pc[3 * tp], x1 = pc[3 * tp + 1], x2 = pc[3 * tp + 2];
        float logit, bce, dx[3] = {0.f, 0.f, 0.f};
        if (dlogit_dp != nullptr)
            decoder_tile<MODE_SUM, true, 2>(W, pl, x0, x1, x2, lane, dc, 0.f, 1.f, logit, bce, dx);
        else
            decoder_tile<MODE_SUM, false, 1>(W, pl, x0, x1, x2, lane, dc, 0.f, 1.f, logit, bce, dx);
        if (lane < 16 && tile * 16 + lane < K) {
            logits[(size_t)cloud * K + tp] = logit;
            if (dlogit_dp != nullptr) {
                float* o = dlogit_dp + ((size_t)cloud * K + tp) * 3;
                o[0] = dx[0]; o[1] = dx[1]; o[2] = dx[2];
            }
        }
    }
}

__global__ __launch_bounds__(OPT_THREADS, 2) void repulsion_kernel(const float* __restrict__ p, int K,
                                                                    float* __restrict__ loss,
                                                                    float* __restrict__ grad,
                                                                    int32_t* __restrict__ knn_idx, RepConst rc) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4* X = LDS_AT(f32x4, smem, RepLds::X);
    long long* F = LDS_AT(long long, smem, RepLds::F);
    float* scratch = LDS_AT(float, smem, RepLds::SCRATCH);
    const int cloud = blockIdx.x, tid = threadIdx.x;
    const float* pc = p + (size_t)cloud * K * 3;
    const int pa = tid, pb = tid + OPT_THREADS;
    if (pa < K) X[pa] = f32x4{pc[3 * pa], pc[3 * pa + 1], pc[3 * pa + 2], 0.f};
    if (pb < K) X[pb] = f32x4{pc[3 * pb], pc[3 * pb + 1], pc[3 * pb + 2], 0.f};
    for (int i = tid; i < MAXK * 3; i += OPT_THREADS) F[i] = 0;
    __syncthreads();
    Top5 ta, tb;
    knn_scan2(X, K, pa, pb, ta, tb);
    float la = 0.f, lb = 0.f;
    long long gca[3] = {0, 0, 0}, gcb[3] = {0, 0, 0};
    if (pa < K) rep_point(X, F, pa, ta, rc, la, gca, grad != nullptr);
    if (pb < K) rep_point(X, F, pb, tb, rc, lb, gcb, grad != nullptr);
    if (knn_idx != nullptr) {
        if (pa < K) {
            int32_t* o = knn_idx + ((size_t)cloud * K + pa) * 5;
            o[0] = ta.i0; o[1] = ta.i1; o[2] = ta.i2; o[3] = ta.i3; o[4] = ta.i4;
        }
        if (pb < K) {
            int32_t* o = knn_idx + ((size_t)cloud * K + pb) * 5;
            o[0] = tb.i0; o[1] = tb.i1; o[2] = tb.i2; o[3] = tb.i3; o[4] = tb.i4;
        }
    }
    const float tot = block_sum((pa < K ? la : 0.f) + (pb < K ? lb : 0.f), scratch);
    if (tid == 0) loss[cloud] = tot / ((float)K * 5.f);
    if (grad != nullptr) {
        const float sc = 1.f / ((float)K * 5.f);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int pt = q ? pb : pa;
            if (pt < K)
#pragma unroll
                for (int a = 0; a < 3; ++a)
                    grad[((size_t)cloud * K + pt) * 3 + a] =
                        __ll2float_rn(F[3 * pt + a] + (q ? gcb[a] : gca[a])) * FIX_INV * sc;
        }
    }
}

__global__ __launch_bounds__(OPT_THREADS, 2) void normalize_kernel(float* __restrict__ p, int K) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    f32x4* X = LDS_AT(f32x4, smem, NrmLds::X);
    float* scratch = LDS_AT(float, smem, NrmLds::SCRATCH);
    float* pc = p + (size_t)blockIdx.x * K * 3;
    const int pa = threadIdx.x, pb = threadIdx.x + OPT_THREADS;
    if (pa < K) X[pa] = f32x4{pc[3 * pa], pc[3 * pa + 1], pc[3 * pa + 2], 0.f};
    if (pb < K) X[pb] = f32x4{pc[3 * pb], pc[3 * pb + 1], pc[3 * pb + 2], 0.f};
    __syncthreads();
    normalize_in_lds(X, K, scratch);
    if (pa < K) { pc[3 * pa] = X[pa].x; pc[3 * pa + 1] = X[pa].y; pc[3 * pa + 2] = X[pa].z; }
    if (pb < K) { pc[3 * pb] = X[pb].x; pc[3 * pb + 1] = X[pb].y; pc[3 * pb + 2] = X[pb].z; }
}

// ---------------------------------------------------------------------------------------------
// Clouds of more than MAXK optimised points (--sample_npoint up to LARGE_MAXK = 10,000)
// ---------------------------------------------------------------------------------------------
// The persistent kernel keeps a cloud's whole optimiser state in one CU's LDS, which ends at 1024 points; the reference
// has no such limit (opt_defense.py:27).  Larger clouds run the same arithmetic as two launches per Adam step:
//   large_occupancy_kernel   decoder forward + input-backward of every point (the stand-alone tile, BCE seed) -> G
//   large_step_kernel        one workgroup per cloud: exact 5-NN by brute-force scan, repulsion terms into the same
//                            fixed-point accumulators, Adam (moments in global memory), new points
// The neighbour search is O(K^2) per step here (no certified lists) - a correct path for the rare large request, not a
// tuned one: ~4x (K = 2048) to ~20x (K = 4096) the per-point cost of the persistent kernel.  Up to LARGE_LDS_MAXK = 4096
// points the fixed-point repulsion accumulators sit in LDS next to the positions (28 bytes per point); above (GF = true) only
// the positions do (16 bytes per point: 10,000 points fill the LDS) and the accumulators are integer atomics on a global
// buffer of the workspace - the same integer sums.
constexpr int LARGE_PPT = (LARGE_MAXK + LARGE_THREADS - 1) / LARGE_THREADS + ((LARGE_MAXK + LARGE_THREADS - 1) / LARGE_THREADS & 1);   // points per thread: 10 (even)

struct LargeLds {
    f32x4* X;
    RepAcc F;
    float* scratch;
};
// f_ws (GF): [B][K] packed xy sums, then [B][K] z sums (large_f_bytes); zero on entry, left zero on exit
template <bool GF>
__device__ __forceinline__ LargeLds large_lds(float* smem, int K, int B, int cloud, void* f_ws) {
    const LargeLdsAt at = large_lds_at<GF>(K);
    LargeLds l;
    l.X = LDS_AT(f32x4, smem, at.X);
    if (GF) {
        l.F.xy = static_cast<long long*>(f_ws) + (size_t)cloud * K;
        l.F.z = reinterpret_cast<int*>(static_cast<long long*>(f_ws) + (size_t)B * K) + (size_t)cloud * K;
        l.scratch = LDS_NEXT(float, l.X, at.X, at.SCRATCH);
    } else {
        l.F.xy = LDS_AT(long long, smem, at.F_XY);
        l.F.z = LDS_AT(int, smem, at.F_Z);
        l.scratch = LDS_AT(float, smem, at.SCRATCH);
    }
    return l;
}
size_t large_f_bytes(int B, int K) { return K <= LARGE_LDS_MAXK ? 0 : (size_t)B * K * 12; }
// what a point received (GF: read past the L1 - the sums were made by atomics in the L2 - and cleared for the next step)
template <bool GF>
__device__ __forceinline__ void large_take_f(const RepAcc F, int pt, int (&fi)[3], unsigned long long* status = nullptr) {
    if (GF) {
        const long long fxy = (long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(F.xy + pt), __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_AGENT);
        fi[2] = __hip_atomic_load(F.z + pt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unpack_xy(fxy, fi[0], fi[1]);
        F.xy[pt] = 0;
        F.z[pt] = 0;
    } else {
        unpack_xy(F.xy[pt], fi[0], fi[1]);
        fi[2] = F.z[pt];
    }
    rep_overflow_check(fi, status);
}

// exact 5-NN + repulsion terms of the points of this thread, two at a time (the persistent kernel's rep_point2)
__device__ __forceinline__ void large_knn_rep(const LargeLds& l, int K, const RepConst rc, float (&rep_l)[LARGE_PPT],
                                              int32_t* __restrict__ knn_idx, bool ref_form = false) {
    const int tid = threadIdx.x;
#pragma unroll 1
    for (int r = 0; r < LARGE_PPT; r += 2) {
        if (r * LARGE_THREADS >= K) break;                                            // block-uniform
        const int pa = tid + r * LARGE_THREADS, pb = pa + LARGE_THREADS;
        Top5 ta, tb;
        if (ref_form) knn_scan_ref2(l.X, K, pa, pb, ta, tb);        // validation: the reference's neighbour choice bug for bug (knn_device.h)
        else knn_scan2(l.X, K, pa, pb, ta, tb);
        float la, lb;
        rep_point2(l.X, l.F, K, pa, pb, ta, tb, rc, la, lb);
        rep_l[r] = pa < K ? la : 0.f;
        rep_l[r + 1] = pb < K ? lb : 0.f;
        if (knn_idx != nullptr) {
            if (pa < K) { int32_t* o = knn_idx + (size_t)pa * 5; o[0] = ta.i0; o[1] = ta.i1; o[2] = ta.i2; o[3] = ta.i3; o[4] = ta.i4; }
            if (pb < K) { int32_t* o = knn_idx + (size_t)pb * 5; o[0] = tb.i0; o[1] = tb.i1; o[2] = tb.i2; o[3] = tb.i3; o[4] = tb.i4; }
        }
    }
}

template <bool GF>
__global__ __launch_bounds__(LARGE_THREADS) void large_step_kernel(float* __restrict__ p, float* __restrict__ m_io,
                                                                    float* __restrict__ v_io, const f32x4* __restrict__ G,
                                                                    int K, const float* __restrict__ adam_tab, int step,
                                                                    const int32_t* __restrict__ loss_batch_per_cloud,
                                                                    int loss_batch, float rep_weight, RepConst rc,
                                                                    float* __restrict__ loss_out, void* f_ws,
                                                                    unsigned long long* status, int ref_form) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int cloud = blockIdx.x, tid = threadIdx.x;
    const LargeLds l = large_lds<GF>(smem, K, (int)gridDim.x, cloud, f_ws);
    float* pc = p + (size_t)cloud * K * 3;
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
        if (pt < K) l.X[pt] = f32x4{pc[3 * pt], pc[3 * pt + 1], pc[3 * pt + 2], 0.f};
        if (!GF && pt < LARGE_LDS_MAXK) { l.F.xy[pt] = 0; l.F.z[pt] = 0; }
    }
    __syncthreads();
    float rep_l[LARGE_PPT];
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) rep_l[r] = 0.f;
    if (rep_weight > 0.f) large_knn_rep(l, K, rc, rep_l, nullptr, ref_form != 0);
    __syncthreads();
    const int lb = loss_batch_per_cloud ? loss_batch_per_cloud[cloud] : loss_batch;
    const float rep_scale = rep_weight / ((float)lb * (float)K * 5.f);
    const float step_size = adam_tab[2 * step], bc2 = adam_tab[2 * step + 1];
    float occ = 0.f, rep = 0.f;
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
        if (pt >= K) continue;
        const f32x4 go = G[(size_t)cloud * K + pt];
        const f32x4 x = l.X[pt];
        const float gocc[3] = {go.x, go.y, go.z};
        float xs[3] = {x.x, x.y, x.z};
        int fi[3];
        large_take_f<GF>(l.F, pt, fi, status);
        const size_t o = ((size_t)cloud * K + pt) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                         // the persistent kernel's adam_phase, term by term
            const float gn = (float)fi[a] * FIX32_INV;
            const float g = __builtin_fmaf(gn, rep_scale, gocc[a]);
            float mr = m_io[o + a], vr = v_io[o + a];
            mr = __builtin_fmaf(g - mr, 1.f - 0.9f, mr);
            vr = __builtin_fmaf((1.f - 0.999f) * g, g, vr * 0.999f);
            const float denom = sqrtf(vr) / bc2 + 1e-8f;
            xs[a] = __builtin_fmaf(-step_size, mr / denom, xs[a]);
            m_io[o + a] = mr;
            v_io[o + a] = vr;
            pc[3 * pt + a] = xs[a];
        }
        occ += go.w;
        rep += rep_l[r];
    }
    if (loss_out != nullptr) {                                // losses at the pre-update points of this (the last) step
        occ = block_sum(occ, l.scratch);
        rep = block_sum(rep, l.scratch);
        if (tid == 0) { loss_out[2 * cloud] = occ; loss_out[2 * cloud + 1] = rep / ((float)K * 5.f); }
    }
}

// ---------------------------------------------------------------------------------------------
// Certified neighbour lists of the launch-per-step path (1025 ... LARGE_LDS_MAXK points; round 6).
//
// large_step_kernel above ranks all K candidates for every point at every step: O(K^2), 2.5 x the per-point cost of the persistent
// kernel at K = 2048.  The reference does the same (defense/pn_utils.py:72-83) - but the answer is the exact 5-NN set either way, and
// between two steps a point moves by ~lr.  large_step_lists_kernel keeps, per point i, the LL_M-entry list of EVERY point that was
// closer than rho_i when the list was built (global memory, 64 bytes per point), and certifies per step that the list still holds
// the five nearest (same inequality as the persistent kernel's lists):
//       r5 < rho_i - |x_i - x_i(t_i)| - (S(now) - S(t_i))
// (a point outside the list was >= rho_i away at build time t_i and every point has moved by at most S(now) - S(t_i) since, S(t) = the
// running sum of the per-step maxima max_j |x_j(s + 1) - x_j(s)|: no epochs, no second position array).  Evaluation: 32-bit keys
// (distance bits | index) through the sorted top-6 network of knn_device.h - the five smallest keys are the five nearest list members
// unless keys 5 and 6 tie above the index bits.
//   * certificate holds, no tie: the five neighbours are the exact 5-NN; repulsion terms at once (rep_point2);
//   * otherwise the point goes to an LDS queue; after a barrier the queued points are shared out FOUR LANES each: one pass over the K
//     candidates gives the exact 5-NN in the scan's own order (per-lane sorted top-5, merged by (distance, index)) and writes the point's
//     new list (radius^2 = the point's own alpha x the failed list's upper bound of d5^2; the nearest hit that did not fit caps the
//     certified radius; a useless list is collected once more around the exact d5), then its terms are added;
//   * the first step of a call: every thread runs the exact scan for its points (knn_scan2: the brute-force kernel's code) and builds
//     their lists itself.  There is NO later whole-cloud rebuild: the step is one launch for all clouds, so a rebuild of any one cloud
//     would set the duration of that step for all of them (measured: epochs every ~7 steps per cloud made EVERY step an epoch step,
//     profiles/r06_time_large_k.txt) - expiring lists are renewed one point at a time instead, a few per cent of the points per step.
// Every path selects the five smallest (distance, index) pairs and the repulsion sums are fixed point: outputs are bit-identical to
// large_step_kernel's (ifd_opt_params.knn_scan_every_step selects that kernel; tests/test_gpu_parity.py holds the two against each other).
// ---------------------------------------------------------------------------------------------
constexpr int LL_M = 64;                            // list entries per point (128 bytes)
constexpr unsigned int LL_IDX_MASK = 8191u;         // 13 index bits: 0 ... LARGE_LDS_MAXK (the dummy entry)
constexpr int LL_DUMMY = LARGE_LDS_MAXK;            // X[LL_DUMMY]: a far-away point (unused list slots)
constexpr float LL_ALPHA = 6.4f;                    // first rho^2 = LL_ALPHA d5^2: ~32 of the 64 entries on a surface, slack rho - r5 = 1.5 r5
constexpr int LL_Q = LL_M / 4;                      // a renewed list is written by four lanes, a quarter each
// (the one layout of the lists' workspace: its count on a null base is large_list_bytes)
LargeLists large_lists(Carve& c, int B, int K) {
    LargeLists L;
    L.cert = c.take<f32x4>((size_t)B * K * 16);
    L.lists = c.take<uint16_t>((size_t)B * K * LL_M * 2);
    L.dbase = c.take<f32x2>((size_t)B * K * 8);
    L.scal = c.take<float>((size_t)B * 16);
    return L;
}
size_t large_list_bytes(int B, int K) {
    Carve c(nullptr);
    if (K <= LARGE_LDS_MAXK) large_lists(c, B, K);
    return c.bytes();
}

__device__ __forceinline__ float ll_dist2(const f32x4& a, const f32x4& b) {
    const float ex = a.x - b.x, ey = a.y - b.y, ez = a.z - b.z;
    return fmaf(ez, ez, fmaf(ey, ey, ex * ex));                  // knn_scan2's expression
}
// one thread builds the list of its point i: every j != i with |x_j - x_i|^2 < r2, r2 = LL_ALPHA d5^2, or half that if that ball
// holds more than LL_M points; returns rho (0: no valid list)
__device__ __forceinline__ float ll_build_thread(const f32x4* __restrict__ X, int K, int i, float d5sq, uint16_t* __restrict__ lst) {
    const f32x4 xi = X[i];
    float rho = 0.f;
#pragma unroll 1
    for (int attempt = 0; attempt < 2; ++attempt) {
        const float r2 = (attempt == 0 ? LL_ALPHA : 0.5f * LL_ALPHA) * d5sq;
        int cnt = 0;
#pragma unroll 4
        for (int j = 0; j < K; ++j) {
            const float d = ll_dist2(X[j], xi);
            if (d < r2 && j != i) {
                if (cnt < LL_M) lst[cnt] = (uint16_t)j;
                ++cnt;
            }
        }
        if (cnt <= LL_M) {
            for (int e = cnt; e < LL_M; ++e) lst[e] = (uint16_t)LL_DUMMY;
            rho = sqrtf(r2);
            break;
        }
    }
    return rho;
}
// keys of the two points' lists (list_keys6_2 with 13 index bits and LL_M entries; the index words in two halves: 128 registers)
__device__ __forceinline__ void ll_keys2(const f32x4* __restrict__ X, const uint16_t* __restrict__ La, const uint16_t* __restrict__ Lb,
                                         int ia, int ib, Keys6& qa, Keys6& qb) {
    const f32x4 xa = X[ia], xb = X[ib];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        u32x4 wa[LL_M / 16], wb[LL_M / 16];
#pragma unroll
        for (int c = 0; c < LL_M / 16; ++c) {
            wa[c] = reinterpret_cast<const u32x4*>(La)[half * (LL_M / 16) + c];
            wb[c] = reinterpret_cast<const u32x4*>(Lb)[half * (LL_M / 16) + c];
        }
#pragma unroll
        for (int c = 0; c < LL_M / 8; ++c) {                                              // four entries of each list at a time
            unsigned int ja[4], jb[4];
            f32x4 pa_[4], pb_[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned int pka = wa[c >> 1][2 * (c & 1) + (e >> 1)], pkb = wb[c >> 1][2 * (c & 1) + (e >> 1)];
                ja[e] = (e & 1) ? (pka >> 16) : (pka & 0xffffu);
                jb[e] = (e & 1) ? (pkb >> 16) : (pkb & 0xffffu);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { pa_[e] = X[ja[e]]; pb_[e] = X[jb[e]]; }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                keys6_insert(qa, (__float_as_uint(ll_dist2(pa_[e], xa)) & ~LL_IDX_MASK) | ja[e]);
                keys6_insert(qb, (__float_as_uint(ll_dist2(pb_[e], xb)) & ~LL_IDX_MASK) | jb[e]);
            }
        }
    }
}
// the five smallest keys as neighbour indices + whether they are certified to be the exact 5-NN of the point
__device__ __forceinline__ bool ll_certify(const Keys6& q, const f32x4& x, const f32x4& cert, float dsum, Top5& t, float& d5ub) {
    t.i0 = (int)(q.k0 & LL_IDX_MASK); t.i1 = (int)(q.k1 & LL_IDX_MASK); t.i2 = (int)(q.k2 & LL_IDX_MASK);
    t.i3 = (int)(q.k3 & LL_IDX_MASK); t.i4 = (int)(q.k4 & LL_IDX_MASK);
    t.d0 = t.d1 = t.d2 = t.d3 = t.d4 = 0.f;
    const bool tie = ((q.k4 ^ q.k5) & ~LL_IDX_MASK) == 0u;
    d5ub = q.k4 >= 0x7f800000u ? INFINITY : __uint_as_float(q.k4 | LL_IDX_MASK);       // upper bound of the squared 5th distance:
    const float r5 = sqrtf(d5ub);                                                       // the list's 5th nearest is no nearer than the true one
    const float ex = x.x - cert.x, ey = x.y - cert.y, ez = x.z - cert.z;
    const float moved = sqrtf(fmaf(ez, ez, fmaf(ey, ey, ex * ex)));
    // (strict, with room for the roundings of the three square roots and of D: all O(1e-7) relative)
    return !tie && cert.w > 0.f && (r5 + moved + dsum) * 1.00001f + 1e-7f < cert.w;
}

__global__ __launch_bounds__(LARGE_THREADS) void large_step_lists_kernel(float* __restrict__ p, float* __restrict__ m_io,
                                                                          float* __restrict__ v_io, const f32x4* __restrict__ G,
                                                                          int K, const float* __restrict__ adam_tab, int step,
                                                                          const int32_t* __restrict__ loss_batch_per_cloud,
                                                                          int loss_batch, float rep_weight, RepConst rc,
                                                                          float* __restrict__ loss_out, LargeLists L,
                                                                          unsigned long long* status) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int cloud = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    using Lds = LargeListsLds;
    f32x4* X = LDS_AT(f32x4, smem, Lds::X);
    long long* fxy = LDS_AT(long long, smem, Lds::F_XY);
    int* fz = LDS_AT(int, smem, Lds::F_Z);
    const RepAcc Fz = {fxy, fz};                                                      // fixed-point repulsion sums (knn_device.h)
    float* RL = LDS_AT(float, smem, Lds::RL);
    float* scratch = LDS_AT(float, smem, Lds::SCRATCH);
    int* qn = LDS_AT(int, smem, Lds::QN);
    float* qd5 = LDS_AT(float, smem, Lds::QD5);
    uint16_t* queue = LDS_AT(uint16_t, smem, Lds::QUEUE);
    float* BB = LDS_AT(float, smem, Lds::BB);
    const size_t cb = (size_t)cloud * K;
    float* pc = p + cb * 3;
    constexpr int PPT = LARGE_LDS_MAXK / LARGE_THREADS;                               // 4 points per thread
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
        if (pt < K) X[pt] = f32x4{pc[3 * pt], pc[3 * pt + 1], pc[3 * pt + 2], 0.f};
        Fz.xy[pt] = 0; Fz.z[pt] = 0; RL[pt] = 0.f; qd5[pt] = -1.f;
    }
    if (tid == 0) { *qn = 0; X[LL_DUMMY] = f32x4{1e18f, 1e18f, 1e18f, 0.f}; }
#ifdef IFD_PROF
    // -DIFD_PROF (scripts/build_variant.sh prof): cycles of cloud 0's phases summed over the call into the counter slots 8 ... 12
    unsigned long long pt_[6];
#define LL_STAMP(k) do { __syncthreads(); pt_[k] = __builtin_readcyclecounter(); } while (0)
#else
#define LL_STAMP(k)
#endif
    LL_STAMP(0);
    const bool epoch = step == 0;                                                     // the call's first step: every list is built
    const float d_now = epoch ? 0.f : L.scal[4 * cloud + 0];                          // S(now)
    __syncthreads();
    if (rep_weight > 0.f) {
#pragma unroll 1
        for (int r = 0; r < PPT; r += 2) {
            if (r * LARGE_THREADS >= K) break;                                        // block-uniform
            const int pa = tid + r * LARGE_THREADS, pb = pa + LARGE_THREADS;
            const bool va = pa < K, vb = pb < K;
            const int ia = min(pa, K - 1), ib = min(pb, K - 1);
            Top5 ta, tb;
            bool oka = va, okb = vb;
            if (epoch) {
                knn_scan2(X, K, pa, pb, ta, tb);
                if (va) {
                    const float rho = ll_build_thread(X, K, pa, ta.d4, L.lists + (cb + pa) * LL_M);
                    const f32x4 x = X[pa];
                    L.cert[cb + pa] = f32x4{x.x, x.y, x.z, rho};
                    L.dbase[cb + pa] = f32x2{0.f, LL_ALPHA};
                }
                if (vb) {
                    const float rho = ll_build_thread(X, K, pb, tb.d4, L.lists + (cb + pb) * LL_M);
                    const f32x4 x = X[pb];
                    L.cert[cb + pb] = f32x4{x.x, x.y, x.z, rho};
                    L.dbase[cb + pb] = f32x2{0.f, LL_ALPHA};
                }
            } else {
                Keys6 qa, qb;
                keys6_init(qa);
                keys6_init(qb);
                ll_keys2(X, L.lists + (cb + ia) * LL_M, L.lists + (cb + ib) * LL_M, ia, ib, qa, qb);
                float ua, ub;
                oka = va && ll_certify(qa, X[ia], L.cert[cb + ia], (d_now - L.dbase[cb + ia].x) * 1.00001f, ta, ua);
                okb = vb && ll_certify(qb, X[ib], L.cert[cb + ib], (d_now - L.dbase[cb + ib].x) * 1.00001f, tb, ub);
                if (va && !oka) qd5[pa] = fmaxf(ua, 0.f);                              // queued (by point: the queue itself is compacted in
                if (vb && !okb) qd5[pb] = fmaxf(ub, 0.f);                              // index order below)
            }
            float la, lb;
            rep_point2(X, Fz, K, oka ? pa : K, okb ? pb : K, ta, tb, rc, la, lb);
            if (oka) RL[pa] = la;
            if (okb) RL[pb] = lb;
        }
        __syncthreads();
        LL_STAMP(1);
        // ---- the queued points: FOUR LANES each (16 points side by side in a wave).  Measured on the way (profiles/r06_time_large_k*):
        //      one point per WAVE with cross-lane minima costs 3 x the brute-force kernel's thread-level scan per point; one point per
        //      THREAD leaves 2 - 3 lone, latency-bound waves walking all K candidates while 13 idle (0.88 ms per step at K = 2048, more
        //      than the brute-force kernel's 0.66).  Lane s of a quad walks the candidates j = s (mod 4) ONCE: it keeps its own exact
        //      sorted top-5 (knn_scan2's insertion, ascending index) and writes the candidates inside the new ball - radius^2 = the
        //      point's alpha x the failed list's own upper bound of d5^2 - into ITS quarter of the list; a hit that finds its quarter
        //      full is dropped and caps the certified radius at its distance (every point nearer than the nearest dropped hit is in the
        //      list).  The four top-5 are merged by (distance, index) through DPP, so every lane ends with the scan's exact answer.
        //      A list that came out useless (no bound to start from, or rho <= r5) is collected once more around the exact d5. -------
        // The queue in INDEX order (a block-wide prefix sum over the per-point flags, four consecutive points per thread): the initial points
        // leave ifd_prepare in Morton order and move little, so the 16 points a wave takes are neighbours in space - and so are the 128
        // consecutive candidates of a block, whose bounding box lets the whole wave skip it when none of its points' balls reaches it.
        {
            int mine = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) mine += (4 * tid + e < K && qd5[4 * tid + e] >= 0.f) ? 1 : 0;
            int incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
            int* wtot = reinterpret_cast<int*>(scratch);
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            int before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < LARGE_THREADS / 64; ++w) { const int tw = wtot[w]; before += w < wave ? tw : 0; all += tw; }
            int at = before + incl - mine;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * tid + e < K && qd5[4 * tid + e] >= 0.f) queue[at++] = (uint16_t)(4 * tid + e);
            if (tid == 0) *qn = all;
            // bounding boxes of the index blocks (wave w: blocks w, w + 16; two points per lane)
            for (int b = wave; b * LL_BLK < K; b += LARGE_THREADS / 64) {
                const int j0 = b * LL_BLK + lane, j1 = j0 + 64;
                const f32x4 p0 = X[min(j0, K - 1)], p1 = X[min(j1, K - 1)];            // (a clamped index repeats a point of the block or of an earlier one: the box only grows)
                const float lo[3] = {fminf(p0.x, p1.x), fminf(p0.y, p1.y), fminf(p0.z, p1.z)};
                const float hi[3] = {fmaxf(p0.x, p1.x), fmaxf(p0.y, p1.y), fmaxf(p0.z, p1.z)};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float mn = -wave_max(-lo[a]), mx = wave_max(hi[a]);
                    if (lane == 0) { BB[8 * b + a] = mn; BB[8 * b + 4 + a] = mx; }
                }
            }
            __syncthreads();
        }
        const int nq = *qn;
        const int sub = lane & 3;
#pragma unroll 1
        for (int base = 0; base < nq; base += LARGE_THREADS / 4) {                      // (block-uniform trip count)
            const int qi = base + (tid >> 2);
            const bool act = qi < nq;                                                   // quad-uniform
            if (__ballot(act) == 0ull) break;                                           // (no barrier in this loop: a wave without a point leaves)
            const int i = act ? (int)queue[qi] : 0;
            const f32x4 xi = X[i];
            uint16_t* lst = L.lists + (cb + i) * LL_M + sub * LL_Q;
            float alpha = act ? L.dbase[cb + i].y : LL_ALPHA;
            // d5 <= tins: only candidates this near can be among the five nearest - the sorted insertion (~30 vector instructions, and a
            // wave runs it whenever ONE of its 64 lanes needs it) is kept off the other ~2000 (measured: 486 -> see r06_time_large_k*)
            float tins = act ? qd5[i] : 0.f;
            float r2 = alpha * tins;
            if (!(r2 < 1e30f)) { r2 = 0.f; tins = INFINITY; }                          // (no usable bound: the second pass sets the radius)
            Top5 t;
            float cap2 = 0.f;
            int total = 0;
#pragma unroll 1
            for (int pass = 0; pass < 2; ++pass) {
#ifdef IFD_PROF
                const unsigned long long q0_ = __builtin_readcyclecounter();
#endif
                top5_init(t);
                int cnt = 0;
                float drop = INFINITY;
                // Branch-free over the candidates: 32 of the lane's candidates (j = w0 + 4 b + s) at a time, one bit each for "inside the
                // ball or possibly among the five nearest"; the few set bits are then handled one by one, in ascending j.  (With a
                // test-and-branch per candidate a wave ran the hit path whenever ONE of its 64 lanes had a hit - two iterations in three -
                // and the sorted insertion likewise: 345 - 486 cycles per candidate and wave, measured.)
                const float lim = fmaxf(r2, tins);                                     // (tins = INF without a bound: every candidate is looked at)
#pragma unroll 1
                for (int w0 = 0; w0 < K; w0 += LL_BLK) {
                    {   // squared distance from the point to the block's box: beyond lim for every point of the wave -> nothing to find there
                        const float* bb = BB + 8 * (w0 / LL_BLK);
                        const float ex = fmaxf(fmaxf(bb[0] - xi.x, xi.x - bb[4]), 0.f), ey = fmaxf(fmaxf(bb[1] - xi.y, xi.y - bb[5]), 0.f),
                                    ez = fmaxf(fmaxf(bb[2] - xi.z, xi.z - bb[6]), 0.f);
                        const float lb2 = fmaf(ez, ez, fmaf(ey, ey, ex * ex)) * 0.99999f;     // (rounded down: a lower bound)
                        if (__ballot(act && lb2 <= lim) == 0ull) continue;
                    }
                    unsigned int hit = 0u;
#pragma unroll 8
                    for (int bb = 0; bb < 32; ++bb) {
                        const float d = ll_dist2(X[min(w0 + 4 * bb + sub, LL_DUMMY)], xi);      // (beyond K: masked below)
                        hit |= (d <= lim ? 1u : 0u) << bb;
                    }
                    while (hit != 0u) {
                        const int j = w0 + 4 * __builtin_ctz(hit) + sub;
                        hit &= hit - 1u;
                        if (j >= K || j == i) continue;
                        const float d = ll_dist2(X[j], xi);
                        if (d <= tins) top5_insert(t, d, j);                            // ascending j within the lane: ties keep the smaller index
                        if (d < r2) {                                                   // (r2 = 0 for the quads without a point)
                            if (cnt < LL_Q) lst[cnt] = (uint16_t)j; else drop = fminf(drop, d);
                            ++cnt;
                        }
                    }
                }
#ifdef IFD_PROF
                const unsigned long long q1_ = __builtin_readcyclecounter();
#endif
                if (act)
                    for (int e = min(cnt, LL_Q); e < LL_Q; ++e) lst[e] = (uint16_t)LL_DUMMY;
                // merge the quad's four sorted top-5 (the other lanes' ORIGINAL entries, by rotation inside the quad)
                const Top5 o = t;
#define IFD_LL_MERGE(CTRL)                                                                                                         \
                {                                                                                                                  \
                    const float od[5] = {o.d0, o.d1, o.d2, o.d3, o.d4};                                                            \
                    const int oi[5] = {o.i0, o.i1, o.i2, o.i3, o.i4};                                                              \
                    _Pragma("unroll") for (int k = 0; k < 5; ++k) {                                                                \
                        const float dd = __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(od[k]), CTRL, 0xf, 0xf, false)); \
                        const int jj = __builtin_amdgcn_update_dpp(0, oi[k], CTRL, 0xf, 0xf, false);                               \
                        if (dd < t.d4 || (dd == t.d4 && jj < t.i4)) top5_insert_lex(t, dd, jj);                                    \
                    }                                                                                                              \
                }
                IFD_LL_MERGE(0x39)        // quad_perm [1, 2, 3, 0]
                IFD_LL_MERGE(0x4E)        // quad_perm [2, 3, 0, 1]
                IFD_LL_MERGE(0x93)        // quad_perm [3, 0, 1, 2]
#undef IFD_LL_MERGE
                // the quad's nearest dropped hit and its hit count
                drop = fminf(drop, __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(drop), 0xB1, 0xf, 0xf, false)));   // [1, 0, 3, 2]
                drop = fminf(drop, __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(drop), 0x4E, 0xf, 0xf, false)));   // [2, 3, 0, 1]
                total = cnt;
                total += __builtin_amdgcn_update_dpp(0, total, 0xB1, 0xf, 0xf, false);
                total += __builtin_amdgcn_update_dpp(0, total, 0x4E, 0xf, 0xf, false);
#ifdef IFD_PROF
                if (tid == 0 && cloud == 0 && status != nullptr) {
                    const unsigned long long q2_ = __builtin_readcyclecounter();
                    atomicAdd(status + 12, q1_ - q0_);          // candidate loop
                    atomicAdd(status + 13, q2_ - q1_);          // fill + merge
                    atomicAdd(status + 14, 1ull);               // passes of wave 0
                }
#endif
                cap2 = fminf(r2, drop);                                                 // everything nearer than this is in the list
                if (drop < INFINITY) alpha *= 0.8f;                                    // the ball was too crowded for a quarter: smaller next time
                else if (total < LL_M / 3) alpha *= 1.15f;                             // ... or mostly empty: larger
                alpha = fminf(fmaxf(alpha, 1.5f), 16.f);
                const bool again = act && pass == 0 && !(cap2 > t.d4);                 // useless list (quad-uniform): once more, around the exact d5
                if (__ballot(again) == 0ull) break;                                     // (wave-uniform exit)
                r2 = again ? alpha * t.d4 : 0.f;                                        // (the quads that are done collect nothing: their list stands)
                tins = t.d4;                                                            // (exact now)
                if (!again) break;
            }
            if (act && sub == 0) {
                L.cert[cb + i] = f32x4{xi.x, xi.y, xi.z, cap2 > t.d4 ? sqrtf(cap2) : 0.f};
                L.dbase[cb + i] = f32x2{d_now, alpha};
                float la, lb;
                rep_point2(X, Fz, K, i, K, t, t, rc, la, lb);
                RL[i] = la;
            }
        }
        __syncthreads();
        LL_STAMP(2);
        if (tid == 0 && status != nullptr) {                                            // diagnostics (ifd_get_counters)
            if (epoch) atomicAdd(status + 0, 1ull);                                     // (whole-cloud list builds: one per cloud and call)
            if (nq > 0) atomicAdd(status + 5, (unsigned long long)nq);
        }
    }
    const int lb_ = loss_batch_per_cloud ? loss_batch_per_cloud[cloud] : loss_batch;
    const float rep_scale = rep_weight / ((float)lb_ * (float)K * 5.f);
    const float step_size = adam_tab[2 * step], bc2 = adam_tab[2 * step + 1];
    float occ = 0.f, rep = 0.f, moved = 0.f;
#pragma unroll
    for (int r = 0; r < PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
        if (pt >= K) continue;
        const f32x4 go = G[cb + pt];
        const f32x4 x = X[pt];
        const float gocc[3] = {go.x, go.y, go.z};
        float xs[3] = {x.x, x.y, x.z};
        int fi[3];
        large_take_f<false>(Fz, pt, fi, status);
        const size_t o = (cb + pt) * 3;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                         // large_step_kernel's update, term by term
            const float gn = (float)fi[a] * FIX32_INV;
            const float g = __builtin_fmaf(gn, rep_scale, gocc[a]);
            float mr = m_io[o + a], vr = v_io[o + a];
            mr = __builtin_fmaf(g - mr, 1.f - 0.9f, mr);
            vr = __builtin_fmaf((1.f - 0.999f) * g, g, vr * 0.999f);
            const float denom = sqrtf(vr) / bc2 + 1e-8f;
            xs[a] = __builtin_fmaf(-step_size, mr / denom, xs[a]);
            m_io[o + a] = mr;
            v_io[o + a] = vr;
            pc[3 * pt + a] = xs[a];
        }
        occ += go.w;
        rep += RL[pt];
        // this step's move (an upper bound: rounded up a little)
        const float ex = xs[0] - x.x, ey = xs[1] - x.y, ez = xs[2] - x.z;
        moved = fmaxf(moved, sqrtf(fmaf(ez, ez, fmaf(ey, ey, ex * ex))) * 1.00001f);
    }
    const float dmax = block_max(moved, scratch);
    if (tid == 0) L.scal[4 * cloud + 0] = d_now + dmax;
    if (loss_out != nullptr) {                                // losses at the pre-update points of this (the last) step
        occ = block_sum(occ, scratch);
        rep = block_sum(rep, scratch);
        if (tid == 0) { loss_out[2 * cloud] = occ; loss_out[2 * cloud + 1] = rep / ((float)K * 5.f); }
    }
#ifdef IFD_PROF
    LL_STAMP(3);
    if (tid == 0 && cloud == 0 && status != nullptr && rep_weight > 0.f && !epoch) {
        atomicAdd(status + 8, pt_[1] - pt_[0]);      // load + list evaluation + certified points' terms
        atomicAdd(status + 9, pt_[2] - pt_[1]);      // the queued points
        atomicAdd(status + 10, pt_[3] - pt_[2]);     // Adam + displacement
        atomicAdd(status + 11, 1ull);
    }
#endif
#undef LL_STAMP
}

// repulsion_loss(p) for K > MAXK (ifd_repulsion): loss [B], optional gradient and neighbour indices
template <bool GF>
__global__ __launch_bounds__(LARGE_THREADS) void large_repulsion_kernel(const float* __restrict__ p, int K,
                                                                         float* __restrict__ loss, float* __restrict__ grad,
                                                                         int32_t* __restrict__ knn_idx, RepConst rc, void* f_ws) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int cloud = blockIdx.x, tid = threadIdx.x;
    const LargeLds l = large_lds<GF>(smem, K, (int)gridDim.x, cloud, f_ws);
    const float* pc = p + (size_t)cloud * K * 3;
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
        if (pt < K) l.X[pt] = f32x4{pc[3 * pt], pc[3 * pt + 1], pc[3 * pt + 2], 0.f};
        if (!GF && pt < LARGE_LDS_MAXK) { l.F.xy[pt] = 0; l.F.z[pt] = 0; }
    }
    __syncthreads();
    float rep_l[LARGE_PPT];
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) rep_l[r] = 0.f;
    large_knn_rep(l, K, rc, rep_l, knn_idx ? knn_idx + (size_t)cloud * K * 5 : nullptr);
    // (the thread's terms added in the order r = 0, 1, 2, ...: the four-point sum of the <= 4096-point layout is a prefix)
    float mine = rep_l[0];
#pragma unroll
    for (int r = 1; r < LARGE_PPT; ++r) mine += rep_l[r];
    const float tot = block_sum(mine, l.scratch);                                            // (barriers inside: F complete)
    if (tid == 0) loss[cloud] = tot / ((float)K * 5.f);
    if (grad != nullptr) {
        const float sc = 1.f / ((float)K * 5.f);
#pragma unroll
        for (int r = 0; r < LARGE_PPT; ++r) {
            const int pt = tid + r * LARGE_THREADS;
            if (pt >= K) continue;
            int fi[3];
            large_take_f<GF>(l.F, pt, fi);
#pragma unroll
            for (int a = 0; a < 3; ++a) grad[((size_t)cloud * K + pt) * 3 + a] = (float)fi[a] * FIX32_INV * sc;
        }
    }
}

// normalize_batch_pc (opt_defense.py:76-83) for K > MAXK
__global__ __launch_bounds__(LARGE_THREADS) void large_normalize_kernel(float* __restrict__ p, int K) {
    __shared__ float scratch[64];
    float* pc = p + (size_t)blockIdx.x * K * 3;
    const int tid = threadIdx.x;
    float x[LARGE_PPT][3];
    float s[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
#pragma unroll
        for (int a = 0; a < 3; ++a) { x[r][a] = pt < K ? pc[3 * pt + a] : 0.f; s[a] += x[r][a]; }
    }
    float c[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) c[a] = block_sum(s[a], scratch) / (float)K;
    float dm = 0.f;
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
#pragma unroll
        for (int a = 0; a < 3; ++a) x[r][a] -= c[a];
        if (pt < K) dm = fmaxf(dm, sqrtf(__builtin_fmaf(x[r][2], x[r][2], __builtin_fmaf(x[r][1], x[r][1], x[r][0] * x[r][0]))));     // (normalize_in_lds's form)
    }
    const float md = block_max(dm, scratch);
#pragma unroll
    for (int r = 0; r < LARGE_PPT; ++r) {
        const int pt = tid + r * LARGE_THREADS;
        if (pt < K)
#pragma unroll
            for (int a = 0; a < 3; ++a) pc[3 * pt + a] = x[r][a] / md;
    }
}

// ---------------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------------

size_t knn_list_bytes(int B) { return (size_t)B * MAXK * LIST_M * sizeof(uint16_t); }
// the exchange blocks of split clouds (at most one partial round of them per launch) sit behind the lists
constexpr int COOP_MAX_CLOUDS = 512;
// ... and behind them the Adam moments of the split-precision kernels (optimize_bf.hip: the piece image takes the moments' place in
// LDS): 24 KB per workgroup of the largest launch
// (optimize_ws: the one layout; its count on a null base is optimize_ws_bytes)
OptWs optimize_ws(Carve& c, int B) {
    OptWs w;
    w.knn_lists = c.take<uint16_t>(knn_list_bytes(B));
    w.coop = c.take<CoopWs>(COOP_MAX_CLOUDS * sizeof(CoopWs));
    w.mv = c.take<f32x4>((size_t)(max(B, COOP_MAX_CLOUDS) + 32) * 3 * OPT_THREADS * sizeof(f32x4));
    return w;
}
size_t optimize_ws_bytes(int B) { Carve c(nullptr); optimize_ws(c, B); return c.bytes(); }
hipError_t configure_optimize_bf_kernels();
hipError_t launch_part_bf(int S, int prec, const float* dec_img, const float* planes, float* p, float* m, float* v, float* loss,
                          const int32_t* lb, uint16_t* knn_lists, unsigned long long* counters, const float* adam_tab, int grid, int K,
                          const OptArgs& a, CoopWs* coop, int n, void* mv_ws, hipStream_t s);

hipError_t configure_optimize_kernels() {
    const hipError_t e = opt_in_dynamic_lds({{optimize_kernel<8, 1>, OptLds<0>::BYTES}, {optimize_kernel<8, 2>, OptLds<0>::BYTES},
                                             {optimize_kernel<8, 4>, OptLds<0>::BYTES}, {decode_kernel, DecImageLds<0>::BYTES},
                                             {large_occupancy3_kernel<0>, DecImageLds<0>::BYTES}, {large_step_lists_kernel, LargeListsLds::BYTES},
                                             {large_step_kernel<false>, large_lds_bytes(LARGE_LDS_MAXK)}, {large_step_kernel<true>, large_lds_bytes(LARGE_MAXK)},
                                             {large_repulsion_kernel<false>, large_lds_bytes(LARGE_LDS_MAXK)},
                                             {large_repulsion_kernel<true>, large_lds_bytes(LARGE_MAXK)}});
    return e != hipSuccess ? e : configure_optimize_bf_kernels();
}

// One launch of `n` clouds starting at cloud `c0`, S workgroups per cloud.
template <int S>
static hipError_t launch_part(const float* dec_img, const float* planes, float* p, float* m, float* v, float* loss,
                              const int32_t* lb, uint16_t* knn_lists, unsigned long long* counters, const float* adam_tab,
                              int c0, int n, int K, const OptArgs& a, CoopWs* coop, void* mv_ws, hipStream_t s) {
    const size_t o3 = (size_t)c0 * K * 3;
    const int grid = S == 1 ? n : ((n + 7) / 8) * 8 * S;       // (split clouds: members 8 workgroups apart, see the kernel)
    if (S > 1) {
        hipError_t e = hipMemsetAsync(coop, 0, (size_t)n * sizeof(CoopWs), s);
        if (e != hipSuccess) return e;
    }
    if (a.precision != 0)
        return launch_part_bf(S, a.precision, dec_img, planes + (a.planes_shared ? 0 : (size_t)c0 * CLOUD_PLANE_FLOATS), p + o3,
                              m ? m + o3 : nullptr, v ? v + o3 : nullptr, loss ? loss + 2 * (size_t)c0 : nullptr, lb ? lb + c0 : nullptr,
                              knn_lists + (size_t)c0 * MAXK * LIST_M, counters, adam_tab, grid, K, a, coop, n, mv_ws, s);
    hipLaunchKernelGGL((optimize_kernel<8, S>), dim3(grid), dim3(512), OptLds<0>::BYTES, s, dec_img,
                       planes + (a.planes_shared ? 0 : (size_t)c0 * CLOUD_PLANE_FLOATS), p + o3, m ? m + o3 : nullptr,
                       v ? v + o3 : nullptr, loss ? loss + 2 * (size_t)c0 : nullptr, lb ? lb + c0 : nullptr,
                       knn_lists + (size_t)c0 * MAXK * LIST_M, counters, adam_tab, K, a, coop, n);
    return hipGetLastError();
}

// The persistent optimiser over B clouds.  One workgroup fills one CU (154 KB of LDS, 8 waves of 256 VGPRs), so clouds run
// in rounds of n_cu.  split = 1: one workgroup per cloud throughout.  split = 0 (default): whole rounds likewise, but the
// clouds of the last, partial round are split over 4 CUs each (up to n_cu / 4 clouds: 0.41 of a round, measured) or 2 (up
// to n_cu / 2: 0.60 of a round) - a launch with fewer clouds than CUs, e.g. one GPU's shard of a file spread over 8 GPUs,
// otherwise costs a full round.  split = 2 / 4:
// every cloud split that way (validation: the results are bit-identical).  ws: neighbour lists of the B clouds, then the
// exchange blocks (optimize_ws_bytes).
hipError_t launch_optimize(const float* dec_img, const float* planes, float* p, float* m, float* v,
                           float* loss, const int32_t* loss_batch_per_cloud, void* ws,
                           unsigned long long* counters, const float* adam_tab, int B, int K, const OptArgs& a,
                           int split, int n_cu, hipStream_t s) {
    Carve c(ws);
    const OptWs w = optimize_ws(c, B);
    uint16_t* knn_lists = w.knn_lists;
    CoopWs* coop = w.coop;
    void* mv_ws = w.mv;
    n_cu = max(8, min(n_cu, COOP_MAX_CLOUDS));
    hipError_t e = hipSuccess;
#define IFD_PART(S_, c0_, n_) \
    launch_part<S_>(dec_img, planes, p, m, v, loss, loss_batch_per_cloud, knn_lists, counters, adam_tab, c0_, n_, K, a, coop, mv_ws, s)
    if (split == 2 || split == 4) {                  // every cloud split; all workgroups of a launch must be resident
        const int per = n_cu / split;
        for (int c0 = 0; c0 < B && e == hipSuccess; c0 += per)
            e = split == 2 ? IFD_PART(2, c0, min(per, B - c0)) : IFD_PART(4, c0, min(per, B - c0));
        return e;
    }
    if (split == 1 || K < 256) return IFD_PART(1, 0, B);      // (tiny clouds: nothing to share out)
    const int full = (B / n_cu) * n_cu, rest = B - full;
    // Measured per launch of n_cu / S clouds, in rounds of the unsplit kernel: S = 2 0.575, S = 4 0.365.  A rest
    // of more than n_cu / 2 clouds runs as one more unsplit round (DESIGN "Retired experiments": the mixed S = 2 + S = 4 tail).
    if (rest == 0 || 2 * rest > n_cu) return IFD_PART(1, 0, B);
    if (full > 0) e = IFD_PART(1, 0, full);
    if (e != hipSuccess) return e;
    return 4 * rest <= n_cu ? IFD_PART(4, full, rest) : IFD_PART(2, full, rest);
#undef IFD_PART
}

// Bias corrections of torch.optim.Adam for steps t0 + 1 ... t0 + steps (torch/optim/adam.py _single_tensor_adam:
// bias_correction1 = 1 - beta1 ** step, step_size = lr / bias_correction1, bias_correction2_sqrt = sqrt(1 - beta2 ** step),
// Python doubles there, doubles here), rounded to float where torch hands them to its float kernels.
__global__ void adam_table_kernel(float* __restrict__ tab, int t0, int steps, double lr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= steps) return;
    const double t = (double)(t0 + i + 1);
    tab[2 * i] = (float)(lr / (1.0 - pow(0.9, t)));
    tab[2 * i + 1] = (float)sqrt(1.0 - pow(0.999, t));
}

hipError_t launch_adam_table(float* tab, int t0, int steps, float lr, hipStream_t s) {
    if (steps <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_table_kernel, dim3((steps + 255) / 256), dim3(256), 0, s, tab, t0, steps, (double)lr);
    return hipGetLastError();
}

hipError_t launch_decode(const float* dec_img, const float* planes, const float* p, int B, int K,
                         float* logits, float* dlogit_dp, DecConst dc, hipStream_t s) {
    hipLaunchKernelGGL(decode_kernel, dim3(B), dim3(OPT_THREADS), DecImageLds<0>::BYTES, s, dec_img, planes, p, K, logits,
                       dlogit_dp, dc);
    return hipGetLastError();
}

hipError_t launch_repulsion(const float* p, int B, int K, float* loss, float* grad, int32_t* knn_idx,
                            float radius, float h, float eps, hipStream_t s) {
    RepConst rc = {radius, h, eps};
    hipLaunchKernelGGL(repulsion_kernel, dim3(B), dim3(OPT_THREADS), RepLds::BYTES, s, p, K, loss, grad, knn_idx, rc);
    return hipGetLastError();
}

// workspace of the launch-per-step path: [G: B K float4 | own moments (if the caller passes none) | global repulsion accumulators
// (K > LARGE_LDS_MAXK) | certified neighbour lists (K <= LARGE_LDS_MAXK)]
LargeWs large_ws(Carve& c, int B, int K, bool own_moments) {
    LargeWs w;
    w.G = c.take<f32x4>((size_t)B * K * 16);
    w.moments = c.take<float>(own_moments ? (size_t)B * K * 3 * 4 * 2 : 0);
    w.f = c.take<void>(large_f_bytes(B, K));
    c.round_up(16);
    w.lists = c.take<void>(large_list_bytes(B, K));
    return w;
}
size_t large_ws_bytes(int B, int K, bool own_moments) { Carve c(nullptr); large_ws(c, B, K, own_moments); return c.bytes(); }
void* large_list_ws(void* ws, int B, int K, bool own_moments) {
    Carve c(ws);
    return K <= LARGE_LDS_MAXK ? large_ws(c, B, K, own_moments).lists : nullptr;
}
// the repulsion accumulators of clouds beyond LARGE_LDS_MAXK points: the LAST large_f_bytes of the workspace, zeroed here
// (every step leaves them zero again)
hipError_t large_f_prepare(void* ws, int B, int K, bool own_moments, void** f_ws, hipStream_t s) {
    *f_ws = nullptr;
    if (K <= LARGE_LDS_MAXK) return hipSuccess;
    Carve c(ws);
    *f_ws = large_ws(c, B, K, own_moments).f;
    return hipMemsetAsync(*f_ws, 0, large_f_bytes(B, K), s);
}
// a.knn_scan_every_step: 0 = certified lists where they exist (K <= LARGE_LDS_MAXK and a list workspace), 1 = the exact brute-force
// scan at every step (validation; always beyond LARGE_LDS_MAXK points), 2 = the reference's neighbour choice (validation)
static void large_step_launch(float* p, float* m, float* v, const f32x4* G, int B, int K, const float* adam_tab, int step,
                              const int32_t* lbpc, const OptArgs& a, const RepConst& rc, float* loss, void* f_ws, void* list_ws,
                              unsigned long long* status, hipStream_t s) {
    const int ref_form = a.knn_scan_every_step == 2 ? 1 : 0;
    Carve lists_c(list_ws);
    if (K <= LARGE_LDS_MAXK && list_ws != nullptr && a.knn_scan_every_step == 0)
        hipLaunchKernelGGL(large_step_lists_kernel, dim3(B), dim3(LARGE_THREADS), LargeListsLds::BYTES, s, p, m, v, G, K, adam_tab, step, lbpc,
                           a.loss_batch, a.rep_weight, rc, loss, large_lists(lists_c, B, K), status);
    else if (K <= LARGE_LDS_MAXK)
        hipLaunchKernelGGL(large_step_kernel<false>, dim3(B), dim3(LARGE_THREADS), large_lds_bytes(K), s, p, m, v, G, K, adam_tab,
                           step, lbpc, a.loss_batch, a.rep_weight, rc, loss, f_ws, status, ref_form);
    else
        hipLaunchKernelGGL(large_step_kernel<true>, dim3(B), dim3(LARGE_THREADS), large_lds_bytes(K), s, p, m, v, G, K, adam_tab,
                           step, lbpc, a.loss_batch, a.rep_weight, rc, loss, f_ws, status, ref_form);
}

// ws: [B][K] f32x4 occupancy gradients, then (m == nullptr) the two moment arrays, zeroed here, then large_f_bytes
hipError_t launch_large_occupancy_bf(int prec, const float* dec_img, const float* planes, const float* p, int B, int parts, int K,
                                     const int32_t* lbpc, int loss_batch, float thr, int want_loss, f32x4* G, DecConst dc, hipStream_t s);
// The occupancy half of a step of the launch-per-step path: the occupancy gradient of every point of B clouds into G ([B, K] f32x4),
// in ifd_opt_params.precision's arithmetic (dec_img = the image of that precision).  One workgroup fills a CU (the persistent kernel's
// tile: 8 waves of 256 registers); `parts` workgroups of 8 waves share a cloud's (K / 32) tiles.  The step loop is api.cpp's
// (large_optimize_in_groups: stream groups, so that one group's occupancy launch fills the CUs another group's list step leaves idle).
hipError_t launch_large_occupancy(int precision, const float* dec_img, const float* planes, const float* p, int B, int parts, int K,
                                  const int32_t* loss_batch_per_cloud, int loss_batch, float thr, int want_loss, void* G, DecConst dc,
                                  hipStream_t s) {
    if (precision != 0)
        return launch_large_occupancy_bf(precision, dec_img, planes, p, B, parts, K, loss_batch_per_cloud, loss_batch, thr, want_loss,
                                         static_cast<f32x4*>(G), dc, s);
    hipLaunchKernelGGL(large_occupancy3_kernel<0>, dim3(B, parts), dim3(OPT_THREADS), DecImageLds<0>::BYTES, s, dec_img, planes, p, K,
                       loss_batch_per_cloud, loss_batch, thr, want_loss, static_cast<f32x4*>(G), dc);
    return hipGetLastError();
}

// One Adam step of the large-cloud path for any decoder (ConvONet above, ONet in onet.hip): G holds the occupancy gradient
// of every point (f32x4: d loss / d xyz, BCE term), large_step_kernel does the exact 5-NN, the repulsion terms and Adam.
// f_ws: large_f_prepare's pointer (nullptr up to LARGE_LDS_MAXK points); list_ws: large_list_ws's (nullptr beyond, or to force the scan)
hipError_t launch_large_step(float* p, float* m, float* v, const void* G, int B, int K, const float* adam_tab, int step,
                             const int32_t* loss_batch_per_cloud, const OptArgs& a, float* loss, void* f_ws, void* list_ws,
                             unsigned long long* counters, hipStream_t s) {
    const RepConst rc = {a.rep_radius, a.rep_h, a.rep_eps};
    large_step_launch(p, m, v, static_cast<const f32x4*>(G), B, K, adam_tab, step, loss_batch_per_cloud, a, rc, loss, f_ws, list_ws, counters, s);
    return hipGetLastError();
}

// f_ws: large_f_bytes(B, K) of scratch (any content; nullptr up to LARGE_LDS_MAXK points)
hipError_t launch_large_repulsion(const float* p, int B, int K, float* loss, float* grad, int32_t* knn_idx, float radius,
                                  float h, float eps, void* f_ws, hipStream_t s) {
    RepConst rc = {radius, h, eps};
    if (K <= LARGE_LDS_MAXK) {
        hipLaunchKernelGGL(large_repulsion_kernel<false>, dim3(B), dim3(LARGE_THREADS), large_lds_bytes(K), s, p, K, loss, grad,
                           knn_idx, rc, nullptr);
    } else {
        hipError_t e = hipMemsetAsync(f_ws, 0, large_f_bytes(B, K), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(large_repulsion_kernel<true>, dim3(B), dim3(LARGE_THREADS), large_lds_bytes(K), s, p, K, loss, grad,
                           knn_idx, rc, f_ws);
    }
    return hipGetLastError();
}

hipError_t launch_large_normalize(float* p, int B, int K, hipStream_t s) {
    hipLaunchKernelGGL(large_normalize_kernel, dim3(B), dim3(LARGE_THREADS), 0, s, p, K);
    return hipGetLastError();
}

hipError_t launch_normalize(float* p, int B, int K, hipStream_t s) {
    hipLaunchKernelGGL(normalize_kernel, dim3(B), dim3(OPT_THREADS), NrmLds::BYTES, s, p, K);
    return hipGetLastError();
}

}  // namespace ifd
