// The PointNet victim classifier of the reference (baselines/model/pointnet.py: PointNetCls, use_bn, eval mode), what
// baselines/inference.py runs on a restored cloud file.  Eval-mode BatchNorm is folded into the weights on the host.
//
//   point_stack_kernel  one per-point stack ending in the max over a cloud's points.  A workgroup (4 waves) owns 256 points of one
//                       cloud, a wave 64 of them as four 16-point MFMA tiles.  The three stacks of the network are instances:
//                         STN3d   xyz -> [3 -> 64] ReLU -> [64 -> 128] ReLU -> [128 -> 1024] ReLU -> max
//                         trunk   xyz . trans -> [3 -> 64] ReLU (-> . trans_feat) -> [64 -> 128] ReLU -> [128 -> 1024] -> max
//                         STNkd   xyz . trans -> [3 -> 64] ReLU -> [64 -> 64] ReLU -> [64 -> 128] ReLU -> [128 -> 1024] ReLU -> max
//                       The 64-wide trunk feature is recomputed from xyz where it is needed (51 FMAs a point) instead of being
//                       written out, and both bmm's of the reference (x . trans, feat . trans_feat) are the prologue of the
//                       stack that consumes them, in the reference's order (transform first, conv after: trans is NOT folded
//                       into conv1).  The 64- and 128-wide activations live in registers in MFMA operand layout; the 128 x 1024
//                       weight is streamed from global memory (every workgroup streams the same 512 KiB, which stays in L2),
//                       one 1 KiB tile per 16 MFMAs, prefetched one output tile ahead.  The [points, 1024] activations never
//                       exist: each 16-channel output tile is reduced to its maximum over the wave's valid points at once.
//   tile_max_kernel     the maxima of a cloud's 256-point tiles -> one [1024] row.  Max is exact and order-independent, so
//                       the result is bit-reproducible however the tiles were scheduled (no atomics, no initialisation pass).
//   fc_kernel           the FC stacks, batched over clouds: a wave = 16 clouds x 16 outputs, bias / ReLU / + identity epilogue.
//   argmax_kernel       lowest class among equal logits (torch.argmax on the CPU).
//
// Matrix layout: punet.hip's.  A wave holds 16 columns (points or clouds; lane l: column l & 15, quarter q = l >> 4); a
// 16-channel activation tile is one f32x4 per lane, register r = channel 16 t + 4 q + r.  The weight image stores, per (output
// tile m, input group g), the 64 lanes' f32x4 of W[16 m + (l & 15)][16 g + 4 (l >> 4) + 0..3].  Columns never mix: a cloud's
// result depends on nothing but its own rows, whatever shares its wave.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "victim_device.h"

namespace ifd {

namespace {

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 max4(f32x4 a, f32x4 b) {
    return f32x4{fmaxf(a[0], b[0]), fmaxf(a[1], b[1]), fmaxf(a[2], b[2]), fmaxf(a[3], b[3])};
}

constexpr int PT = 4;                   // 16-point tiles of one wave

// acc[t][m] = bias + W X_t for the MT output tiles of a layer with SG input groups, for the wave's PT point tiles: every weight
// tile is loaded once and used PT times.  wt(m, g) yields the lane's f32x4 of the weight tile, bias may be null (no bias).
template <int SG, int MT, bool RELU, class Wt>
__device__ __forceinline__ void dense(Wt wt, const float* __restrict__ bias, const f32x4 (&in)[PT][SG], f32x4 (&acc)[PT][MT]) {
    const int l = threadIdx.x & 63;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
        const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + 16 * m + 4 * (l >> 4)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < PT; ++t) acc[t][m] = bv;
    }
#pragma unroll
    for (int g = 0; g < SG; ++g) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const f32x4 a = wt(m, g);
#pragma unroll
            for (int t = 0; t < PT; ++t) acc[t][m] = mfma4(a, in[t][g], acc[t][m]);
        }
    }
    if (RELU) {
#pragma unroll
        for (int t = 0; t < PT; ++t)
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[t][m] = relu4(acc[t][m]);
    }
}

// trans: [B][16] (the 3 x 3 transform in the first 9), tfeat: [B][64][64]; either may be null.  part: [B][T][1024].
// KD: the STNkd stack (one more 64 -> 64 layer).  RELU_LAST: ReLU after the 1024-wide layer (the STNs; not the trunk).
// WIN (the input-gradient path, include/ifd_atk.h): also part_idx [B][T][1024], the point each maximum was taken from - the
// lowest index among equal values.  The maxima are computed exactly as without WIN; the index is found afterwards, by
// comparing against the finished maximum.
template <bool KD, bool RELU_LAST, bool WIN = false>
__global__ __launch_bounds__(256, 2) void point_stack_kernel(const float* __restrict__ img, ClsStack S, const float* __restrict__ pc,
                                                             const int32_t* __restrict__ n_points, int stride,
                                                             const float* __restrict__ trans, const float* __restrict__ tfeat,
                                                             float* __restrict__ part, int T, int32_t* __restrict__ part_idx = nullptr) {
    __shared__ __attribute__((aligned(16))) float red[4][CLS_FEAT];
    __shared__ __attribute__((aligned(16))) int32_t redi[WIN ? 4 : 1][WIN ? CLS_FEAT : 4];
    const int b = blockIdx.y, tile = blockIdx.x;
    int n = n_points ? n_points[b] : stride;
    n = min(max(n, 0), stride);
    if (tile * CLS_TILE >= n) return;                                  // the whole workgroup: nothing of this cloud here
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int base = tile * CLS_TILE + wv * 64;
    if (base >= n) {                                                   // the whole wave
        for (int c = l; c < CLS_FEAT; c += 64) {
            red[wv][c] = -INFINITY;
            if (WIN) redi[wv][c] = INT32_MAX;
        }
    } else {
        const float* P = pc + (size_t)b * stride * 3;
        bool valid[PT];
        f32x4 h[PT][4];
        {
            float tr[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            if (trans) {
#pragma unroll
                for (int k = 0; k < 9; ++k) tr[k] = trans[(size_t)b * 16 + k];
            }
            f32x4 w1[4][4];                                            // [channel tile][r] = {w0, w1, w2, bias} of channel 16 ct + 4 q + r
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                for (int r = 0; r < 4; ++r) w1[ct][r] = *reinterpret_cast<const f32x4*>(img + S.first + (16 * ct + 4 * q + r) * 4);
#pragma unroll
            for (int t = 0; t < PT; ++t) {
                const int i = base + 16 * t + p;
                valid[t] = i < n;
                float x = 0.f, y = 0.f, z = 0.f;
                if (valid[t]) { x = P[(size_t)i * 3]; y = P[(size_t)i * 3 + 1]; z = P[(size_t)i * 3 + 2]; }
                if (trans) {                                           // row vector times matrix: out_j = sum_i x_i trans[i][j]
                    const float xx = fmaf(z, tr[6], fmaf(y, tr[3], x * tr[0]));
                    const float yy = fmaf(z, tr[7], fmaf(y, tr[4], x * tr[1]));
                    const float zz = fmaf(z, tr[8], fmaf(y, tr[5], x * tr[2]));
                    x = xx; y = yy; z = zz;
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const f32x4 w = w1[ct][r];
                        h[t][ct][r] = fmaxf(fmaf(w[2], z, fmaf(w[1], y, fmaf(w[0], x, w[3]))), 0.f);
                    }
            }
        }
        if (tfeat) {                                                   // feat . trans_feat: W[o][i] = trans_feat[i][o], no bias
            const float* TF = tfeat + (size_t)b * 4096;
            f32x4 hf[PT][4];
            dense<4, 4, false>([&](int m, int g) {
                const float* c = TF + (16 * g + 4 * q) * 64 + 16 * m + p;
                return f32x4{c[0], c[64], c[128], c[192]};
            }, nullptr, h, hf);
#pragma unroll
            for (int t = 0; t < PT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) h[t][g] = hf[t][g];
        }
        if (KD) {
            f32x4 hm[PT][4];
            dense<4, 4, true>([&](int m, int g) { return *reinterpret_cast<const f32x4*>(img + S.mid_w + ((m * 4 + g) * 64 + l) * 4); },
                              img + S.mid_b, h, hm);
#pragma unroll
            for (int t = 0; t < PT; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) h[t][g] = hm[t][g];
        }
        f32x4 a2[PT][8];
        dense<4, 8, true>([&](int m, int g) { return *reinterpret_cast<const f32x4*>(img + S.w2 + ((m * 4 + g) * 64 + l) * 4); },
                          img + S.b2, h, a2);
        // the 1024-wide layer, one 16-channel output tile at a time; the next tile's weights are in flight during this one's MFMAs
        const float* W3 = img + S.w3 + l * 4;
        const float* B3 = img + S.b3 + 4 * q;
        f32x4 cur[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) cur[g] = *reinterpret_cast<const f32x4*>(W3 + g * 256);
#pragma unroll 1
        for (int m = 0; m < CLS_FEAT / 16; ++m) {
            const int mn = min(m + 1, CLS_FEAT / 16 - 1);
            f32x4 nxt[8];
#pragma unroll
            for (int g = 0; g < 8; ++g) nxt[g] = *reinterpret_cast<const f32x4*>(W3 + (size_t)(mn * 8 + g) * 256);
            const f32x4 bv = *reinterpret_cast<const f32x4*>(B3 + 16 * m);
            f32x4 acc[PT];
#pragma unroll
            for (int t = 0; t < PT; ++t) acc[t] = bv;
#pragma unroll
            for (int g = 0; g < 8; ++g)
#pragma unroll
                for (int t = 0; t < PT; ++t) acc[t] = mfma4(cur[g], a2[t][g], acc[t]);
            f32x4 r = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
            for (int t = 0; t < PT; ++t) {
                const f32x4 v = RELU_LAST ? relu4(acc[t]) : acc[t];
                if (valid[t]) r = max4(r, v);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x = r[k];
                x = fmaxf(x, __shfl_xor(x, 1)); x = fmaxf(x, __shfl_xor(x, 2));
                x = fmaxf(x, __shfl_xor(x, 4)); x = fmaxf(x, __shfl_xor(x, 8));
                r[k] = x;
            }
            if (p == 0) *reinterpret_cast<f32x4*>(&red[wv][16 * m + 4 * q]) = r;
            if (WIN) {                                                 // the lowest point of this wave that holds the maximum
                i32x4 wi = i32x4{INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};
#pragma unroll
                for (int t = PT - 1; t >= 0; --t) {
                    const f32x4 v = RELU_LAST ? relu4(acc[t]) : acc[t];
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (valid[t] && v[k] == r[k]) wi[k] = base + 16 * t + p;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int x = wi[k];
                    x = min(x, __shfl_xor(x, 1)); x = min(x, __shfl_xor(x, 2));
                    x = min(x, __shfl_xor(x, 4)); x = min(x, __shfl_xor(x, 8));
                    wi[k] = x;
                }
                if (p == 0) *reinterpret_cast<i32x4*>(&redi[wv][16 * m + 4 * q]) = wi;
            }
#pragma unroll
            for (int g = 0; g < 8; ++g) cur[g] = nxt[g];
        }
    }
    __syncthreads();
    const int c = threadIdx.x * 4;
    const f32x4 r = max4(max4(*reinterpret_cast<const f32x4*>(&red[0][c]), *reinterpret_cast<const f32x4*>(&red[1][c])),
                         max4(*reinterpret_cast<const f32x4*>(&red[2][c]), *reinterpret_cast<const f32x4*>(&red[3][c])));
    *reinterpret_cast<f32x4*>(part + ((size_t)b * T + tile) * CLS_FEAT + c) = r;
    if (WIN) {                                                         // waves own ascending point ranges: the first wave that holds it
        i32x4 wi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int x = INT32_MAX;
#pragma unroll
            for (int w = 3; w >= 0; --w)
                if (red[w][c + k] == r[k]) x = redi[w][c + k];
            wi[k] = x;
        }
        *reinterpret_cast<i32x4*>(part_idx + ((size_t)b * T + tile) * CLS_FEAT + c) = wi;
    }
}

__global__ __launch_bounds__(256) void tile_max_kernel(const float* __restrict__ part, const int32_t* __restrict__ n_points, int stride,
                                                       int T, float* __restrict__ gmax) {
    const int b = blockIdx.x, c = threadIdx.x * 4;
    int n = n_points ? n_points[b] : stride;
    n = min(max(n, 1), stride);
    const int tiles = (n + CLS_TILE - 1) / CLS_TILE;                   // the tiles point_stack_kernel wrote (n == 0: refused by the host)
    const float* Pp = part + (size_t)b * T * CLS_FEAT + c;
    f32x4 r = *reinterpret_cast<const f32x4*>(Pp);
    for (int t = 1; t < tiles; ++t) r = max4(r, *reinterpret_cast<const f32x4*>(Pp + (size_t)t * CLS_FEAT));
    *reinterpret_cast<f32x4*>(gmax + (size_t)b * CLS_FEAT + c) = r;
}

// tile_max_kernel and the winners: the first tile (tiles own ascending point ranges) that holds the maximum.  The index is
// clamped into the cloud, so that whatever the values were (NaN input) it can be used as a row number.
__global__ __launch_bounds__(256) void tile_max_win_kernel(const float* __restrict__ part, const int32_t* __restrict__ part_idx,
                                                           const int32_t* __restrict__ n_points, int stride, int T,
                                                           float* __restrict__ gmax, int32_t* __restrict__ win) {
    const int b = blockIdx.x, c = threadIdx.x * 4;
    int n = n_points ? n_points[b] : stride;
    n = min(max(n, 1), stride);
    const int tiles = (n + CLS_TILE - 1) / CLS_TILE;
    const float* Pp = part + (size_t)b * T * CLS_FEAT + c;
    const int32_t* Pi = part_idx + (size_t)b * T * CLS_FEAT + c;
    f32x4 r = *reinterpret_cast<const f32x4*>(Pp);
    for (int t = 1; t < tiles; ++t) r = max4(r, *reinterpret_cast<const f32x4*>(Pp + (size_t)t * CLS_FEAT));
    i32x4 wi = i32x4{INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX};
    for (int t = tiles - 1; t >= 0; --t) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(Pp + (size_t)t * CLS_FEAT);
        const i32x4 vi = *reinterpret_cast<const i32x4*>(Pi + (size_t)t * CLS_FEAT);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (v[k] == r[k]) wi[k] = vi[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) wi[k] = min(max(wi[k], 0), n - 1);
    *reinterpret_cast<f32x4*>(gmax + (size_t)b * CLS_FEAT + c) = r;
    *reinterpret_cast<i32x4*>(win + (size_t)b * CLS_FEAT + c) = wi;
}

// out[b][o] = act(bias[o] + sum_k W[o][k] x[b][k]) (+ 1 where o is a diagonal element of an eye x eye matrix).  x: [B][L.n_in]
// (n_in a multiple of 64), out: [B][ldo], o < L.n_out.  A wave = 16 clouds x one 16-output tile; 4 tiles a workgroup.
__global__ __launch_bounds__(256) void fc_kernel(const float* __restrict__ img, ClsFc L, const float* __restrict__ x, int B, int relu,
                                                 int eye, float* __restrict__ out, int ldo) {
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int m = blockIdx.x * 4 + wv, cb = blockIdx.y * 16 + p;
    if (16 * m >= L.n_out) return;
    const int SG = L.n_in / 16;
    const bool live = cb < B;
    const float* X = x + (size_t)(live ? cb : 0) * L.n_in + 4 * q;
    const float* W = img + L.w + ((size_t)m * SG * 64 + l) * 4;
    // four independent chains over interleaved input groups, summed pairwise: the MFMAs of one chain depend on each other,
    // and a 1024-term sum in one chain would also carry four times the rounding of four 256-term ones
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 a0 = *reinterpret_cast<const f32x4*>(img + L.b + 16 * m + 4 * q), a1 = zero, a2 = zero, a3 = zero;
    for (int g = 0; g < SG; g += 4) {                                  // n_in is a multiple of 64
        const f32x4 x0 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g) : zero;
        const f32x4 x1 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g + 16) : zero;
        const f32x4 x2 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g + 32) : zero;
        const f32x4 x3 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g + 48) : zero;
        a0 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256), x0, a0);
        a1 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256 + 256), x1, a1);
        a2 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256 + 512), x2, a2);
        a3 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256 + 768), x3, a3);
    }
    f32x4 acc = (a0 + a1) + (a2 + a3);
    if (relu) acc = relu4(acc);
    if (!live) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = 16 * m + 4 * q + r;
        if (o < L.n_out) {
            float v = acc[r];
            if (eye > 0 && o / eye == o % eye) v += 1.f;
            out[(size_t)cb * ldo + o] = v;
        }
    }
}

__global__ __launch_bounds__(256) void argmax_kernel(const float* __restrict__ logits, int B, int n_classes, int32_t* __restrict__ pred) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float* L = logits + (size_t)b * n_classes;
    float bv = L[0];
    int bi = 0;
    for (int c = 1; c < n_classes; ++c)
        if (L[c] > bv) { bv = L[c]; bi = c; }                          // strict: the lowest class among equals
    pred[b] = bi;
}

__global__ __launch_bounds__(256) void check_counts_kernel(const int32_t* __restrict__ n_points, int B, int lo, int hi, int32_t* __restrict__ bad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B && (n_points[b] < lo || n_points[b] > hi)) atomicAdd(bad, 1);
}

void launch_fc(const float* img, const ClsFc& L, const float* x, int B, int relu, int eye, float* out, int ldo, hipStream_t s) {
    const int tiles = (L.n_out + 15) / 16;
    hipLaunchKernelGGL(fc_kernel, dim3((tiles + 3) / 4, (B + 15) / 16), dim3(256), 0, s, img, L, x, B, relu, eye, out, ldo);
}

// max-pooled stack output (w.gmax) -> fc1 -> fc2 -> fc3 -> out
void launch_fc_stack(const float* img, const ClsFc (&F)[3], int B, const ClsWs& w, int eye, float* out, int ldo, hipStream_t s) {
    launch_fc(img, F[0], w.gmax, B, 1, 0, w.f1, F[0].n_out, s);
    launch_fc(img, F[1], w.f1, B, 1, 0, w.f2, F[1].n_out, s);
    launch_fc(img, F[2], w.f2, B, 0, eye, out, ldo, s);
}

}  // namespace

hipError_t launch_count_check(const int32_t* n_points, int B, int lo, int hi, int32_t* bad, hipStream_t s) {
    hipError_t e = hipMemsetAsync(bad, 0, sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(check_counts_kernel, dim3((B + 255) / 256), dim3(256), 0, s, n_points, B, lo, hi, bad);
    return hipGetLastError();
}

hipError_t launch_argmax(const float* logits, int B, int n_classes, int32_t* pred, hipStream_t s) {
    hipLaunchKernelGGL(argmax_kernel, dim3((B + 255) / 256), dim3(256), 0, s, logits, B, n_classes, pred);
    return hipGetLastError();
}

hipError_t launch_cls(const float* img, const ClsImage& I, bool feature_transform, const float* pc, const int32_t* n_points, int B,
                      int stride, const ClsWs& w, float* logits, int n_classes, int32_t* pred, hipStream_t s) {
    const int T = (stride + CLS_TILE - 1) / CLS_TILE;
    const dim3 grid(T, B), block(256);
    hipLaunchKernelGGL((point_stack_kernel<false, true>), grid, block, 0, s, img, I.stn, pc, n_points, stride, (const float*)nullptr,
                       (const float*)nullptr, w.part, T);
    hipLaunchKernelGGL(tile_max_kernel, dim3(B), block, 0, s, (const float*)w.part, n_points, stride, T, w.gmax);
    launch_fc_stack(img, I.stn_fc, B, w, 3, w.trans, 16, s);
    if (feature_transform) {
        hipLaunchKernelGGL((point_stack_kernel<true, true>), grid, block, 0, s, img, I.fstn, pc, n_points, stride, (const float*)w.trans,
                           (const float*)nullptr, w.part, T);
        hipLaunchKernelGGL(tile_max_kernel, dim3(B), block, 0, s, (const float*)w.part, n_points, stride, T, w.gmax);
        launch_fc_stack(img, I.fstn_fc, B, w, 64, w.tfeat, 4096, s);
    }
    hipLaunchKernelGGL((point_stack_kernel<false, false>), grid, block, 0, s, img, I.trunk, pc, n_points, stride, (const float*)w.trans,
                       feature_transform ? (const float*)w.tfeat : (const float*)nullptr, w.part, T);
    hipLaunchKernelGGL(tile_max_kernel, dim3(B), block, 0, s, (const float*)w.part, n_points, stride, T, w.gmax);
    launch_fc_stack(img, I.head_fc, B, w, 0, logits, n_classes, s);
    return pred ? launch_argmax(logits, B, n_classes, pred, s) : hipGetLastError();
}

// launch_cls without feature_transform, keeping what the backward pass needs (ClsGradWs): both stacks' maxima and winners and
// both FC stacks' activations.  The same kernels in the same order on the same arithmetic: logits, pred and the global
// feature are launch_cls's, bit for bit.
hipError_t launch_cls_win(const float* img, const ClsImage& I, const float* pc, const int32_t* n_points, int B, int stride,
                          const ClsGradWs& w, int n_classes, hipStream_t s) {
    const int T = (stride + CLS_TILE - 1) / CLS_TILE;
    const dim3 grid(T, B), block(256);
    ClsWs a{w.part, w.gmax_stn, w.f1_stn, w.f2_stn, w.trans, nullptr}, h{w.part, w.gmax, w.f1, w.f2, w.trans, nullptr};
    hipLaunchKernelGGL((point_stack_kernel<false, true, true>), grid, block, 0, s, img, I.stn, pc, n_points, stride, (const float*)nullptr,
                       (const float*)nullptr, w.part, T, w.part_idx);
    hipLaunchKernelGGL(tile_max_win_kernel, dim3(B), block, 0, s, (const float*)w.part, (const int32_t*)w.part_idx, n_points, stride, T,
                       w.gmax_stn, w.win_stn);
    launch_fc_stack(img, I.stn_fc, B, a, 3, w.trans, 16, s);
    hipLaunchKernelGGL((point_stack_kernel<false, false, true>), grid, block, 0, s, img, I.trunk, pc, n_points, stride, (const float*)w.trans,
                       (const float*)nullptr, w.part, T, w.part_idx);
    hipLaunchKernelGGL(tile_max_win_kernel, dim3(B), block, 0, s, (const float*)w.part, (const int32_t*)w.part_idx, n_points, stride, T,
                       w.gmax, w.win);
    launch_fc_stack(img, I.head_fc, B, h, 0, w.logits, n_classes, s);
    return launch_argmax(w.logits, B, n_classes, w.pred, s);
}

}  // namespace ifd
