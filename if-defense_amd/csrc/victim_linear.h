// The one dense layer of the DGCNN and PointNet++ victims on v_mfma_f32_16x16x4_f32: Y = act(W X + b), weights row-major
// [n_out][n_in] as the canonical vector has them.  A workgroup owns 64 rows (points, or clouds in an FC head) x 64 outputs; wave w
// owns the row half (w & 1) x the output half (w >> 1), two 16 x 16 tiles each way.  Columns of an MFMA never mix: a row's result
// depends on nothing but that row, whatever shares its wave.
//
// What differs between the layers is a policy P of four compile-time choices and nothing else:
//   ACT    LeakyReLU(0.2) or ReLU, applied where `act` is set (always in a pooling layer).
//   CUT64  how the K inputs are summed.  false: the bias starts chain 0, four chains over the interleaved 16-input groups run
//          across all of K and are added pairwise once, (c0 + c1) + (c2 + c3).  true: the inputs go in blocks of 64; a block is
//          four chains of 16 inputs from zero, added pairwise, and the blocks are added to the bias in ascending order - chains of
//          16, not of K / 4, which is what PointNet++'s 512-wide layers need to stay within the float32 oracle's error.
//   XYZ    where wx is not null, wx[o] . xyz[row] is added to the sum by three FMAs (x, then y, then z) before the activation.
//   POOL   none: Y is stored.  Otherwise nothing is stored but the maximum (and the sum) over the workgroup's valid rows,
//          part_max / part_sum [b][T][M] at tile blockIdx.x: a butterfly d = 1, 2, 4, 8 over the 16 rows of the lanes, then the
//          two row halves through LDS.  Every lane runs the same tree, so the sum depends on nothing but the cloud's own rows.
// The order of the floating-point operations is part of each victim's contract with its oracle: a new policy value
// is a new contract, not a tuning knob.  The four policies at the end of this file are the only instantiations.
#pragma once
#include "ifd_internal.h"
#include "lds_layout.h"
#include "victim_device.h"

namespace ifd {

constexpr int LINEAR_TILE = 64;         // rows of one workgroup of linear_kernel, and of one partial maximum / sum of its pool

enum class LinearAct { LEAKY, RELU };
enum class LinearPool { NONE, MAX, MAX_SUM };

// One block of 64 inputs, columns g .. g + 63 of the rows xr[t] (a wave's two 16-row tiles) and of the weight rows wr[m] (its two
// 16-output tiles): four chains of 16 inputs from zero, added pairwise into sum[t][m].
__device__ __forceinline__ void linear_block64(const float* (&xr)[2], const float* (&wr)[2], int g, f32x4 (&sum)[2][2]) {
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 xv[2][4], wt[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            xv[t][c] = *reinterpret_cast<const f32x4*>(xr[t] + g + 16 * c);
            wt[t][c] = *reinterpret_cast<const f32x4*>(wr[t] + g + 16 * c);
        }
    f32x4 acc[2][2][4];                                                // [row tile][output tile][chain]
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) acc[t][m][c] = mfma4(wt[m][c], xv[t][c], zero);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m) sum[t][m] += (acc[t][m][0] + acc[t][m][1]) + (acc[t][m][2] + acc[t][m][3]);
}

// One layer of a grouped MLP (pointnet2.hip, pointconv.hip) on a 64-row tile in LDS: v[t][m] = bias + sum_c W[o][c] Xs[row][c], row = 32 (wv & 1) + 16 t + p, o = obase + 16 m +
// 4 q + r, then ReLU.  linear_kernel's CUT64 arithmetic (victim_linear.h): the blocks of 64 inputs are added to the bias in ascending
// order.  W row-major [..][K] in global memory.
template <int K, int LDX>
__device__ __forceinline__ void tile_layer(const float* __restrict__ Xs, const float* __restrict__ W, const float* __restrict__ bias,
                                           int obase, int wv, int q, int p, f32x4 (&v)[2][2]) {
    const float* xr[2];
    const float* wr[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        xr[t] = Xs + (32 * (wv & 1) + 16 * t + p) * LDX + 4 * q;
        wr[t] = W + (size_t)(obase + 16 * t + p) * K + 4 * q;
    }
    f32x4 sum[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + obase + 16 * m + 4 * q);
#pragma unroll
        for (int t = 0; t < 2; ++t) sum[t][m] = bv;
    }
#pragma unroll
    for (int g = 0; g < K; g += 64) linear_block64(xr, wr, g, sum);
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m) v[t][m] = relu4(sum[t][m]);
}

// the tile's next layer input: Ys[row][o]
template <int LDY>
__device__ __forceinline__ void tile_store(float* __restrict__ Ys, int obase, int wv, int q, int p, const f32x4 (&v)[2][2]) {
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m)
            *reinterpret_cast<f32x4*>(Ys + (32 * (wv & 1) + 16 * t + p) * LDY + obase + 16 * m + 4 * q) = v[t][m];
}

// Ys[row][obase + ..] = sum_c WT[o][c] Xs[row][c], no bias, no activation: a transposed layer on the tile, tile_layer's block
// arithmetic (the 64-input blocks from zero, added in ascending order).
template <int K, int LD>
__device__ __forceinline__ void tile_layer_t(const float* __restrict__ Xs, const float* __restrict__ WT, float* __restrict__ Ys, int obase,
                                             int wv, int q, int p) {
    const float* xr[2];
    const float* wr[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        xr[t] = Xs + (32 * (wv & 1) + 16 * t + p) * LD + 4 * q;
        wr[t] = WT + (size_t)(obase + 16 * t + p) * K + 4 * q;
    }
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 sum[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int t = 0; t < 2; ++t) sum[t][m] = zero;
#pragma unroll
    for (int g = 0; g < K; g += 64) linear_block64(xr, wr, g, sum);
    tile_store<LD>(Ys, obase, wv, q, p, sum);
}

// Y[row][o] = act(bias[o] + sum_c W[o][c] X[row][c] (+ wx[o] . xyz[row])), o < M (a multiple of 4), K a multiple of 64.  Rows: the
// first cloud_points(n_points, b, stride) of cloud b = blockIdx.z; X rows of ldx floats from X + b * xb, Y rows of ldy floats from
// Y + b * yb, xyz rows of 3 floats from xyz + b * stride * 3; wx [M][4] = {w0, w1, w2, -}.
template <class P>
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ W, const float* __restrict__ bias, int M, int K,
                                                     const float* __restrict__ X, int ldx, size_t xb,
                                                     const int32_t* __restrict__ n_points, int stride, float* __restrict__ Y, int ldy,
                                                     size_t yb, int act, const float* __restrict__ wx, const float* __restrict__ xyz,
                                                     float* __restrict__ part_max, float* __restrict__ part_sum, int T) {
    constexpr bool POOL = P::POOL != LinearPool::NONE, POOL_SUM = P::POOL == LinearPool::MAX_SUM;
    using Lds = LinearPoolLds<POOL_SUM>;
    __shared__ __attribute__((aligned(16))) float red[POOL ? Lds::BYTES / 4 : 4];
    const int b = blockIdx.z;
    const int n = cloud_points(n_points, b, stride);
    const int row0 = blockIdx.x * LINEAR_TILE;
    if (row0 >= n) return;                                             // the whole workgroup
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int rbase = row0 + 32 * (wv & 1), obase = blockIdx.y * 64 + 32 * (wv >> 1);
    const float* Xb = X + (size_t)b * xb;
    const float* xr[2];
    const float* wr[2];
    bool valid[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = rbase + 16 * t + p;
        valid[t] = i < n;
        xr[t] = Xb + (size_t)min(i, n - 1) * ldx + 4 * q;              // rows beyond the cloud compute on its last row, unused
        wr[t] = W + (size_t)min(obase + 16 * t + p, M - 1) * K + 4 * q;
    }
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 bv[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = obase + 16 * m + 4 * q + r;
            bv[m][r] = o < M ? bias[o] : 0.f;
        }
    f32x4 sum[2][2];                                                   // [row tile][output tile]
    if constexpr (P::CUT64) {
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) sum[t][m] = bv[m];
        for (int g = 0; g < K; g += 64) linear_block64(xr, wr, g, sum);
    } else {
        f32x4 acc[2][2][4];                                            // [row tile][output tile][chain]
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                acc[t][m][0] = bv[m];
                acc[t][m][1] = acc[t][m][2] = acc[t][m][3] = zero;
            }
        for (int g = 0; g < K; g += 64) {
            f32x4 xv[2][4], wt[2][4];
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    xv[t][c] = *reinterpret_cast<const f32x4*>(xr[t] + g + 16 * c);
                    wt[t][c] = *reinterpret_cast<const f32x4*>(wr[t] + g + 16 * c);
                }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[t][m][c] = mfma4(wt[m][c], xv[t][c], acc[t][m][c]);
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int m = 0; m < 2; ++m) sum[t][m] = (acc[t][m][0] + acc[t][m][1]) + (acc[t][m][2] + acc[t][m][3]);
    }
    f32x4 v[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        float px = 0.f, py = 0.f, pz = 0.f;
        if constexpr (P::XYZ) {
            if (wx) {
                const float* pt = xyz + ((size_t)b * stride + min(rbase + 16 * t + p, n - 1)) * 3;
                px = pt[0]; py = pt[1]; pz = pt[2];
            }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            v[t][m] = sum[t][m];
            if constexpr (P::XYZ) {
                if (wx) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(wx + (size_t)min(obase + 16 * m + 4 * q + r, M - 1) * 4);
                        v[t][m][r] = fmaf(w[2], pz, fmaf(w[1], py, fmaf(w[0], px, v[t][m][r])));
                    }
                }
            }
            if (POOL || act) v[t][m] = P::ACT == LinearAct::LEAKY ? leaky4(v[t][m]) : relu4(v[t][m]);
        }
    }
    if constexpr (!POOL) {
        float* Yb = Y + (size_t)b * yb;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int i = rbase + 16 * t + p, o = obase + 16 * m + 4 * q;
                if (valid[t] && o < M) *reinterpret_cast<f32x4*>(Yb + (size_t)i * ldy + o) = v[t][m];
            }
    } else {
        float* rmax = LDS_AT(float, red, Lds::MAX);
        float* rsum = LDS_AT(float, red, POOL_SUM ? Lds::SUM : Lds::MAX);  // read and written only with POOL_SUM
        const int slot = (wv & 1) * 64 + 32 * (wv >> 1) + 4 * q;
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            f32x4 mx = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY}, sm = zero;
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (valid[t]) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        mx[r] = fmaxf(mx[r], v[t][m][r]);
                        if constexpr (POOL_SUM) sm[r] += v[t][m][r];
                    }
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) {                              // over the 16 rows of the lanes: a butterfly, every lane the same tree
                float x = mx[r], s = sm[r];
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    x = fmaxf(x, __shfl_xor(x, d));
                    if constexpr (POOL_SUM) s += __shfl_xor(s, d);
                }
                mx[r] = x; sm[r] = s;
            }
            if (p == 0) {
                *reinterpret_cast<f32x4*>(rmax + slot + 16 * m) = mx;
                if constexpr (POOL_SUM) *reinterpret_cast<f32x4*>(rsum + slot + 16 * m) = sm;
            }
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            const size_t at = ((size_t)b * T + blockIdx.x) * M + blockIdx.y * 64 + threadIdx.x;
            part_max[at] = fmaxf(rmax[threadIdx.x], rmax[64 + threadIdx.x]);
            if constexpr (POOL_SUM) part_sum[at] = rsum[threadIdx.x] + rsum[64 + threadIdx.x];
        }
    }
}

// One layer on [B clouds][cloud_points rows].  A pooling policy writes part_max (and part_sum) [B][T][n_out], T =
// ceil(stride / LINEAR_TILE), instead of Y.
template <class P>
void launch_linear(const float* img, const DenseLayer& L, const float* X, int ldx, size_t xb, const int32_t* n_points, int B, int stride,
                   float* Y, int ldy, size_t yb, int act, hipStream_t s, const float* wx = nullptr, const float* xyz = nullptr,
                   float* part_max = nullptr, float* part_sum = nullptr) {
    const int T = (stride + LINEAR_TILE - 1) / LINEAR_TILE;
    hipLaunchKernelGGL((linear_kernel<P>), dim3(T, (L.n_out + 63) / 64, B), dim3(256), 0, s, img + L.w, img + L.b, L.n_out, L.n_in, X,
                       ldx, xb, n_points, stride, Y, ldy, yb, act, wx, xyz, part_max, part_sum, T);
}

template <LinearAct ACT_, bool CUT64_, bool XYZ_, LinearPool POOL_>
struct LinearPolicy {
    static constexpr LinearAct ACT = ACT_;
    static constexpr bool CUT64 = CUT64_, XYZ = XYZ_;
    static constexpr LinearPool POOL = POOL_;
};
// DGCNN: the split edge convolutions' P | Q and the head; conv5, reduced to the maximum and the sum of each 64-point tile
using DgLinear = LinearPolicy<LinearAct::LEAKY, false, false, LinearPool::NONE>;
using DgConv5 = LinearPolicy<LinearAct::LEAKY, false, false, LinearPool::MAX_SUM>;
// PointNet++: sa2's U, sa3's first two layers (the first with its xyz columns) and the head; sa3's last, reduced to its tiles' maxima.
// Both keep the run-time wx test of the kernel they replace, sa3's last too, which never passes one: without it the compiler packs the
// block's adds differently and that layer measured 2 % slower.
using Pn2Linear = LinearPolicy<LinearAct::RELU, true, true, LinearPool::NONE>;
using Pn2Sa3Last = LinearPolicy<LinearAct::RELU, true, true, LinearPool::MAX>;

// d times the activation's derivative at the saved activation: 1 where it is > 0, else LeakyReLU's 0.2, or ReLU's 0 written as such
// (0 * d would keep d's sign, and a non-finite d)
template <LinearAct ACT>
__global__ __launch_bounds__(256) void act_gate_kernel(float* __restrict__ d, const float* __restrict__ act, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if constexpr (ACT == LinearAct::LEAKY) d[i] = act[i] > 0.f ? d[i] : 0.2f * d[i];
    else d[i] = act[i] > 0.f ? d[i] : 0.f;
}
template <class P>
void launch_act_gate(float* d, const float* act, int n, hipStream_t s) {
    hipLaunchKernelGGL((act_gate_kernel<P::ACT>), dim3((n + 255) / 256), dim3(256), 0, s, d, act, n);
}

// The classifier head's backward pass, a cloud a row: loss and d_out from the logits (launch_loss_grad), then the three FC layers
// transposed (fct: fc1^T, fc2^T, fc3^T on a zero bias) with the gates of the saved f2 and f1 between them -> dg [B][emb].
// w: the victim's *GradWs (logits, loss, d_out, d2, d1, and the forward's f.f1, f.f2).
template <class P, class Ws>
hipError_t launch_head_backward(const float* gimg, const DenseLayer (&fct)[3], const Ws& w, const int32_t* target, int B, int n_classes,
                                int loss_kind, float kappa, float scale, float* dg, int emb, hipStream_t s) {
    hipError_t e = launch_loss_grad(w.logits, target, B, n_classes, loss_kind, kappa, scale, w.loss, w.d_out, s);
    if (e != hipSuccess) return e;
    launch_linear<P>(gimg, fct[2], w.d_out, 64, 0, nullptr, 1, B, w.d2, 256, 0, 0, s);
    launch_act_gate<P>(w.d2, w.f.f2, B * 256, s);
    launch_linear<P>(gimg, fct[1], w.d2, 256, 0, nullptr, 1, B, w.d1, 512, 0, 0, s);
    launch_act_gate<P>(w.d1, w.f.f1, B * 512, s);
    launch_linear<P>(gimg, fct[0], w.d1, 512, 0, nullptr, 1, B, dg, emb, 0, 0, s);
    return hipSuccess;
}

}  // namespace ifd
