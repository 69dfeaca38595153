// Input gradients of the DGCNN victim (include/ifd_dgcnn_atk.h): d loss / d points for the two adversarial losses of
// include/ifd_atk.h, with the four neighbour tables held fixed (topk's indices carry no gradient in the reference either).
// The forward half is launch_dgcnn itself (dgcnn.hip), so logits, pred, feat, the global feature and the tables are its bits;
// it leaves feat, the four tables, the tiles' maxima, f1 and f2 behind.  The backward half, in launch order:
//
//   launch_head_backward     (victim_linear.h) loss_grad_kernel: logits, target -> loss, scale * d loss / d logits; the three FC
//                            layers transposed (DgGradImage.fct, zero bias, no activation), a cloud a row; act_gate_kernel between
//                            them: times LeakyReLU's derivative at the saved activation, 1 where it is > 0, else 0.2
//   dg_pool_wtile_kernel     per channel the first 64-point tile whose maximum is the cloud's
//   dg_conv5_bwd_kernel      the hot kernel, a workgroup a 64-point tile.  conv5's [points, 1024] output is never stored: per chunk
//                            of 64 channels, ascending, the tile's pre-activations are recomputed by linear_kernel<DgConv5>'s own
//                            instruction sequence (bias first, four interleaved chains, added pairwise), so their signs and the
//                            maxima are the forward's bits; the winner of a channel is the lowest row of the first tile whose
//                            activation equals the cloud's maximum;
//                                dY[i][c] = leaky'(y[i][c]) * (g_mean[c] / n + (i == win[c] ? g_max[c] : 0))
//                            goes through LDS and dfeat[i][0..512) += dY[i][chunk] . W5[chunk][:] runs on v_mfma_f32_16x16x4_f32 into
//                            a 64 x 512 accumulator tile held in registers (128 a lane): per element one chain over the channels.
//   per edge convolution 4 .. 1:
//   launch_dg_pq             P | Q of the layer again, by the forward's kernels
//   dg_edge_win_kernel       j* = the neighbour holding max_j P_j[c], the lowest point index among equal values; s = leaky'(saved
//                            feat) * dfeat; dQ_i[c] = s overwrites Q in place
//   dg_edge_scatter_kernel   dP[j*][c] += s without atomics: a wave owns one channel of one cloud and walks i in ascending order
//                            into an LDS column; dP overwrites P in place
//   linear_kernel<DgLinear>  dx = [dP | dQ] . [Wa ; Wb - Wa] (DgGradImage.pqt), then dg_add_cols_kernel adds it into the input
//                            layer's columns of dfeat, which conv5 has already written; layer 1 ends in dg_first_bwd_kernel, one
//                            chain of plain FMAs over the 128 rows of P | Q per coordinate, which writes grad.
// Every sum has a fixed order, nothing here uses float atomics, and every kernel works on one cloud's rows alone.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "victim_linear.h"

namespace ifd {

namespace {

constexpr int DGB_LD = 68;              // floats of a row of the dY chunk in LDS: 64 channels + 4, so a quarter wave's b128 reads spread over all banks
constexpr int DGB_NONE = 0x7fffffff;
static_assert(DG_TILE == 64 && DG_FEAT == 512 && DG_EMB == 1024, "dg_conv5_bwd_kernel's tiling");

__global__ __launch_bounds__(256) void dg_pool_wtile_kernel(const float* __restrict__ part_max, const float* __restrict__ gfeat,
                                                            const int32_t* __restrict__ n_points, int stride, int T,
                                                            int32_t* __restrict__ wtile) {
    const int b = blockIdx.x;
    const int n = cloud_points(n_points, b, stride);
    const int tiles = (n + DG_TILE - 1) / DG_TILE;
    for (int c = threadIdx.x; c < DG_EMB; c += 256) {
        const float m = gfeat[(size_t)b * 2 * DG_EMB + c];
        int wt = DGB_NONE;
        for (int t = tiles - 1; t >= 0; --t)
            if (part_max[((size_t)b * T + t) * DG_EMB + c] == m) wt = t;
        wtile[(size_t)b * DG_EMB + c] = wt;
    }
}

// W5 [1024][512], b5 [1024]: the forward's conv5; W5T [512][1024].  gfeat: the forward's max | mean, g: d loss / d of it.
__global__ __launch_bounds__(256) void dg_conv5_bwd_kernel(const float* __restrict__ W5, const float* __restrict__ b5,
                                                           const float* __restrict__ W5T, const float* __restrict__ feat,
                                                           const int32_t* __restrict__ n_points, int stride,
                                                           const float* __restrict__ gfeat, const float* __restrict__ g,
                                                           const int32_t* __restrict__ wtile, int32_t* __restrict__ win_pool,
                                                           uint32_t* __restrict__ act5, float* __restrict__ dfeat) {
    __shared__ __attribute__((aligned(16))) float dYs[DG_TILE * DGB_LD];
    __shared__ int wrow[2][64];
    const int b = blockIdx.y, tile = blockIdx.x;
    const int n = cloud_points(n_points, b, stride);
    const int row0 = tile * DG_TILE;
    if (row0 >= n) return;                                             // the whole workgroup
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int rhalf = wv & 1, ohalf = wv >> 1, rbase = row0 + 32 * rhalf;
    const float* Xb = feat + (size_t)b * stride * DG_FEAT;
    const float* xr[2];
    bool valid[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int i = rbase + 16 * t + p;
        valid[t] = i < n;
        xr[t] = Xb + (size_t)min(i, n - 1) * DG_FEAT + 4 * q;
    }
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    const float fn = (float)n;
    const float* Gf = gfeat + (size_t)b * 2 * DG_EMB;
    const float* Gg = g + (size_t)b * 2 * DG_EMB;
    f32x4 dacc[4][8];                                                  // [row tile][column tile of this wave's 128 columns]
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int ct = 0; ct < 8; ++ct) dacc[rt][ct] = zero;
#pragma unroll 1
    for (int chunk = 0; chunk < DG_EMB / 64; ++chunk) {
        const int obase = chunk * 64 + 32 * ohalf;
        // the pre-activations of 32 rows x 32 channels: linear_kernel<DgConv5>, instruction for instruction
        f32x4 sum[2][2];
        {
            const float* wr[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) wr[t] = W5 + (size_t)(obase + 16 * t + p) * DG_FEAT + 4 * q;
            f32x4 acc[2][2][4];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(b5 + obase + 16 * m + 4 * q);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    acc[t][m][0] = bv;
                    acc[t][m][1] = acc[t][m][2] = acc[t][m][3] = zero;
                }
            }
#pragma unroll 1
            for (int gk = 0; gk < DG_FEAT; gk += 64) {
                f32x4 xv[2][4], wt[2][4];
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        xv[t][c] = *reinterpret_cast<const f32x4*>(xr[t] + gk + 16 * c);
                        wt[t][c] = *reinterpret_cast<const f32x4*>(wr[t] + gk + 16 * c);
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
        // the lowest row of this tile whose activation is the cloud's maximum, per channel: over the lanes' 16 rows, then the two halves
        f32x4 gmx[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            gmx[m] = *reinterpret_cast<const f32x4*>(Gf + obase + 16 * m + 4 * q);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int cand = DGB_NONE;
#pragma unroll
                for (int t = 1; t >= 0; --t)
                    if (valid[t] && leaky(sum[t][m][r]) == gmx[m][r]) cand = rbase + 16 * t + p;
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) cand = min(cand, __shfl_xor(cand, d));
                if (p == 0) wrow[rhalf][32 * ohalf + 16 * m + 4 * q + r] = cand;
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int ch = obase + 16 * m + 4 * q, lc = 32 * ohalf + 16 * m + 4 * q;
            const f32x4 gmax = *reinterpret_cast<const f32x4*>(Gg + ch);
            const f32x4 gmean = *reinterpret_cast<const f32x4*>(Gg + DG_EMB + ch);
            f32x4 dy[2];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool here = wtile[(size_t)b * DG_EMB + ch + r] == tile;
                const int wr_ = min(wrow[0][lc + r], wrow[1][lc + r]);
                const float gm = gmean[r] / fn;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const float d = gm + (here && rbase + 16 * t + p == wr_ ? gmax[r] : 0.f);
                    dy[t][r] = !valid[t] ? 0.f : sum[t][m][r] > 0.f ? d : 0.2f * d;
                }
                if (win_pool && here && rhalf == 0 && p == 0) win_pool[(size_t)b * DG_EMB + ch + r] = wr_;
            }
#pragma unroll
            for (int t = 0; t < 2; ++t) *reinterpret_cast<f32x4*>(dYs + (32 * rhalf + 16 * t + p) * DGB_LD + lc) = dy[t];
        }
        if (act5) {                                                    // wave-uniform
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                uint32_t bits = 0;
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (sum[t][m][r] > 0.f) bits |= 1u << (16 * m + 4 * q + r);
                bits |= __shfl_xor(bits, 16);
                bits |= __shfl_xor(bits, 32);
                if (q == 0 && valid[t]) act5[((size_t)b * stride + rbase + 16 * t + p) * (DG_EMB / 32) + chunk * 2 + ohalf] = bits;
            }
        }
        __syncthreads();
        // dfeat[64 rows][this wave's 128 columns] += dY[64][64 channels] . W5[channels][columns]
        {
            const float* wt_base = W5T + (size_t)(128 * wv + p) * DG_EMB + chunk * 64 + 4 * q;
#pragma unroll 1
            for (int c = 0; c < 4; ++c) {
                f32x4 av[8], bvv[4];
#pragma unroll
                for (int ct = 0; ct < 8; ++ct) av[ct] = *reinterpret_cast<const f32x4*>(wt_base + (size_t)16 * ct * DG_EMB + 16 * c);
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) bvv[rt] = *reinterpret_cast<const f32x4*>(dYs + (16 * rt + p) * DGB_LD + 16 * c + 4 * q);
#pragma unroll
                for (int ct = 0; ct < 8; ++ct)
#pragma unroll
                    for (int rt = 0; rt < 4; ++rt) dacc[rt][ct] = mfma4(av[ct], bvv[rt], dacc[rt][ct]);
            }
        }
        __syncthreads();
    }
    float* Db = dfeat + (size_t)b * stride * DG_FEAT;
#pragma unroll
    for (int rt = 0; rt < 4; ++rt) {
        const int i = row0 + 16 * rt + p;
        if (i < n) {
#pragma unroll
            for (int ct = 0; ct < 8; ++ct) *reinterpret_cast<f32x4*>(Db + (size_t)i * DG_FEAT + 128 * wv + 16 * ct + 4 * q) = dacc[rt][ct];
        }
    }
}

// pq rows of DG_FEAT floats, P in [0, cout), Q in [cout, 2 cout): Q is overwritten by dQ.  win [b][stride][cout].
// dg_gather_kernel's threads: one point x four channels.
__global__ __launch_bounds__(256) void dg_edge_win_kernel(float* __restrict__ pq, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ feat, const float* __restrict__ dfeat,
                                                          const int32_t* __restrict__ n_points, int stride, int k, int cout, int col,
                                                          int32_t* __restrict__ win) {
    const int per = cout >> 2, b = blockIdx.y;
    const int i = blockIdx.x * (256 / per) + threadIdx.x / per, c = (threadIdx.x % per) * 4;
    const int n = cloud_points(n_points, b, stride);
    if (i >= n) return;
    float* Pb = pq + (size_t)b * stride * DG_FEAT;
    const int32_t* nb = idx + ((size_t)b * stride + i) * k;
    const int kk = min(k, n);
    f32x4 m = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int mj[4] = {DGB_NONE, DGB_NONE, DGB_NONE, DGB_NONE};
    for (int e = 0; e < kk; ++e) {
        const int j = min(max(nb[e], 0), n - 1);
        const f32x4 v = *reinterpret_cast<const f32x4*>(Pb + (size_t)j * DG_FEAT + c);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (v[r] > m[r] || (v[r] == m[r] && j < mj[r])) { m[r] = v[r]; mj[r] = j; }
    }
    const size_t at = ((size_t)b * stride + i) * DG_FEAT + col + c;
    const f32x4 a = *reinterpret_cast<const f32x4*>(feat + at), d = *reinterpret_cast<const f32x4*>(dfeat + at);
    f32x4 s;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        s[r] = a[r] > 0.f ? d[r] : 0.2f * d[r];
        mj[r] = min(mj[r], n - 1);
    }
    *reinterpret_cast<f32x4*>(Pb + (size_t)i * DG_FEAT + cout + c) = s;
    int32_t* wo = win + ((size_t)b * stride + i) * cout + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) wo[r] = mj[r];
}

// A wave = one channel of one cloud: dP[j][c] = sum over the points i with win[i][c] == j, ascending, of dQ[i][c].  The lane
// j % 64 owns row j of the column; the wave walks i in ascending order, one addition a step.  dP overwrites P.
__global__ __launch_bounds__(256) void dg_edge_scatter_kernel(float* __restrict__ pq, const int32_t* __restrict__ win,
                                                              const int32_t* __restrict__ n_points, int stride, int cout) {
    __shared__ float colmem[4][DG_MAX_POINTS];
    const int b = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63, c = blockIdx.x * 4 + wv;
    const int n = cloud_points(n_points, b, stride);
    float* col = colmem[wv];
    float* Pb = pq + (size_t)b * stride * DG_FEAT;
    const int32_t* Wb = win + (size_t)b * stride * cout;
    for (int j = lane; j < n; j += 64) col[j] = 0.f;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int wj = i < n ? min(max(Wb[(size_t)i * cout + c], 0), n - 1) : 0;
        const float sv = i < n ? Pb[(size_t)i * DG_FEAT + cout + c] : 0.f;
        const int cnt = min(64, n - i0);
        for (int t = 0; t < cnt; ++t) {
            const int j = __shfl(wj, t);
            const float v = __shfl(sv, t);
            if ((j & 63) == lane) col[j] += v;
        }
    }
    for (int j = lane; j < n; j += 64) Pb[(size_t)j * DG_FEAT + c] = col[j];
}

// dfeat[b][i][col + c] += dx[b][i][c], c < C (dx rows of 128 floats); a thread = one point x four channels
__global__ __launch_bounds__(256) void dg_add_cols_kernel(const float* __restrict__ dx, const int32_t* __restrict__ n_points, int stride,
                                                          int C, int col, float* __restrict__ dfeat) {
    const int per = C >> 2, b = blockIdx.y;
    const int i = blockIdx.x * (256 / per) + threadIdx.x / per, c = (threadIdx.x % per) * 4;
    const int n = cloud_points(n_points, b, stride);
    if (i >= n) return;
    float* d = dfeat + ((size_t)b * stride + i) * DG_FEAT + col + c;
    *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(d) + *reinterpret_cast<const f32x4*>(dx + ((size_t)b * stride + i) * 128 + c);
}

// first: [128][4] = {w0, w1, w2, bias}, rows 0 .. 63 P, 64 .. 127 Q; grad[b][i][a] = sum over o = 0 .. 127, ascending, of
// dPQ[i][o] first[o][a]; zeros in the rows beyond the cloud.  A thread = one point.
__global__ __launch_bounds__(256) void dg_first_bwd_kernel(const float* __restrict__ first, const float* __restrict__ pq,
                                                           const int32_t* __restrict__ n_points, int stride, float* __restrict__ grad) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= stride) return;
    const int n = cloud_points(n_points, b, stride);
    float gx = 0.f, gy = 0.f, gz = 0.f;
    if (i < n) {
        const float* d = pq + ((size_t)b * stride + i) * DG_FEAT;
        for (int o = 0; o < 128; o += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(d + o);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(first + (o + r) * 4);
                gx = fmaf(v[r], w[0], gx);
                gy = fmaf(v[r], w[1], gy);
                gz = fmaf(v[r], w[2], gz);
            }
        }
    }
    float* o = grad + ((size_t)b * stride + i) * 3;
    o[0] = gx; o[1] = gy; o[2] = gz;
}

}  // namespace

hipError_t launch_dgcnn_grad(const float* img, const DgImage& I, const float* gimg, const DgGradImage& G, const float* pc,
                             const int32_t* n_points, int B, int stride, int k, const int32_t* target, int loss_kind, float kappa,
                             float scale, const DgGradWs& w, const DgGradOut& out, int n_classes, float* grad, hipStream_t s) {
    const dim3 block(256);
    const size_t fb = (size_t)stride * DG_FEAT;
    DgOut o{};
    const int32_t* idx[4];
    for (int l = 0; l < 4; ++l) idx[l] = o.idx[l] = out.idx[l] ? out.idx[l] : w.idx[l];
    const float* feat = o.feat = out.feat ? out.feat : w.f.feat;
    o.pred = w.pred;
    hipError_t e = launch_dgcnn(img, I, pc, n_points, B, stride, k, w.f, o, w.logits, n_classes, s);
    if (e != hipSuccess) return e;
    e = launch_head_backward<DgLinear>(gimg, G.fct, w, target, B, n_classes, loss_kind, kappa, scale, w.g, 2 * DG_EMB, s);
    if (e != hipSuccess) return e;
    // the pool and conv5
    const int T = (stride + DG_TILE - 1) / DG_TILE;
    hipLaunchKernelGGL(dg_pool_wtile_kernel, dim3(B), block, 0, s, (const float*)w.f.part_max, (const float*)w.f.gfeat, n_points, stride, T,
                       w.wtile);
    hipLaunchKernelGGL(dg_conv5_bwd_kernel, dim3(T, B), block, 0, s, img + I.conv5.w, img + I.conv5.b, gimg + G.w5t, feat,
                       n_points, stride, (const float*)w.f.gfeat, (const float*)w.g, (const int32_t*)w.wtile, w.win_pool, out.act5, w.dfeat);
    // the edge convolutions, last to first
    const int cout[4] = {64, 64, 128, 256}, col_out[4] = {0, 64, 128, 256}, cin[4] = {3, 64, 64, 128}, col_in[4] = {0, 0, 64, 128};
    for (int l = 3; l >= 0; --l) {
        e = launch_dg_pq(img, I, l, pc, feat, n_points, B, stride, w.f.pq, s);
        if (e != hipSuccess) return e;
        int32_t* win = out.win_edge[l] ? out.win_edge[l] : w.win;
        const int ppb = 1024 / cout[l];
        hipLaunchKernelGGL(dg_edge_win_kernel, dim3((stride + ppb - 1) / ppb, B), block, 0, s, w.f.pq, idx[l], feat,
                           (const float*)w.dfeat, n_points, stride, k, cout[l], col_out[l], win);
        hipLaunchKernelGGL(dg_edge_scatter_kernel, dim3(cout[l] / 4, B), block, 0, s, w.f.pq, (const int32_t*)win, n_points, stride, cout[l]);
        if (l > 0) {
            launch_linear<DgLinear>(gimg, G.pqt[l - 1], w.f.pq, DG_FEAT, fb, n_points, B, stride, w.dx, 128, (size_t)stride * 128, 0, s);
            const int ppa = 1024 / cin[l];
            hipLaunchKernelGGL(dg_add_cols_kernel, dim3((stride + ppa - 1) / ppa, B), block, 0, s, (const float*)w.dx, n_points, stride,
                               cin[l], col_in[l], w.dfeat);
        } else {
            hipLaunchKernelGGL(dg_first_bwd_kernel, dim3((stride + 255) / 256, B), block, 0, s, img + I.first, (const float*)w.f.pq, n_points,
                               stride, grad);
        }
    }
    return hipGetLastError();
}

}  // namespace ifd
