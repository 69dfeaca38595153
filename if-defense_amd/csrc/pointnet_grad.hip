// Input gradients of the PointNet victim (include/ifd_atk.h): d loss / d points for the two adversarial losses of the
// reference's attacks (baselines/attack/util/adv_utils.py), and the in-place updates of its FGM family
// (baselines/attack/FGM/FGM.py).  Runs after launch_cls_win (pointnet.hip), which keeps both max-pools' winners and both
// FC stacks' activations.  PointNet's backward pass is sparse: a max-pool passes gradient to one point per channel, so at
// most 1024 points of a cloud receive any, per stack.
//
//   loss_grad_kernel       logits, target -> loss and scale * d loss / d logits, one thread a cloud.
//   fc_t_kernel            a transposed FC layer batched over clouds, fc_kernel's MFMA tiling on the transposed weight image,
//                          times the ReLU mask of the layer below (its saved activation > 0).
//   stack_backward_kernel  one workgroup a cloud.  The distinct winner points in ascending order; 64 of them at a time:
//                          h1 and the 128-wide pre-activation recomputed (fused chains in the order the forward's MFMAs are
//                          taken to sum in - not measured, so a gate within rounding of zero may differ from the forward's),
//                          dH2[p] = sum over the channels c won by p, ascending, of g[c] W3[c], then back through
//                          [64 -> 128] and [3 -> 64] under the ReLU masks, through the 3 x 3 transform, and
//                          d loss / d trans = sum over the points, ascending, of x_p^T (x) d(x trans)_p.
//                          Every sum has a fixed order and no atomics: a cloud's gradient is the same bits wherever it runs.
//                          The trunk's pass writes grad (zeros where no gradient arrives), the STN's pass adds to it.
//   fgm_update_kernel      one workgroup a cloud: two fixed-order reductions and an elementwise pass.
//   atk_check_kernel       counts in [lo, hi] and targets of the one blocking check of every attack call (CW, kNN and Add too).
//
// The dense work here is small beside the forward's (at most 1024 points x 3 small layers, under 4 % of its FLOPs), so the
// stack's backward is plain FMAs; the FC transposes are MFMA (v_mfma_f32_16x16x4_f32), like the forward's.
#include "atk_device.h"
#include "victim_device.h"

namespace ifd {

namespace {

constexpr int ATK_MAXN = 10000;         // IFD_CLS_MAX_POINTS (api.cpp refuses a larger stride)
constexpr int ATK_PASS = 64;            // winner points of one pass of stack_backward_kernel
constexpr int LOSS_LOGITS = 0;          // IFD_ATK_LOSS_LOGITS / _CE
constexpr int KIND_FGM = 0, KIND_MIFGM = 2;   // IFD_FGM_FGM, _IFGM (1), _MIFGM, _PGD (3)

__global__ __launch_bounds__(256) void atk_check_kernel(const int32_t* __restrict__ n_points, const int32_t* __restrict__ target, int B,
                                                        int lo, int hi, int n_classes, int32_t* __restrict__ bad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    if (n_points && (n_points[b] < lo || n_points[b] > hi)) atomicAdd(bad, 1);
    if (target[b] < 0 || target[b] >= n_classes) atomicAdd(bad + 1, 1);
}

// d_out [B][64]: scale * d loss_b / d logits in the first n_classes, zeros behind.
__global__ __launch_bounds__(256) void loss_grad_kernel(const float* __restrict__ logits, const int32_t* __restrict__ target, int B,
                                                        int n_classes, int loss_kind, float kappa, float scale, float* __restrict__ loss,
                                                        float* __restrict__ d_out) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float* L = logits + (size_t)b * n_classes;
    float* D = d_out + (size_t)b * 64;
    const int t = min(max(target[b], 0), n_classes - 1);
    for (int c = 0; c < 64; ++c) D[c] = 0.f;
    if (loss_kind == LOSS_LOGITS) {
        // LogitsAdvLoss: the target's entry is -10000 for the max over the others; the first index among equal maxima
        float ov = t == 0 ? -10000.f : L[0];
        int oi = 0;
        for (int c = 1; c < n_classes; ++c) {
            const float v = c == t ? -10000.f : L[c];
            if (v > ov) { ov = v; oi = c; }
        }
        const float h = ov - L[t] + kappa;
        loss[b] = fmaxf(h, 0.f);
        if (h >= 0.f) {                                                // clamp(min=0) passes the gradient at its corner
            if (oi != t) D[oi] = scale;                                // (oi == t: the constant -10000 won, no gradient)
            D[t] -= scale;
        }
    } else {
        float mx = L[0];
        for (int c = 1; c < n_classes; ++c) mx = fmaxf(mx, L[c]);
        float sum = 0.f;
        for (int c = 0; c < n_classes; ++c) sum += expf(L[c] - mx);
        loss[b] = logf(sum) + mx - L[t];
        for (int c = 0; c < n_classes; ++c) D[c] = scale * (expf(L[c] - mx) / sum - (c == t ? 1.f : 0.f));
    }
}

// out[b][o] = (mask ? mask[b][o] > 0 : 1) * sum_k Wt[o][k] x[b][k]: fc_kernel (pointnet.hip) on a transposed layer, no bias.
// x: [B][L.n_in] (a multiple of 64), out and mask: [B][L.n_out] (a multiple of 16).
__global__ __launch_bounds__(256) void fc_t_kernel(const float* __restrict__ gimg, ClsFc L, const float* __restrict__ x, int B,
                                                   const float* __restrict__ mask, float* __restrict__ out) {
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int m = blockIdx.x * 4 + wv, cb = blockIdx.y * 16 + p;
    if (16 * m >= L.n_out) return;
    const int SG = L.n_in / 16;
    const bool live = cb < B;
    const float* X = x + (size_t)(live ? cb : 0) * L.n_in + 4 * q;
    const float* W = gimg + L.w + ((size_t)m * SG * 64 + l) * 4;
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 a0 = zero, a1 = zero, a2 = zero, a3 = zero;
    for (int g = 0; g < SG; g += 4) {
        const f32x4 x0 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g) : zero;
        const f32x4 x1 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g + 16) : zero;
        const f32x4 x2 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g + 32) : zero;
        const f32x4 x3 = live ? *reinterpret_cast<const f32x4*>(X + 16 * g + 48) : zero;
        a0 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256), x0, a0);
        a1 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256 + 256), x1, a1);
        a2 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256 + 512), x2, a2);
        a3 = mfma4(*reinterpret_cast<const f32x4*>(W + (size_t)g * 256 + 768), x3, a3);
    }
    const f32x4 acc = (a0 + a1) + (a2 + a3);
    if (!live) return;
    const size_t o = (size_t)cb * L.n_out + 16 * m + 4 * q;
    f32x4 v = acc;
    if (mask) {
        const f32x4 mk = *reinterpret_cast<const f32x4*>(mask + o);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = mk[r] > 0.f ? acc[r] : 0.f;
    }
    *reinterpret_cast<f32x4*>(out + o) = v;
}

// TRUNK: the input is x . trans, grad is written (every row of the cloud, zeros where nothing arrives) and
// dtrans [B][64] (9 used, zeros behind) is produced.  Otherwise (the STN3d stack): raw input, grad is added to.
template <bool TRUNK>
__global__ __launch_bounds__(256) void stack_backward_kernel(const float* __restrict__ img, int first, const float* __restrict__ gimg,
                                                             ClsGradStack S, const float* __restrict__ pc,
                                                             const int32_t* __restrict__ n_points, int stride,
                                                             const float* __restrict__ trans, const int32_t* __restrict__ win,
                                                             const float* __restrict__ g, float* __restrict__ grad,
                                                             float* __restrict__ dtrans) {
    __shared__ unsigned short slot_of[ATK_MAXN];                       // point -> its rank among the winner points (0xFFFF: none)
    __shared__ unsigned short cslot[CLS_FEAT];                         // channel -> the slot of its winner (0xFFFF: no gradient)
    __shared__ float cg[CLS_FEAT];
    __shared__ int pts[CLS_FEAT];
    __shared__ int cnt[256];
    __shared__ float dH[ATK_PASS][128];
    __shared__ float h1[ATK_PASS][64];
    __shared__ float dh1[ATK_PASS][64];
    __shared__ float xr[ATK_PASS][3];
    __shared__ float dxt[ATK_PASS][3];
    const int b = blockIdx.x, tid = threadIdx.x;
    int n = n_points ? n_points[b] : stride;
    n = min(max(n, 1), stride);
    const float* P = pc + (size_t)b * stride * 3;
    float* G = grad + (size_t)b * stride * 3;
    if (TRUNK)
        for (int i = tid; i < stride * 3; i += 256) G[i] = 0.f;
    for (int i = tid; i < n; i += 256) slot_of[i] = 0;
    __syncthreads();
    for (int c = tid; c < CLS_FEAT; c += 256) {
        const float gc = g[(size_t)b * CLS_FEAT + c];
        cg[c] = gc;
        if (gc != 0.f) slot_of[min(max(win[(size_t)b * CLS_FEAT + c], 0), n - 1)] = 1;
    }
    __syncthreads();
    // the marked points in ascending order: thread t ranks its own contiguous range behind the ranges before it
    const int per = (n + 255) / 256, i0 = min(tid * per, n), i1 = min(i0 + per, n);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += slot_of[i];
    cnt[tid] = mine;
    __syncthreads();
    int rank = 0, D = 0;
    for (int t = 0; t < 256; ++t) {
        const int v = cnt[t];
        if (t < tid) rank += v;
        D += v;
    }
    for (int i = i0; i < i1; ++i) {
        if (slot_of[i]) { slot_of[i] = (unsigned short)rank; pts[rank] = i; ++rank; }
        else slot_of[i] = 0xFFFF;
    }
    __syncthreads();
    for (int c = tid; c < CLS_FEAT; c += 256)
        cslot[c] = cg[c] != 0.f ? slot_of[min(max(win[(size_t)b * CLS_FEAT + c], 0), n - 1)] : (unsigned short)0xFFFF;
    float tr[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (TRUNK) {
#pragma unroll
        for (int k = 0; k < 9; ++k) tr[k] = trans[(size_t)b * 16 + k];
    }
    const float* W1 = img + first;                                     // [64][4] = {w0, w1, w2, bias}
    const float* W2 = gimg + S.w2;                                     // [128][64]
    const float* W3 = gimg + S.w3;                                     // [1024][128]
    float dt = 0.f;                                                    // threads 0..8: d loss / d trans[tid / 3][tid % 3]
    __syncthreads();
    for (int base = 0; base < D; base += ATK_PASS) {
        const int np = min(ATK_PASS, D - base);
        for (int i = tid; i < ATK_PASS * 128; i += 256) (&dH[0][0])[i] = 0.f;
        {   // the 64-wide activation of the pass's points, as point_stack_kernel computes it
            const int s = tid >> 2, c0 = (tid & 3) * 16;
            float x = 0.f, y = 0.f, z = 0.f;
            if (s < np) {
                const int i = pts[base + s];
                x = P[(size_t)i * 3]; y = P[(size_t)i * 3 + 1]; z = P[(size_t)i * 3 + 2];
            }
            if ((tid & 3) == 0) { xr[s][0] = x; xr[s][1] = y; xr[s][2] = z; }
            if (TRUNK) {
                const float xx = fmaf(z, tr[6], fmaf(y, tr[3], x * tr[0]));
                const float yy = fmaf(z, tr[7], fmaf(y, tr[4], x * tr[1]));
                const float zz = fmaf(z, tr[8], fmaf(y, tr[5], x * tr[2]));
                x = xx; y = yy; z = zz;
            }
            for (int c = c0; c < c0 + 16; ++c) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(W1 + c * 4);
                h1[s][c] = s < np ? fmaxf(fmaf(w[2], z, fmaf(w[1], y, fmaf(w[0], x, w[3]))), 0.f) : 0.f;
            }
        }
        __syncthreads();
        {   // dH[s] = sum over the channels won by slot s, ascending, of g[c] W3[c]: half a workgroup owns 32 slots
            const int j = tid & 127, half = tid >> 7;
            for (int c = 0; c < CLS_FEAT; ++c) {
                const int s = (int)cslot[c] - base;
                if (s >= 0 && s < ATK_PASS && (s >> 5) == half) dH[s][j] = fmaf(cg[c], W3[(size_t)c * 128 + j], dH[s][j]);
            }
        }
        __syncthreads();
        {   // the 128-wide pre-activation (bias, then per 16-input group the k order assumed of the MFMA), its ReLU mask
            const int o = tid & 127, s0 = (tid >> 7) * 32, s1 = min(s0 + 32, np);
            float w[64];
#pragma unroll
            for (int k = 0; k < 64; ++k) w[k] = W2[o * 64 + k];
            const float bias = gimg[S.b2 + o];
            for (int s = s0; s < s1; ++s) {
                float acc = bias;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                        for (int qq = 0; qq < 4; ++qq) {
                            const int k = 16 * gq + 4 * qq + jj;
                            acc = fmaf(w[k], h1[s][k], acc);
                        }
                if (!(acc > 0.f)) dH[s][o] = 0.f;
            }
        }
        __syncthreads();
        {   // back through [64 -> 128]: a thread owns input channel i of 16 slots
            const int i = tid & 63, s0 = (tid >> 6) * 16;
            float acc[16];
#pragma unroll
            for (int s = 0; s < 16; ++s) acc[s] = 0.f;
            if (s0 < np) {
                for (int o = 0; o < 128; ++o) {
                    const float w = W2[o * 64 + i];
#pragma unroll
                    for (int s = 0; s < 16; ++s) acc[s] = fmaf(w, dH[s0 + s][o], acc[s]);
                }
            }
#pragma unroll
            for (int s = 0; s < 16; ++s) dh1[s0 + s][i] = h1[s0 + s][i] > 0.f ? acc[s] : 0.f;
        }
        __syncthreads();
        if (tid < ATK_PASS * 3) {                                      // back through [3 -> 64]
            const int s = tid / 3, a = tid % 3;
            float acc = 0.f;
            for (int i = 0; i < 64; ++i) acc = fmaf(W1[i * 4 + a], dh1[s][i], acc);
            dxt[s][a] = acc;
        }
        __syncthreads();
        if (tid < np) {
            const int i = pts[base + tid];
            const float a0 = dxt[tid][0], a1 = dxt[tid][1], a2 = dxt[tid][2];
            float* Gp = G + (size_t)i * 3;
            if (TRUNK) {                                               // x . trans backwards: dx_i = sum_j d(xT)_j trans[i][j]
                Gp[0] = fmaf(a2, tr[2], fmaf(a1, tr[1], a0 * tr[0]));
                Gp[1] = fmaf(a2, tr[5], fmaf(a1, tr[4], a0 * tr[3]));
                Gp[2] = fmaf(a2, tr[8], fmaf(a1, tr[7], a0 * tr[6]));
            } else {
                Gp[0] += a0; Gp[1] += a1; Gp[2] += a2;
            }
        }
        if (TRUNK && tid < 9)
            for (int s = 0; s < np; ++s) dt = fmaf(xr[s][tid / 3], dxt[s][tid % 3], dt);
        __syncthreads();
    }
    if (TRUNK && tid < 64) dtrans[(size_t)b * 64 + tid] = tid < 9 ? dt : 0.f;
}

__global__ __launch_bounds__(256) void fgm_update_kernel(int kind, const float* __restrict__ grad, float* __restrict__ pc,
                                                         const float* __restrict__ ori_pc, float* __restrict__ momentum, float step,
                                                         float budget, float mu, const int32_t* __restrict__ n_points, int stride) {
    __shared__ float sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int E = atk_rows(n_points, b, stride) * 3;
    const size_t off = (size_t)b * stride * 3;
    const float* Gd = grad + off;
    float* P = pc + off;
    const float* D = Gd;                                               // the direction that is L2-normalised
    if (kind == KIND_MIFGM) {
        float* M = momentum + off;
        float a = 0.f;
        for (int i = tid; i < E; i += 256) a += fabsf(Gd[i]);
        const float l1 = atk_block_sum(a, sh) + 1e-9f;
        for (int i = tid; i < E; i += 256) M[i] = mu * M[i] + Gd[i] / l1;
        D = M;                                                         // each thread reads back what it wrote itself
    }
    float a = 0.f;
    for (int i = tid; i < E; i += 256) a = fmaf(D[i], D[i], a);
    const float norm = sqrtf(atk_block_sum(a, sh)) + 1e-9f;
    for (int i = tid; i < E; i += 256) P[i] = P[i] - step * (D[i] / norm);
    if (kind == KIND_FGM) return;
    // ClipPointsL2 against ori_pc
    const float* O = ori_pc + off;
    a = 0.f;
    for (int i = tid; i < E; i += 256) { const float d = P[i] - O[i]; a = fmaf(d, d, a); }
    const float sf = fminf(budget / (sqrtf(atk_block_sum(a, sh)) + 1e-9f), 1.f);
    for (int i = tid; i < E; i += 256) P[i] = O[i] + (P[i] - O[i]) * sf;
}

__global__ __launch_bounds__(256) void success_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ target, int B,
                                                      int32_t* __restrict__ success) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < B) success[b] = pred[b] == target[b] ? 1 : 0;
}

void launch_fc_t(const float* gimg, const ClsFc& L, const float* x, int B, const float* mask, float* out, hipStream_t s) {
    hipLaunchKernelGGL(fc_t_kernel, dim3((L.n_out / 16 + 3) / 4, (B + 15) / 16), dim3(256), 0, s, gimg, L, x, B, mask, out);
}

}  // namespace

hipError_t launch_atk_check(const int32_t* n_points, const int32_t* target, int B, int lo, int hi, int n_classes, int32_t* bad,
                            hipStream_t s) {
    hipError_t e = hipMemsetAsync(bad, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(atk_check_kernel, dim3((B + 255) / 256), dim3(256), 0, s, n_points, target, B, lo, hi, n_classes, bad);
    return hipGetLastError();
}

hipError_t launch_cls_backward(const float* img, const ClsImage& I, const float* gimg, const ClsGradImage& G, const float* pc,
                               const int32_t* n_points, int B, int stride, const int32_t* target, int loss_kind, float kappa, float scale,
                               const ClsGradWs& w, int n_classes, float* grad, hipStream_t s) {
    const dim3 block(256);
    hipLaunchKernelGGL(loss_grad_kernel, dim3((B + 255) / 256), block, 0, s, (const float*)w.logits, target, B, n_classes, loss_kind, kappa,
                       scale, w.loss, w.d_out);
    launch_fc_t(gimg, G.head_fct[2], w.d_out, B, w.f2, w.d2, s);
    launch_fc_t(gimg, G.head_fct[1], w.d2, B, w.f1, w.d1, s);
    launch_fc_t(gimg, G.head_fct[0], w.d1, B, nullptr, w.g, s);
    hipLaunchKernelGGL((stack_backward_kernel<true>), dim3(B), block, 0, s, img, I.trunk.first, gimg, G.trunk, pc, n_points, stride,
                       (const float*)w.trans, (const int32_t*)w.win, (const float*)w.g, grad, w.d_out);
    launch_fc_t(gimg, G.stn_fct[2], w.d_out, B, w.f2_stn, w.d2, s);
    launch_fc_t(gimg, G.stn_fct[1], w.d2, B, w.f1_stn, w.d1, s);
    launch_fc_t(gimg, G.stn_fct[0], w.d1, B, w.gmax_stn, w.g, s);       // the STN's max-pool sits behind a ReLU
    hipLaunchKernelGGL((stack_backward_kernel<false>), dim3(B), block, 0, s, img, I.stn.first, gimg, G.stn, pc, n_points, stride,
                       (const float*)nullptr, (const int32_t*)w.win_stn, (const float*)w.g, grad, (float*)nullptr);
    return hipGetLastError();
}

hipError_t launch_loss_grad(const float* logits, const int32_t* target, int B, int n_classes, int loss_kind, float kappa, float scale,
                            float* loss, float* d_out, hipStream_t s) {
    hipLaunchKernelGGL(loss_grad_kernel, dim3((B + 255) / 256), dim3(256), 0, s, logits, target, B, n_classes, loss_kind, kappa, scale, loss,
                       d_out);
    return hipGetLastError();
}

hipError_t launch_fgm_update(int kind, const float* grad, float* pc, const float* ori_pc, float* momentum, float step_size, float budget,
                             float mu, const int32_t* n_points, int B, int stride, hipStream_t s) {
    hipLaunchKernelGGL(fgm_update_kernel, dim3(B), dim3(256), 0, s, kind, grad, pc, ori_pc, momentum, step_size, budget, mu, n_points,
                       stride);
    return hipGetLastError();
}

hipError_t launch_atk_success(const int32_t* pred, const int32_t* target, int B, int32_t* success, hipStream_t s) {
    hipLaunchKernelGGL(success_kernel, dim3((B + 255) / 256), dim3(256), 0, s, pred, target, B, success);
    return hipGetLastError();
}

}  // namespace ifd
