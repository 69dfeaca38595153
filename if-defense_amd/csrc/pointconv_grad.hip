// Input gradients of the PointConv victim (include/ifd_pc_atk.h): d loss / d points for the two adversarial losses of
// include/ifd_atk.h, with the four index tables (fps1, fps2, knn1, knn2) held fixed.  Everything else carries gradient: the
// differences to the centroids through the MLPs and through WeightNet, the centroids, sa3's mean, and the Gaussian density.
// The forward half is launch_pc itself (pointconv.hip), so logits, pred, the tables, the densities and the features are its bits;
// it leaves xyz1 .. xyz3, the tables, dens1 .. dens3, l1_feat, u2, l2_feat, s3a, s3b, s3c, wn3, gfeat, f1 and f2 behind, and its
// contraction buffer g, dead by then, takes d G of one level after the other.  The backward half, in launch order:
//
//   launch_head_backward      (victim_linear.h) loss_grad_kernel: logits, target -> loss, scale * d loss / d logits; the head's layers
//   linear_kernel<Pn2Linear>  every dense layer transposed (PcGradImage, zero bias, no activation): the head, the three wide linears
//                             (d G = W_l^T d Y), sa3's MLP, sa2's U; act_gate_kernel applies ReLU's derivative at the saved activation
//   pc_sa3_bwd_kernel         a workgroup a row k of sa3: d t, d Wn, d s and d F from d G; WeightNet backward
//   pc_density_a_kernel       the forward's density again (a wave a point), DensityNet forward and backward: a_j = d rho_j / (n c2)
//   pc_centre_bwd_kernel      sa3's centre: d xyz2[g] = d delta[g] - mean of all d delta
//   pc_density_nbody_kernel   a wave a point p: sum_j (a_p + a_j) e_pj (2 / c1) (x_j - x_p), in the forward density's order
//   pc_sa_bwd_kernel<2>, <1>  the hot path: a 64-row tile as the forward's (one group of sa2, two of sa1).  The MLP tile and WeightNet
//                             again by the forward's instruction sequence; per 64 channels of the last layer d t, d Wn, d s and d F,
//                             whose transposed layer accumulates on v_mfma_f32_16x16x4_f32 across the passes; the middle layer
//                             transposed on the same MFMA; the first layer and WeightNet backward by plain FMAs
//   pc_l1_gather_kernel       rows of sa2 -> level-1 points (d U, d delta, d s), then the level-2 centroids, ascending, no atomics
//   pc_point_gather_kernel    rows of sa1 -> cloud points (d delta, d s), then the level-1 centroids
// Every sum has a fixed order, nothing here uses float atomics, and every kernel works on one cloud's rows alone.
#include "ifd_device.h"
#include "ifd_internal.h"
#include "lds_layout.h"
#include "pc_device.h"
#include "victim_fps.h"
#include "victim_linear.h"

namespace ifd {

namespace {

constexpr int PC_ROWS1 = PC_NP1 * PC_K1, PC_ROWS2 = PC_NP2 * PC_K2;
constexpr int PC_PG_THREADS = 128;                                      // points of a workgroup of pc_point_gather_kernel
constexpr size_t PC_GB = (size_t)PC_NP1 * 128 * PC_WN;                 // floats of a cloud's contraction buffer
static_assert(PC_NP1 == 512 && PC_K1 == 32 && PC_NP2 == 128 && PC_K2 == 64 && PC_EMB == 1024 && PC_WN == 16 && LINEAR_TILE == 64,
              "the tilings of the backward kernels");

// mgate3 [B][128][56]: words 0 .. 7 of a row s3a's 256 channels, 8 .. 23 s3b's 512, 24 .. 55 s3c's 1024
__global__ __launch_bounds__(256) void pc_act3_kernel(const float* __restrict__ s3a, const float* __restrict__ s3b, const float* __restrict__ s3c,
                                                      int B, uint32_t* __restrict__ mgate3) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * PC_NP2 * 56) return;
    const int w = i % 56;
    const size_t row = (size_t)(i / 56);
    const float* x = w < 8 ? s3a + row * 256 + 32 * w : (w < 24 ? s3b + row * 512 + 32 * (w - 8) : s3c + row * PC_EMB + 32 * (w - 24));
    uint32_t bits = 0;
    for (int e = 0; e < 32; ++e)
        if (x[e] > 0.f) bits |= 1u << e;
    mgate3[i] = bits;
}

// WeightNet again on one difference (the forward's chains), then backward from dW [16]: dd [3] = d (dx, dy, dz).  Every transposed
// layer is one fused chain from 0 over the layer's outputs in ascending order.  Returns the gates: bits 0 .. 7 the first layer, 8 ..
// 15 the second, 16 .. 31 the third.
__device__ __forceinline__ uint32_t weight_net_bwd(const float* __restrict__ wn, float dx, float dy, float dz, const float (&dW)[PC_WN],
                                                   float (&dd)[3]) {
    const float x[3] = {dx, dy, dz};
    float h1[8], h2[8], o[PC_WN];
    small_layer<8, 3>(wn, wn + 24, x, h1);
    small_layer<8, 8>(wn + 32, wn + 96, h1, h2);
    small_layer<PC_WN, 8>(wn + 104, wn + 232, h2, o);
    uint32_t bits = 0;
    float g3[PC_WN], g2[8], g1[8];
#pragma unroll
    for (int i = 0; i < PC_WN; ++i) {
        const bool on = o[i] > 0.f;
        bits |= (uint32_t)on << (16 + i);
        g3[i] = on ? dW[i] : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < PC_WN; ++i) acc = fmaf(g3[i], wn[104 + i * 8 + c], acc);
        const bool on = h2[c] > 0.f;
        bits |= (uint32_t)on << (8 + c);
        g2[c] = on ? acc : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = fmaf(g2[i], wn[32 + i * 8 + c], acc);
        const bool on = h1[c] > 0.f;
        bits |= (uint32_t)on << c;
        g1[c] = on ? acc : 0.f;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc = fmaf(g1[i], wn[i * 3 + a], acc);
        dd[a] = acc;
    }
    return bits;
}

// sa3 backward, a workgroup a row k of a cloud.  dG [16384] at dG + b * gb; F = s3c [B][128][1024]; dens [B][128]; wn3 [B][128][16];
// xyz3 [B][128][3].  Thread t takes the channels c = t, t + 256, t + 512, t + 768 in that order:
//   dt = chain over w of dG[c][w] Wn[k][w];  d Wn[w] += dG[c][w] * (F s);  d s += dt F;  dF[k][c] = F > 0 ? dt * s : 0.
// d Wn and d s of the 256 threads: a butterfly 1, 2, ..., 32 in each wave, the four waves (w0 + w1) + (w2 + w3).
// Out: dF [B][128][1024], ds [B][128], dwn [B][128][4] = WeightNet^T d Wn, wgate [B][128].
__global__ __launch_bounds__(256) void pc_sa3_bwd_kernel(const float* __restrict__ dG, size_t gb, const float* __restrict__ F,
                                                         const float* __restrict__ dens, const float* __restrict__ wn3,
                                                         const float* __restrict__ xyz3, const float* __restrict__ wn, float* __restrict__ dF,
                                                         float* __restrict__ ds, float* __restrict__ dwn, uint32_t* __restrict__ wgate) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcSa3BwdLds::BYTES];
    float* red = LDS_AT(float, smem, PcSa3BwdLds::RED);
    const int k = blockIdx.x, b = blockIdx.y, wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const size_t row = (size_t)b * PC_NP2 + k;
    const float s = dens[row];
    float wr[PC_WN], acc[PC_WN + 1];
#pragma unroll
    for (int w = 0; w < PC_WN; ++w) {
        wr[w] = wn3[row * PC_WN + w];
        acc[w] = 0.f;
    }
    acc[PC_WN] = 0.f;
    const float* Gb = dG + (size_t)b * gb;
#pragma unroll 1
    for (int c = threadIdx.x; c < PC_EMB; c += 256) {
        const float f = F[row * PC_EMB + c];
        float dg[PC_WN];
#pragma unroll
        for (int w = 0; w < PC_WN; w += 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(Gb + (size_t)c * PC_WN + w);
            dg[w] = v[0]; dg[w + 1] = v[1]; dg[w + 2] = v[2]; dg[w + 3] = v[3];
        }
        float dt = 0.f;
#pragma unroll
        for (int w = 0; w < PC_WN; ++w) dt = fmaf(dg[w], wr[w], dt);
        const float tv = f * s;
#pragma unroll
        for (int w = 0; w < PC_WN; ++w) acc[w] = fmaf(dg[w], tv, acc[w]);
        acc[PC_WN] = fmaf(dt, f, acc[PC_WN]);
        dF[row * PC_EMB + c] = f > 0.f ? dt * s : 0.f;
    }
#pragma unroll
    for (int w = 0; w <= PC_WN; ++w) {
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) acc[w] += __shfl_xor(acc[w], off);
        if (l == 0) red[wv * (PC_WN + 1) + w] = acc[w];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float dW[PC_WN], dd[3];
        constexpr int R = PC_WN + 1;
#pragma unroll
        for (int w = 0; w < PC_WN; ++w) dW[w] = (red[w] + red[R + w]) + (red[2 * R + w] + red[3 * R + w]);
        ds[row] = (red[PC_WN] + red[R + PC_WN]) + (red[2 * R + PC_WN] + red[3 * R + PC_WN]);
        const uint32_t bits = weight_net_bwd(wn, xyz3[row * 3], xyz3[row * 3 + 1], xyz3[row * 3 + 2], dW, dd);
        *reinterpret_cast<f32x4*>(dwn + row * 4) = f32x4{dd[0], dd[1], dd[2], 0.f};
        if (wgate) wgate[row] = bits;
    }
}

// sa3's centre backward, 128 threads a cloud.  d delta[k] = dx3m[k] + dwn3[k]; per axis the 128 added in ascending k from 0, times
// 1/128; dx2a[g] = d delta[g] - that mean.
__global__ __launch_bounds__(PC_NP2) void pc_centre_bwd_kernel(const float* __restrict__ dx3m, const float* __restrict__ dwn3,
                                                               float* __restrict__ dx2a) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcCentreLds::BYTES];
    float* mean = LDS_AT(float, smem, PcCentreLds::MEAN);
    const int b = blockIdx.x, k = threadIdx.x;
    const float* A = dx3m + (size_t)b * PC_NP2 * 4;
    const float* W = dwn3 + (size_t)b * PC_NP2 * 4;
    if (k < 3) {
        float sum = 0.f;
        for (int j = 0; j < PC_NP2; ++j) sum += A[4 * j + k] + W[4 * j + k];
        mean[k] = sum * (1.f / PC_NP2);
    }
    __syncthreads();
    f32x4 o;
#pragma unroll
    for (int a = 0; a < 3; ++a) o[a] = (A[4 * k + a] + W[4 * k + a]) - mean[a];
    o[3] = 0.f;
    *reinterpret_cast<f32x4*>(dx2a + ((size_t)b * PC_NP2 + k) * 4) = o;
}

// pc_density_kernel again (the same sums, so rho_j and DensityNet's activations are the forward's bits), then DensityNet backward
// from ds[b][j]: a[b][j] = (d rho_j / (float)n) / c2.  dgate: bits 0 .. 7 the first layer, 8 .. 15 the second, 16 the third.
__global__ __launch_bounds__(256) void pc_density_a_kernel(const float* __restrict__ X, size_t xb, const int32_t* __restrict__ n_points,
                                                           int n_fixed, const float* __restrict__ dn, float c1, float c2,
                                                           const float* __restrict__ ds, int lds, float* __restrict__ aj,
                                                           uint32_t* __restrict__ dgate, int ldg) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcDensityBwdLds::BYTES];
    float* sx = LDS_AT(float, smem, PcDensityBwdLds::X);
    const int b = blockIdx.y, wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int n = cloud_points(n_points, b, n_fixed);
    if (blockIdx.x * 32 >= n) return;                                  // the whole workgroup
    const float* Xb = X + (size_t)b * xb;
    for (int e = threadIdx.x; e < 3 * n; e += 256) sx[e] = Xb[e];
    __syncthreads();
    const float nf = (float)n;
    for (int jj = 0; jj < 8; ++jj) {
        const int j = blockIdx.x * 32 + jj * 4 + wv;
        if (j >= n) continue;                                          // the whole wave
        const float xj = sx[3 * j], yj = sx[3 * j + 1], zj = sx[3 * j + 2];
        float acc = 0.f;
        for (int i = l; i < n; i += 64) acc += expf(-(pn2_dist(sx[3 * i], sx[3 * i + 1], sx[3 * i + 2], xj, yj, zj) / c1));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
        const float rho[1] = {(acc / nf) / c2};
        float h1[8], h2[8], out[1];
        small_layer<8, 1>(dn, dn + 8, rho, h1);
        small_layer<8, 8>(dn + 16, dn + 80, h1, h2);
        small_layer<1, 8>(dn + 88, dn + 96, h2, out);
        uint32_t bits = 0;
        const bool on3 = out[0] > 0.f;
        bits |= (uint32_t)on3 << 16;
        const float g3 = on3 ? ds[(size_t)b * lds + j] : 0.f;
        float g2[8], g1[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const bool on = h2[c] > 0.f;
            bits |= (uint32_t)on << (8 + c);
            g2[c] = on ? g3 * dn[88 + c] : 0.f;
        }
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float a = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) a = fmaf(g2[i], dn[16 + i * 8 + c], a);
            const bool on = h1[c] > 0.f;
            bits |= (uint32_t)on << c;
            g1[c] = on ? a : 0.f;
        }
        float drho = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) drho = fmaf(g1[i], dn[i], drho);
        if (l == 0) {
            aj[(size_t)b * PC_MAX_POINTS + j] = (drho / nf) / c2;
            if (dgate) dgate[(size_t)b * ldg + j] = bits;
        }
    }
}

// The density's term of the gradient of point p among the n points of a level's input: per axis
//     (2 / c1) * sum_i ((a_p + a_i) * e_ip) * (x_i - x_p),    e_ip = expf(-(d_ip / c1)),
// lane l a fused chain over i = l, l + 64, ... from 0, the 64 lanes in the butterfly 1, 2, ..., 32: the forward density's order.
// out[b][p][0 .. 2] (rows of ldo floats, `so` rows a cloud) = base[b][p][0 .. 2] (rows of 4 floats, `sb` rows a cloud) + that term.
// zero_beyond: rows p in [n, so) are written as zeros.
__global__ __launch_bounds__(256) void pc_density_nbody_kernel(const float* __restrict__ X, size_t xb, const int32_t* __restrict__ n_points,
                                                               int n_fixed, float c1, const float* __restrict__ aj, const float* base, int sb,
                                                               float* out, int so, int ldo, int zero_beyond) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcDensityBwdLds::BYTES];
    float* sx = LDS_AT(float, smem, PcDensityBwdLds::X);
    float* sa = LDS_AT(float, smem, PcDensityBwdLds::AJ);
    const int b = blockIdx.y, wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int n = cloud_points(n_points, b, n_fixed);
    if (zero_beyond && threadIdx.x < 32) {
        const int p = blockIdx.x * 32 + threadIdx.x;
        if (p >= n && p < so) {
            float* o = out + ((size_t)b * so + p) * ldo;
            o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
        }
    }
    if (blockIdx.x * 32 >= n) return;                                  // the whole workgroup
    const float* Xb = X + (size_t)b * xb;
    for (int e = threadIdx.x; e < 3 * n; e += 256) sx[e] = Xb[e];
    for (int e = threadIdx.x; e < n; e += 256) sa[e] = aj[(size_t)b * PC_MAX_POINTS + e];
    __syncthreads();
    const float tc = 2.f / c1;
    for (int jj = 0; jj < 8; ++jj) {
        const int p = blockIdx.x * 32 + jj * 4 + wv;
        if (p >= n) continue;                                          // the whole wave
        const float xp = sx[3 * p], yp = sx[3 * p + 1], zp = sx[3 * p + 2], ap = sa[p];
        float ax = 0.f, ay = 0.f, az = 0.f;
        for (int i = l; i < n; i += 64) {
            const float xi = sx[3 * i], yi = sx[3 * i + 1], zi = sx[3 * i + 2];
            const float k = (ap + sa[i]) * expf(-(pn2_dist(xi, yi, zi, xp, yp, zp) / c1));
            ax = fmaf(k, xi - xp, ax);
            ay = fmaf(k, yi - yp, ay);
            az = fmaf(k, zi - zp, az);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            ax += __shfl_xor(ax, off); ay += __shfl_xor(ay, off); az += __shfl_xor(az, off);
        }
        if (l == 0) {
            const float* bs = base + ((size_t)b * sb + p) * 4;
            float* o = out + ((size_t)b * so + p) * ldo;
            const float gx = bs[0] + ax * tc, gy = bs[1] + ay * tc, gz = bs[2] + az * tc;
            o[0] = gx; o[1] = gy; o[2] = gz;
        }
    }
}

struct PcSaBwdArgs {
    const float* first;     // sa1: [64][4] = {w0, w1, w2, bias}; sa2: [128][4] = {w0, w1, w2, -}
    const float* U;         // sa2: [B][512][128]
    const float *W2, *b2, *W3, *b3, *wn;
    const float *W3T, *W2T; // the last layer^T [MID][C], the middle layer^T [MID][MID]
    const float* X;         // sa1: the clouds (rows of `stride`); sa2: xyz1
    const int32_t* n_points;
    int stride;
    const int32_t* knn;
    const float* cen;
    const float* dens;
    int ldd;
    const float* dG;        // d G of the level, a cloud's at dG + b * PC_GB
    const float* above;     // [B][groups][4] what the levels above leave for the centroids
    float* dh;              // sa2: [B][128][64][128] d U per row
    float* dd;              // [B][rows][4] per row: d (x_j - c_i), and d s_j in the fourth place
    float* dx;              // [B][groups][4] d of the centroids
    uint32_t* mgate;        // [B][rows][8 LV] or null
    uint32_t* wgate;        // [B][rows] or null
};

// two threads' 16 gate bits as one word (the even thread's in the low half); the even thread stores it
__device__ __forceinline__ void store_gate_pair(uint32_t* __restrict__ at, uint32_t bits16, int part) {
    uint32_t word = bits16 << (16 * (part & 1));
    word |= __shfl_xor(word, 1);
    if ((part & 1) == 0) at[part >> 1] = word;
}

// sa1 (LV 1: two groups of 32 rows a workgroup, MLP 3 -> 64 -> 64 -> 128) and sa2 (LV 2: one group of 64 rows, 131 -> 128 -> 128 ->
// 256) backward.  The elementwise passes: a thread = a row x a quarter (`part`) of the channels.  Per 64 channels of the last layer, in
// ascending order, a thread takes 16 of them in ascending order:
//   dt = chain over w from 0 of dG[c][w] Wn[w];  d Wn[w] = fma(dG[c][w], F s, d Wn[w]);  d s = fma(dt, F, d s);  dF = F > 0 ? dt * s : 0
// so that a quarter's d Wn and d s are ONE chain each over its 16 channels of every pass, and the quarters are added (q0 + q1) +
// (q2 + q3).  d a2 = W3^T dF accumulates pass after pass in the MFMA's registers (blocks of 64 inputs from 0, ascending).
template <int LV>
__global__ __launch_bounds__(256) void pc_sa_bwd_kernel(const PcSaBwdArgs a) {
    constexpr int MID = 64 * LV, C = 128 * LV, KG = LV == 1 ? PC_K1 : PC_K2, NPG = LV == 1 ? PC_NP1 : PC_NP2, PT = MID / 4, NT = MID / 64;
    constexpr int NW = 8 * LV;                                         // gate words of a row: MID / 32 + MID / 32 + C / 32
    using L = PcSaBwdLds<MID + 4, 256>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* A = LDS_AT(float, smem, L::A);
    float* Bm = LDS_AT(float, smem, L::B);
    float* DGs = LDS_AT(float, smem, L::DG);
    float* WN = LDS_AT(float, smem, L::WN);
    float* S = LDS_AT(float, smem, L::S);
    float* DD = LDS_AT(float, smem, L::DD);
    constexpr int LD = L::LD, XLD = L::XLD;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, q = l >> 4, p = l & 15;
    const int row = threadIdx.x >> 2, part = threadIdx.x & 3, o0 = part * PT;
    const int g = LV == 1 ? tile * 2 + (row >> 5) : tile;
    const size_t grow = ((size_t)b * NPG + g) * KG + (row & (KG - 1));  // this row among the cloud's
    const int n = LV == 1 ? cloud_points(a.n_points, b, a.stride) : PC_NP1, xs = LV == 1 ? a.stride : PC_NP1;
    uint32_t gate1 = 0;                                                // first layer > 0 of the thread's PT channels
    float dx, dy, dz;
    {                                                                  // the forward's first layer, WeightNet and scales
        const int j = min(max(a.knn[grow], 0), n - 1);
        const float* x = a.X + ((size_t)b * xs + j) * 3;
        const float* c = a.cen + ((size_t)b * NPG + g) * 3;
        dx = x[0] - c[0]; dy = x[1] - c[1]; dz = x[2] - c[2];
#pragma unroll
        for (int e = 0; e < PT; e += 4) {
            f32x4 v;
            if constexpr (LV == 2) v = *reinterpret_cast<const f32x4*>(a.U + ((size_t)b * PC_NP1 + j) * 128 + o0 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(a.first + (o0 + e + r) * 4);
                v[r] = fmaxf(fmaf(w[2], dz, fmaf(w[1], dy, fmaf(w[0], dx, LV == 1 ? w[3] : v[r]))), 0.f);
                if (v[r] > 0.f) gate1 |= 1u << (e + r);
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = v;
        }
        float w4[4];
        weight_net<4>(a.wn, dx, dy, dz, part * 4, w4);
        *reinterpret_cast<f32x4*>(WN + row * PC_WN + part * 4) = f32x4{w4[0], w4[1], w4[2], w4[3]};
        if (part == 0) S[row] = a.dens[(size_t)b * a.ldd + j];
        const float* Gt = a.dG + (size_t)b * PC_GB + (size_t)tile * (256 * PC_WN);   // the tile's group(s): 4096 floats
#pragma unroll
        for (int e = 0; e < 4; ++e)
            *reinterpret_cast<f32x4*>(DGs + (e * 256 + threadIdx.x) * 4) = *reinterpret_cast<const f32x4*>(Gt + (e * 256 + threadIdx.x) * 4);
    }
    if (a.mgate) {                                                     // wave-uniform
        if constexpr (LV == 1) store_gate_pair(a.mgate + grow * NW, gate1, part);
        else a.mgate[grow * NW + part] = gate1;
    }
    __syncthreads();
    f32x4 v[2][2];
#pragma unroll
    for (int ob = 0; ob < MID; ob += 64) {
        const int obase = ob + 32 * (wv >> 1);
        tile_layer<MID, LD>(A, a.W2, a.b2, obase, wv, q, p, v);
        tile_store<LD>(Bm, obase, wv, q, p, v);
    }
    __syncthreads();
    float wnr[PC_WN], dwp[PC_WN], dsp = 0.f;
#pragma unroll
    for (int w = 0; w < PC_WN; ++w) {
        wnr[w] = WN[row * PC_WN + w];
        dwp[w] = 0.f;
    }
    const float s = S[row];
    const float* dgr = DGs + (LV == 1 ? (row >> 5) * (128 * PC_WN) : 0);
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 sum[NT][2][2];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int m = 0; m < 2; ++m) sum[nt][t][m] = zero;
    float* Xs = A;                                                     // the first layer is in gate1 now
#pragma unroll 1
    for (int ob = 0; ob < C; ob += 64) {
        tile_layer<MID, LD>(Bm, a.W3, a.b3, ob + 32 * (wv >> 1), wv, q, p, v);
        __syncthreads();                                               // the pass before has read Xs (the first: the middle layer has read A)
        tile_store<XLD>(Xs, 32 * (wv >> 1), wv, q, p, v);              // channels ob .. ob + 63 at columns 0 .. 63
        __syncthreads();
        uint32_t gate3 = 0;
#pragma unroll
        for (int e = 0; e < 16; e += 4) {
            f32x4 f = *reinterpret_cast<const f32x4*>(Xs + row * XLD + part * 16 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* gp = dgr + (ob + part * 16 + e + r) * PC_WN;
                float dg[PC_WN];
#pragma unroll
                for (int w = 0; w < PC_WN; w += 4) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(gp + w);
                    dg[w] = t4[0]; dg[w + 1] = t4[1]; dg[w + 2] = t4[2]; dg[w + 3] = t4[3];
                }
                float dt = 0.f;
#pragma unroll
                for (int w = 0; w < PC_WN; ++w) dt = fmaf(dg[w], wnr[w], dt);
                const float tv = f[r] * s;
#pragma unroll
                for (int w = 0; w < PC_WN; ++w) dwp[w] = fmaf(dg[w], tv, dwp[w]);
                dsp = fmaf(dt, f[r], dsp);
                const bool on = f[r] > 0.f;
                gate3 |= (uint32_t)on << (e + r);
                f[r] = on ? dt * s : 0.f;
            }
            *reinterpret_cast<f32x4*>(Xs + row * XLD + part * 16 + e) = f;
        }
        if (a.mgate) store_gate_pair(a.mgate + grow * NW + 4 * NT + 2 * (ob >> 6), gate3, part);   // wave-uniform
        __syncthreads();
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float* xr[2];
            const float* wr[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                xr[t] = Xs + (32 * (wv & 1) + 16 * t + p) * XLD + 4 * q;
                wr[t] = a.W3T + (size_t)(64 * nt + 32 * (wv >> 1) + 16 * t + p) * C + ob + 4 * q;
            }
            linear_block64(xr, wr, 0, sum[nt]);
        }
    }
    // the quarters of a row: (q0 + q1) + (q2 + q3), every lane the same tree
    dsp += __shfl_xor(dsp, 1); dsp += __shfl_xor(dsp, 2);
#pragma unroll
    for (int w = 0; w < PC_WN; ++w) {
        dwp[w] += __shfl_xor(dwp[w], 1); dwp[w] += __shfl_xor(dwp[w], 2);
    }
    float dwd[3];
    const uint32_t wbits = weight_net_bwd(a.wn, dx, dy, dz, dwp, dwd);
    __syncthreads();                                                   // the last pass has read Xs
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) tile_store<LD>(A, 64 * nt + 32 * (wv >> 1), wv, q, p, sum[nt]);
    __syncthreads();
    {                                                                  // the middle layer's gate
        uint32_t gate2 = 0;
#pragma unroll
        for (int e = 0; e < PT; e += 4) {
            const f32x4 act = *reinterpret_cast<const f32x4*>(Bm + row * LD + o0 + e);
            f32x4 d = *reinterpret_cast<const f32x4*>(A + row * LD + o0 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (act[r] > 0.f) gate2 |= 1u << (e + r);
                else d[r] = 0.f;
            }
            *reinterpret_cast<f32x4*>(A + row * LD + o0 + e) = d;
        }
        if (a.mgate) {                                                 // wave-uniform
            if constexpr (LV == 1) store_gate_pair(a.mgate + grow * NW + 2, gate2, part);
            else a.mgate[grow * NW + 4 + part] = gate2;
        }
    }
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) tile_layer_t<MID, LD>(A, a.W2T, Bm, 64 * nt + 32 * (wv >> 1), wv, q, p);
    __syncthreads();
    {                                                                  // the first layer's gate; d U of the row; d delta = Wxyz^T d a1 + WeightNet's
        float px = 0.f, py = 0.f, pz = 0.f;
#pragma unroll
        for (int e = 0; e < PT; e += 4) {
            f32x4 d = *reinterpret_cast<const f32x4*>(Bm + row * LD + o0 + e);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (!((gate1 >> (e + r)) & 1u)) d[r] = 0.f;
                const f32x4 w = *reinterpret_cast<const f32x4*>(a.first + (o0 + e + r) * 4);
                px = fmaf(d[r], w[0], px);
                py = fmaf(d[r], w[1], py);
                pz = fmaf(d[r], w[2], pz);
            }
            if constexpr (LV == 2) *reinterpret_cast<f32x4*>(a.dh + grow * 128 + o0 + e) = d;
        }
        px += __shfl_xor(px, 1); py += __shfl_xor(py, 1); pz += __shfl_xor(pz, 1);
        px += __shfl_xor(px, 2); py += __shfl_xor(py, 2); pz += __shfl_xor(pz, 2);
        if (part == 0) {
            const f32x4 d = f32x4{px + dwd[0], py + dwd[1], pz + dwd[2], dsp};
            *reinterpret_cast<f32x4*>(a.dd + grow * 4) = d;
            *reinterpret_cast<f32x4*>(DD + row * 4) = d;
            if (a.wgate) a.wgate[grow] = wbits;
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 * (64 / KG)) {                                 // d c = (0 - d delta_0 - d delta_1 ...) + the levels above's term
        const int grp = threadIdx.x >> 2, ax = threadIdx.x & 3;
        const size_t at = ((size_t)b * NPG + (LV == 1 ? tile * 2 + grp : tile)) * 4 + ax;
        float acc = 0.f;
        for (int k = 0; k < KG; ++k) acc -= DD[(KG * grp + k) * 4 + ax];
        a.dx[at] = ax < 3 ? acc + a.above[at] : 0.f;
    }
}

// A wave = a level-1 point j of a cloud.  du[j] = the sum over the rows (g, k) of sa2 with knn2[g][k] == j, ascending, of dh[g][k];
// ds2[j] the same of the rows' d s (de's fourth place); dx1a[j] the same of de, then over the groups g with fps2[g] == j, ascending, of
// dx2[g].
__global__ __launch_bounds__(256) void pc_l1_gather_kernel(const int32_t* __restrict__ knn2, const int32_t* __restrict__ fps2,
                                                           const float* __restrict__ dh, const float* __restrict__ de,
                                                           const float* __restrict__ dx2, float* __restrict__ du, float* __restrict__ dx1a,
                                                           float* __restrict__ ds2) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcGatherLds::BYTES];
    uint16_t* fps = LDS_AT(uint16_t, smem, PcGatherLds::FPS);
    uint16_t* tab = LDS_AT(uint16_t, smem, PcGatherLds::TAB);
    const int b = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int e = threadIdx.x; e < PC_ROWS2; e += 256) tab[e] = (uint16_t)min(max(knn2[(size_t)b * PC_ROWS2 + e], 0), PC_NP1 - 1);
    if (threadIdx.x < PC_NP2) fps[threadIdx.x] = (uint16_t)min(max(fps2[(size_t)b * PC_NP2 + threadIdx.x], 0), PC_NP1 - 1);
    __syncthreads();
    const float* H = dh + (size_t)b * PC_ROWS2 * 128 + 2 * lane;
    const float* E = de + (size_t)b * PC_ROWS2 * 4 + (lane & 3);           // lanes 0 .. 2: d delta; lane 3: d s
#pragma unroll 1
    for (int jj = 0; jj < 2; ++jj) {
        const int j = blockIdx.x * 8 + wv * 2 + jj;
        float a0 = 0.f, a1 = 0.f, ex = 0.f;
        for (int r0 = 0; r0 < PC_ROWS2; r0 += 64) {
            unsigned long long m = __ballot(tab[r0 + lane] == j);
            while (m) {                                                // wave-uniform
                const int r = r0 + __builtin_ctzll(m);
                m &= m - 1;
                const float2 h = *reinterpret_cast<const float2*>(H + (size_t)r * 128);
                a0 += h.x; a1 += h.y;
                if (lane < 4) ex += E[(size_t)r * 4];
            }
        }
        for (int g = 0; g < PC_NP2; ++g)
            if (fps[g] == j && lane < 3) ex += dx2[((size_t)b * PC_NP2 + g) * 4 + lane];
        *reinterpret_cast<float2*>(du + ((size_t)b * PC_NP1 + j) * 128 + 2 * lane) = float2{a0, a1};
        if (lane < 4) dx1a[((size_t)b * PC_NP1 + j) * 4 + lane] = lane < 3 ? ex : 0.f;
        if (lane == 3) ds2[(size_t)b * PC_NP1 + j] = ex;
    }
}

// A thread = a point p of a cloud: gpre[p] = the sum over the rows (i, k) of sa1 with knn1[i][k] == p, ascending, of dd[i][k], then
// over the centroids i with fps1[i] == p, ascending, of dx1[i]; ds1[p] = the sum over the same rows of d s (dd's fourth place); one
// chain each.  128 points a workgroup: a chunk of 32 clouds of 1024 points then fills the compute units.
__global__ __launch_bounds__(PC_PG_THREADS) void pc_point_gather_kernel(const int32_t* __restrict__ knn1, const int32_t* __restrict__ fps1,
                                                              const float* __restrict__ dd, const float* __restrict__ dx1, const int32_t* __restrict__ n_points, int stride,
                                                              float* __restrict__ gpre, float* __restrict__ ds1) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[PcGatherLds::BYTES];
    uint16_t* fps = LDS_AT(uint16_t, smem, PcGatherLds::FPS);
    uint16_t* tab = LDS_AT(uint16_t, smem, PcGatherLds::TAB);
    const int b = blockIdx.y, pt = blockIdx.x * PC_PG_THREADS + threadIdx.x;
    const int n = cloud_points(n_points, b, stride);
    if (blockIdx.x * PC_PG_THREADS >= n) return;                         // the whole workgroup
    for (int e = threadIdx.x; e < PC_ROWS1; e += PC_PG_THREADS) tab[e] = (uint16_t)min(max(knn1[(size_t)b * PC_ROWS1 + e], 0), n - 1);
    for (int e = threadIdx.x; e < PC_NP1; e += PC_PG_THREADS) fps[e] = (uint16_t)min(max(fps1[(size_t)b * PC_NP1 + e], 0), n - 1);
    __syncthreads();
    float gx = 0.f, gy = 0.f, gz = 0.f, gs = 0.f;
    const float* D = dd + (size_t)b * PC_ROWS1 * 4;
    for (int r0 = 0; r0 < PC_ROWS1; r0 += 8) {
        const uint4 t = *reinterpret_cast<const uint4*>(tab + r0);
        const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int j = (int)((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
            if (j == pt) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(D + (size_t)(r0 + e) * 4);
                gx += d[0]; gy += d[1]; gz += d[2]; gs += d[3];
            }
        }
    }
    const float* X = dx1 + (size_t)b * PC_NP1 * 4;
    for (int i = 0; i < PC_NP1; ++i)
        if (fps[i] == pt) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(X + (size_t)i * 4);
            gx += d[0]; gy += d[1]; gz += d[2];
        }
    if (pt < n) {
        *reinterpret_cast<f32x4*>(gpre + ((size_t)b * PC_MAX_POINTS + pt) * 4) = f32x4{gx, gy, gz, 0.f};
        ds1[(size_t)b * PC_MAX_POINTS + pt] = gs;
    }
}

}  // namespace

hipError_t configure_pc_grad_kernels() {
    return opt_in_dynamic_lds({{pc_sa_bwd_kernel<1>, PcSa1BwdLds::BYTES}, {pc_sa_bwd_kernel<2>, PcSa2BwdLds::BYTES}});
}

hipError_t launch_pc_grad(const float* img, const PcImage& I, const float* gimg, const PcGradImage& G, const float* pc,
                          const int32_t* n_points, const int32_t* fps_start, int B, int stride, const int32_t* target, int loss_kind,
                          float kappa, float scale, const PcGradWs& w, const PcGradOut& out, int n_classes, float* grad, hipStream_t s) {
    const dim3 block(256);
    PcOut o = out.f;
    o.pred = w.pred;
    hipError_t e = launch_pc(img, I, pc, n_points, fps_start, B, stride, w.f, o, w.logits, n_classes, s);
    if (e != hipSuccess) return e;
    const int32_t* fps1 = o.fps1 ? o.fps1 : w.f.fps1;
    const int32_t* fps2 = o.fps2 ? o.fps2 : w.f.fps2;
    const int32_t* knn1 = o.knn1 ? o.knn1 : w.f.knn1;
    const int32_t* knn2 = o.knn2 ? o.knn2 : w.f.knn2;
    const float* dens1 = o.dens1 ? o.dens1 : w.f.dens1;
    const int ldd1 = o.dens1 ? stride : PC_MAX_POINTS;
    const float* dens2 = o.dens2 ? o.dens2 : w.f.dens2;
    const float* dens3 = o.dens3 ? o.dens3 : w.f.dens3;
    const float* l1 = o.l1_feat ? o.l1_feat : w.f.l1_feat;
    const float* l2 = o.l2_feat ? o.l2_feat : w.f.l2_feat;
    const float* gfeat = o.gfeat ? o.gfeat : w.f.gfeat;
    const PcLevel &S1 = I.sa[0], &S2 = I.sa[1], &S3 = I.sa[2];
    const PcGradLevel &T1 = G.sa[0], &T2 = G.sa[1], &T3 = G.sa[2];
    e = launch_head_backward<Pn2Linear>(gimg, G.fct, w, target, B, n_classes, loss_kind, kappa, scale, w.dg, PC_EMB, s);
    if (e != hipSuccess) return e;
    auto gate = [&](float* d, const float* act, int n) { launch_act_gate<Pn2Linear>(d, act, n, s); };
    // a level's density: a_j from d s, then the N-body term added to `base`
    auto density = [&](int level, const float* X, int xs, const int32_t* np, const float* ds, int lds, uint32_t* dgate, int ldg,
                       const float* base, int sb, float* dst, int so, int ldo, int zero_beyond) {
        const dim3 grid((xs + 31) / 32, B);
        hipLaunchKernelGGL(pc_density_a_kernel, grid, block, 0, s, X, (size_t)xs * 3, np, xs, img + I.sa[level].dn, pc_two_bw2(level),
                           pc_norm(level), ds, lds, w.aj, dgate, ldg);
        hipLaunchKernelGGL(pc_density_nbody_kernel, grid, block, 0, s, X, (size_t)xs * 3, np, xs, pc_two_bw2(level), (const float*)w.aj, base,
                           sb, dst, so, ldo, zero_beyond);
    };
    // sa3's wide linear
    gate(w.dg, gfeat, B * PC_EMB);
    launch_linear<Pn2Linear>(gimg, T3.lint, w.dg, PC_EMB, 0, nullptr, 1, B, w.f.g, (int)PC_GB, 0, 0, s);
    // sa3
    hipLaunchKernelGGL(pc_sa3_bwd_kernel, dim3(PC_NP2, B), block, 0, s, (const float*)w.f.g, PC_GB, (const float*)w.f.s3c, dens3,
                       (const float*)w.f.wn3, (const float*)w.f.xyz3, img + S3.wn, w.ds3c, w.ds3, w.dwn3, out.wgate3);
    launch_linear<Pn2Linear>(gimg, T3.w3t, w.ds3c, PC_EMB, (size_t)PC_NP2 * PC_EMB, nullptr, B, PC_NP2, w.ds3b, 512, (size_t)PC_NP2 * 512, 0, s);
    gate(w.ds3b, w.f.s3b, B * PC_NP2 * 512);
    launch_linear<Pn2Linear>(gimg, T3.w2t, w.ds3b, 512, (size_t)PC_NP2 * 512, nullptr, B, PC_NP2, w.ds3a, 256, (size_t)PC_NP2 * 256, 0, s);
    gate(w.ds3a, w.f.s3a, B * PC_NP2 * 256);
    launch_linear<Pn2Linear>(gimg, T3.ut, w.ds3a, 256, (size_t)PC_NP2 * 256, nullptr, B, PC_NP2, w.dl2, 256, (size_t)PC_NP2 * 256, 0, s);
    launch_linear<Pn2Linear>(gimg, T3.xt, w.ds3a, 256, (size_t)PC_NP2 * 256, nullptr, B, PC_NP2, w.dx3m, 4, (size_t)PC_NP2 * 4, 0, s);
    if (out.mgate3)
        hipLaunchKernelGGL(pc_act3_kernel, dim3((B * PC_NP2 * 56 + 255) / 256), block, 0, s, (const float*)w.f.s3a, (const float*)w.f.s3b,
                           (const float*)w.f.s3c, B, out.mgate3);
    hipLaunchKernelGGL(pc_centre_bwd_kernel, dim3(B), dim3(PC_NP2), 0, s, (const float*)w.dx3m, (const float*)w.dwn3, w.dx2a);
    density(2, w.f.xyz2, PC_NP2, nullptr, w.ds3, PC_NP2, out.dgate3, PC_NP2, w.dx2a, PC_NP2, w.dx2a, PC_NP2, 4, 0);
    // sa2
    gate(w.dl2, l2, B * PC_NP2 * 256);
    launch_linear<Pn2Linear>(gimg, T2.lint, w.dl2, 256, (size_t)PC_NP2 * 256, nullptr, B, PC_NP2, w.f.g, 256 * PC_WN, PC_GB, 0, s);
    PcSaBwdArgs a2{};
    a2.first = img + S2.first_xyz; a2.U = w.f.u2;
    a2.W2 = img + S2.mlp[0].w; a2.b2 = img + S2.mlp[0].b; a2.W3 = img + S2.mlp[1].w; a2.b3 = img + S2.mlp[1].b; a2.wn = img + S2.wn;
    a2.W3T = gimg + T2.w3t.w; a2.W2T = gimg + T2.w2t.w;
    a2.X = w.f.xyz1; a2.n_points = nullptr; a2.stride = PC_NP1; a2.knn = knn2; a2.cen = w.f.xyz2; a2.dens = dens2; a2.ldd = PC_NP1;
    a2.dG = w.f.g; a2.above = w.dx2a; a2.dh = w.dh; a2.dd = w.de; a2.dx = w.dx2; a2.mgate = out.mgate2; a2.wgate = out.wgate2;
    hipLaunchKernelGGL(pc_sa_bwd_kernel<2>, dim3(PC_NP2, B), block, (size_t)PcSa2BwdLds::BYTES, s, a2);
    hipLaunchKernelGGL(pc_l1_gather_kernel, dim3(PC_NP1 / 8, B), block, 0, s, knn2, fps2, (const float*)w.dh, (const float*)w.de,
                       (const float*)w.dx2, w.du, w.dx1a, w.ds2);
    density(1, w.f.xyz1, PC_NP1, nullptr, w.ds2, PC_NP1, out.dgate2, PC_NP1, w.dx1a, PC_NP1, w.dx1a, PC_NP1, 4, 0);
    launch_linear<Pn2Linear>(gimg, T2.ut, w.du, 128, (size_t)PC_NP1 * 128, nullptr, B, PC_NP1, w.dl1, 128, (size_t)PC_NP1 * 128, 0, s);
    // sa1
    gate(w.dl1, l1, B * PC_NP1 * 128);
    launch_linear<Pn2Linear>(gimg, T1.lint, w.dl1, 128, (size_t)PC_NP1 * 128, nullptr, B, PC_NP1, w.f.g, 128 * PC_WN, PC_GB, 0, s);
    PcSaBwdArgs a1{};
    a1.first = img + S1.first_xyz; a1.U = nullptr;
    a1.W2 = img + S1.mlp[0].w; a1.b2 = img + S1.mlp[0].b; a1.W3 = img + S1.mlp[1].w; a1.b3 = img + S1.mlp[1].b; a1.wn = img + S1.wn;
    a1.W3T = gimg + T1.w3t.w; a1.W2T = gimg + T1.w2t.w;
    a1.X = pc; a1.n_points = n_points; a1.stride = stride; a1.knn = knn1; a1.cen = w.f.xyz1; a1.dens = dens1; a1.ldd = ldd1;
    a1.dG = w.f.g; a1.above = w.dx1a; a1.dh = nullptr; a1.dd = w.dd; a1.dx = w.dx1; a1.mgate = out.mgate1; a1.wgate = out.wgate1;
    hipLaunchKernelGGL(pc_sa_bwd_kernel<1>, dim3(PC_NP1 / 2, B), block, (size_t)PcSa1BwdLds::BYTES, s, a1);
    hipLaunchKernelGGL(pc_point_gather_kernel, dim3((stride + PC_PG_THREADS - 1) / PC_PG_THREADS, B), dim3(PC_PG_THREADS), 0, s, knn1, fps1, (const float*)w.dd,
                       (const float*)w.dx1, n_points, stride, w.gpre, w.ds1);
    density(0, pc, stride, n_points, w.ds1, PC_MAX_POINTS, out.dgate1, stride, w.gpre, PC_MAX_POINTS, grad, stride, 3, 1);
    return hipGetLastError();
}

}  // namespace ifd
