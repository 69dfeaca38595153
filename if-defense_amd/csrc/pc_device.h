// The small fused layers of the PointConv victim (include/ifd_pc.h), shared by the forward (pointconv.hip) and the backward pass
// (pointconv_grad.hip), which recomputes them with this very instruction sequence so that its gates are the forward's bits.
#pragma once
#include "ifd_device.h"

namespace ifd {

// y[o] = relu(b[o] + sum_c W[o][c] x[c]), one fused chain from the bias over the inputs in ascending order
template <int OUT, int IN>
__device__ __forceinline__ void small_layer(const float* __restrict__ W, const float* __restrict__ bias, const float (&x)[IN], float (&y)[OUT],
                                            int o0 = 0) {
#pragma unroll
    for (int o = 0; o < OUT; ++o) {
        float a = bias[o0 + o];
#pragma unroll
        for (int c = 0; c < IN; ++c) a = fmaf(W[(o0 + o) * IN + c], x[c], a);
        y[o] = fmaxf(a, 0.f);
    }
}

// WeightNet 3 -> 8 -> 8 -> 16 on one difference; wn: {[8][3], [8], [8][8], [8], [16][8], [16]}.  Outputs o0 .. o0 + N - 1.
template <int N>
__device__ __forceinline__ void weight_net(const float* __restrict__ wn, float dx, float dy, float dz, int o0, float (&out)[N]) {
    const float x[3] = {dx, dy, dz};
    float h1[8], h2[8];
    small_layer<8, 3>(wn, wn + 24, x, h1);
    small_layer<8, 8>(wn + 32, wn + 96, h1, h2);
    small_layer<N, 8>(wn + 104, wn + 232, h2, out, o0);
}

}  // namespace ifd
