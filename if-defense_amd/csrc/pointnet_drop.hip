// The saliency point-dropping attack on the PointNet victim (include/ifd_drop.h; the reference's baselines/attack/Saliency/Drop.py)
// behind ifd_cls_input_grad's forward / backward pass (pointnet_grad.hip).
//
//   drop_step_kernel    one workgroup of 256 threads a cloud, the cloud (12 bytes a point), its saliencies, ranks and the caller's
//                       index rows in LDS (DropLds, lds_layout.h: 49 KB whatever n is).  Thread t owns the points t, t + 256, ...
//                       1. The centre: per coordinate the element of rank (n - 1) / 2, found by counting the points in front of
//                          each owned point in the order (value ascending, row ascending) - ONE pass over the cloud serves the
//                          three coordinates of all owned points (each LDS read is a broadcast).
//                       2. The saliency of every owned point, in the header's order of operations.
//                       3. Its rank in the drop order (saliency descending, row ascending), by counting again.
//                       4. dropped = rank < k.  Thread t then takes the rows 8 t .. 8 t + 7: a prefix count of the survivors over
//                          the workgroup gives every survivor its new row, so the survivors keep their order for any k.
//                       Every load from global memory ends before the first barrier; the in-place stores come behind the last.
//                       Work per cloud and round: 4 n^2 compares (4.2 M at 1024 points) - VALU-bound; global traffic is the cloud
//                       and its gradient once in, the cloud once out.
//   drop_begin_kernel   the counts and the identity index a whole attack starts from.
#include "atk_device.h"
#include "lds_layout.h"

namespace ifd {

namespace {

constexpr int DROP_PPT = DROP_MAX_POINTS / DROP_THREADS;     // points a thread owns at the most

// the header's SALIENCY, term by term
__device__ __forceinline__ float drop_saliency(float x, float y, float z, float cx, float cy, float cz, float gx, float gy, float gz,
                                               float alpha) {
#pragma clang fp contract(off)
    const float dx = x - cx, dy = y - cy, dz = z - cz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    const float xy = xx + yy;
    const float r = sqrtf(xy + zz);
    const float px = dx * gx, py = dy * gy, pz = dz * gz;
    const float pxy = px + py;
    const float dot = pxy + pz;
    const float ra = alpha == 1.f ? r : powf(r, alpha);
    return -(ra * dot);
}

__global__ __launch_bounds__(DROP_THREADS) void drop_step_kernel(const float* __restrict__ grad, float* __restrict__ pc,
                                                                 int32_t* __restrict__ n_points, int32_t* __restrict__ index, int stride,
                                                                 int k, float alpha, DropOut D) {
    extern __shared__ float lds_f[];
    float* sX = LDS_AT(float, lds_f, DropLds::X);
    float* sS = LDS_AT(float, lds_f, DropLds::S);
    int* sR = LDS_AT(int, lds_f, DropLds::RANK);
    int* sI = LDS_AT(int, lds_f, DropLds::INDEX);
    int* sScan = LDS_AT(int, lds_f, DropLds::SCAN);
    float* sC = LDS_AT(float, lds_f, DropLds::CENTER);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = n_points[b];
    if (n <= k || n > DROP_MAX_POINTS || n > stride) return;    // the header: left untouched (block-uniform)
    const size_t off = (size_t)b * stride * 3, ioff = (size_t)b * stride;
    for (int i = tid; i < n * 3; i += DROP_THREADS) sX[i] = pc[off + i];
    if (index)
        for (int i = tid; i < n; i += DROP_THREADS) sI[i] = index[ioff + i];
    float gx[DROP_PPT], gy[DROP_PPT], gz[DROP_PPT];
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) {
        const int i = r * DROP_THREADS + tid;
        const bool in = i < n;
        gx[r] = in ? grad[off + 3 * i] : 0.f;
        gy[r] = in ? grad[off + 3 * i + 1] : 0.f;
        gz[r] = in ? grad[off + 3 * i + 2] : 0.f;
    }
    __syncthreads();

    // ---- 1. the centre: the lower median of every coordinate ----
    float x[DROP_PPT], y[DROP_PPT], z[DROP_PPT];
    int rx[DROP_PPT], ry[DROP_PPT], rz[DROP_PPT];
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) {
        const int i = min(r * DROP_THREADS + tid, n - 1);       // a slot beyond n repeats the last point; never used
        x[r] = sX[3 * i]; y[r] = sX[3 * i + 1]; z[r] = sX[3 * i + 2];
        rx[r] = ry[r] = rz[r] = 0;
    }
    for (int j = 0; j < n; ++j) {
        const float xj = sX[3 * j], yj = sX[3 * j + 1], zj = sX[3 * j + 2];      // broadcast reads
#pragma unroll
        for (int r = 0; r < DROP_PPT; ++r) {
            const bool before = j < r * DROP_THREADS + tid;
            rx[r] += (xj < x[r] || (xj == x[r] && before)) ? 1 : 0;
            ry[r] += (yj < y[r] || (yj == y[r] && before)) ? 1 : 0;
            rz[r] += (zj < z[r] || (zj == z[r] && before)) ? 1 : 0;
        }
    }
    const int mid = (n - 1) / 2;
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) {
        if (r * DROP_THREADS + tid >= n) continue;
        if (rx[r] == mid) sC[0] = x[r];
        if (ry[r] == mid) sC[1] = y[r];
        if (rz[r] == mid) sC[2] = z[r];
    }
    __syncthreads();
    const float cx = sC[0], cy = sC[1], cz = sC[2];
    if (D.center && tid < 3) D.center[(size_t)b * 3 + tid] = sC[tid];

    // ---- 2. the saliencies ----
    float s[DROP_PPT];
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) {
        const int i = r * DROP_THREADS + tid;
        s[r] = drop_saliency(x[r], y[r], z[r], cx, cy, cz, gx[r], gy[r], gz[r], alpha);
        if (i < n) {
            sS[i] = s[r];
            if (D.saliency) D.saliency[ioff + i] = s[r];
        }
    }
    __syncthreads();

    // ---- 3. the rank of every owned point in the drop order ----
    int rank[DROP_PPT];
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) rank[r] = 0;
    for (int j = 0; j < n; ++j) {
        const float sj = sS[j];                                 // broadcast read
#pragma unroll
        for (int r = 0; r < DROP_PPT; ++r) rank[r] += (sj > s[r] || (sj == s[r] && j < r * DROP_THREADS + tid)) ? 1 : 0;
    }
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) {
        const int i = r * DROP_THREADS + tid;
        if (i >= n) continue;
        sR[i] = rank[r];
        if (D.dropped && rank[r] < k) D.dropped[(size_t)b * k + rank[r]] = i;
    }
    __syncthreads();

    // ---- 4. stable compaction: thread t takes the rows DROP_PPT t .. DROP_PPT t + DROP_PPT - 1 ----
    const int first = tid * DROP_PPT;
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) cnt += (first + r < n && sR[first + r] >= k) ? 1 : 0;
    sScan[tid] = cnt;
    __syncthreads();
    for (int w = 1; w < DROP_THREADS; w <<= 1) {
        const int v = tid >= w ? sScan[tid - w] : 0;
        __syncthreads();
        sScan[tid] += v;
        __syncthreads();
    }
    int dst = sScan[tid] - cnt;                                 // survivors in front of my rows
#pragma unroll
    for (int r = 0; r < DROP_PPT; ++r) {
        const int i = first + r;
        if (i >= n || sR[i] < k) continue;
        pc[off + 3 * dst] = sX[3 * i];
        pc[off + 3 * dst + 1] = sX[3 * i + 1];
        pc[off + 3 * dst + 2] = sX[3 * i + 2];
        if (index) index[ioff + dst] = sI[i];
        ++dst;
    }
    for (int i = n - k + tid; i < n; i += DROP_THREADS) {       // the rows the cloud lost (a NaN saliency may leave more: outside the contract)
        pc[off + 3 * i] = 0.f;
        pc[off + 3 * i + 1] = 0.f;
        pc[off + 3 * i + 2] = 0.f;
        if (index) index[ioff + i] = -1;
    }
    if (tid == 0) n_points[b] = n - k;
}

__global__ __launch_bounds__(256) void drop_begin_kernel(const int32_t* __restrict__ n_points, int stride, int32_t* __restrict__ n_out,
                                                         int32_t* __restrict__ kept) {
    const int b = blockIdx.x, n = n_points ? n_points[b] : stride;
    if (kept)
        for (int i = threadIdx.x; i < stride; i += 256) kept[(size_t)b * stride + i] = i < n ? i : -1;
    if (threadIdx.x == 0) n_out[b] = n;
}

}  // namespace

hipError_t launch_drop_step(const float* grad, float* pc, int32_t* n_points, int32_t* index, int B, int stride, int k, float alpha,
                            const DropOut& D, hipStream_t s) {
    hipLaunchKernelGGL(drop_step_kernel, dim3(B), dim3(DROP_THREADS), DropLds::BYTES, s, grad, pc, n_points, index, stride, k, alpha, D);
    return hipGetLastError();
}

hipError_t launch_drop_begin(const int32_t* n_points, int B, int stride, int32_t* n_out, int32_t* kept, hipStream_t s) {
    hipLaunchKernelGGL(drop_begin_kernel, dim3(B), dim3(256), 0, s, n_points, stride, n_out, kept);
    return hipGetLastError();
}

}  // namespace ifd
