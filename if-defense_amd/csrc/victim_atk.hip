// The one device-side check of the attack loops on a victim that samples (include/ifd_victim_atk.h): counts and starts of a call
// whose clouds may SHRINK before the last network pass.
//
//   victim_sample_check_kernel   pn2_check_kernel / pc_check_kernel with the count's lower end and the shrink as arguments.
//
// One start table serves every round of a Drop attack and its final forward while the counts fall by `shrink` rows: a start of
// the first sampling has to name a row of the cloud that is written, [0, n - shrink).  With lo the victim's minimum and shrink 0
// this is the victims' own check, counter for counter.
#include "ifd_device.h"
#include "ifd_internal.h"

namespace ifd {

namespace {

__global__ __launch_bounds__(256) void victim_sample_check_kernel(const int32_t* __restrict__ n_points, const int32_t* __restrict__ fps_start,
                                                                  int B, int lo, int hi, int shrink, int np1, int32_t* __restrict__ bad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int n = hi;
    if (n_points) {
        n = n_points[b];
        if (n < lo || n > hi) { atomicAdd(bad, 1); return; }
    }
    if (fps_start) {
        const int s1 = fps_start[2 * b], s2 = fps_start[2 * b + 1];
        if (s1 < 0 || s1 >= n - shrink || s2 < 0 || s2 >= np1) atomicAdd(bad + 1, 1);
    }
}

}  // namespace

hipError_t launch_victim_sample_check(const int32_t* n_points, const int32_t* fps_start, int B, int lo, int hi, int shrink, int np1,
                                      int32_t* bad, hipStream_t s) {
    hipError_t e = hipMemsetAsync(bad, 0, 2 * sizeof(int32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(victim_sample_check_kernel, dim3((B + 255) / 256), dim3(256), 0, s, n_points, fps_start, B, lo, hi, shrink, np1, bad);
    return hipGetLastError();
}

}  // namespace ifd
