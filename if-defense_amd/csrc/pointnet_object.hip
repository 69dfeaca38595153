// The CW object-adding attack on the PointNet victim (include/ifd_object.h; the reference's baselines/attack/CW/Add_Objects.py with
// L2ChamferDist(num_add, 'adv2ori', 0.2)) behind ifd_cls_input_grad's forward / backward pass (pointnet_grad.hip).  The begin and the
// end of the whole attack are pointnet_add.hip's add_begin / add_finish kernels.
//
//   object_place_kernel   world = rotate_shift(obj, angle, shift) into the added rows of the concatenated cloud: object_place(), the
//                         ONE function every kernel here places and rotates with.
//   object_step_kernel    one workgroup of 256 threads a cloud, the originals and the forwarded world rows in LDS (ObjectStepLds,
//                         61 KB).  Thread t owns the added rows t, t + 256, ...  The Chamfer part is add_step_kernel's, restated; the L2
//                         part is cw_step_kernel's strided sum and tree on obj - objects.  Every owned row then leaves its world-row
//                         gradient and its angle term in LDS ([A][4]), takes Adam on its object row and keeps the new row in
//                         registers; thread 4 c + k sums component k of object c over the object's rows in ascending order in
//                         float64, rounds once and takes Adam on that shift coordinate (k < 3) or on the angle (k == 3, then the
//                         remainder and the new cos / sin); behind a barrier every row is placed again into `cat`.
//                         Work per cloud: A * n_ori distances as Add's, + 4 A LDS reads for the per-object sums.
//   object_start_kernel   the start of a search step: obj, shift, angle from the caller's arrays, the pose moments zeroed, placed.
#include "atk_device.h"
#include "lds_layout.h"

namespace ifd {

namespace {

constexpr int OBJ_PPT = ADD_MAX_ADD / OBJECT_THREADS;       // added rows a thread owns at the most
constexpr float OBJ_TWO_PI = (float)(2.0 * 3.141592653589793);          // the Python scalar 2. * np.pi as torch hands it to a float kernel

// the header's rotation: r = (x, y, z) about the y axis, y unchanged
__device__ __forceinline__ void object_rotate(float x, float z, float c, float s, float& rx, float& rz) {
#pragma clang fp contract(off)
    const float zs = z * s, zc = z * c;
    rx = __builtin_fmaf(x, c, -zs);
    rz = __builtin_fmaf(x, s, zc);
}

// THE PLACEMENT of the header
__device__ __forceinline__ void object_place(float x, float y, float z, float c, float s, float sx, float sy, float sz, float& wx,
                                             float& wy, float& wz) {
#pragma clang fp contract(off)
    float rx, rz;
    object_rotate(x, z, c, s, rx, rz);
    wx = rx + sx;
    wy = y + sy;
    wz = rz + sz;
}

// torch.remainder(a, (float)(2 pi)) in float32
__device__ __forceinline__ float object_wrap(float a) {
    float r = fmodf(a, OBJ_TWO_PI);
    if (r != 0.f && r < 0.f) r += OBJ_TWO_PI;
    return r;
}

// the header's dist and info[1], term by term
__device__ __forceinline__ float object_dist(float l2, float cd) {
#pragma clang fp contract(off)
    const float c = cd * 0.2f;
    return l2 + c;
}
__device__ __forceinline__ float object_dist_loss(float l2, float cd, float w) {
#pragma clang fp contract(off)
    const float f = l2 * w, c = cd * w;
    const float c1 = c * 0.2f;
    return f + c1;
}

// the cloud's original rows, or -1 where the cloud is outside the header's limits (block-uniform)
__device__ __forceinline__ int object_rows(const int32_t* n_ori, int b, int cat_stride, int A) {
    const int n = n_ori ? n_ori[b] : cat_stride - A;
    return (n < 1 || n > ADD_MAX_ORI || n > cat_stride - A) ? -1 : n;
}

__global__ __launch_bounds__(OBJECT_THREADS) void object_place_kernel(const float* __restrict__ obj, const float* __restrict__ angle,
                                                                      const float* __restrict__ shift, float* __restrict__ cat,
                                                                      const int32_t* __restrict__ n_ori, int cat_stride, int num_add, int P) {
    const int b = blockIdx.x, A = num_add * P;
    const int n = object_rows(n_ori, b, cat_stride, A);
    if (n < 0) return;                                          // the header: left untouched
    const float* X = obj + (size_t)b * A * 3;
    float* Wd = cat + ((size_t)b * cat_stride + n) * 3;
    for (int p = threadIdx.x; p < A; p += OBJECT_THREADS) {
        const size_t oc = (size_t)b * num_add + p / P;
        float s, c, wx, wy, wz;
        sincosf(angle[oc], &s, &c);
        object_place(X[3 * p], X[3 * p + 1], X[3 * p + 2], c, s, shift[3 * oc], shift[3 * oc + 1], shift[3 * oc + 2], wx, wy, wz);
        Wd[3 * p] = wx; Wd[3 * p + 1] = wy; Wd[3 * p + 2] = wz;
    }
}

// step_size, bc2, omb1, omb2: adam_step_consts (ifd_internal.h)
__global__ __launch_bounds__(OBJECT_THREADS) void object_step_kernel(ObjectState S, const float* __restrict__ objects,
                                                                     const float* __restrict__ grad, const int32_t* __restrict__ pred,
                                                                     const float* __restrict__ loss, const int32_t* __restrict__ target,
                                                                     float* __restrict__ cat, const int32_t* __restrict__ n_ori,
                                                                     float* __restrict__ last_input, float* __restrict__ info, ObjectDiag D,
                                                                     float step_size, float bc2, float omb1, float omb2, float scale,
                                                                     int cat_stride, int num_add, int P) {
    extern __shared__ float lds_f[];
    float* sO = LDS_AT(float, lds_f, ObjectStepLds::O);
    float* sW = LDS_AT(float, lds_f, ObjectStepLds::W);
    float* sG = LDS_AT(float, lds_f, ObjectStepLds::G);
    float* sCS = LDS_AT(float, lds_f, ObjectStepLds::CS);
    float* sh = LDS_AT(float, lds_f, ObjectStepLds::SH);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int A = num_add * P;
    const int n = object_rows(n_ori, b, cat_stride, A);
    if (n < 0) return;                                          // the header: left untouched (block-uniform)
    const size_t coff = (size_t)b * cat_stride * 3, aoff = (size_t)b * A * 3, poff = (size_t)b * num_add;
    float* X = cat + coff + (size_t)n * 3;                      // the added (world) rows
    float* OBJ = S.obj + aoff;
    for (int i = tid; i < n * 3; i += OBJECT_THREADS) sO[i] = cat[coff + i];
    for (int i = tid; i < A * 3; i += OBJECT_THREADS) sW[i] = X[i];
    for (int c = tid; c < num_add; c += OBJECT_THREADS) sincosf(S.angle[poff + c], &sCS[2 * c + 1], &sCS[2 * c]);
    __syncthreads();

    // ---- 1. the nearest original of every owned world row, one pass over the originals (add_step_kernel's) ----
    float ax[OBJ_PPT], ay[OBJ_PPT], az[OBJ_PPT], best[OBJ_PPT];
    int bi[OBJ_PPT];
#pragma unroll
    for (int r = 0; r < OBJ_PPT; ++r) {
        const int p = min(r * OBJECT_THREADS + tid, A - 1);     // a slot beyond A repeats the last row; never used
        ax[r] = sW[3 * p]; ay[r] = sW[3 * p + 1]; az[r] = sW[3 * p + 2];
        best[r] = INFINITY;
        bi[r] = 0;
    }
#pragma unroll 2
    for (int j = 0; j < n; ++j) {
        const float ox = sO[3 * j], oy = sO[3 * j + 1], oz = sO[3 * j + 2];
#pragma unroll
        for (int r = 0; r < OBJ_PPT; ++r) {
            const float dx = ax[r] - ox, dy = ay[r] - oy, dz = az[r] - oz;
            const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (d < best[r]) { best[r] = d; bi[r] = j; }        // strict: the lowest index among equal distances
        }
    }
    float part = 0.f;
#pragma unroll
    for (int r = 0; r < OBJ_PPT; ++r) part += (r * OBJECT_THREADS + tid < A) ? best[r] : 0.f;
    const float cd = atk_block_sum(part, sh) / (float)A;

    // ---- 2, 3. the L2 part (cw_step_kernel's sum) and the distance ----
    float a2 = 0.f;
    for (int i = tid; i < A * 3; i += OBJECT_THREADS) { const float d = OBJ[i] - objects[i]; a2 = fmaf(d, d, a2); }
    const float l2 = sqrtf(atk_block_sum(a2, sh));
    const float dist = object_dist(l2, cd);

    // ---- 4. the records: every thread reads the old values, thread 0 writes the new ones behind a barrier ----
    const CwState& R = S.cw;
    const bool hit = pred[b] == target[b];
    const bool rec = hit && dist < R.bestdist[b], orec = hit && dist < R.o_bestdist[b];
    const float w = (float)R.weight[b];
    __syncthreads();
    if (tid == 0) {
        if (rec) { R.bestdist[b] = dist; R.bestscore[b] = pred[b]; }
        if (orec) { R.o_bestdist[b] = dist; R.o_bestscore[b] = pred[b]; }
        if (info) {
            info[(size_t)b * 3] = loss ? loss[b] : 0.f;
            info[(size_t)b * 3 + 1] = object_dist_loss(l2, cd, w);
            info[(size_t)b * 3 + 2] = dist;
        }
        if (D.l2) D.l2[b] = l2;
        if (D.cd) D.cd[b] = cd;
    }

    // ---- 5, 6. per owned row: the world-row gradient and the angle term into LDS, Adam on the object row ----
    const float c_w = scale * w;
    const float c_cd = (c_w * 0.2f) * (2.f / (float)A);
    const float c_l2 = l2 > 0.f ? c_w / l2 : 0.f;               // l2 == 0: no L2 term (the header's deviation)
    const float* G = grad + coff + (size_t)n * 3;
    float* M = R.m + aoff;
    float* V = R.v + aoff;
    float* OB = R.o_bestattack + aoff;
    float* LI = last_input ? last_input + aoff : nullptr;
    float nx[OBJ_PPT][3];
#pragma unroll
    for (int r = 0; r < OBJ_PPT; ++r) {
        const int p = r * OBJECT_THREADS + tid;
        if (p >= A) continue;
        const float c = sCS[2 * (p / P)], s = sCS[2 * (p / P) + 1];
        if (D.nn_ori) D.nn_ori[(size_t)b * A + p] = bi[r];
        float x[3], gw[3], go[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * p + k;
            const float wv = sW[i];
            if (orec) OB[i] = wv;
            if (LI) LI[i] = wv;
            x[k] = OBJ[i];
            gw[k] = __builtin_fmaf(c_cd, wv - sO[3 * bi[r] + k], G[i]);
        }
        float rx, rz;
        object_rotate(x[0], x[2], c, s, rx, rz);
        {
#pragma clang fp contract(off)
            const float t0 = gw[2] * s, t1 = gw[0] * s, t2 = gw[0] * rz;
            go[0] = __builtin_fmaf(gw[0], c, t0);
            go[1] = gw[1];
            go[2] = __builtin_fmaf(gw[2], c, -t1);
            sG[4 * p + 3] = __builtin_fmaf(gw[2], rx, -t2);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = 3 * p + k;
            sG[4 * p + k] = gw[k];
            const float g = __builtin_fmaf(c_l2, x[k] - objects[i], go[k]);
            if (D.obj_grad) D.obj_grad[aoff + i] = g;
            float mr = M[i], vr = V[i];
            nx[r][k] = atk_adam(x[k], g, mr, vr, step_size, bc2, omb1, omb2);
            OBJ[i] = nx[r][k];
            M[i] = mr;
            V[i] = vr;
        }
    }
    __syncthreads();                                            // sG is complete; sW and sCS are no longer read

    // ---- 5 - 7. per object: the sums in ascending p in float64, Adam on the shift and the angle, the remainder ----
    for (int q = tid; q < 4 * num_add; q += OBJECT_THREADS) {
        const int c = q >> 2, k = q & 3;
        double acc = 0.0;
        for (int p = c * P; p < (c + 1) * P; ++p) acc += (double)sG[4 * p + k];
        const float g = (float)acc;
        if (k < 3) {
            const size_t i = (poff + c) * 3 + k;
            if (D.g_shift) D.g_shift[i] = g;
            float mr = S.shift_m[i], vr = S.shift_v[i];
            const float v = atk_adam(S.shift[i], g, mr, vr, step_size, bc2, omb1, omb2);
            S.shift[i] = v;
            S.shift_m[i] = mr;
            S.shift_v[i] = vr;
            sW[3 * c + k] = v;
        } else {
            const size_t i = poff + c;
            if (D.g_angle) D.g_angle[i] = g;
            float mr = S.angle_m[i], vr = S.angle_v[i];
            const float v = object_wrap(atk_adam(S.angle[i], g, mr, vr, step_size, bc2, omb1, omb2));
            S.angle[i] = v;
            S.angle_m[i] = mr;
            S.angle_v[i] = vr;
            sincosf(v, &sCS[2 * c + 1], &sCS[2 * c]);
        }
    }
    __syncthreads();

    // ---- 8. the new world rows ----
#pragma unroll
    for (int r = 0; r < OBJ_PPT; ++r) {
        const int p = r * OBJECT_THREADS + tid;
        if (p >= A) continue;
        const int c = p / P;
        float wx, wy, wz;
        object_place(nx[r][0], nx[r][1], nx[r][2], sCS[2 * c], sCS[2 * c + 1], sW[3 * c], sW[3 * c + 1], sW[3 * c + 2], wx, wy, wz);
        X[3 * p] = wx; X[3 * p + 1] = wy; X[3 * p + 2] = wz;
    }
}

__global__ __launch_bounds__(OBJECT_THREADS) void object_start_kernel(ObjectState S, const float* __restrict__ objects,
                                                                      const float* __restrict__ centers, const float* __restrict__ noise_obj,
                                                                      const float* __restrict__ noise_shift, const float* __restrict__ angles0,
                                                                      const int32_t* __restrict__ n_cat, int out_stride, int num_add, int P,
                                                                      float* __restrict__ pc_out) {
    const int b = blockIdx.x, tid = threadIdx.x, A = num_add * P;
    const size_t aoff = (size_t)b * A * 3, poff = (size_t)b * num_add;
    float* Wd = pc_out + ((size_t)b * out_stride + (n_cat[b] - A)) * 3;
    for (int i = tid; i < num_add * 3; i += OBJECT_THREADS) {
        const size_t j = poff * 3 + i;
        S.shift[j] = noise_shift ? centers[j] + noise_shift[j] : centers[j];
        S.shift_m[j] = 0.f;
        S.shift_v[j] = 0.f;
    }
    for (int c = tid; c < num_add; c += OBJECT_THREADS) {
        S.angle[poff + c] = angles0[poff + c];
        S.angle_m[poff + c] = 0.f;
        S.angle_v[poff + c] = 0.f;
    }
    for (int p = tid; p < A; p += OBJECT_THREADS) {
        const size_t oc = poff + p / P;
        float x[3], sft[3], s, c, wx, wy, wz;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t i = aoff + 3 * p + k;
            x[k] = noise_obj ? objects[3 * p + k] + noise_obj[i] : objects[3 * p + k];
            S.obj[i] = x[k];
            sft[k] = noise_shift ? centers[3 * oc + k] + noise_shift[3 * oc + k] : centers[3 * oc + k];
        }
        sincosf(angles0[oc], &s, &c);
        object_place(x[0], x[1], x[2], c, s, sft[0], sft[1], sft[2], wx, wy, wz);
        Wd[3 * p] = wx; Wd[3 * p + 1] = wy; Wd[3 * p + 2] = wz;
    }
}

}  // namespace

hipError_t launch_object_place(const float* obj, const float* angle, const float* shift, float* cat, const int32_t* n_ori, int B,
                               int cat_stride, int num_add, int obj_num_p, hipStream_t s) {
    hipLaunchKernelGGL(object_place_kernel, dim3(B), dim3(OBJECT_THREADS), 0, s, obj, angle, shift, cat, n_ori, cat_stride, num_add,
                       obj_num_p);
    return hipGetLastError();
}

hipError_t launch_object_step(const ObjectState& S, const float* objects, const float* grad, const int32_t* pred, const float* loss,
                              const int32_t* target, float* cat, const int32_t* n_ori, float* last_input, float* info,
                              const ObjectDiag& D, int t, float lr, float scale, int B, int cat_stride, int num_add, int obj_num_p,
                              hipStream_t s) {
    const AdamStep a = adam_step_consts(t, lr);
    hipLaunchKernelGGL(object_step_kernel, dim3(B), dim3(OBJECT_THREADS), ObjectStepLds::BYTES, s, S, objects, grad, pred, loss, target,
                       cat, n_ori, last_input, info, D, a.step_size, a.bc2, a.omb1, a.omb2, scale, cat_stride, num_add, obj_num_p);
    return hipGetLastError();
}

hipError_t launch_object_start(const ObjectState& S, const float* objects, const float* centers, const float* noise_obj,
                               const float* noise_shift, const float* angles0, const int32_t* n_cat, int B, int out_stride, int num_add,
                               int obj_num_p, float* pc_out, hipStream_t s) {
    hipLaunchKernelGGL(object_start_kernel, dim3(B), dim3(OBJECT_THREADS), 0, s, S, objects, centers, noise_obj, noise_shift, angles0, n_cat,
                       out_stride, num_add, obj_num_p, pc_out);
    return hipGetLastError();
}

}  // namespace ifd
