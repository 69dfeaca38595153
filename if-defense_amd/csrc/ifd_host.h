// Host-only helpers of api.cpp: the owners of a context's HIP resources.  (The cursor that lays a workspace out, Carve, is in
// lds_layout.h, where the .hip launchers reach it too.)  No kernel translation unit includes this file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#include "lds_layout.h"

namespace ifd {

// A block of device or pinned host memory (DeviceBuffer, PinnedBuffer) that is released with its owner.
template <bool Pinned>
class Buffer {
    void* p_ = nullptr;
    size_t n_ = 0;
    static hipError_t mem_alloc(void** p, size_t n) { return Pinned ? hipHostMalloc(p, n, hipHostMallocDefault) : hipMalloc(p, n); }
    static hipError_t mem_free(void* p) { return Pinned ? hipHostFree(p) : hipFree(p); }

public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
    ~Buffer() { if (p_) (void)mem_free(p_); }

    size_t bytes() const { return n_; }
    template <class T = void>
    T* get() const { return static_cast<T*>(p_); }

    hipError_t alloc(size_t bytes) {
        *this = Buffer();                              // the old block goes first
        const hipError_t e = mem_alloc(&p_, bytes);
        if (e == hipSuccess) n_ = bytes; else p_ = nullptr;
        return e;
    }
    // allocate and fill from host memory; the copy blocks
    hipError_t upload(const void* host, size_t bytes) {
        const hipError_t e = alloc(bytes);
        return e == hipSuccess ? hipMemcpy(p_, host, bytes, hipMemcpyHostToDevice) : e;
    }
    // Make room for `bytes`, contents not kept.  Nothing happens when the block is large enough, which is every call in steady
    // state.  Otherwise the device is synchronised first (work enqueued earlier may still use the old block); if that fails
    // the error is returned and the old block stays as it is.
    hipError_t grow(size_t bytes) {
        if (bytes <= n_) return hipSuccess;
        if (p_) {
            const hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return e;
        }
        return alloc(bytes);
    }
};
using DeviceBuffer = Buffer<false>;
using PinnedBuffer = Buffer<true>;

// A HIP handle that is created on first use and destroyed with its owner.
template <class H, hipError_t (*Create)(H*), hipError_t (*Destroy)(H)>
class Lazy {
    H h_ = nullptr;

public:
    Lazy() = default;
    Lazy(Lazy&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Lazy& operator=(Lazy&& o) noexcept { std::swap(h_, o.h_); return *this; }
    ~Lazy() { if (h_) (void)Destroy(h_); }
    hipError_t ensure() { return h_ ? hipSuccess : Create(&h_); }
    H get() const { return h_; }
};
inline hipError_t create_event(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
inline hipError_t create_stream(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
using Event = Lazy<hipEvent_t, create_event, hipEventDestroy>;          // without timing
using Stream = Lazy<hipStream_t, create_stream, hipStreamDestroy>;      // non-blocking

}  // namespace ifd
