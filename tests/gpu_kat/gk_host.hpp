// gk_host.hpp -- host plumbing of the device known-answer library (tests/gpu_kat): a device buffer that frees itself and the
// return convention of every entry point.
//
// An entry point takes HOST pointers, checks that every case lies inside the domain its kernel can address, allocates its own
// device buffers, copies, launches ONCE, synchronises, copies back, frees, and returns
//     0            everything ran,
//     a hipError_t (> 0) a HIP call failed,
//     -(i + 1)     case i lies outside the domain: nothing was launched.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>

struct GkBuf {
    void *p = nullptr;
    ~GkBuf() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
    template <class T>
    T *as() const { return reinterpret_cast<T *>(p); }
};

#define GK_TRY(x)                              \
    do {                                       \
        const hipError_t e_ = (x);             \
        if (e_ != hipSuccess) return (int)e_;  \
    } while (0)

// behind a launch: launch errors first, then the kernel's own
#define GK_RAN()                       \
    do {                               \
        GK_TRY(hipGetLastError());     \
        GK_TRY(hipDeviceSynchronize()); \
    } while (0)
