// pais_host.hpp -- host-side owners of device and pinned host memory for the C ABI sources (pais_capi.hip,
// pais_pyramid.hip, pais_seed.hip).  No device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

// An allocation and its capacity in bytes.  Reads as the typed pointer wherever one is expected; not copyable.
// The destructor frees: the owner must die with its device current and its work finished (hipFree / hipHostFree
// need neither a stream nor the one the memory was used on, so they are sound after that stream is destroyed).
template <typename T, bool Pinned> struct PaisBuf {
    T *p = nullptr;
    size_t bytes = 0;

    PaisBuf() = default;
    PaisBuf(const PaisBuf &) = delete;
    PaisBuf &operator=(const PaisBuf &) = delete;
    ~PaisBuf() { release(); }
    operator T *() const { return p; }

    void release()
    {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        bytes = 0;
    }
    // exactly n bytes in place of whatever was held ({nullptr, 0} behind a failure); the caller knows the old block is idle
    hipError_t alloc(size_t n)
    {
        release();
        void *q = nullptr;
        const hipError_t e = Pinned ? hipHostMalloc(&q, n, hipHostMallocDefault) : hipMalloc(&q, n);
        if (e != hipSuccess) return e;
        p = (T *)q;
        bytes = n;
        return hipSuccess;
    }
    // Room for needBytes: nothing when they fit; else the stream is synchronised, the block freed and one half larger
    // allocated (contents are not kept; buffers only grow).  Synchronising `stream` alone suffices for a context's
    // buffers although its sub-streams use them too: a sub-stream only ever works between a fork from and a join back to
    // the context's stream, so whatever touches the old block is ordered before the end of that stream.
    hipError_t reserve(hipStream_t stream, size_t needBytes)
    {
        if (needBytes <= bytes) return hipSuccess;
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        return alloc(needBytes + needBytes / 2 + 4096);
    }
};
template <typename T> using DevBuf = PaisBuf<T, false>;
template <typename T> using PinBuf = PaisBuf<T, true>;
