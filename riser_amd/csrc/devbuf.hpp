// Device buffers that are freed with their holder, and the upload of a host vector into one (ConvNet models and the
// sequential conv programs).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace rs {
namespace {
// a device allocation that is freed with its holder (move-only)
template <class T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    operator T*() const { return p; }
};

// one pinned host word a kernel can store into, freed with its holder (move-only)
struct PinnedWord {
    unsigned* p = nullptr;
    PinnedWord() = default;
    PinnedWord(PinnedWord&& o) noexcept : p(o.p) { o.p = nullptr; }
    PinnedWord& operator=(PinnedWord&& o) noexcept {
        std::swap(p, o.p);
        return *this;
    }
    ~PinnedWord() {
        if (p) (void)hipHostFree(p);
    }
    hipError_t alloc() {
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(unsigned), hipHostMallocDefault);
        if (e == hipSuccess) *p = 0u;
        return e;
    }
    operator unsigned*() const { return p; }
};

// (at least 16 bytes: the kernels copy weights in 16-byte pieces, and an empty vector still gets an allocation)
template <class T>
hipError_t upload(DevBuf<T>& d, const std::vector<T>& h) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d.p), std::max<size_t>(h.size() * sizeof(T), 16));
    if (e == hipSuccess) e = hipMemcpy(d.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}
}  // namespace
}  // namespace rs
