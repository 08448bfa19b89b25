// What every hand-written conv kernel starts from: the four-lane vector types, the compile-time loop, the out-of-range
// buffer offset and the buffer descriptor.  Device-only, force-inlined, in an anonymous namespace: a kernel's code is what it
// was with the definitions in its own file.
#pragma once
#include "common.hpp"

#include <utility>

namespace rs {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// a buffer offset past every buffer (num_records < 2^31, host-checked): loads return zeros, LDS-DMA writes zeros, stores
// are dropped - rows before the first / after the last row of a buffer, the K padding of the last chunk, idle threads and the
// prefetch behind the last item need no branch and no zero page
constexpr unsigned kOob = 0x80000000u;

// compile-time loop: the body sees its index as a constant expression, so every register-array index in it is static
// whatever hipcc's unroll heuristics decide
template <int... I, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, F&& f) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F&&>(f));
}

// raw buffer descriptor over `bytes` bytes at p (dword 3 = 0x00020000: raw 32-bit offsets, out-of-range checked)
template <class T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const T* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p), 0, bytes, 0x00020000);
}

}  // namespace
}  // namespace rs
