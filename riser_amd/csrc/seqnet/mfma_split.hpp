// MFMA operand vectors and the bf16 SPLIT of fp32 operands (hi = bf16(v), lo = bf16(v - hi); a product is hi*hi + lo*hi + hi*lo
// on three v_mfma_f32_16x16x32_bf16 with fp32 accumulate): shared by the split-precision kernels of seqnet.hip and tcn_x3.hip.
// The f16 twins (split2_f16 / mfma_f16 / mfma_x3_f16 on v_mfma_f32_16x16x32_f16) serve crnn/x3.hpp, whose split operands are
// bounded (hidden states) or scaled by the packer (weights): f16's range of 65504 is the caller's business.
#pragma once
#include "../common.hpp"

namespace rs {
namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
// eight floats -> their bf16 hi parts and the bf16 roundings of the residuals
__device__ __forceinline__ void split8(const f32x4& a, const f32x4& b, u32x4& hi, u32x4& lo) {
    hi[0] = pack_bf16x2(a[0], a[1]);
    hi[1] = pack_bf16x2(a[2], a[3]);
    hi[2] = pack_bf16x2(b[0], b[1]);
    hi[3] = pack_bf16x2(b[2], b[3]);
    auto lo_of = [](unsigned h, float e0, float e1) {
        return pack_bf16x2(e0 - __builtin_bit_cast(float, h << 16), e1 - __builtin_bit_cast(float, h & 0xffff0000u));
    };
    lo[0] = lo_of(hi[0], a[0], a[1]);
    lo[1] = lo_of(hi[1], a[2], a[3]);
    lo[2] = lo_of(hi[2], b[0], b[1]);
    lo[3] = lo_of(hi[3], b[2], b[3]);
}
__device__ __forceinline__ f32x4 mfma_x3(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl, f32x4 c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ah), __builtin_bit_cast(bf16x8_t, bh), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, al), __builtin_bit_cast(bf16x8_t, bh), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, ah), __builtin_bit_cast(bf16x8_t, bl), c, 0, 0, 0);
}

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

// two fp32 -> their f16 hi parts and the f16 roundings of the residuals
__device__ __forceinline__ void split2_f16(float a, float b, unsigned& hi, unsigned& lo) {
    const _Float16 ha = (_Float16)a, hb = (_Float16)b;
    const f16x2_t h = {ha, hb};
    const f16x2_t l = {(_Float16)(a - (float)ha), (_Float16)(b - (float)hb)};
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
__device__ __forceinline__ f32x4 mfma_f16(const u32x4& a, const u32x4& b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_x3_f16(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl, f32x4 c) {
    c = mfma_f16(ah, bh, c);
    c = mfma_f16(al, bh, c);
    return mfma_f16(ah, bl, c);
}
}  // namespace
}  // namespace rs
