// Device-side primitives of the ConvNet's 16-bit conv kernels (conv_ring_h16.hip, conv_ring_f8.hip, conv_wres_h16.hip,
// conv_thin_h16.hip, conv_stream_h16.hip): the 16-bit vector types (f32x4, u32x4, kOob and static_for are device_prelude.hpp's), the 16-bit MFMA, the 16-bit <-> fp32 conversions of plain and split
// precision, the LDS-DMA piece, and the epilogue step the tiled kernels share.  Device-only, everything
// force-inlined into an anonymous namespace: a kernel's code is what it was with the definitions in its own file.
#pragma once
#include "device_prelude.hpp"

namespace rs {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

template <bool F16>
__device__ __forceinline__ f32x4 mfma16(const u32x4& a, const u32x4& b, const f32x4& c) {
    if constexpr (F16)
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c,
                                                      0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b),
                                                       c, 0, 0, 0);
}

// two fp32 -> one dword of two 16-bit values (lo in bits 0-15), round to nearest even (v_cvt_pk_{f16,bf16}_f32)
template <bool F16>
__device__ __forceinline__ unsigned pack2(float lo, float hi) {
    const f32x2 v = {lo, hi};
    if constexpr (F16)
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2));
    else
        return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
template <bool F16>
__device__ __forceinline__ float widen16(unsigned short u) {
    if constexpr (F16)
        return (float)__builtin_bit_cast(_Float16, u);
    else
        return __builtin_bit_cast(float, (unsigned)u << 16);
}
// split precision: the lo dword of a pair of values whose hi dword (two 16-bit roundings) is `hi`
template <bool F16>
__device__ __forceinline__ unsigned pack2_lo(float a, float b, unsigned hi) {
    return pack2<F16>(a - widen16<F16>((unsigned short)(hi & 0xffffu)), b - widen16<F16>((unsigned short)(hi >> 16)));
}

// value of the lane that holds the neighbouring output column (lane ^ 1)
__device__ __forceinline__ float swap_pair(float x) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), 0xB1 /* quad_perm [1,0,3,2] */,
                                                              0xF, 0xF, true));
}

// physical element index of logical output column c inside a row (X3: 32-channel panels of [hi x 32 | lo x 32])
template <bool X3>
__device__ __forceinline__ int phys_col(int c) {
    return X3 ? ((c >> 5) << 6) + (c & 31) : c;
}

// one LDS-DMA piece: lane l's 16 bytes at rsrc + voff land at LDS byte lds_addr + 16 l (zeros if voff is out of range)
__device__ __forceinline__ void dma_piece(unsigned voff, const __amdgpu_buffer_rsrc_t rsrc, unsigned lds_addr) {
    // the LDS address is wave-uniform by construction; readfirstlane makes that provable to the compiler ("s" operand)
    const unsigned m0v = (unsigned)__builtin_amdgcn_readfirstlane((int)lds_addr);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds"
                 :: "v"(voff), "s"(m0v), "s"(rsrc) : "memory");
#if defined(RS_EMU_DMA_X) && RS_EMU_DMA_X == 2       // measurement build: every staging piece issued twice (2 x the L2 -> LDS bytes)
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %2, 0 offen lds"
                 :: "v"(voff), "s"(m0v), "s"(rsrc) : "memory");
#endif
}

// ---- the tiled kernels' epilogue (conv_ring_h16.hip describes it): per 16-row block a wave parks 8 pooled rows x NT x 16
// channels in a wave-private LDS image laid out like the output row segment and stores the image in 16-byte pieces -----------
template <int NT, bool X3>
struct EpiImage {
    static constexpr int PW = X3 ? 4 : 2;                           // 16-byte pieces per 16-channel group of an output row
    static constexpr int PITCH = NT * PW * 16 + 16;                 // image row pitch: rows 2g of the 4 lane groups on distinct banks
    static constexpr int NPIECE = 8 * NT * PW;                      // pieces of one block's 8 pooled rows
};

// One 16 x 16 accumulator of lane (r, g): MaxPool, + bias, ReLU - max(a, b) + c == max(a + c, b + c) bit for bit (rounding is
// monotonic); the sums are canonical, so the compiler emits one v_max3_f32 instead of two canonicalising v_max + max + max;
// fmaf(x, 1, b) == x + b bit for bit: `us` changes nothing outside f16.  Neighbouring lanes (channels c, c + 1) then exchange
// one value so that the lane owns channels (r & ~1, r | 1) of pooled row 2g + odd, packs them to the hi dword, ORs its overflow
// bits into `sat` BEFORE the row mask `keep` is applied, and returns (hi, lo) & keep (lo: split precision only, else 0): the two
// dwords of the pair's place in the image, lo 64 bytes behind hi.
template <bool F16, bool X3>
__device__ __forceinline__ u32x2 pool_pack_pair(const f32x4& acc, float us, float bias, bool odd, unsigned keep, unsigned& sat) {
    const float v0 = fmaxf(fmaxf(fmaf(acc[0], us, bias), fmaf(acc[1], us, bias)), 0.0f);
    const float v1 = fmaxf(fmaxf(fmaf(acc[2], us, bias), fmaf(acc[3], us, bias)), 0.0f);
    const float got = swap_pair(odd ? v0 : v1);
    const float ca = odd ? got : v0, cb = odd ? v1 : got;
    const unsigned hi = pack2<F16>(ca, cb);
    if constexpr (F16) sat |= f16_overflow_bits(hi);
    return (u32x2){hi & keep, X3 ? keep & pack2_lo<F16>(ca, cb, hi) : 0u};
}

}  // namespace
}  // namespace rs
