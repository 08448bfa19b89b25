// The order-preserving integer image of a floating-point value: key(a) < key(b) as unsigned integers exactly where a < b as
// floats (-0.0 below +0.0), so that order statistics of floats are found by counting on integer digits
// (signal/radix_select.hpp).  kPasses: 8-bit digits per key.  A NaN has no order: its image lies above key(+inf) or, with the
// sign bit set, below key(-inf), so is_nan tells it from the key alone and the select can answer as np.median does; kNanBinLo
// and kNanBinHi are the first digits of key(-inf) and key(+inf): a NaN's first digit is at most the one, or at least the other.
// -0.0 below +0.0 is an order numpy does not have (its partition holds the two equal), and it is harmless: an order statistic
// that is a zero is a zero under either order, only its sign can differ, and np.median never shows that sign - it is np.mean of
// the middle value(s), whose sum starts from +0.0, and block_median adds the same way.  The MAD's keys are absolute values.
#pragma once

namespace rs {

template <class T> struct Bits;
template <> struct Bits<_Float16> {
    typedef unsigned type;
    static constexpr int kPasses = 2, kNanBinLo = 0x03, kNanBinHi = 0xfc;
    __device__ static unsigned key(_Float16 v) {
        const unsigned u = (unsigned)__builtin_bit_cast(unsigned short, v);
        return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
    }
    __device__ static _Float16 value(unsigned k) {
        const unsigned u = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
        return __builtin_bit_cast(_Float16, (unsigned short)u);
    }
    __device__ static bool is_nan(unsigned k) { return k > 0xfc00u || k < 0x03ffu; }          // key(+inf), key(-inf)
};
template <> struct Bits<float> {
    typedef unsigned type;
    static constexpr int kPasses = 4, kNanBinLo = 0x00, kNanBinHi = 0xff;
    __device__ static unsigned key(float v) {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    __device__ static float value(unsigned k) {
        const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
        return __builtin_bit_cast(float, u);
    }
    __device__ static bool is_nan(unsigned k) { return k > 0xff800000u || k < 0x007fffffu; }
};
template <> struct Bits<double> {
    typedef unsigned long long type;
    static constexpr int kPasses = 8, kNanBinLo = 0x00, kNanBinHi = 0xff;
    __device__ static unsigned long long key(double v) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    __device__ static double value(unsigned long long k) {
        const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
        return __builtin_bit_cast(double, u);
    }
    __device__ static bool is_nan(unsigned long long k) { return k > 0xfff0000000000000ull || k < 0x000fffffffffffffull; }
};

}  // namespace rs
