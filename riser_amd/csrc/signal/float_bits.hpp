// The order-preserving integer image of a floating-point value: key(a) < key(b) as unsigned integers exactly where a < b as
// floats (-0.0 below +0.0), so that order statistics of floats are found by counting on integer digits
// (signal/radix_select.hpp).  kPasses: 8-bit digits per key.
#pragma once

namespace rs {

template <class T> struct Bits;
template <> struct Bits<_Float16> {
    typedef unsigned type;
    static constexpr int kPasses = 2;
    __device__ static unsigned key(_Float16 v) {
        const unsigned u = (unsigned)__builtin_bit_cast(unsigned short, v);
        return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
    }
    __device__ static _Float16 value(unsigned k) {
        const unsigned u = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
        return __builtin_bit_cast(_Float16, (unsigned short)u);
    }
};
template <> struct Bits<float> {
    typedef unsigned type;
    static constexpr int kPasses = 4;
    __device__ static unsigned key(float v) {
        const unsigned u = __builtin_bit_cast(unsigned, v);
        return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    }
    __device__ static float value(unsigned k) {
        const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
        return __builtin_bit_cast(float, u);
    }
};
template <> struct Bits<double> {
    typedef unsigned long long type;
    static constexpr int kPasses = 8;
    __device__ static unsigned long long key(double v) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    __device__ static double value(unsigned long long k) {
        const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
        return __builtin_bit_cast(double, u);
    }
};

}  // namespace rs
