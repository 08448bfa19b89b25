// One operation of numpy on scalars / arrays of dtype T, one rounding each (-ffp-contract=off, IEEE division).  float16: numpy
// evaluates every half-precision operation as float32(a) op float32(b) rounded to half, and np.median's mean of the two middle
// values with a float32 accumulator rounded once.
#pragma once

namespace rs {

template <class T> struct Arith {
    __device__ static T add(T a, T b) { return a + b; }
    __device__ static T sub(T a, T b) { return a - b; }
    __device__ static T mul(T a, T b) { return a * b; }
    __device__ static T div(T a, T b) { return a / b; }
    __device__ static T abs(T a) { return __builtin_elementwise_abs(a); }
    __device__ static T mean2(T a, T b) { return (T)((T)(a + b) / (T)2); }     // np.mean([a, b]) in T
};
template <> struct Arith<_Float16> {
    typedef _Float16 H;
    __device__ static H add(H a, H b) { return (H)((float)a + (float)b); }
    __device__ static H sub(H a, H b) { return (H)((float)a - (float)b); }
    __device__ static H mul(H a, H b) { return (H)((float)a * (float)b); }
    __device__ static H div(H a, H b) { return (H)((float)a / (float)b); }
    __device__ static H abs(H a) { return __builtin_elementwise_abs(a); }
    __device__ static H mean2(H a, H b) { return (H)(((float)a + (float)b) / 2.0f); }   // float32 accumulator, one rounding
};

}  // namespace rs
