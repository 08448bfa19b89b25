// K1f: MAD normalisation + outlier smoothing of FLOATING-POINT signals (float16, float32 or float64), one 256-thread workgroup
// per read.  The live path feeds raw int16 ADC counts (normalise.hip); this kernel covers the other input the
// reference's SignalProcessor.mad_normalise accepts (riser/preprocess.py:108-147): the retrain path normalises
// pA-scaled float signals (riser/retrain/preprocess.py:79).  numpy keeps the input's precision end to end (NEP 50:
// the Python float 1.4826 adopts the array's dtype), so everything here is evaluated in T:
//   med = np.median(x)                       exact order statistics (mean of the two middle values for even n, in T)
//   mad = np.median(np.abs(x - med))         |x - med| rounded in T, then the same select
//   y   = (x - med) / (T(1.4826) * mad)      one rounding per operation (-ffp-contract=off, IEEE division)
//   the sequential in-place smoothing of {|y| > 3.5} of normalise.hip, in T.
// float16: numpy evaluates every half-precision operation as float32(a) op float32(b) rounded to half, and np.median's
// mean of the two middle values with a float32 accumulator rounded once - Arith<_Float16> (signal/float_arith.hpp) spells
// exactly that.
// Order statistics are exact: the workgroup radix select of signal/radix_select.hpp on the order-preserving integer image of the
// value, over the read in global memory (it is a few tens of KB: L2-resident after the first pass); one select per median and a
// min reduction for an even n.  The output pass is signal/smooth.hpp.  rs_retrain_prepare (retrain_prep.hip) runs the same two
// headers over LDS, in float32, with the retraining script's rule: no zero-MAD guard, the limit a parameter.
#include "common.hpp"
#include "signal/radix_select.hpp"
#include "signal/smooth.hpp"

namespace rs {
namespace {

constexpr int kThreads = 256;

template <class T>
__global__ __launch_bounds__(kThreads) void normalise_float_kernel(const T* __restrict__ sig, const int64_t* __restrict__ off,
                                                                   const int32_t* __restrict__ len, T* __restrict__ out,
                                                                   int64_t ld, double* __restrict__ stats) {
    typedef typename Bits<T>::type K;
    __shared__ __attribute__((aligned(16))) unsigned hist[kThreads / 64 * 256];
    __shared__ K red[kThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = len[b];
    const T* x = sig + off[b];
    T* o = out + (int64_t)b * ld;
    const T med = block_median<T, kThreads>([&](int i) { return Bits<T>::key(x[i]); }, n, hist, red, tid);
    const T mad = block_median<T, kThreads>([&](int i) { return Bits<T>::key(Arith<T>::abs(Arith<T>::sub(x[i], med))); }, n,
                                            hist, red, tid);
    if (stats && tid == 0) {
        stats[2 * b + 0] = (double)med;
        stats[2 * b + 1] = (double)mad;
    }
    if (mad == (T)0) {                                               // riser/preprocess.py:123-124
        for (int i = tid; i < n; i += kThreads) o[i] = (T)0;
        return;
    }
    const T denom = Arith<T>::mul((T)1.4826, mad);                   // the Python float adopts the array's dtype
    smooth_write<T, kThreads>([&](int j) { return x[j]; }, n, med, denom, (T)3.5, o, tid);
}

}  // namespace

int launch_normalise_float(const void* d_sig, int elem_bytes, const int64_t* d_off, const int32_t* d_len, int B, void* d_out,
                           int64_t ld, double* d_stats, hipStream_t st) {
    if (B <= 0) return RS_OK;
    if (elem_bytes == 2)
        hipLaunchKernelGGL(normalise_float_kernel<_Float16>, dim3(B), dim3(kThreads), 0, st,
                           static_cast<const _Float16*>(d_sig), d_off, d_len, static_cast<_Float16*>(d_out), ld, d_stats);
    else if (elem_bytes == 4)
        hipLaunchKernelGGL(normalise_float_kernel<float>, dim3(B), dim3(kThreads), 0, st, static_cast<const float*>(d_sig),
                           d_off, d_len, static_cast<float*>(d_out), ld, d_stats);
    else
        hipLaunchKernelGGL(normalise_float_kernel<double>, dim3(B), dim3(kThreads), 0, st,
                           static_cast<const double*>(d_sig), d_off, d_len, static_cast<double*>(d_out), ld, d_stats);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

}  // namespace rs
