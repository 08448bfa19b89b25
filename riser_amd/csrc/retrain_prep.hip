// The reference's retraining preprocessing (riser/retrain/preprocess.py) for a batch of reads: raw int16 samples and the
// channel's calibration (or float32 pA) in, the MAD-normalised, outlier-smoothed first n samples out for EVERY requested
// prefix length n (the README runs the script three times, for 2 s, 3 s and 4 s), with the script's semantics:
//   x   = float32(scale * (float64(raw) + offset))[:n]      one rounding (get_raw_data(scale=True) as numpy evaluates it)
//   med = np.median(x), mad = np.median(|x - med|)           float32, the mean of the two middle values for an even n
//   y   = (x - med) / (float32(1.4826) * mad)                one rounding per operation, IEEE division, NO zero-MAD guard
//         (:42-44, "TODO: Handle divide by zero"): a zero MAD gives NaN where x == med and +-inf elsewhere
//   the sequential in-place smoothing of {|y| > lim} (:18-33), lim a float32: NaN is no outlier, +-inf is one.
// rs_normalise_float is the LIVE rule on float input (zeros for a zero MAD, 3.5 built in).
//
// One 512-thread workgroup per read.  The pA values of the longest prefix that applies to the read are staged ONCE in LDS
// (4 B x n, up to 128 KiB) and every prefix is served from there: HBM sees a read once and an output row once.
// Order statistics are exact: the workgroup radix select of signal/radix_select.hpp (per-wave histograms, ballot-aggregated
// counting, one select and a min reduction per median) over LDS.  The output pass is signal/smooth.hpp with lim as given; a zero
// MAD makes denom zero there, which that header accepts.  rs_normalise_float (normalise_float.hip) runs the same two headers on
// float16 / float32 / float64 reads in global memory.
#include "common.hpp"
#include "signal/radix_select.hpp"
#include "signal/smooth.hpp"

#include <cmath>

namespace rs {
namespace {

constexpr int kThreads = 512;                      // riser_amd/retrain.py: WORKGROUP_THREADS (the tests' shape edges)
constexpr int kWaves = kThreads / 64;
constexpr int kMaxCutoffs = 4;
constexpr int kMaxCutoff = 32768;                  // 128 KiB of pA values beside 8 KiB of histograms in the CU's 160 KiB

struct PrepArgs {
    const void* sig;
    const int64_t* off;
    const int32_t* len;
    const double* calib;
    const int64_t* rows;
    double* stats;
    float* out[kMaxCutoffs];
    int32_t cut[kMaxCutoffs];
    int n_cut, B;
    float lim;
};

// 8 waves per SIMD by registers: short cutoffs leave LDS for four workgroups per CU, and the registers must too
template <bool RAW16>
__global__ __launch_bounds__(kThreads, 8) void retrain_prep_kernel(PrepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ __attribute__((aligned(16))) unsigned hist[kWaves * 256];
    __shared__ unsigned red[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = a.len[b];
    int n_max = 0;
#pragma unroll
    for (int c = 0; c < kMaxCutoffs; ++c)
        if (c < a.n_cut && len >= a.cut[c] && a.rows[(int64_t)c * a.B + b] >= 0) n_max = a.cut[c];
    if (n_max == 0) return;                                           // the whole workgroup
    if (RAW16) {
        // a read starts at any int16 offset: 2-byte loads, 128 contiguous bytes per wave instruction
        const int16_t* s = static_cast<const int16_t*>(a.sig) + a.off[b];
        const double offset = a.calib[2 * (int64_t)b], scale = a.calib[2 * (int64_t)b + 1];
        for (int i = tid; i < n_max; i += kThreads) xs[i] = (float)(scale * ((double)s[i] + offset));
    } else {
        const float* s = static_cast<const float*>(a.sig) + a.off[b];
        for (int i = tid; i < n_max; i += kThreads) xs[i] = s[i];
    }
    __syncthreads();
    const float lim = a.lim;
#pragma unroll 1
    for (int c = 0; c < a.n_cut; ++c) {
        const int n = a.cut[c];
        const int64_t row = a.rows[(int64_t)c * a.B + b];
        if (row < 0 || len < n) continue;                             // workgroup-uniform
        const float med = block_median<float, kThreads>([&](int i) { return Bits<float>::key(xs[i]); }, n, hist, red, tid);
        const float mad = block_median<float, kThreads>([&](int i) { return Bits<float>::key(__builtin_fabsf(xs[i] - med)); }, n,
                                                        hist, red, tid);
        if (a.stats && tid == 0) {
            double* st = a.stats + 2 * ((int64_t)c * a.B + b);
            st[0] = (double)med;
            st[1] = (double)mad;
        }
        const float denom = 1.4826f * mad;                            // the Python float adopts float32 (NEP 50); :44, unguarded
        smooth_write<float, kThreads>([&](int j) { return xs[j]; }, n, med, denom, lim, a.out[c] + row * (int64_t)n, tid);
    }
}

}  // namespace
}  // namespace rs

extern "C" {

int rs_retrain_prepare(const void* d_sig, int elem_bytes, const int64_t* d_off, const int32_t* d_len, const double* d_calib,
                       int B, const int32_t* cutoffs, int n_cut, float outlier_lim, const int64_t* d_rows,
                       float* const* d_out, double* d_stats, void* stream) {
    using namespace rs;
    if (elem_bytes != 2 && elem_bytes != 4) {
        set_error("rs_retrain_prepare: element size %d not 2 (raw int16) or 4 (float32 pA)", elem_bytes);
        return RS_ERR_ARG;
    }
    if (n_cut < 1 || n_cut > kMaxCutoffs || !cutoffs) {
        set_error("rs_retrain_prepare: %d cutoffs (1 .. %d, in a host array)", n_cut, kMaxCutoffs);
        return RS_ERR_ARG;
    }
    for (int c = 0; c < n_cut; ++c) {
        if (cutoffs[c] < 2 || cutoffs[c] > kMaxCutoff) {
            set_error("rs_retrain_prepare: cutoff %d outside [2, %d]", cutoffs[c], kMaxCutoff);
            return RS_ERR_ARG;
        }
        if (c > 0 && cutoffs[c] <= cutoffs[c - 1]) {
            set_error("rs_retrain_prepare: cutoffs not strictly ascending (%d behind %d)", cutoffs[c], cutoffs[c - 1]);
            return RS_ERR_ARG;
        }
    }
    if (B < 0) {
        set_error("rs_retrain_prepare: negative B %d", B);
        return RS_ERR_ARG;
    }
    if (!std::isfinite(outlier_lim) || outlier_lim < 0.0f) {
        set_error("rs_retrain_prepare: outlier limit %g not finite or negative", (double)outlier_lim);
        return RS_ERR_ARG;
    }
    if (B == 0) return RS_OK;
    if (!d_sig || !d_off || !d_len || !d_rows || !d_out) {
        set_error("rs_retrain_prepare: null argument");
        return RS_ERR_ARG;
    }
    if (elem_bytes == 2 && !d_calib) {
        set_error("rs_retrain_prepare: null calibration with raw int16 input");
        return RS_ERR_ARG;
    }
    PrepArgs a = {};
    for (int c = 0; c < n_cut; ++c) {
        if (!d_out[c]) {
            set_error("rs_retrain_prepare: null output for cutoff %d", cutoffs[c]);
            return RS_ERR_ARG;
        }
        a.out[c] = d_out[c];
        a.cut[c] = cutoffs[c];
    }
    a.sig = d_sig;
    a.off = d_off;
    a.len = d_len;
    a.calib = d_calib;
    a.rows = d_rows;
    a.stats = d_stats;
    a.n_cut = n_cut;
    a.B = B;
    a.lim = outlier_lim;
    auto fn = elem_bytes == 2 ? retrain_prep_kernel<true> : retrain_prep_kernel<false>;
    const size_t lds = (size_t)cutoffs[n_cut - 1] * sizeof(float);
    RS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                               kMaxCutoff * (int)sizeof(float)));
    hipLaunchKernelGGL(fn, dim3((unsigned)B), dim3(kThreads), lds, static_cast<hipStream_t>(stream), a);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

}  // extern "C"
