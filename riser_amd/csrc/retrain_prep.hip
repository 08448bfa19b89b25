// The reference's retraining preprocessing (riser/retrain/preprocess.py) for a batch of reads: raw int16 samples and the
// channel's calibration (or float32 pA) in, the MAD-normalised, outlier-smoothed first n samples out for EVERY requested
// prefix length n (the README runs the script three times, for 2 s, 3 s and 4 s), with the script's semantics:
//   x   = float32(scale * (float64(raw) + offset))[:n]      one rounding (get_raw_data(scale=True) as numpy evaluates it)
//   med = np.median(x), mad = np.median(|x - med|)           float32, the mean of the two middle values for an even n
//   y   = (x - med) / (float32(1.4826) * mad)                one rounding per operation, IEEE division, NO zero-MAD guard
//         (:42-44, "TODO: Handle divide by zero"): a zero MAD gives NaN where x == med and +-inf elsewhere
//   the sequential in-place smoothing of {|y| > lim} (:18-33), lim a float32: NaN is no outlier, +-inf is one.
// rs_normalise_float is the LIVE rule on float input (zeros for a zero MAD, 3.5 built in) and stays as it is.
//
// One 512-thread workgroup per read.  The pA values of the longest prefix that applies to the read are staged ONCE in LDS
// (4 B x n, up to 128 KiB) and every prefix is served from there: HBM sees a read once and an output row once.
// Order statistics are exact: MSB-first radix select, 8 bits per pass, on the order-preserving integer image of float32
// (signal/float_bits.hpp), over LDS.  Each wave counts into a histogram of its own; pA values share their sign and most of their
// exponent, so whole waves meet in one bin: the bin of a wave's first counting lane (and then the next one's) is counted
// once, by ballot, and only what is left goes through LDS atomics.  The two middle values of an even n are adjacent order
// statistics: the last pass tells whether rank k + 1 carries the same value, and if not it is the smallest value above -
// one min reduction, not a second selection.
// The output pass is the run-head walk of normalise_float_kernel: every thread writes the elements that are no outliers,
// and the first element of a run of outliers walks its run, since each replacement needs the one before it.  With a zero MAD
// every element off the median is +-inf, a run can span the whole read and one lane walks it: rare (more than half of the
// samples equal) and accepted.
#include "common.hpp"
#include "signal/float_bits.hpp"

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

// k-th smallest (0-based) of the n keys key(0 .. n-1); every thread returns it, and next_same = rank k + 1 holds it too
template <class KeyF>
__device__ unsigned block_select(KeyF key, int n, int k, unsigned* hist, int tid, bool& next_same) {
    const int lane = tid & 63, wave = tid >> 6;
    unsigned* mine = hist + wave * 256;
    unsigned prefix = 0;
    int count = 0;
#pragma unroll 1
    for (int pass = 0; pass < Bits<float>::kPasses; ++pass) {
        const int shift = 8 * (Bits<float>::kPasses - 1 - pass);
#pragma unroll
        for (int j = 0; j < 4; ++j) mine[lane + 64 * j] = 0u;
        __syncthreads();
        for (int base = wave * 64; base < n; base += kThreads) {     // wave-uniform trip count: the ballots below see all lanes
            const int i = base + lane;
            int bin = -1;
            if (i < n) {
                const unsigned q = key(i);
                if (pass == 0 || (q >> (shift + 8)) == prefix) bin = (int)((q >> shift) & 255u);
            }
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const unsigned long long act = __ballot(bin >= 0);
                if (!act) break;
                const int leader = __ffsll((long long)act) - 1;
                const int lb = __builtin_amdgcn_readlane(bin, leader);       // wave-uniform lane: no trip through LDS
                const unsigned long long same = __ballot(bin == lb);
                if (lane == leader) atomicAdd(&mine[lb], (unsigned)__popcll(same));
                if (bin == lb) bin = -1;
            }
            if (bin >= 0) atomicAdd(&mine[bin], 1u);
        }
        __syncthreads();
        // every wave finds the bin of rank k for itself: lane l holds the batch-wide counts of bins 4 l .. 4 l + 3
        int c[4] = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const uint4 h = *reinterpret_cast<const uint4*>(hist + w * 256 + 4 * lane);
            c[0] += (int)h.x;
            c[1] += (int)h.y;
            c[2] += (int)h.z;
            c[3] += (int)h.w;
        }
        const int t = c[0] + c[1] + c[2] + c[3];
        int incl = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        int run = incl - t, bin = -1, rest = 0, cnt = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (k >= run && k < run + c[j]) {
                bin = 4 * lane + j;
                rest = k - run;
                cnt = c[j];
            }
            run += c[j];
        }
        const unsigned long long found = __ballot(bin >= 0);          // one lane: 0 <= k < the counted keys
        const int src = found ? __ffsll((long long)found) - 1 : 0;
        prefix = (prefix << 8) | (unsigned)(__builtin_amdgcn_readlane(bin, src) & 255);
        k = __builtin_amdgcn_readlane(rest, src);
        count = __builtin_amdgcn_readlane(cnt, src);
        __syncthreads();                                              // all waves have read: the next pass clears
    }
    next_same = k + 1 < count;
    return prefix;
}

// np.median of the n float32 values whose images are key(i)
template <class KeyF>
__device__ float block_median(KeyF key, int n, unsigned* hist, unsigned* red, int tid) {
    bool same;
    const unsigned k_lo = block_select(key, n, (n - 1) >> 1, hist, tid, same);
    const float lo = Bits<float>::value(k_lo);
    if (n & 1) return lo;
    unsigned k_hi = k_lo;
    if (!same) {                                                      // workgroup-uniform; rank n / 2: the smallest key above
        unsigned m = 0xffffffffu;
        for (int i = tid; i < n; i += kThreads) {
            const unsigned q = key(i);
            if (q > k_lo) m = min(m, q);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, d, 64));
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) m = min(m, red[w]);
        __syncthreads();
        k_hi = m;
    }
    return (lo + Bits<float>::value(k_hi)) / 2.0f;                    // np.mean of the two middle values, in float32
}

template <bool RAW16>
__global__ __launch_bounds__(kThreads) void retrain_prep_kernel(PrepArgs a) {
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
        const float med = block_median([&](int i) { return Bits<float>::key(xs[i]); }, n, hist, red, tid);
        const float mad = block_median([&](int i) { return Bits<float>::key(__builtin_fabsf(xs[i] - med)); }, n, hist, red, tid);
        if (a.stats && tid == 0) {
            double* st = a.stats + 2 * ((int64_t)c * a.B + b);
            st[0] = (double)med;
            st[1] = (double)mad;
        }
        const float denom = 1.4826f * mad;                            // the Python float adopts float32 (NEP 50)
        float* o = a.out[c] + row * (int64_t)n;
        auto yv = [&](int j) -> float { return (xs[j] - med) / denom; };      // :44, unguarded
        auto is_out = [&](int j) { return __builtin_fabsf(yv(j)) > lim; };    // :20; false for NaN
        for (int i = tid; i < n; i += kThreads) {
            if (!is_out(i)) {
                o[i] = yv(i);
                continue;
            }
            if (i > 0 && is_out(i - 1)) continue;                     // inside a run: its head writes it
            float prev = i > 0 ? yv(i - 1) : 0.0f;
            int j = i;
            do {
                float nv;
                if (j == 0) {
                    nv = yv(1);                                       // :23 (not clipped)
                } else if (j == n - 1) {
                    nv = prev;                                        // :25 (not clipped)
                } else {
                    nv = (prev + yv(j + 1)) / 2.0f;                   // :27
                    nv = nv > lim ? lim : (nv < -lim ? -lim : nv);    // :29-32; NaN passes
                }
                o[j] = nv;
                prev = nv;
                ++j;
            } while (j < n && is_out(j));
        }
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
