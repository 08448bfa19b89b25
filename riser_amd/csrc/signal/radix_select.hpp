// Exact order statistics of floating-point values by one workgroup of THREADS threads: MSB-first radix select, 8 bits per pass, on
// the order-preserving integer image of T (signal/float_bits.hpp).  Each wave counts into a histogram of its own (hist: THREADS / 64
// x 256 counters, 16-byte aligned); signal values share their sign and most of their exponent, so whole waves meet in one bin: the
// bin of a wave's first counting lane (and then the next one's) is counted once, by ballot, and only what is left goes through LDS
// atomics.  The two middle values of an even n are adjacent order statistics: the last pass tells whether rank k + 1 carries the
// same value, and if not it is the smallest value above - one min reduction, not a second selection.
// NaN: np.median answers NaN as soon as one of the n values is a NaN, for an odd and an even n alike.  A NaN's image lies beyond
// those of the infinities (Bits<T>::is_nan), so it can only have been counted into the outermost bins of the first pass
// (Bits<T>::kNanBinLo and below, kNanBinHi and above), which hold nothing else but the infinities and, in float32 and float64, the
// finite values of the largest exponent(s).  The counting loop stays as it is; where the first pass's totals show a key in one of
// those bins - no signal does - block_median looks at every key once more (block_has_nan, n keys) and answers NaN if one is a
// NaN's image.  With a NaN median every |x - med| is NaN, so the MAD's select answers NaN in the same way, as it does for an
// infinite median (inf - inf).
// Signed zeros: np.median is np.mean of the middle value(s), a sum that starts from +0.0, so a median that is a zero is +0.0
// whatever the signs of the zeros in the read - also for an odd n, and for two middle values of -0.0.  block_median adds in that
// order (float_bits.hpp on why the image's own order of the two zeros does not matter).
#pragma once

#include "float_arith.hpp"
#include "float_bits.hpp"
#include "wave_rank.hpp"

namespace rs {

// k-th smallest (0-based) of the n keys key(0 .. n-1); every thread returns it, and next_same = rank k + 1 holds it too.
// nan_bins (workgroup-uniform): a key was counted into one of the bins that a NaN's image falls into
template <class T, int THREADS, class KeyF>
__device__ typename Bits<T>::type block_select(KeyF key, int n, int k, unsigned* hist, int tid, bool& next_same,
                                               bool& nan_bins) {
    typedef typename Bits<T>::type K;
    const int lane = tid & 63, wave = tid >> 6;
    unsigned* mine = hist + wave * 256;
    K prefix = 0;
    int count = 0;
#pragma unroll 1
    for (int pass = 0; pass < Bits<T>::kPasses; ++pass) {
        const int shift = 8 * (Bits<T>::kPasses - 1 - pass);
#pragma unroll
        for (int j = 0; j < 4; ++j) mine[lane + 64 * j] = 0u;
        __syncthreads();
        for (int base = wave * 64; base < n; base += THREADS) {      // wave-uniform trip count: the ballots below see all lanes
            const int i = base + lane;
            int bin = -1;
            if (i < n) {
                const K q = key(i);
                // pass 0 of a 32- or 64-bit key: shift + 8 is the key's full width, which no shift may be
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
        // every wave finds the bin of rank k for itself: lane l holds the workgroup-wide counts of bins 4 l .. 4 l + 3
        int c[4] = {0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) {
            const uint4 h = *reinterpret_cast<const uint4*>(hist + w * 256 + 4 * lane);
            c[0] += (int)h.x;
            c[1] += (int)h.y;
            c[2] += (int)h.z;
            c[3] += (int)h.w;
        }
        if (pass == 0) {                                              // every wave holds the same totals
            bool outer = false;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                outer |= c[j] != 0 && (4 * lane + j <= Bits<T>::kNanBinLo || 4 * lane + j >= Bits<T>::kNanBinHi);
            nan_bins = __ballot(outer) != 0;
        }
        int bin, rest;
        wave_find_rank(c, lane, k, bin, rest, count);
        prefix = (prefix << 8) | (K)bin;
        k = rest;
        __syncthreads();                                              // all waves have read: the next pass clears
    }
    next_same = k + 1 < count;
    return prefix;
}

// one of the n keys is the image of a NaN; every thread returns it.  flag: one LDS word that no thread is still reading
template <class T, int THREADS, class KeyF>
__device__ bool block_has_nan(KeyF key, int n, typename Bits<T>::type* flag, int tid) {
    bool nan = false;
    for (int i = tid; i < n; i += THREADS) nan |= Bits<T>::is_nan(key(i));
    if (tid == 0) *flag = 0;
    __syncthreads();
    if (__ballot(nan) && (tid & 63) == 0) *flag = 1;                  // every writer writes the same word
    __syncthreads();
    const bool any = *flag != 0;
    __syncthreads();                                                  // all have read: the caller may use the word again
    return any;
}

// np.median of the n values of dtype T whose images are key(i), NaN if one of them is a NaN; red: THREADS / 64 keys
template <class T, int THREADS, class KeyF>
__device__ T block_median(KeyF key, int n, unsigned* hist, typename Bits<T>::type* red, int tid) {
    typedef typename Bits<T>::type K;
    bool same, nan_bins;
    const K k_lo = block_select<T, THREADS>(key, n, (n - 1) >> 1, hist, tid, same, nan_bins);
    if (nan_bins && block_has_nan<T, THREADS>(key, n, red, tid)) return (T)__builtin_nanf("");      // workgroup-uniform
    const T lo = Arith<T>::add((T)0, Bits<T>::value(k_lo));          // np.mean's sum starts from +0.0: -0.0 becomes +0.0
    if (n & 1) return lo;
    K k_hi = k_lo;
    if (!same) {                                                      // workgroup-uniform; rank n / 2: the smallest key above
        K m = ~(K)0;
        for (int i = tid; i < n; i += THREADS) {
            const K q = key(i);
            if (q > k_lo) m = min(m, q);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) m = min(m, (K)__shfl_xor(m, d, 64));
        if ((tid & 63) == 0) red[tid >> 6] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) m = min(m, red[w]);
        __syncthreads();
        k_hi = m;
    }
    return Arith<T>::mean2(lo, Bits<T>::value(k_hi));                 // np.mean of the two middle values, in T
}

}  // namespace rs
