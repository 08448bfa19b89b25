// Finding the bin that holds a rank in a 256-bin histogram, by one wave: lane l holds the counts of bins 4 l .. 4 l + 3, an
// inclusive scan over the 64 lanes gives every lane the count below its bins (signal/radix_select.hpp; polya_coords.hip asks for
// two ranks at once and uses the scan alone).
#pragma once

namespace rs {

// inclusive prefix sum of v over the 64 lanes of a wave
__device__ __forceinline__ int wave_scan_inclusive(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d, 64);
        if (lane >= d) v += u;
    }
    return v;
}

// rank k (0-based, below the sum of all counts) -> the bin that holds it, the rank inside that bin and the bin's count; wave-uniform
__device__ __forceinline__ void wave_find_rank(const int (&c)[4], int lane, int k, int& bin, int& rest, int& count) {
    const int t = c[0] + c[1] + c[2] + c[3];
    int run = wave_scan_inclusive(t, lane) - t, b = -1, r = 0, n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (k >= run && k < run + c[j]) {
            b = 4 * lane + j;
            r = k - run;
            n = c[j];
        }
        run += c[j];
    }
    const unsigned long long found = __ballot(b >= 0);                // one lane: 0 <= k < the counted keys
    const int src = found ? __ffsll((long long)found) - 1 : 0;
    bin = __builtin_amdgcn_readlane(b, src) & 255;                    // wave-uniform lane: no trip through LDS
    rest = __builtin_amdgcn_readlane(r, src);
    count = __builtin_amdgcn_readlane(n, src);
}

}  // namespace rs
