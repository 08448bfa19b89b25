// poly(A) start and end at any window size and MAD threshold: the window rule of the reference's offline evaluation script
// (riser/test.py:80-117), which takes both from its command line, where the live rule (riser/preprocess.py:42-79, polya.hip)
// has them fixed at 500 and 20 and returns the end alone.
//
// Two launches, no global atomics:
//   1. one wave per window of R samples, four windows of one read per workgroup (one where R > 3584).  The wave stages its window in LDS (int16)
//      and SELECTS by counting, since a window of any size cannot be sorted in registers: a 256-bin histogram (LDS atomics) of
//      a key's high byte finds the bin that holds rank k, a second one of the low byte inside that bin finds the key.  The
//      median is selected on u = x + 32768 (16 bits) as the two middle order statistics, med2 = their sum = twice the median for
//      either parity of R; the MAD on d = |2 x - med2|: every d has med2's parity, so d >> 1 is a 16-bit key as well, and the sum
//      of the two middle d is FOUR times the MAD, an integer.  The window sum rides along with the staging.  (sum, 4 MAD) go to
//      a rectangular table [B][max_len / R] in the caller's workspace; every entry that is read has been written by this call.
//   2. one wave per read walks its table row.  The rule's two conditions are functions of a window's own (sum, 4 MAD) and the
//      sums of the two windows before it, so 64 windows are judged at once and the first start, then the first end at or
//      behind it, are picked from a ballot; the float64 expressions keep the reference's operation order (-ffp-contract=off).
#include "common.hpp"
#include "signal/wave_rank.hpp"

#include <algorithm>

namespace rs {
namespace {

constexpr int kMaxResolution = 16384;              // one window as int16 plus the histogram: 33 KB of LDS for a lone wave
constexpr int kHistBytes = 256 * 4;

__host__ __device__ inline int window_lds_bytes(int R) { return ((2 * R + 15) & ~15) + kHistBytes; }
// waves (= windows) per workgroup: four while the workgroup stays within 32 KB of LDS, else a lone wave (<= 33 KB)
inline int waves_per_group(int R) { return window_lds_bytes(R) <= 8192 ? 4 : 1; }

// LDS traffic of ONE wave on its own arrays: the hardware executes it in program order; the fence keeps the compiler to it
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// histogram of bin(S[i]) over the window (bin < 0: the sample is not counted); lane l then holds bins 4 l .. 4 l + 3
template <typename BinF>
__device__ __forceinline__ void histogram(const int16_t* S, unsigned* H, int R, int lane, BinF bin, int (&c)[4]) {
    wave_sync();                                   // the previous pass has read its counts
#pragma unroll
    for (int j = 0; j < 4; ++j) H[lane + 64 * j] = 0u;
    wave_sync();
    for (int i = lane; i < R; i += 64) {
        const int b = bin((int)S[i]);
        if (b >= 0) atomicAdd(&H[b], 1u);
    }
    wave_sync();
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = (int)H[4 * lane + j];
}

// ranks k0 <= k1 among the counted samples -> (bin << 16) | rank inside the bin, for each
__device__ __forceinline__ void find_ranks(const int (&c)[4], int lane, int k0, int k1, int& r0, int& r1) {
    const int t = c[0] + c[1] + c[2] + c[3];
    int run = wave_scan_inclusive(t, lane) - t;
    r0 = -1;
    r1 = -1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (k0 >= run && k0 < run + c[j]) r0 = ((4 * lane + j) << 16) | (k0 - run);
        if (k1 >= run && k1 < run + c[j]) r1 = ((4 * lane + j) << 16) | (k1 - run);
        run += c[j];
    }
    r0 = wave_max(r0);
    r1 = wave_max(r1);
}

// order statistics k0 <= k1 (0-based) of the 16-bit keys key(S[i]), i < R
template <typename KeyF>
__device__ __forceinline__ void select2(const int16_t* S, unsigned* H, int R, int lane, int k0, int k1, KeyF key, int& v0,
                                        int& v1) {
    int c[4], r0, r1;
    histogram(S, H, R, lane, [&](int x) { return key(x) >> 8; }, c);
    find_ranks(c, lane, k0, k1, r0, r1);
    const int hi0 = r0 >> 16, hi1 = r1 >> 16;
    int q0, q1;
    histogram(S, H, R, lane, [&](int x) { const int k = key(x); return (k >> 8) == hi0 ? (k & 255) : -1; }, c);
    find_ranks(c, lane, r0 & 0xffff, hi1 == hi0 ? (r1 & 0xffff) : (r0 & 0xffff), q0, q1);
    if (hi1 != hi0) {                              // the two middles straddle a bin boundary (wave-uniform)
        int unused;
        histogram(S, H, R, lane, [&](int x) { const int k = key(x); return (k >> 8) == hi1 ? (k & 255) : -1; }, c);
        find_ranks(c, lane, r1 & 0xffff, r1 & 0xffff, q1, unused);
    }
    v0 = (hi0 << 8) | (q0 >> 16);
    v1 = (hi1 << 8) | (q1 >> 16);
}

// grid: (workgroups per read) x (reads of this launch), flattened; waves: 64-lane waves per workgroup
__global__ __launch_bounds__(256) void coords_windows_kernel(const int16_t* __restrict__ sig,
                                                             const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ len, int b0, int groups_per_read,
                                                             int max_len, int R, int pitch, int2* __restrict__ table) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int waves = blockDim.x >> 6;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = b0 + (int)(blockIdx.x / (unsigned)groups_per_read);
    const int w = (int)(blockIdx.x % (unsigned)groups_per_read) * waves + wave;
    const int n = min(len[b], max_len);
    if (n < R || w >= n / R) return;               // no workgroup barrier anywhere below: a wave may leave alone
    unsigned char* mine = lds + (size_t)wave * window_lds_bytes(R);
    unsigned* H = reinterpret_cast<unsigned*>(mine);
    int16_t* S = reinterpret_cast<int16_t*>(mine + kHistBytes);
    // a read starts at any int16 offset: 2-byte loads, 128 contiguous bytes per wave instruction
    const int16_t* src = sig + off[b] + (int64_t)w * R;
    int s = 0;
    for (int i = lane; i < R; i += 64) {
        const int16_t x = src[i];
        S[i] = x;
        s += x;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    const int k0 = (R - 1) >> 1, k1 = R >> 1;      // the two middles (the same one for an odd R)
    int u0, u1;
    select2(S, H, R, lane, k0, k1, [](int x) { return x + 32768; }, u0, u1);
    const int med2 = u0 + u1 - 65536;              // twice the median
    const int par = med2 & 1;
    int e0, e1;
    select2(S, H, R, lane, k0, k1, [=](int x) { return abs(2 * x - med2) >> 1; }, e0, e1);
    if (lane == 0) table[(size_t)b * pitch + w] = make_int2(s, 2 * (e0 + e1) + 2 * par);   // (sum, 4 x MAD)
}

__global__ __launch_bounds__(64) void coords_scan_kernel(const int2* __restrict__ table, const int32_t* __restrict__ len,
                                                         int max_len, int R, int mad_threshold, int pitch,
                                                         int32_t* __restrict__ d_start, int32_t* __restrict__ d_end) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = min(len[b], max_len);
    const int nw = n >= R ? n / R : 0;
    const int2* row = table + (size_t)b * pitch;
    int start = -1, end = -1;
    for (int w0 = 0; w0 < nw && end < 0; w0 += 64) {
        const int w = w0 + lane;
        bool sc = false, ec = false;
        if (w < nw) {
            const int2 t = row[w];
            const double mad = (double)t.y * 0.25;
            const double mean = (double)t.x / (double)R;
            double rolling = mean;
            // i > 2 R, strictly (riser/test.py:95): from the fourth window on
            if (w > 2) rolling = (double)((int64_t)row[w - 1].x + (int64_t)row[w - 2].x) / (double)(2 * (int64_t)R);
            const double change = (mean - rolling) / rolling * 100.0;        // inf / nan compare as IEEE does
            sc = change > 20.0 && mad <= (double)mad_threshold;
            ec = mad > 20.0;                                                  // the literal of riser/test.py:104
        }
        if (start < 0) {
            const unsigned long long m = __ballot(sc);
            if (m) start = (w0 + __ffsll((long long)m) - 1) * R;              // >= 3 R: never the index 0 `not polyA_start` re-opens
        }
        if (start >= 0) {
            const unsigned long long m = __ballot(ec && w * R >= start);      // the start's own window may end it
            if (m) end = (w0 + __ffsll((long long)m) - 1) * R;
        }
    }
    if (lane == 0) {
        d_start[b] = start;
        d_end[b] = end;
    }
}

}  // namespace
}  // namespace rs

extern "C" {

size_t rs_polya_coords_workspace_bytes(int B, int max_len, int resolution) {
    if (B <= 0 || max_len < 0 || resolution < 1 || resolution > rs::kMaxResolution) return 0;
    const size_t pitch = (size_t)(max_len / resolution);
    return (pitch > 0 ? (size_t)B * pitch : 1) * sizeof(int2);
}

int rs_polya_coords(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B, int max_len, int resolution,
                    int mad_threshold, int32_t* d_start, int32_t* d_end, void* d_ws, size_t ws_bytes, void* stream) {
    using namespace rs;
    if (resolution < 1 || resolution > kMaxResolution) {
        set_error("rs_polya_coords: resolution %d outside [1, %d]", resolution, kMaxResolution);
        return RS_ERR_ARG;
    }
    if (B < 0 || max_len < 0) {
        set_error("rs_polya_coords: negative B %d or max_len %d", B, max_len);
        return RS_ERR_ARG;
    }
    if (B == 0) return RS_OK;
    if (!d_sig || !d_off || !d_len || !d_start || !d_end || !d_ws) {
        set_error("rs_polya_coords: null argument");
        return RS_ERR_ARG;
    }
    const size_t need = rs_polya_coords_workspace_bytes(B, max_len, resolution);
    if (ws_bytes < need) {
        set_error("rs_polya_coords: workspace of %zu bytes, rs_polya_coords_workspace_bytes() asks for %zu", ws_bytes, need);
        return RS_ERR_WORKSPACE;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int R = resolution, pitch = max_len / R;
    int2* table = static_cast<int2*>(d_ws);
    if (pitch > 0) {
        const int waves = waves_per_group(R);
        const int gpr = (pitch + waves - 1) / waves;                         // workgroups per read, <= 2^29
        const int reads_per_launch = std::max(1, (1 << 30) / gpr);            // a grid stays below 2^31 workgroups
        for (int b0 = 0; b0 < B; b0 += reads_per_launch) {
            const int nb = std::min(reads_per_launch, B - b0);
            hipLaunchKernelGGL(coords_windows_kernel, dim3((unsigned)nb * (unsigned)gpr), dim3(64 * waves),
                               (size_t)waves * window_lds_bytes(R), st, d_sig, d_off, d_len, b0, gpr, max_len, R, pitch, table);
            RS_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(coords_scan_kernel, dim3(B), dim3(64), 0, st, table, d_len, max_len, R, mad_threshold, pitch, d_start,
                       d_end);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

}  // extern "C"
