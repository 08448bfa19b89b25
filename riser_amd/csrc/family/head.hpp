// The two classifier heads of the sequential families: Linear(c -> 2) + softmax on one row per read (TCN, CNN-RNN), and
// GAP + FC + softmax over a read's rows (seqnet.hip's conv programs, the generic ConvNets).  The order of every
// floating-point operation is fixed: a read's logits do not depend on the batch, the pitch or the caller.
#pragma once
#include "../common.hpp"

namespace rs {
namespace {

// the TCN's validity rule: every read has a last position
struct AlwaysValid {
    __device__ bool operator()(int) const { return true; }
};

// Linear(c -> 2) + softmax (riser/model.py:27) on row b of h [B][pitch], one thread per read.  valid(b) false: the read is
// too short for the net and gets NaN.
template <class Valid>
__global__ __launch_bounds__(256) void last_row_head_kernel(const float* __restrict__ h, int B, int pitch, int c,
                                                            const float* __restrict__ fw, const float* __restrict__ fb,
                                                            const Valid valid, float* __restrict__ probs,
                                                            float* __restrict__ logits) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float* x = h + (int64_t)b * pitch;
    float l0 = fb[0], l1 = fb[1];
    for (int i = 0; i < c; ++i) {
        l0 = fmaf(fw[i], x[i], l0);
        l1 = fmaf(fw[c + i], x[i], l1);
    }
    if (!valid(b)) l0 = l1 = __builtin_nanf("");
    const float mx = fmaxf(l0, l1);
    const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
    const float s = e0 + e1;
    probs[2 * b] = e0 / s;
    probs[2 * b + 1] = e1 / s;
    if (logits) {
        logits[2 * b] = l0;
        logits[2 * b + 1] = l1;
    }
}

// GAP over the read's own T rows -> FC(c, 2) -> softmax (riser/nets/cnn.py:28-33, riser/model.py:27) on x [B][rows_pitch]
// [channel_pitch]; T = rows[b], or rows_pitch for every read where rows is null.  One 256-thread workgroup per read: wave w
// sums the rows t = w (mod 4) of each channel (coalesced 256-byte row segments, eight rows in flight per lane: the loop is
// a chain of dependent-looking loads otherwise, T / 4 round trips), LDS combines the four partial sums in a fixed order,
// wave 0 finishes.  NAN_EMPTY: a read with no row left gets NaN by assignment (shorter than the net's minimum: the
// reference's max_pool raises).
template <bool NAN_EMPTY>
__global__ __launch_bounds__(256) void gap_head_kernel(const float* __restrict__ x, int rows_pitch, int channel_pitch, int c,
                                                       const float* __restrict__ fcw, const float* __restrict__ fcb,
                                                       const int32_t* __restrict__ rows, float* __restrict__ probs,
                                                       float* __restrict__ logits) {
    __shared__ float part[4][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cp = channel_pitch;
    const int T = rows ? as_const_len(rows)[b] : rows_pitch;
    float a0 = 0.f, a1 = 0.f;
    for (int c0 = 0; c0 < c; c0 += 64) {
        const int ch = c0 + lane;
        float s = 0.f;
        if (ch < c) {
            const float* col = x + (int64_t)b * rows_pitch * cp + ch;
            int t = wave;
            for (; t + 28 < T; t += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)(t + 4 * u) * cp];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; t < T; t += 4) s += col[(int64_t)t * cp];
        }
        part[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && ch < c) {
            const float m = (((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane]) / (float)T;
            a0 = fmaf(m, fcw[ch], a0);
            a1 = fmaf(m, fcw[c + ch], a1);
        }
        __syncthreads();
    }
    if (wave != 0) return;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a0 += __shfl_xor(a0, d, 64);
        a1 += __shfl_xor(a1, d, 64);
    }
    if (lane == 0) {
        float l0 = a0 + fcb[0], l1 = a1 + fcb[1];
        if (NAN_EMPTY && T < 1) l0 = l1 = __builtin_nanf("");
        const float mx = fmaxf(l0, l1);
        const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
        probs[2 * b] = e0 / (e0 + e1);
        probs[2 * b + 1] = e1 / (e0 + e1);
        if (logits) {
            logits[2 * b] = l0;
            logits[2 * b + 1] = l1;
        }
    }
}

}  // namespace
}  // namespace rs
