// Sequential conv programs (seqnet.hip): the tail of a program - unfused max-pool, GAP + FC + softmax head, ragged lengths.
#pragma once
#include "../common.hpp"

namespace rs {
namespace {
__global__ __launch_bounds__(256) void seq_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y, int B,
                                                          int T_in, int T_out, int c, int pad) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (int64_t)B * T_out * c) return;
    const int ch = (int)(g % c);
    const int64_t bt = g / c;
    const int t = (int)(bt % T_out);
    const int b = (int)(bt / T_out);
    const int t0 = 2 * t - pad, t1 = 2 * t + 1 - pad;             // window of MaxPool1d(2, 2, padding pad)
    float v = -INFINITY;
    if (t0 >= 0 && t0 < T_in) v = fmaxf(v, x[((int64_t)b * T_in + t0) * c + ch]);
    if (t1 >= 0 && t1 < T_in) v = fmaxf(v, x[((int64_t)b * T_in + t1) * c + ch]);
    y[g] = v;
}

// GAP over T rows -> FC(c, 2) -> softmax; one 256-thread workgroup per read: wave w sums the rows t = w (mod 4) of
// each channel (coalesced 256-byte row segments, four rows in flight per channel group), LDS combines the four partial
// sums in a fixed order, wave 0 finishes
__global__ __launch_bounds__(256) void seq_head_kernel(const float* __restrict__ x, int T_pitch, int c,
                                                       const float* __restrict__ fcw, const float* __restrict__ fcb,
                                                       float* __restrict__ probs, float* __restrict__ logits,
                                                       const int32_t* __restrict__ rt /* ragged batches: rows of read b (null: T_pitch) */) {
    __shared__ float part[4][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int T = rt ? as_const_len(rt)[b] : T_pitch;
    float a0 = 0.f, a1 = 0.f;
    for (int c0 = 0; c0 < c; c0 += 64) {
        const int ch = c0 + lane;
        float s = 0.f;
        if (ch < c) {
            // eight rows in flight per lane (the loop is a chain of dependent-looking loads otherwise: T / 4 round trips)
            const float* col = x + (int64_t)b * T_pitch * c + ch;
            int t = wave;
            for (; t + 28 < T; t += 32) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = col[(int64_t)(t + 4 * u) * c];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; t < T; t += 4) s += col[(int64_t)t * c];
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
        const float l0 = a0 + fcb[0], l1 = a1 + fcb[1];
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

// Ragged batches (rs_seqnet_forward_ragged): table[k + 1][b] = rows of read b after op k, table[0][b] = its samples.  One thread per
// read walks the program's ops (a conv: (T + 2 pad - k) / stride + 1, or 0 when the kernel does not fit; MaxPool1d(2, 2, pad)).
struct LenRecipe {
    int n_ops;
    signed char kind[64], pad[64];
    short k[64], stride[64], prod[64];        // prod: the op that wrote this op's input buffer, -1 = the program's input
};
__global__ __launch_bounds__(256) void seq_lengths_kernel(const int32_t* __restrict__ len, int B, int ld, const LenRecipe rc,
                                                          int32_t* __restrict__ table) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    table[b] = min(max(len[b], 0), ld);                      // a length beyond the row pitch would read the next read's row
    for (int i = 0; i < rc.n_ops; ++i) {
        const int t = table[(size_t)(rc.prod[i] + 1) * B + b];
        int o;
        if (rc.kind[i] == 0)
            o = t + 2 * rc.pad[i] < rc.k[i] ? 0 : (t + 2 * rc.pad[i] - rc.k[i]) / rc.stride[i] + 1;
        else
            o = t <= 0 ? 0 : (rc.pad[i] ? t / 2 + 1 : t / 2);
        table[(size_t)(i + 1) * B + b] = o;
    }
}
}  // namespace
}  // namespace rs
