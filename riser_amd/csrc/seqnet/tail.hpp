// Sequential conv programs (seqnet.hip): the tail of a program - unfused max-pool, ragged lengths; the GAP + FC + softmax head is
// family/head.hpp: gap_head_kernel.
#pragma once
#include "../common.hpp"
#include "../family/head.hpp"

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
