// Sequential conv programs (seqnet.hip): the unfused CONV kernels - scalar, f32-input MFMA, and MFMA with the weights in LDS.
#pragma once
#include "mfma_split.hpp"

namespace rs {
namespace {
// one thread = one (b, t_out) position x 4 output channels; weights packed [k][c_in][c_out4*4]
__global__ __launch_bounds__(256) void seq_conv_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const float* __restrict__ add,
                                                       float* __restrict__ y, int B, int T_in, int T_out, int c_in,
                                                       int c_out, int cq, int k, int stride, int pad, int relu) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)B * T_out * cq;
    if (g >= total) return;
    const int q = (int)(g % cq);
    const int64_t bt = g / cq;
    const int t = (int)(bt % T_out);
    const int b = (int)(bt / T_out);
    float4 acc = *reinterpret_cast<const float4*>(bias + 4 * q);
    for (int kk = 0; kk < k; ++kk) {
        const int ti = t * stride - pad + kk;
        if (ti < 0 || ti >= T_in) continue;
        const float* xr = x + ((int64_t)b * T_in + ti) * c_in;
        const float* wr = w + ((int64_t)kk * c_in) * (cq * 4) + 4 * q;
        for (int ci = 0; ci < c_in; ++ci) {
            const float xv = xr[ci];
            const float4 wv = *reinterpret_cast<const float4*>(wr + (int64_t)ci * (cq * 4));
            acc.x = fmaf(xv, wv.x, acc.x);
            acc.y = fmaf(xv, wv.y, acc.y);
            acc.z = fmaf(xv, wv.z, acc.z);
            acc.w = fmaf(xv, wv.w, acc.w);
        }
    }
    float o[4] = {acc.x, acc.y, acc.z, acc.w};
    const int64_t obase = ((int64_t)b * T_out + t) * c_out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int co = 4 * q + j;
        if (co < c_out) {
            float v = o[j];
            if (add) v += add[obase + co];
            if (relu) v = fmaxf(v, 0.0f);
            y[obase + co] = v;
        }
    }
}

// CONV on the f32-input MFMA: a 256-thread workgroup = 4 waves x (16 output rows x 16 * NT output channels)
template <int NT>
__global__ __launch_bounds__(256) void seq_conv_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, const float* __restrict__ add,
                                                            float* __restrict__ y, int B, int T_in, int T_out, int c_in,
                                                            int c_out, int wpitch, int K, int stride, int pad, int relu) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int64_t rows = (int64_t)B * T_out;
    const int64_t g = (int64_t)blockIdx.x * 64 + wave * 16 + r;          // the output row whose im2col row this lane feeds
    const bool row_ok = g < rows;
    const int b = row_ok ? (int)(g / T_out) : 0;
    const int t = row_ok ? (int)(g - (int64_t)b * T_out) : 0;
    const int off0 = (t * stride - pad) * c_in;                            // first element of the im2col row inside the element
    const int lim = T_in * c_in;
    const float* xb = x + (int64_t)b * lim;
    const int n0 = blockIdx.y * (16 * NT);
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int steps = (K + 3) / 4;
    constexpr int U = 4;                                                   // k-steps in flight
    for (int s0 = 0; s0 < steps; s0 += U) {
        float av[U], bv[U][NT];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kidx = 4 * (s0 + u) + kq;
            const int o = off0 + kidx;
            av[u] = (row_ok && kidx < K && o >= 0 && o < lim) ? xb[o] : 0.0f;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = n0 + 16 * j + r;
                bv[u][j] = (kidx < K && col < wpitch) ? w[(int64_t)kidx * wpitch + col] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u][j], acc[j], 0, 0, 0);
    }
    // accumulator element e of lane (col = lane & 15, row group = lane >> 4) is output row 4 * (lane >> 4) + e
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int col = n0 + 16 * j + r;
        if (col >= c_out) continue;
        const float bcol = bias[col];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + 4 * kq + e;
            if (row < rows) {
                float v = acc[j][e] + bcol;
                if (add) v += add[row * c_out + col];
                if (relu) v = fmaxf(v, 0.0f);
                y[row * c_out + col] = v;
            }
        }
    }
}

// CONV on the f32-input MFMA, weights resident in LDS: the layers of these nets are narrow (K * N * 4 bytes fits LDS
// many times over), so a persistent workgroup loads the whole packed weight matrix once - [K / 4][Npad][4], so that
// lane (column, k-group) reads the B operands of FOUR k-steps with one ds_read_b128 - and walks 128-row tiles of the
// GEMM: a wave owns 32 output rows x all Npad columns and per 16 K elements issues 2 (16-byte) loads of its im2col rows,
// NT ds_read_b128 and 8 * NT MFMAs.  The k index is permuted (lane kq of step 4u + i holds element 16u + 4kq + i) so
// that a lane's four A values of a 16-element chunk are one contiguous 16-byte load of the position-major input.
template <int NT>
__global__ __launch_bounds__(256) void seq_conv_mfma_lds_kernel(const float* __restrict__ x, unsigned x_bytes,
                                                                const float* __restrict__ wq /* [K16/4][16 NT][4] */,
                                                                const float* __restrict__ bias, const float* __restrict__ add,
                                                                float* __restrict__ y, int B, int T_in, int T_out, int c_in,
                                                                int c_out, int K, int stride, int pad, int relu, int n_tiles) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    constexpr int NP = 16 * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int K16 = (K + 15) & ~15;
    for (int i = threadIdx.x; i < K16 / 4 * NP; i += 256)
        reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(wq)[i];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, x_bytes, 0x00020000);
    const int64_t rows = (int64_t)B * T_out;
    const int lim = T_in * c_in;
    float bcol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bcol[j] = 16 * j + r < c_out ? bias[16 * j + r] : 0.0f;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row0 = (int64_t)tile * 128 + wave * 32;
        int off0[2];
        int64_t base[2];
        bool ok[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int64_t g = row0 + 16 * m + r;
            ok[m] = g < rows;
            const int b = ok[m] ? (int)(g / T_out) : 0;
            const int t = ok[m] ? (int)(g - (int64_t)b * T_out) : 0;
            off0[m] = (t * stride - pad) * c_in;
            base[m] = (int64_t)b * lim;
        }
        f32x4 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        // this lane's four im2col elements of rows m = 0, 1 for the chunk at k0 (the next chunk is loaded ahead of the
        // current chunk's MFMAs: the loop is otherwise bound by the round trip of these loads)
        auto load_a = [&](int k0, f32x4 (&av)[2]) {
            const int kidx = k0 + 4 * kq;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int o = off0[m] + kidx;
                if (ok[m] && o >= 0 && o + 3 < lim && kidx + 3 < K) {
                    av[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((base[m] + o) * 4), 0, 0));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        av[m][i] = (ok[m] && kidx + i < K && o + i >= 0 && o + i < lim) ? x[base[m] + o + i] : 0.0f;
                }
            }
        };
        f32x4 av[2], avn[2];
        load_a(0, av);
        for (int k0 = 0; k0 < K16; k0 += 16) {
            f32x4 bv[NT];
            if (k0 + 16 < K16) load_a(k0 + 16, avn);
#pragma unroll
            for (int j = 0; j < NT; ++j) bv[j] = *reinterpret_cast<const f32x4*>(wl + ((k0 / 4 + kq) * NP + 16 * j + r) * 4);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int m = 0; m < 2; ++m)
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][i], bv[j][i], acc[m][j], 0, 0, 0);
            av[0] = avn[0];
            av[1] = avn[1];
        }
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = 16 * j + r;
                if (col >= c_out) continue;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t row = row0 + 16 * m + 4 * kq + e;
                    if (row < rows) {
                        float v = acc[m][j][e] + bcol[j];
                        if (add) v += add[row * c_out + col];
                        if (relu) v = fmaxf(v, 0.0f);
                        y[row * c_out + col] = v;
                    }
                }
            }
    }
}
}  // namespace
}  // namespace rs
