// Sequential conv programs (seqnet.hip): the fused stem (conv + ReLU + max-pool) in split precision (bf16x3).
#pragma once
#include "mfma_split.hpp"

namespace rs {
namespace {
// The stem (conv(1 -> C; k, stride, pad) + BN + ReLU + MaxPool1d(2, 2, padding 1), riser/nets/resnet.py:79-84) in the same split
// precision: the GEMM of seq_stem_pool_kernel with k-steps of 32 samples (a 19-tap stem is ONE k-step of three bf16 MFMAs
// instead of eight f32-input ones), the lane's eight consecutive samples split in registers.  Output through a WAVE-PRIVATE fp32
// image in LDS: a wave's 32 GEMM rows are 16 pooled rows = 16 c_out consecutive floats of y (pooled rows are contiguous across
// reads: g / 2 = b TP + p), always 64-byte aligned, stored 16 bytes per lane; LDS operations of one wave execute in order, so
// the image needs no barrier.
template <int NT>
__global__ __launch_bounds__(512) void seq_stem_pool_x3_kernel(const float* __restrict__ x, unsigned x_bytes,
                                                               const unsigned short* __restrict__ wq /* planes [hi | lo] [S][4][16 NT][8] */,
                                                               const float* __restrict__ bias, float* __restrict__ y, int B, int L,
                                                               int T_conv, int TP, int c_out, int K, int S, int stride, int pad,
                                                               int n_tiles,
        const int32_t* __restrict__ rlen /* ragged batches: samples of read b (null: L) */,
        const int32_t* __restrict__ rtconv /* ... and its conv positions (null: T_conv) */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds8[];
    constexpr int NP = 16 * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int plane = S * 4 * NP * 8;
    unsigned short* wl = reinterpret_cast<unsigned short*>(lds8);
    float* img = reinterpret_cast<float*>(lds8 + (size_t)2 * plane * 2) + wave * 16 * c_out;      // 16 pooled rows x c_out
    for (int i = threadIdx.x; i < 2 * plane / 8; i += 256) reinterpret_cast<u32x4*>(wl)[i] = reinterpret_cast<const u32x4*>(wq)[i];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, x_bytes, 0x00020000);
    const int rpr = 2 * TP;
    const int rows = B * rpr;
    const int64_t y_floats = (int64_t)B * TP * c_out;
    float bcol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bcol[j] = 16 * j + r < c_out ? bias[16 * j + r] : 0.0f;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row0 = tile * 128 + wave * 32;
        const int tb0 = __builtin_amdgcn_readfirstlane((tile * 128) / rpr);
        auto locate = [&](int g, int& b, int& j) {
            b = tb0;
            j = g - tb0 * rpr;
            while (j >= rpr) {
                j -= rpr;
                ++b;
            }
        };
        int off0[2], base[2], Lr[2];
        bool ok[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int g = row0 + 16 * m + r;
            int b, j;
            locate(g, b, j);
            const int tc = j - 1;
            const int bq = min(b, B - 1);
            Lr[m] = rlen ? rlen[bq] : L;
            ok[m] = g < rows && tc >= 0 && tc < (rtconv ? rtconv[bq] : T_conv);
            off0[m] = tc * stride - pad;
            base[m] = b * L;
        }
        const int jw = row0 - tb0 * rpr;
        const int bw = min(tb0, B - 1);                         // (wave-uniform: scalar loads)
        const int Lw = rlen ? as_const_len(rlen)[bw] : L, Tw = rtconv ? as_const_len(rtconv)[bw] : T_conv;
        const bool interior = row0 + 32 <= rows && jw >= 1 && jw + 32 <= rpr - 2 && jw + 31 <= Tw && (jw - 1) * stride - pad >= 0 &&
                              (jw + 31) * stride - pad + 32 * S + 8 < Lw;
        f32x4 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < S; ++s) {
            u32x4 bh[NT], bl[NT];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const unsigned short* q = wl + ((s * 4 + kq) * NP + 16 * j + r) * 8;
                bh[j] = *reinterpret_cast<const u32x4*>(q);
                bl[j] = *reinterpret_cast<const u32x4*>(q + plane);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int kidx = 32 * s + 8 * kq;
                const int o = off0[m] + kidx;
                f32x4 xa, xb;
                // (samples at K index >= K meet zero weights: inside the read they need no mask)
                if (interior || (ok[m] && o >= 0 && o + 7 < Lr[m])) {
                    xa = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)(base[m] + o) * 4u, 0, 0));
                    xb = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)(base[m] + o) * 4u + 16u, 0, 0));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        xa[i] = (ok[m] && kidx + i < K && o + i >= 0 && o + i < Lr[m]) ? x[(int64_t)base[m] + o + i] : 0.0f;
                        xb[i] = (ok[m] && kidx + 4 + i < K && o + 4 + i >= 0 && o + 4 + i < Lr[m]) ? x[(int64_t)base[m] + o + 4 + i] : 0.0f;
                    }
                }
                u32x4 ah, al;
                split8(xa, xb, ah, al);
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[m][j] = mfma_x3(ah, al, bh[j], bl[j], acc[m][j]);
            }
        }
        // lane (column r, row group kq) holds GEMM rows 4 kq + e: (e = 0, 1) and (2, 3) are pooling windows -> the wave's image
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                const int g = row0 + 16 * m + 4 * kq + e;              // even
                if (g >= rows) continue;
                int b, j0;
                locate(g, b, j0);
                const int ta = j0 - 1, tb = j0;                        // the window's conv positions (MaxPool pads with -inf)
                const int tcb = rtconv ? rtconv[min(b, B - 1)] : T_conv;
                const bool va = ta >= 0 && ta < tcb, vb = tb < tcb;
                float* ir = img + (8 * m + 2 * kq + (e >> 1)) * c_out;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int col = 16 * j + r;
                    if (col >= c_out) continue;
                    float v = -INFINITY;
                    if (va) v = fmaxf(v, acc[m][j][e] + bcol[j]);
                    if (vb) v = fmaxf(v, acc[m][j][e + 1] + bcol[j]);
                    ir[col] = fmaxf(v, 0.0f);                          // relu(max) == max(relu)
                }
            }
        {
            const int64_t f0 = (int64_t)(row0 >> 1) * c_out;           // first float of the wave's span in y
            const int n_q = 4 * c_out;                                 // 16 c_out floats in 16-byte pieces
            for (int q = lane; q < n_q; q += 64) {
                if (f0 + 4 * q + 3 < y_floats)
                    *reinterpret_cast<f32x4*>(y + f0 + 4 * q) = *reinterpret_cast<const f32x4*>(img + 4 * q);
                else
                    for (int i = 0; i < 4; ++i)
                        if (f0 + 4 * q + i < y_floats) y[f0 + 4 * q + i] = img[4 * q + i];
            }
        }
    }
}
}  // namespace
}  // namespace rs
