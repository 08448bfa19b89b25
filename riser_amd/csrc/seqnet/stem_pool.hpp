// Sequential conv programs (seqnet.hip): the fused stem (conv + ReLU + max-pool) in fp32.
#pragma once
#include "mfma_split.hpp"

namespace rs {
namespace {
// ---- fused residual block and fused stem (riser/nets/resnet.py:39-43,54-57,79-84) ------------------------------------
// The launch-per-conv program above moves every intermediate through HBM: a basic block reads its input three times
// (conv, shortcut, residual), writes and re-reads the intermediate.  The two kernels below are what rs_seqnet_create
// substitutes when it recognises the patterns build_program emits:
//
//   STEM   conv1d(1 -> C; k, stride, pad) + BN + ReLU -> MaxPool1d(2, 2, padding 1): the GEMM rows of a tile start at an
//          odd conv position, so a pooling pair is two accumulator registers of one lane and the un-pooled activations
//          never exist in memory.
//   BLOCK  y = relu( conv3(relu(conv3(x; stride) + b1)) + b2 + shortcut(x) ), shortcut = x or conv1(x; stride) + b:
//          a workgroup owns R - 2 output positions of one read; phase 1 computes the R rows of the intermediate they
//          need (one halo row each side) into LDS, phase 2 runs the second conv with its im2col rows read from that LDS
//          tile (a row of the tile is a run of the next conv's K index, exactly as in global memory) and the 1x1 shortcut
//          conv as extra K chunks of the same GEMM read from x; both weight matrices stay in LDS for the whole launch.
//          x is read once (plus the halo), y written once.
// Same MFMA orientation and K order as seq_conv_mfma_lds_kernel (so the intermediate has the bits the unfused program
// computes); fp32 throughout.

template <int NT>
__global__ __launch_bounds__(256) void seq_stem_pool_kernel(const float* __restrict__ x, unsigned x_bytes,
                                                            const float* __restrict__ wq, const float* __restrict__ bias,
                                                            float* __restrict__ y, int B, int L, int T_conv, int TP,
                                                            int c_out, int K, int stride, int pad, int n_tiles,
        const int32_t* __restrict__ rlen /* ragged batches: samples of read b (null: L) */,
        const int32_t* __restrict__ rtconv /* ... and its conv positions (null: T_conv) */) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    constexpr int NP = 16 * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int K16 = (K + 15) & ~15;
    for (int i = threadIdx.x; i < K16 / 4 * NP; i += 256)
        reinterpret_cast<f32x4*>(wl)[i] = reinterpret_cast<const f32x4*>(wq)[i];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, x_bytes, 0x00020000);
    // GEMM row g = b * 2 TP + j holds conv position j - 1 of read b: rows (2p, 2p + 1) are the window of pooled row p
    const int rpr = 2 * TP;
    const int rows = B * rpr;
    float bcol[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) bcol[j] = 16 * j + r < c_out ? bias[16 * j + r] : 0.0f;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row0 = tile * 128 + wave * 32;
        // (read, row in it) of a GEMM row: one division per tile, then a step or two (integer division per lane and row
        // cost more VALU time than the tile's MFMAs)
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
        // a wave whose 32 rows and all their samples lie inside one read takes the loads without bounds tests
        const int jw = row0 - tb0 * rpr;                        // first row of the wave in read tb0 (or beyond: then not interior)
        const int bw = min(tb0, B - 1);                         // (wave-uniform: scalar loads)
        const int Lw = rlen ? as_const_len(rlen)[bw] : L, Tw = rtconv ? as_const_len(rtconv)[bw] : T_conv;
        const bool interior = row0 + 32 <= rows && jw >= 1 && jw + 32 <= rpr - 2 && jw + 31 <= Tw && (jw - 1) * stride - pad >= 0 &&
                              (jw + 31) * stride - pad + K16 + 3 < Lw;
        f32x4 acc[2][NT];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        auto load_a = [&](int k0, f32x4 (&av)[2]) {
            const int kidx = k0 + 4 * kq;
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int o = off0[m] + kidx;
                // (elements at K index >= K meet zero weights: inside the read they need no mask)
                if (interior || (ok[m] && o >= 0 && o + 3 < Lr[m])) {
                    av[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)(base[m] + o) * 4u, 0, 0));
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        av[m][i] = (ok[m] && kidx + i < K && o + i >= 0 && o + i < Lr[m]) ? x[(int64_t)base[m] + o + i] : 0.0f;
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
        // lane (column r, row group kq) holds GEMM rows 4 kq + e: (e = 0, 1) and (2, 3) are pooling windows
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
                float* yr = y + ((int64_t)b * TP + (j0 >> 1)) * c_out;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int col = 16 * j + r;
                    if (col >= c_out) continue;
                    float v = -INFINITY;
                    if (va) v = fmaxf(v, acc[m][j][e] + bcol[j]);
                    if (vb) v = fmaxf(v, acc[m][j][e + 1] + bcol[j]);
                    yr[col] = fmaxf(v, 0.0f);                          // relu(max) == max(relu)
                }
            }
    }
}
}  // namespace
}  // namespace rs
