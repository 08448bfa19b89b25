// Sequential conv programs (seqnet.hip): the fused residual basic block, fp32 and split precision (bf16x3).
#pragma once
#include <type_traits>

#include "mfma_split.hpp"

namespace rs {
namespace {
struct BlockArgs {
    const float* x;           // [B][T_in][c_in]
    unsigned x_bytes;
    float* y;                 // [B][T_out][c_out]
    const float* w1q;         // [K1_16 / 4][NPs][4], K index = tap * c_in + c
    const float* b1;          // [16 NT]
    const float* w2q;         // [K2_16 / 4][NPs][4], K index = tap * Cp + c for the 3x3 part, K2a16 + c for the 1x1 shortcut
    const float* b2;          // [16 NT] (the shortcut conv's bias included)
    int NPs;                  // column pitch of the weight matrices: c_out rounded up to 4 (the columns behind it are zeros
                              // that a lane takes from a register, not from LDS)
    int B, T_in, T_out, c_in, c_out, Cp, stride;
    int K1, K2a, Ksc;         // 3 c_in; 3 Cp; c_in if the shortcut is a conv, else 0 (identity: c_in == c_out, stride 1)
    int tiles_per_read, n_tiles;
    // RAGGED batches (rs_seqnet_forward_ragged): rows of read b valid in x / in y, or null = T_in / T_out for every read.  The
    // buffers keep the uniform row pitches T_in / T_out (those of the longest read); a read's tiles behind its own end are skipped
    const int32_t* tin;
    const int32_t* tout;
};

template <int NT, int MTW, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void seq_basic_block_kernel(const BlockArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int NP = a.NPs;
    constexpr int R = 16 * MTW * WAVES;            // rows of the intermediate tile (WAVES waves x MTW x 16)
    constexpr int kThr = 64 * WAVES;
    constexpr int TO = R - 2;                      // output positions per tile
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int K1_16 = (a.K1 + 15) & ~15, K2a16 = (a.K2a + 15) & ~15, Ksc16 = (a.Ksc + 15) & ~15;
    float* wl1 = lds;
    float* wl2 = wl1 + K1_16 * NP;
    float* tl = wl2 + (K2a16 + Ksc16) * NP;        // [(R + 4)][Cp]: row j = intermediate position to0 - 1 + j; 4 zero rows behind
    for (int i = threadIdx.x; i < K1_16 / 4 * NP; i += kThr)
        reinterpret_cast<f32x4*>(wl1)[i] = reinterpret_cast<const f32x4*>(a.w1q)[i];
    for (int i = threadIdx.x; i < (K2a16 + Ksc16) / 4 * NP; i += kThr)
        reinterpret_cast<f32x4*>(wl2)[i] = reinterpret_cast<const f32x4*>(a.w2q)[i];
    for (int i = threadIdx.x; i < (R + 4) * a.Cp; i += kThr) tl[i] = 0.0f;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const int lim_max = a.T_in * a.c_in;              // row pitch of a read in x (the longest read's)
    float b1c[NT], b2c[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        b1c[j] = a.b1[16 * j + r];
        b2c[j] = a.b2[16 * j + r];
    }
    // EDGE = false: a tile whose every intermediate row, output and x access lies inside its read (all but the first
    // and the last tiles of a read): no per-row masks, no bounds tests in front of the loads - in fp32 every such VALU
    // instruction is issue time next to the MFMAs, not hidden behind them
    auto do_tile = [&](int tile, auto EDGE_) {
        constexpr bool EDGE = decltype(EDGE_)::value;
        const int b = tile / a.tiles_per_read;
        const int to0 = (tile - b * a.tiles_per_read) * TO;
        const int64_t xbase = (int64_t)b * lim_max;
        const int T_in = a.tin ? as_const_len(a.tin)[b] : a.T_in, T_out = a.tout ? as_const_len(a.tout)[b] : a.T_out;
        const int lim = T_in * a.c_in;                     // elements of read b that hold data
        // ---- phase 1: the intermediate rows j = 0 .. R-1 (positions to0 - 1 + j) = relu(conv3(x; stride) + b1) -> LDS ----
        {
            int off0[MTW];
            bool ok[MTW];
#pragma unroll
            for (int m = 0; m < MTW; ++m) {
                const int p = to0 - 1 + (wave * MTW + m) * 16 + r;
                ok[m] = !EDGE || (p >= 0 && p < T_out);
                off0[m] = (p * a.stride - 1) * a.c_in;
            }
            f32x4 acc[MTW][NT];
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            auto load_a = [&](int k0, f32x4 (&av)[MTW]) {
                const int kidx = k0 + 4 * kq;
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const int o = off0[m] + kidx;
                    // (elements at K index >= K1 meet zero weights: inside the read they need no mask)
                    if (!EDGE || (ok[m] && o >= 0 && o + 3 < lim)) {
                        av[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((xbase + o) * 4), 0, 0));
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            av[m][i] = (ok[m] && kidx + i < a.K1 && o + i >= 0 && o + i < lim) ? a.x[xbase + o + i] : 0.0f;
                    }
                }
            };
            f32x4 av[MTW], avn[MTW];
            load_a(0, av);
            for (int k0 = 0; k0 < K1_16; k0 += 16) {
                f32x4 bv[NT];
                if (k0 + 16 < K1_16) load_a(k0 + 16, avn);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    bv[j] = 16 * j + r < NP ? *reinterpret_cast<const f32x4*>(wl1 + ((k0 / 4 + kq) * NP + 16 * j + r) * 4)
                                            : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int m = 0; m < MTW; ++m)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][i], bv[j][i], acc[m][j], 0, 0, 0);
#pragma unroll
                for (int m = 0; m < MTW; ++m) av[m] = avn[m];
            }
            // rows outside [0, T_out) are the second conv's zero padding; channels >= c_out of a row stay zero
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int jrow = (wave * MTW + m) * 16 + 4 * kq + e;
                    const int p = to0 - 1 + jrow;
                    const bool okp = !EDGE || (p >= 0 && p < T_out);
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int col = 16 * j + r;
                        if (col < a.c_out) tl[jrow * a.Cp + col] = okp ? fmaxf(acc[m][j][e] + b1c[j], 0.0f) : 0.0f;
                    }
                }
        }
        __syncthreads();
        // ---- phase 2: output rows i = 0 .. TO-1 (positions to0 + i): conv3 over LDS rows i .. i+2 (+ the 1x1 shortcut) ----
        {
            f32x4 acc[MTW][NT];
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* trow[MTW];
#pragma unroll
            for (int m = 0; m < MTW; ++m) trow[m] = tl + ((wave * MTW + m) * 16 + r) * a.Cp + 4 * kq;
            for (int k0 = 0; k0 < K2a16; k0 += 16) {
                f32x4 bv[NT], av[MTW];
#pragma unroll
                for (int m = 0; m < MTW; ++m) av[m] = *reinterpret_cast<const f32x4*>(trow[m] + k0);
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    bv[j] = 16 * j + r < NP ? *reinterpret_cast<const f32x4*>(wl2 + ((k0 / 4 + kq) * NP + 16 * j + r) * 4)
                                            : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int m = 0; m < MTW; ++m)
#pragma unroll
                        for (int j = 0; j < NT; ++j)
                            acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][i], bv[j][i], acc[m][j], 0, 0, 0);
            }
            if (a.Ksc) {                                             // 1x1 shortcut conv: x[(to0 + i) * stride][0 .. c_in)
                int off0[MTW];
                bool ok[MTW];
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const int i = (wave * MTW + m) * 16 + r;
                    ok[m] = i < TO && (!EDGE || to0 + i < T_out);
                    off0[m] = (to0 + i) * a.stride * a.c_in;
                }
                auto load_sc = [&](int k0, f32x4 (&av)[MTW]) {
                    const int kidx = k0 + 4 * kq;
#pragma unroll
                    for (int m = 0; m < MTW; ++m) {
                        const int o = off0[m] + kidx;
                        if (ok[m] && (!EDGE || o + 3 < lim)) {
                            av[m] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((xbase + o) * 4), 0, 0));
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i) av[m][i] = (ok[m] && kidx + i < a.Ksc && o + i < lim) ? a.x[xbase + o + i] : 0.0f;
                        }
                    }
                };
                f32x4 av[MTW], avn[MTW];
                load_sc(0, av);
                for (int k0 = 0; k0 < Ksc16; k0 += 16) {
                    f32x4 bv[NT];
                    if (k0 + 16 < Ksc16) load_sc(k0 + 16, avn);
#pragma unroll
                    for (int j = 0; j < NT; ++j)
                        bv[j] = 16 * j + r < NP ? *reinterpret_cast<const f32x4*>(wl2 + (((K2a16 + k0) / 4 + kq) * NP + 16 * j + r) * 4)
                                                : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int m = 0; m < MTW; ++m)
#pragma unroll
                            for (int j = 0; j < NT; ++j)
                                acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][i], bv[j][i], acc[m][j], 0, 0, 0);
#pragma unroll
                    for (int m = 0; m < MTW; ++m) av[m] = avn[m];
                }
            }
            // ---- output through an fp32 IMAGE of the tile's outputs in LDS (round 5, as seq_basic_block_x3_kernel does): the
            // tile's outputs are ONE contiguous span of y, a lane holds one channel of four rows - direct stores are 4 bytes wide
            // in 64-byte segments.  The image aliases the intermediate tile (read by nobody behind the barrier; what it leaves in
            // the tile's padding channels and rows is finite fp32 that meets zero weights), offset by `mis` floats so that image
            // and span share their 16-byte phase; an identity shortcut's residual is the same span of x, added in the copy-out.
            __syncthreads();
            const int n_out = min(TO, T_out - to0);
            const int64_t s0 = ((int64_t)b * a.T_out + to0) * a.c_out;
            const int mis = (int)(s0 & 3);
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = (wave * MTW + m) * 16 + 4 * kq + e;
                    if (i >= n_out) continue;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int col = 16 * j + r;
                        if (col < a.c_out) tl[mis + i * a.c_out + col] = acc[m][j][e] + b2c[j];
                    }
                }
            __syncthreads();
            {
                const int n_f = n_out * a.c_out;
                const int n_q = (mis + n_f + 3) >> 2;
                const float* xres = a.x + xbase + (int64_t)to0 * a.c_in - mis;
                float* ydst = a.y + (s0 - mis);
                for (int q = threadIdx.x; q < n_q; q += kThr) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(tl + 4 * q);
                    const int lo = 4 * q - mis;
                    if (lo >= 0 && lo + 3 < n_f) {
                        if (!a.Ksc) v += *reinterpret_cast<const f32x4*>(xres + 4 * q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.0f);
                        *reinterpret_cast<f32x4*>(ydst + 4 * q) = v;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (lo + i >= 0 && lo + i < n_f) {
                                float w = v[i];
                                if (!a.Ksc) w += xres[4 * q + i];
                                ydst[4 * q + i] = fmaxf(w, 0.0f);
                            }
                    }
                }
            }
        }
        __syncthreads();                                             // the next tile's phase 1 overwrites the LDS tile
    };
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int tt = tile % a.tiles_per_read;
        const int to0 = tt * TO;
        const int bb = tile / a.tiles_per_read;
        const int T_in = a.tin ? as_const_len(a.tin)[bb] : a.T_in, T_out = a.tout ? as_const_len(a.tout)[bb] : a.T_out;
        if (to0 >= T_out) continue;                            // ragged batch: this read ended before the tile
        const bool interior = to0 >= 2 && to0 + TO <= T_out && (to0 + R - 2) * a.stride + 6 <= T_in;
        if (interior)
            do_tile(tile, std::false_type{});
        else
            do_tile(tile, std::true_type{});
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The same residual basic block in SPLIT PRECISION on the bf16 MFMA (rs_seqnet_set_mode(m, RS_BF16X3); BASELINE.json's
// north_star names "the nets/ 1D-ResNet forward pass ... im2col -> MFMA bf16").  Arithmetic of conv_ring_h16.hip: every
// activation and weight is a pair hi = bf16(v), lo = bf16(v - hi); a product is hi*hi + lo*hi + hi*lo on three
// v_mfma_f32_16x16x32_bf16 with fp32 accumulate (~2^-17 per operand).  What changes against the fp32 kernel above:
//   * a k-step is 32 K elements: lane (row r, k-group kq) supplies K elements 8 kq .. 8 kq + 7 - eight CONSECUTIVE floats of the
//     position's im2col run (two 16-byte loads), split into a hi and a lo fragment in registers (24 VALU per fragment, shared by
//     the NT column tiles);
//   * the weights are split on the host and live in LDS as two planes [k-step][kq][n][8 x bf16] (a 16-lane group reads 256
//     contiguous bytes: conflict-free ds_read_b128), the same 4 bytes per (k, n) as the fp32 matrices;
//   * the intermediate tile is stored ALREADY SPLIT (two bf16 planes [row][Cp]): phase 2 reads its fragments with two
//     ds_read_b128 and converts nothing.  Cp = 8 (mod 16) halfwords keeps those reads 16-byte aligned and the 16 rows of a group
//     on distinct banks (row pitch 12 / 20 / 28 / 36 dwords);
//   * activations between blocks stay fp32 in HBM (x in, y out, as before).
// 3 MFMAs of 16 cycles per 32 K elements and accumulator tile against 8 of 32 cycles: 5.3 x less matrix-pipe time; the
// kernel becomes bound by the split's VALU work and its loads.
struct BlockX3Args {
    const float* x;
    unsigned x_bytes;
    float* y;
    const unsigned short* w1;  // planes [hi | lo], each [S1][4][NPs][8]
    const float* b1;
    const unsigned short* w2;  // planes [hi | lo], each [S2a + Ssc][4][NPs][8]; the shortcut's k-steps behind the 3x3 conv's
    const float* b2;
    int NPs;
    int B, T_in, T_out, c_in, c_out, Cp, stride;
    int K1, Ksc;               // 3 c_in; c_in if the shortcut is a conv, else 0
    int S1, S2a, Ssc;          // k-steps of 32: ceil(3 c_in / 32), ceil(3 Cp / 32), ceil(Ksc / 32)
    int tiles_per_read, n_tiles;
    const int32_t* tin;        // ragged batches: see BlockArgs
    const int32_t* tout;
};

template <int NT, int MTW, int WAVES>
// (launch bound 512 also for the four-wave form: with 256 the compiler keeps MFMA accumulators in AGPRs and copies them in
// and out - 192 extra instructions around the 72 MFMAs of a <2, 2, 4> tile; worth 1 % here, 17 % in conv_wino4.hip's thin shapes)
__global__ __launch_bounds__(512) void seq_basic_block_x3_kernel(const BlockX3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds8[];
    const int NP = a.NPs;
    constexpr int R = 16 * MTW * WAVES;
    constexpr int kThr = 64 * WAVES;
    constexpr int TO = R - 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int S2 = a.S2a + a.Ssc;
    const int w1_plane = a.S1 * 4 * NP * 8, w2_plane = S2 * 4 * NP * 8;          // halfwords per plane
    unsigned short* wl1 = reinterpret_cast<unsigned short*>(lds8);                // [hi plane | lo plane]
    unsigned short* wl2 = wl1 + 2 * w1_plane;
    unsigned short* tlh = wl2 + 2 * w2_plane;                                     // [(R + 4)][Cp] hi, then the same lo
    unsigned short* tll = tlh + (R + 4) * a.Cp;
    for (int i = threadIdx.x; i < 2 * w1_plane / 8; i += kThr)
        reinterpret_cast<u32x4*>(wl1)[i] = reinterpret_cast<const u32x4*>(a.w1)[i];
    for (int i = threadIdx.x; i < 2 * w2_plane / 8; i += kThr)
        reinterpret_cast<u32x4*>(wl2)[i] = reinterpret_cast<const u32x4*>(a.w2)[i];
    for (int i = threadIdx.x; i < 2 * (R + 4) * a.Cp / 2; i += kThr) reinterpret_cast<unsigned*>(tlh)[i] = 0u;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const int lim_max = a.T_in * a.c_in;              // row pitch of a read in x (the longest read's)
    float b1c[NT], b2c[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        b1c[j] = a.b1[16 * j + r];
        b2c[j] = a.b2[16 * j + r];
    }
    // weight fragments of k-step s: column 16 j + r, k-group kq; columns behind the compact pitch are zeros from a register
    auto load_b = [&](const unsigned short* w, int plane, int s, u32x4 (&bh)[NT], u32x4 (&bl)[NT]) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = 16 * j + r;
            if (n < NP) {
                const unsigned short* q = w + ((s * 4 + kq) * NP + n) * 8;
                bh[j] = *reinterpret_cast<const u32x4*>(q);
                bl[j] = *reinterpret_cast<const u32x4*>(q + plane);
            } else {
                bh[j] = (u32x4){0u, 0u, 0u, 0u};
                bl[j] = (u32x4){0u, 0u, 0u, 0u};
            }
        }
    };
    auto do_tile = [&](int tile, auto EDGE_) {
        constexpr bool EDGE = decltype(EDGE_)::value;
        const int b = tile / a.tiles_per_read;
        const int to0 = (tile - b * a.tiles_per_read) * TO;
        const int64_t xbase = (int64_t)b * lim_max;
        const int T_in = a.tin ? as_const_len(a.tin)[b] : a.T_in, T_out = a.tout ? as_const_len(a.tout)[b] : a.T_out;
        const int lim = T_in * a.c_in;                     // elements of read b that hold data
        // eight consecutive floats of x from element offset o of read b (zeros outside the read; inside it every element is
        // real data - K indices behind the conv's own meet zero weights)
        auto load8 = [&](bool ok, int o, int klim, int kidx, f32x4& lo4, f32x4& hi4) {
            if (!EDGE || (ok && o >= 0 && o + 7 < lim)) {
                lo4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((xbase + o) * 4), 0, 0));
                hi4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((xbase + o) * 4 + 16), 0, 0));
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    lo4[i] = (ok && kidx + i < klim && o + i >= 0 && o + i < lim) ? a.x[xbase + o + i] : 0.0f;
                    hi4[i] = (ok && kidx + 4 + i < klim && o + 4 + i >= 0 && o + 4 + i < lim) ? a.x[xbase + o + 4 + i] : 0.0f;
                }
            }
        };
        // ---- phase 1: the intermediate rows j = 0 .. R-1 (positions to0 - 1 + j) = relu(conv3(x; stride) + b1) -> LDS, split ----
        {
            int off0[MTW];
            bool ok[MTW];
#pragma unroll
            for (int m = 0; m < MTW; ++m) {
                const int p = to0 - 1 + (wave * MTW + m) * 16 + r;
                ok[m] = !EDGE || (p >= 0 && p < T_out);
                off0[m] = (p * a.stride - 1) * a.c_in;
            }
            f32x4 acc[MTW][NT];
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            f32x4 xa[MTW], xb[MTW], xan[MTW], xbn[MTW];
#pragma unroll
            for (int m = 0; m < MTW; ++m) load8(ok[m], off0[m] + 8 * kq, a.K1, 8 * kq, xa[m], xb[m]);
            for (int s = 0; s < a.S1; ++s) {
                if (s + 1 < a.S1) {
#pragma unroll
                    for (int m = 0; m < MTW; ++m)
                        load8(ok[m], off0[m] + 32 * (s + 1) + 8 * kq, a.K1, 32 * (s + 1) + 8 * kq, xan[m], xbn[m]);
                }
                u32x4 bh[NT], bl[NT];
                load_b(wl1, w1_plane, s, bh, bl);
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    u32x4 ah, al;
                    split8(xa[m], xb[m], ah, al);
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[m][j] = mfma_x3(ah, al, bh[j], bl[j], acc[m][j]);
                }
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    xa[m] = xan[m];
                    xb[m] = xbn[m];
                }
            }
            // rows outside [0, T_out) are the second conv's zero padding; channels >= c_out of a row stay zero.  A lane holds
            // one channel of four rows: neighbouring lanes (channels c, c + 1) exchange two values by DPP so that the even lane
            // owns the channel PAIR of rows 0 and 1 and the odd lane that of rows 2 and 3 - a dword per row and plane instead of
            // two halfwords
            const bool odd = r & 1;
#pragma unroll
            for (int m = 0; m < MTW; ++m) {
                const int jrow0 = (wave * MTW + m) * 16 + 4 * kq;
                bool okp[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) okp[e] = !EDGE || (to0 - 1 + jrow0 + e >= 0 && to0 - 1 + jrow0 + e < T_out);
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int col = 16 * j + r;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (okp[e] && col < a.c_out) ? fmaxf(acc[m][j][e] + b1c[j], 0.0f) : 0.0f;
                    const float g02 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, odd ? v[0] : v[2]), 0xB1, 0xF, 0xF, true));
                    const float g13 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, odd ? v[1] : v[3]), 0xB1, 0xF, 0xF, true));
                    const int c2 = 16 * j + (r & ~1);
                    if (c2 < a.c_out) {
                        // even lane: rows 0, 1 = (own, neighbour's); odd lane: rows 2, 3 = (neighbour's, own)
                        const float a0 = odd ? g02 : v[0], b0 = odd ? v[2] : g02;
                        const float a1 = odd ? g13 : v[1], b1 = odd ? v[3] : g13;
                        const int at = (jrow0 + (odd ? 2 : 0)) * a.Cp + c2;
                        const unsigned h0 = pack_bf16x2(a0, b0), h1 = pack_bf16x2(a1, b1);
                        *reinterpret_cast<unsigned*>(tlh + at) = h0;
                        *reinterpret_cast<unsigned*>(tlh + at + a.Cp) = h1;
                        *reinterpret_cast<unsigned*>(tll + at) =
                            pack_bf16x2(a0 - __builtin_bit_cast(float, h0 << 16), b0 - __builtin_bit_cast(float, h0 & 0xffff0000u));
                        *reinterpret_cast<unsigned*>(tll + at + a.Cp) =
                            pack_bf16x2(a1 - __builtin_bit_cast(float, h1 << 16), b1 - __builtin_bit_cast(float, h1 & 0xffff0000u));
                    }
                }
            }
        }
        __syncthreads();
        // ---- phase 2: output rows i = 0 .. TO-1 (positions to0 + i): conv3 over LDS rows i .. i+2 (+ the 1x1 shortcut) ----
        {
            f32x4 acc[MTW][NT];
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            int trow[MTW];                                   // halfword index of the lane's fragment in a tile plane
#pragma unroll
            for (int m = 0; m < MTW; ++m) trow[m] = ((wave * MTW + m) * 16 + r) * a.Cp + 8 * kq;
            for (int s = 0; s < a.S2a; ++s) {
                u32x4 bh[NT], bl[NT];
                load_b(wl2, w2_plane, s, bh, bl);
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const u32x4 ah = *reinterpret_cast<const u32x4*>(tlh + trow[m] + 32 * s);
                    const u32x4 al = *reinterpret_cast<const u32x4*>(tll + trow[m] + 32 * s);
#pragma unroll
                    for (int j = 0; j < NT; ++j) acc[m][j] = mfma_x3(ah, al, bh[j], bl[j], acc[m][j]);
                }
            }
            if (a.Ksc) {                                             // 1x1 shortcut conv: x[(to0 + i) * stride][0 .. c_in)
                int off0[MTW];
                bool ok[MTW];
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const int i = (wave * MTW + m) * 16 + r;
                    ok[m] = i < TO && (!EDGE || to0 + i < T_out);
                    off0[m] = (to0 + i) * a.stride * a.c_in;
                }
                for (int s = 0; s < a.Ssc; ++s) {
                    u32x4 bh[NT], bl[NT];
                    load_b(wl2, w2_plane, a.S2a + s, bh, bl);
#pragma unroll
                    for (int m = 0; m < MTW; ++m) {
                        f32x4 xa, xb;
                        // a row past the tile's outputs (i >= TO) is never stored: it may read anything finite - keep it zero
                        if (ok[m] || !EDGE) {
                            if (ok[m])
                                load8(true, off0[m] + 32 * s + 8 * kq, a.Ksc, 32 * s + 8 * kq, xa, xb);
                            else
                                xa = xb = (f32x4){0.f, 0.f, 0.f, 0.f};
                        } else {
                            xa = xb = (f32x4){0.f, 0.f, 0.f, 0.f};
                        }
                        u32x4 ah, al;
                        split8(xa, xb, ah, al);
#pragma unroll
                        for (int j = 0; j < NT; ++j) acc[m][j] = mfma_x3(ah, al, bh[j], bl[j], acc[m][j]);
                    }
                }
            }
            // ---- output: through an fp32 IMAGE of the tile's outputs in LDS, so that the tile leaves in coalesced 16-byte
            // pieces.  y[b][to0 .. to0 + n_out)[0 .. c_out) is ONE contiguous span of memory (rows hold exactly c_out floats), a
            // lane of the accumulator holds one channel of four rows: direct stores are 4 bytes wide in 64-byte segments.  The
            // image aliases the intermediate tile (every wave has finished reading it behind the barrier); it starts `mis` floats
            // in, so that image float 4 q and global float (s0 - mis) + 4 q are both 16-byte aligned.  An identity shortcut's
            // residual is the same span of x (c_in == c_out, stride 1): it is added in the copy-out, from coalesced loads.
            __syncthreads();
            float* img = reinterpret_cast<float*>(tlh);
            const int n_out = min(TO, T_out - to0);                                  // valid output rows of this tile
            const int64_t s0 = ((int64_t)b * a.T_out + to0) * a.c_out;                 // first float of the span in y
            const int mis = (int)(s0 & 3);
#pragma unroll
            for (int m = 0; m < MTW; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = (wave * MTW + m) * 16 + 4 * kq + e;
                    if (i >= n_out) continue;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int col = 16 * j + r;
                        if (col < a.c_out) img[mis + i * a.c_out + col] = acc[m][j][e] + b2c[j];
                    }
                }
            __syncthreads();
            {
                const int n_f = n_out * a.c_out;                                       // floats of the span
                const int n_q = (mis + n_f + 3) >> 2;                                  // 16-byte pieces that touch it
                const float* xres = a.x + xbase + (int64_t)to0 * a.c_in - mis;          // identity: same span, same phase
                float* ydst = a.y + (s0 - mis);
                for (int q = threadIdx.x; q < n_q; q += kThr) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(img + 4 * q);
                    const int lo = 4 * q - mis;                                        // span index of the piece's first float
                    if (lo >= 0 && lo + 3 < n_f) {
                        if (!a.Ksc) v += *reinterpret_cast<const f32x4*>(xres + 4 * q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = fmaxf(v[i], 0.0f);
                        *reinterpret_cast<f32x4*>(ydst + 4 * q) = v;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (lo + i >= 0 && lo + i < n_f) {
                                float w = v[i];
                                if (!a.Ksc) w += xres[4 * q + i];
                                ydst[4 * q + i] = fmaxf(w, 0.0f);
                            }
                    }
                }
            }
            __syncthreads();
            // the image overwrote zeros the tile must keep: its padding channels [c_out, Cp) and the 4 rows behind it (phase 2
            // multiplies them by zero weights - a float's halfword may be a bf16 NaN).  Phase 1 rewrites every (row < R,
            // channel < c_out) itself.
            {
                const int n_pad = a.Cp - a.c_out;
                for (int row = threadIdx.x; row < R + 4; row += kThr)
                    for (int c = a.c_out; c < a.Cp; ++c) {
                        tlh[row * a.Cp + c] = 0;
                        tll[row * a.Cp + c] = 0;
                    }
                for (int t = threadIdx.x; t < 4 * a.c_out; t += kThr) {
                    tlh[R * a.Cp + (t / a.c_out) * a.Cp + t % a.c_out] = 0;
                    tll[R * a.Cp + (t / a.c_out) * a.Cp + t % a.c_out] = 0;
                }
                (void)n_pad;
            }
        }
        // (no barrier here: the next tile's phase 1 writes rows < R x channels < c_out only, which nobody reads before its
        // own barrier, and the copy-out above ended with one)
    };
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int tt = tile % a.tiles_per_read;
        const int to0 = tt * TO;
        const int bb = tile / a.tiles_per_read;
        const int T_in = a.tin ? as_const_len(a.tin)[bb] : a.T_in, T_out = a.tout ? as_const_len(a.tout)[bb] : a.T_out;
        if (to0 >= T_out) continue;                            // ragged batch: this read ended before the tile
        const int lim = T_in * a.c_in;
        // interior: every intermediate row, output and x access (the k-steps' over-read of up to 31 elements included) lies
        // inside the read
        const bool interior = to0 >= 2 && to0 + TO <= T_out && ((to0 + R - 2) * a.stride + 2) * a.c_in + 32 * (a.S1 + 1) <= lim;
        if (interior)
            do_tile(tile, std::false_type{});
        else
            do_tile(tile, std::true_type{});
    }
}
}  // namespace
}  // namespace rs
