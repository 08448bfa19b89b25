// Sequential conv programs (seqnet.hip): the fused residual bottleneck block, fp32 and split precision (bf16x3).
#pragma once
#include "mfma_split.hpp"

namespace rs {
namespace {
// BOTTLENECK block (riser/nets/resnet.py:60-70): y = relu( conv1(relu(conv3(relu(conv1(x) + b1); stride) + b2)) + b3 +
// shortcut(x) ) in one launch, three GEMM phases with two LDS tiles between them:
//   A  t1 = relu(conv1x1(x) + b1) for the RA = 128 input positions (to0 * stride - 1 ..) the tile's 3x3 conv reads (zero
//      rows outside the read: the 3x3 conv's padding), A operand = rows of x;
//   B  t2 = relu(conv3(t1; stride) + b2) for the tile's R2 = (RA - 3) / stride + 1 outputs (126 / 63): the im2col row of
//      output i is the run of three t1 rows from row i * stride of the LDS tile;
//   C  y = relu(conv1x1(t2) + b3 + shortcut): rows of the t2 tile, the 1x1 shortcut conv as extra K chunks read from x
//      (or the identity residual).
// All three weight matrices stay in LDS; x is read once (plus one halo row each side), y written once.
struct BneckArgs {
    const float* x;
    unsigned x_bytes;
    float* y;
    const float *w1q, *b1, *w2q, *b2, *w3q, *b3;   // [K16 / 4][NP][4] packings, biases padded to 16 NT
    int NPm, NPo;             // column pitches of the mid / out weight matrices
    int B, T_in, T_out, c_in, c_mid, c_out, Cmp, stride;
    int Ksc;                  // c_in if the shortcut is a conv, else 0
    int R2, tiles_per_read, n_tiles;
    const int32_t* tin;       // ragged batches: rows of read b valid in x / in y (null: T_in / T_out); see BlockArgs
    const int32_t* tout;
};

template <int NTM, int NTO>
__global__ __launch_bounds__(256) void seq_bottleneck_block_kernel(const BneckArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int RA = 128;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int K1_16 = (a.c_in + 15) & ~15, K2_16 = (3 * a.Cmp + 15) & ~15, K3_16 = (a.Cmp + 15) & ~15, Ksc16 = (a.Ksc + 15) & ~15;
    float* wl1 = lds;
    float* wl2 = wl1 + K1_16 * a.NPm;
    float* wl3 = wl2 + K2_16 * a.NPm;
    float* t1 = wl3 + (K3_16 + Ksc16) * a.NPo;     // [RA + 4][Cmp]
    float* t2 = t1 + (RA + 4) * a.Cmp;             // [RA + 4][Cmp]
    for (int i = threadIdx.x; i < K1_16 / 4 * a.NPm; i += 256) reinterpret_cast<f32x4*>(wl1)[i] = reinterpret_cast<const f32x4*>(a.w1q)[i];
    for (int i = threadIdx.x; i < K2_16 / 4 * a.NPm; i += 256) reinterpret_cast<f32x4*>(wl2)[i] = reinterpret_cast<const f32x4*>(a.w2q)[i];
    for (int i = threadIdx.x; i < (K3_16 + Ksc16) / 4 * a.NPo; i += 256)
        reinterpret_cast<f32x4*>(wl3)[i] = reinterpret_cast<const f32x4*>(a.w3q)[i];
    for (int i = threadIdx.x; i < 2 * (RA + 4) * a.Cmp; i += 256) t1[i] = 0.0f;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const int lim_max = a.T_in * a.c_in;              // row pitch of a read in x (the longest read's)
    int lim = lim_max, T_in = a.T_in, T_out = a.T_out;   // of the read a tile belongs to (set per tile)
    float b1c[NTM], b2c[NTM], b3c[NTO];
#pragma unroll
    for (int j = 0; j < NTM; ++j) {
        b1c[j] = a.b1[16 * j + r];
        b2c[j] = a.b2[16 * j + r];
    }
#pragma unroll
    for (int j = 0; j < NTO; ++j) b3c[j] = a.b3[16 * j + r];
    const int n_mt = (a.R2 + 15) / 16;             // 16-row tiles of phases B and C (8 or 4)
    auto wfrag = [&](const float* wl, int NP, int k0, int j) -> f32x4 {
        return 16 * j + r < NP ? *reinterpret_cast<const f32x4*>(wl + ((k0 / 4 + kq) * NP + 16 * j + r) * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    };
    // a lane's four consecutive x values at element o of the read (zero outside it), K index kidx .. kidx + 3 of Klim
    auto xload = [&](int64_t xbase, bool ok, int o, int kidx, int Klim) -> f32x4 {
        if (ok && o >= 0 && o + 3 < lim)
            return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((xbase + o) * 4), 0, 0));
        f32x4 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (ok && kidx + i < Klim && o + i >= 0 && o + i < lim) ? a.x[xbase + o + i] : 0.0f;
        return v;
    };
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int b = tile / a.tiles_per_read;
        const int to0 = (tile - b * a.tiles_per_read) * a.R2;
        const int64_t xbase = (int64_t)b * lim_max;
        if (a.tin) {
            T_in = as_const_len(a.tin)[b];
            T_out = as_const_len(a.tout)[b];
            lim = T_in * a.c_in;
        }
        if (to0 >= T_out) continue;                            // ragged batch: this read ended before the tile
        // ---- phase A: t1 rows j = 0 .. RA-1 <-> input positions q0 + j ------------------------------------------------
        {
            const int q0 = to0 * a.stride - 1;
            f32x4 acc[2][NTM];
            int off0[2];
            bool ok[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int q = q0 + (wave * 2 + m) * 16 + r;
                ok[m] = q >= 0 && q < T_in;
                off0[m] = q * a.c_in;
#pragma unroll
                for (int j = 0; j < NTM; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            for (int k0 = 0; k0 < K1_16; k0 += 16) {
                f32x4 av[2], bv[NTM];
#pragma unroll
                for (int m = 0; m < 2; ++m) av[m] = xload(xbase, ok[m], off0[m] + k0 + 4 * kq, k0 + 4 * kq, a.c_in);
#pragma unroll
                for (int j = 0; j < NTM; ++j) bv[j] = wfrag(wl1, a.NPm, k0, j);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int m = 0; m < 2; ++m)
#pragma unroll
                        for (int j = 0; j < NTM; ++j)
                            acc[m][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m][i], bv[j][i], acc[m][j], 0, 0, 0);
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int jrow = (wave * 2 + m) * 16 + 4 * kq + e;
                    const int q = q0 + jrow;
                    const bool okq = q >= 0 && q < T_in;
#pragma unroll
                    for (int j = 0; j < NTM; ++j) {
                        const int col = 16 * j + r;
                        if (col < a.c_mid) t1[jrow * a.Cmp + col] = okq ? fmaxf(acc[m][j][e] + b1c[j], 0.0f) : 0.0f;
                    }
                }
        }
        __syncthreads();
        // ---- phase B: t2 row i <-> output position to0 + i: conv3 over t1 rows i * stride .. + 2 -----------------------
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int mt = wave + 4 * m;
            if (mt >= n_mt) break;
            f32x4 acc[NTM];
#pragma unroll
            for (int j = 0; j < NTM; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* trow = t1 + ((mt * 16 + r) * a.stride) * a.Cmp + 4 * kq;
            for (int k0 = 0; k0 < K2_16; k0 += 16) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(trow + k0);
#pragma unroll
                for (int j = 0; j < NTM; ++j) {
                    const f32x4 bv = wfrag(wl2, a.NPm, k0, j);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = mt * 16 + 4 * kq + e;
#pragma unroll
                for (int j = 0; j < NTM; ++j) {
                    const int col = 16 * j + r;
                    if (col < a.c_mid) t2[i * a.Cmp + col] = fmaxf(acc[j][e] + b2c[j], 0.0f);
                }
            }
        }
        __syncthreads();
        // ---- phase C: y row i = conv1x1(t2 row i) + b3 + shortcut -> ReLU ------------------------------------------------
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int mt = wave + 4 * m;
            if (mt >= n_mt) break;
            f32x4 acc[NTO];
#pragma unroll
            for (int j = 0; j < NTO; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* trow = t2 + (mt * 16 + r) * a.Cmp + 4 * kq;
            for (int k0 = 0; k0 < K3_16; k0 += 16) {
                const f32x4 av = *reinterpret_cast<const f32x4*>(trow + k0);
#pragma unroll
                for (int j = 0; j < NTO; ++j) {
                    const f32x4 bv = wfrag(wl3, a.NPo, k0, j);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[j], 0, 0, 0);
                }
            }
            if (a.Ksc) {
                const int i_r = mt * 16 + r;
                const bool okr = i_r < a.R2 && to0 + i_r < T_out;
                const int off0 = (to0 + i_r) * a.stride * a.c_in;
                for (int k0 = 0; k0 < Ksc16; k0 += 16) {
                    const f32x4 av = xload(xbase, okr, off0 + k0 + 4 * kq, k0 + 4 * kq, a.Ksc);
#pragma unroll
                    for (int j = 0; j < NTO; ++j) {
                        const f32x4 bv = wfrag(wl3, a.NPo, K3_16 + k0, j);
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[i], acc[j], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = mt * 16 + 4 * kq + e;
                const int pos = to0 + i;
                if (i >= a.R2 || pos >= T_out) continue;
                const int64_t orow = ((int64_t)b * a.T_out + pos) * a.c_out;
#pragma unroll
                for (int j = 0; j < NTO; ++j) {
                    const int col = 16 * j + r;
                    if (col >= a.c_out) continue;
                    float v = acc[j][e] + b3c[j];
                    if (!a.Ksc) v += a.x[xbase + (int64_t)pos * a.c_in + col];    // identity shortcut
                    a.y[orow + col] = fmaxf(v, 0.0f);
                }
            }
        }
        __syncthreads();
    }
}

// The bottleneck block in split precision on the bf16 MFMA (the arithmetic and operand layouts of seq_basic_block_x3_kernel:
// k-steps of 32, weights as two bf16 planes [k-step][kq][n][8], both LDS tiles stored already split with a row pitch of
// 8 (mod 16) halfwords).  Three GEMM phases as above; the output keeps the fp32 kernel's per-lane stores (c_out = 4 c_mid: an
// image of the tile's outputs does not fit next to the weights).
struct BneckX3Args {
    const float* x;
    unsigned x_bytes;
    float* y;
    const unsigned short *w1, *w2, *w3;            // planes [hi | lo]: [S1][4][NPm][8], [S2][4][NPm][8], [S3 + Ssc][4][NPo][8]
    const float *b1, *b2, *b3;
    int NPm, NPo;
    int B, T_in, T_out, c_in, c_mid, c_out, Cmp, stride;
    int Ksc, S1, S2, S3, Ssc;
    int R2, tiles_per_read, n_tiles;
    const int32_t* tin;       // ragged batches: see BlockArgs
    const int32_t* tout;
};

template <int NTM, int NTO>
__global__ __launch_bounds__(256) void seq_bottleneck_block_x3_kernel(const BneckX3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds8[];
    constexpr int RA = 128;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int p1 = a.S1 * 4 * a.NPm * 8, p2 = a.S2 * 4 * a.NPm * 8, p3 = (a.S3 + a.Ssc) * 4 * a.NPo * 8;   // halfwords per plane
    unsigned short* wl1 = reinterpret_cast<unsigned short*>(lds8);
    unsigned short* wl2 = wl1 + 2 * p1;
    unsigned short* wl3 = wl2 + 2 * p2;
    const int tplane = (RA + 4) * a.Cmp;
    unsigned short* t1h = wl3 + 2 * p3;            // t1: [hi plane | lo plane], then t2 the same
    unsigned short* t1l = t1h + tplane;
    unsigned short* t2h = t1l + tplane;
    unsigned short* t2l = t2h + tplane;
    for (int i = threadIdx.x; i < 2 * p1 / 8; i += 256) reinterpret_cast<u32x4*>(wl1)[i] = reinterpret_cast<const u32x4*>(a.w1)[i];
    for (int i = threadIdx.x; i < 2 * p2 / 8; i += 256) reinterpret_cast<u32x4*>(wl2)[i] = reinterpret_cast<const u32x4*>(a.w2)[i];
    for (int i = threadIdx.x; i < 2 * p3 / 8; i += 256) reinterpret_cast<u32x4*>(wl3)[i] = reinterpret_cast<const u32x4*>(a.w3)[i];
    for (int i = threadIdx.x; i < 4 * tplane / 2; i += 256) reinterpret_cast<unsigned*>(t1h)[i] = 0u;
    __syncthreads();
    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.x), 0, a.x_bytes, 0x00020000);
    const int lim_max = a.T_in * a.c_in;              // row pitch of a read in x (the longest read's)
    int lim = lim_max, T_in = a.T_in, T_out = a.T_out;   // of the read a tile belongs to (set per tile)
    float b1c[NTM], b2c[NTM], b3c[NTO];
#pragma unroll
    for (int j = 0; j < NTM; ++j) {
        b1c[j] = a.b1[16 * j + r];
        b2c[j] = a.b2[16 * j + r];
    }
#pragma unroll
    for (int j = 0; j < NTO; ++j) b3c[j] = a.b3[16 * j + r];
    const int n_mt = (a.R2 + 15) / 16;
    auto wfrag = [&](const unsigned short* w, int plane, int NP, int s, int j, u32x4& bh, u32x4& bl) {
        const int n = 16 * j + r;
        if (n < NP) {
            const unsigned short* q = w + ((s * 4 + kq) * NP + n) * 8;
            bh = *reinterpret_cast<const u32x4*>(q);
            bl = *reinterpret_cast<const u32x4*>(q + plane);
        } else {
            bh = bl = (u32x4){0u, 0u, 0u, 0u};
        }
    };
    // a lane's eight consecutive x values at element o of the read (zero outside it), K index kidx .. kidx + 7 of Klim
    auto xload8 = [&](int64_t xbase, bool ok, int o, int kidx, int Klim, f32x4& lo4, f32x4& hi4) {
        if (ok && o >= 0 && o + 7 < lim) {
            lo4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((xbase + o) * 4), 0, 0));
            hi4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, (unsigned)((xbase + o) * 4 + 16), 0, 0));
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lo4[i] = (ok && kidx + i < Klim && o + i >= 0 && o + i < lim) ? a.x[xbase + o + i] : 0.0f;
                hi4[i] = (ok && kidx + 4 + i < Klim && o + 4 + i >= 0 && o + 4 + i < lim) ? a.x[xbase + o + 4 + i] : 0.0f;
            }
        }
    };
    // relu(acc + bias) of one accumulator register -> the split tile (one channel of one row)
    auto put_split = [&](unsigned short* th, unsigned short* tl, int at, float v) {
        const __bf16 h = (__bf16)v;
        th[at] = __builtin_bit_cast(unsigned short, h);
        tl[at] = __builtin_bit_cast(unsigned short, (__bf16)(v - (float)h));
    };
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int b = tile / a.tiles_per_read;
        const int to0 = (tile - b * a.tiles_per_read) * a.R2;
        const int64_t xbase = (int64_t)b * lim_max;
        if (a.tin) {
            T_in = as_const_len(a.tin)[b];
            T_out = as_const_len(a.tout)[b];
            lim = T_in * a.c_in;
        }
        if (to0 >= T_out) continue;                            // ragged batch: this read ended before the tile
        // ---- phase A: t1 rows j = 0 .. RA-1 <-> input positions q0 + j ------------------------------------------------
        {
            const int q0 = to0 * a.stride - 1;
            f32x4 acc[2][NTM];
            int off0[2];
            bool ok[2];
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                const int q = q0 + (wave * 2 + m) * 16 + r;
                ok[m] = q >= 0 && q < T_in;
                off0[m] = q * a.c_in;
#pragma unroll
                for (int j = 0; j < NTM; ++j) acc[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            for (int s = 0; s < a.S1; ++s) {
                u32x4 bh[NTM], bl[NTM];
#pragma unroll
                for (int j = 0; j < NTM; ++j) wfrag(wl1, p1, a.NPm, s, j, bh[j], bl[j]);
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    f32x4 xa, xb;
                    xload8(xbase, ok[m], off0[m] + 32 * s + 8 * kq, 32 * s + 8 * kq, a.c_in, xa, xb);
                    u32x4 ah, al;
                    split8(xa, xb, ah, al);
#pragma unroll
                    for (int j = 0; j < NTM; ++j) acc[m][j] = mfma_x3(ah, al, bh[j], bl[j], acc[m][j]);
                }
            }
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int jrow = (wave * 2 + m) * 16 + 4 * kq + e;
                    const int q = q0 + jrow;
                    const bool okq = q >= 0 && q < T_in;
#pragma unroll
                    for (int j = 0; j < NTM; ++j) {
                        const int col = 16 * j + r;
                        if (col < a.c_mid) put_split(t1h, t1l, jrow * a.Cmp + col, okq ? fmaxf(acc[m][j][e] + b1c[j], 0.0f) : 0.0f);
                    }
                }
        }
        __syncthreads();
        // ---- phase B: t2 row i <-> output position to0 + i: conv3 over t1 rows i * stride .. + 2 -----------------------
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int mt = wave + 4 * m;
            if (mt >= n_mt) break;
            f32x4 acc[NTM];
#pragma unroll
            for (int j = 0; j < NTM; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int trow = ((mt * 16 + r) * a.stride) * a.Cmp + 8 * kq;
            for (int s = 0; s < a.S2; ++s) {
                const u32x4 ah = *reinterpret_cast<const u32x4*>(t1h + trow + 32 * s);
                const u32x4 al = *reinterpret_cast<const u32x4*>(t1l + trow + 32 * s);
#pragma unroll
                for (int j = 0; j < NTM; ++j) {
                    u32x4 bh, bl;
                    wfrag(wl2, p2, a.NPm, s, j, bh, bl);
                    acc[j] = mfma_x3(ah, al, bh, bl, acc[j]);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = mt * 16 + 4 * kq + e;
#pragma unroll
                for (int j = 0; j < NTM; ++j) {
                    const int col = 16 * j + r;
                    if (col < a.c_mid) put_split(t2h, t2l, i * a.Cmp + col, fmaxf(acc[j][e] + b2c[j], 0.0f));
                }
            }
        }
        __syncthreads();
        // ---- phase C: y row i = conv1x1(t2 row i) + b3 + shortcut -> ReLU ------------------------------------------------
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const int mt = wave + 4 * m;
            if (mt >= n_mt) break;
            f32x4 acc[NTO];
#pragma unroll
            for (int j = 0; j < NTO; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int trow = (mt * 16 + r) * a.Cmp + 8 * kq;
            for (int s = 0; s < a.S3; ++s) {
                const u32x4 ah = *reinterpret_cast<const u32x4*>(t2h + trow + 32 * s);
                const u32x4 al = *reinterpret_cast<const u32x4*>(t2l + trow + 32 * s);
#pragma unroll
                for (int j = 0; j < NTO; ++j) {
                    u32x4 bh, bl;
                    wfrag(wl3, p3, a.NPo, s, j, bh, bl);
                    acc[j] = mfma_x3(ah, al, bh, bl, acc[j]);
                }
            }
            if (a.Ksc) {
                const int i_r = mt * 16 + r;
                const bool okr = i_r < a.R2 && to0 + i_r < T_out;
                const int off0 = (to0 + i_r) * a.stride * a.c_in;
                for (int s = 0; s < a.Ssc; ++s) {
                    f32x4 xa, xb;
                    xload8(xbase, okr, off0 + 32 * s + 8 * kq, 32 * s + 8 * kq, a.Ksc, xa, xb);
                    u32x4 ah, al;
                    split8(xa, xb, ah, al);
#pragma unroll
                    for (int j = 0; j < NTO; ++j) {
                        u32x4 bh, bl;
                        wfrag(wl3, p3, a.NPo, a.S3 + s, j, bh, bl);
                        acc[j] = mfma_x3(ah, al, bh, bl, acc[j]);
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = mt * 16 + 4 * kq + e;
                const int pos = to0 + i;
                if (i >= a.R2 || pos >= T_out) continue;
                const int64_t orow = ((int64_t)b * a.T_out + pos) * a.c_out;
#pragma unroll
                for (int j = 0; j < NTO; ++j) {
                    const int col = 16 * j + r;
                    if (col >= a.c_out) continue;
                    float v = acc[j][e] + b3c[j];
                    if (!a.Ksc) v += a.x[xbase + (int64_t)pos * a.c_in + col];    // identity shortcut
                    a.y[orow + col] = fmaxf(v, 0.0f);
                }
            }
        }
        __syncthreads();
    }
}
}  // namespace
}  // namespace rs
