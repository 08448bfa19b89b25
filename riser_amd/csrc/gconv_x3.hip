// Generic ConvNets (csrc/gconv.hip) in SPLIT PRECISION on the bf16 MFMA (rs_gconv_set_mode(m, RS_BF16X3)).
//
// gconv_tile_x3_kernel is gconv_tile_kernel's sibling: the same tile shapes, K chunks, grid, length table, epilogue and fp32
// activation buffers [read][t][cp4(C)]; a workgroup of 4 waves owns 16 RT conv positions of ONE read times 16 WC WGC output
// channels.  What changes is the arithmetic: every activation and weight is a pair hi = bf16(v), lo = bf16(v - hi) (round to
// nearest even) and a product is hi*hi + lo*hi + hi*lo on three v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
//   * Slab.  Per K chunk the workgroup loads the chunk's fp32 activation rows once, makes a row before 0, a row at or behind
//     the read's own row count and a pad channel an exact zero by select BEFORE the split (what lies behind a read may be
//     NaN), splits, and stages two bf16 planes [row][xpitch].  xpitch = kc + 8: an odd number of 16-byte units per row keeps
//     the 16 rows of a fragment read off shared banks.  The slab serves all k taps.
//   * K order within a chunk is tap-major, (tap, channel), in k-steps of 32: lane (rl, kq) of step s takes pair p = 4 s + kq,
//     tap = p / (kc / 8), channels 8 (p % (kc / 8)) .. + 7: one 16-byte LDS read per plane from slab row rl + tap.  With
//     kc = 16 and k odd the last step's pairs 2 and 3 have tap = k: their weights are zero, and the slab owns one spare row
//     beyond the halo, staged as zeros, so that their A operand is finite and no row past the slab is read.
//   * Weights are split on the host (gconv/plan.hpp: pack_weights_x3) in the order the lanes read them; the chunk's panel is
//     copied to LDS next to the slab, both planes.
//   * Every output is one fixed chain - chunks ascending, steps ascending, hi*hi, lo*hi, hi*lo - whatever the batch or ld.
// Convs with c_in <= 4 (the first conv: K of a few dozen, bandwidth-bound) stay on gconv_tile_kernel in both modes.
#include "gconv_x3.hpp"
#include "seqnet/mfma_split.hpp"

namespace rs {
namespace {

template <int RT, int WGC, int WC, bool POOL>
__global__ __launch_bounds__(256) void gconv_tile_x3_kernel(const GconvX3Args a) {
    constexpr int WGR = 4 / WGC, RW = RT / WGR;             // wave rows of the workgroup, row tiles per wave
    constexpr int ROWS = 16 * RT, NCOL = 16 * WC * WGC;
    static_assert(RW >= 1 && RW * WGR == RT, "row tiles split evenly over the wave rows");
    extern __shared__ __attribute__((aligned(16))) unsigned short lds16[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int q0 = tile * ROWS;
    const int T = as_const_len(a.rows)[b];
    if (q0 >= T) return;                                    // the whole workgroup: no barrier is skipped by a part of it
    const int nb = blockIdx.y;
    const int wr = wave / WGC, wc = wave - wr * WGC;
    unsigned short* slab = lds16;                           // hi plane; lo plane slab_half behind it
    unsigned short* panel = lds16 + 2 * a.slab_half;        // hi plane; lo plane panel_half behind it
    const int c8n = a.kc >> 3, c8m = c8n - 1;
    const int pad = a.k >> 1, rows_in = ROWS + a.k - 1;
    const float* xb = a.x + (int64_t)b * a.in_rows * a.in_pitch;
    const unsigned short* wp = a.w + (int64_t)nb * a.nchunk * a.panel_half;
    const int col0 = nb * NCOL + 16 * WC * wc;              // this wave's first column

    f32x4 acc[RW][WC];
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
        for (int j = 0; j < WC; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int chunk = 0; chunk < a.nchunk; ++chunk) {
        if (chunk) __syncthreads();
        for (int e = threadIdx.x; e < a.slab_rows * c8n; e += 256) {
            const int r = e >> a.c8_shift, c8 = e & c8m;
            const int q = q0 - pad + r, ch = chunk * a.kc + 8 * c8;
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
            if (r < rows_in && q >= 0 && q < T && ch < a.c_in) {             // r >= rows_in: the spare row, zero
                const float* p = xb + (int64_t)q * a.in_pitch + ch;
                const f32x4 t0 = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                for (int i = 0; i < 4; ++i) v0[i] = ch + i < a.c_in ? t0[i] : 0.0f;         // pad channels are never written
                if (ch + 4 < a.c_in) {                      // then ch + 4 < cp4(c_in) = in_pitch as well
                    const f32x4 t1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v1[i] = ch + 4 + i < a.c_in ? t1[i] : 0.0f;
                }
            }
            u32x4 hi, lo;
            split8(v0, v1, hi, lo);
            unsigned short* d = slab + r * a.xpitch + 8 * c8;
            *reinterpret_cast<u32x4*>(d) = hi;
            *reinterpret_cast<u32x4*>(d + a.slab_half) = lo;
        }
        {
            const u32x4* src = reinterpret_cast<const u32x4*>(wp + (int64_t)chunk * a.panel_half);
            const u32x4* src_lo = reinterpret_cast<const u32x4*>(wp + (int64_t)chunk * a.panel_half + a.w_plane);
            u32x4* dst = reinterpret_cast<u32x4*>(panel);
            const int n = a.panel_half >> 3;
            for (int e = threadIdx.x; e < n; e += 256) {
                dst[e] = src[e];
                dst[n + e] = src_lo[e];
            }
        }
        __syncthreads();
        if (col0 >= a.c_out) continue;                      // a wave without columns only stages
        const unsigned short* A0 = slab + (16 * RW * wr + rl) * a.xpitch;
        const unsigned short* B0 = panel + (WC * wc * a.steps * 64 + lane) * 8;
        for (int s = 0; s < a.steps; ++s) {
            const int p = 4 * s + kq;
            const unsigned short* Ar = A0 + (p >> a.c8_shift) * a.xpitch + 8 * (p & c8m);
            const unsigned short* Bp = B0 + s * 512;
            u32x4 ah[RW], al[RW], bh[WC], bl[WC];
#pragma unroll
            for (int i = 0; i < RW; ++i) {
                ah[i] = *reinterpret_cast<const u32x4*>(Ar + 16 * i * a.xpitch);
                al[i] = *reinterpret_cast<const u32x4*>(Ar + 16 * i * a.xpitch + a.slab_half);
            }
#pragma unroll
            for (int j = 0; j < WC; ++j) {
                bh[j] = *reinterpret_cast<const u32x4*>(Bp + j * a.steps * 512);
                bl[j] = *reinterpret_cast<const u32x4*>(Bp + j * a.steps * 512 + a.panel_half);
            }
#pragma unroll
            for (int i = 0; i < RW; ++i)
#pragma unroll
                for (int j = 0; j < WC; ++j) acc[i][j] = mfma_x3(ah[i], al[i], bh[j], bl[j], acc[i][j]);
        }
    }
    // lane element e of row tile i: conv row q0 + 16 (RW wr + i) + 4 kq + e, column col0 + 16 j + rl
    float* yb = a.y + (int64_t)b * a.out_rows * a.out_pitch;
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        const int col = col0 + 16 * j + rl;
        if (col >= a.c_out) continue;
        const float bias = a.b[col];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const int row = q0 + 16 * (RW * wr + i) + 4 * kq;
            if constexpr (POOL) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int p = (row >> 1) + h;
                    // max(relu(u + bias), relu(v + bias)) == relu(max(u, v) + bias): rounding is monotonic
                    if (p < (T >> 1))
                        yb[(int64_t)p * a.out_pitch + col] = fmaxf(fmaxf(acc[i][j][2 * h], acc[i][j][2 * h + 1]) + bias, 0.0f);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (row + e < T) yb[(int64_t)(row + e) * a.out_pitch + col] = fmaxf(acc[i][j][e] + bias, 0.0f);
            }
        }
    }
}

typedef void (*X3Fn)(const GconvX3Args);

template <int RT, int WGC, int WC>
X3Fn x3_fn_of(bool pool) {
    return pool ? gconv_tile_x3_kernel<RT, WGC, WC, true> : gconv_tile_x3_kernel<RT, WGC, WC, false>;
}

X3Fn x3_fn(int shape, bool pool) {                          // gconv/plan.hpp: kShapes
    switch (shape) {
        case 0: return x3_fn_of<4, 1, 2>(pool);
        case 1: return x3_fn_of<4, 2, 2>(pool);
        case 2: return x3_fn_of<4, 4, 2>(pool);
        case 3: return x3_fn_of<1, 4, 1>(pool);
        default: return x3_fn_of<1, 4, 2>(pool);
    }
}

}  // namespace

hipError_t gconv_x3_allow_lds(int shape, bool pool, int bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(x3_fn(shape, pool)), hipFuncAttributeMaxDynamicSharedMemorySize,
                               bytes);
}

hipError_t gconv_x3_launch(int shape, bool pool, const GconvX3Args& a, dim3 grid, size_t lds_bytes, hipStream_t st) {
    hipLaunchKernelGGL(x3_fn(shape, pool), grid, dim3(256), lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace rs
