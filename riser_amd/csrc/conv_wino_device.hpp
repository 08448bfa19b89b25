// What the fp32 Winograd conv kernels share, parameterised by the transform size M (F(M,3): M = 2 or 4): the plane layout of
// the input rows in LDS, the input transform, the output transform with its max over the pooling pairs, and
// the zero fill of a tile that lies in a shorter read's padding.  Users: conv_wino_kernel.hpp (F(2,3), tiled), conv_wino4.hip
// (F(4,3), tiled), conv_wres_f32.hip (both, weights resident), conv_stream_f32.hip (F(2,3), layers 0 + 1), conv_small_f32.hip
// (the layout) and conv_f32.hip (the fill).  The slot loops - MFMA order, look-ahead of the fragment reads, where the transform
// sits behind the MFMAs, the scheduling barriers - stay with their kernels.
// Every kernel of the family is held to the others' bits (tests/test_gpu_f32_shapes.py, _thin, _wres, test_gpu_small.py): the
// order of operations and the fmaf placement in the two transforms below are the contract, and this is their one copy.
#pragma once
#include "tile_plan.hpp"

namespace rs {

// ---- the tiled kernels' LDS rows: host-usable (tests/wino_lds_check.cpp walks every read and write pattern through them) -----
// Row pitch in floats: kc + 2 (= 2 mod 4), so that the 16 rows x 2 k-lanes of a 32-lane group of a ds_read_b32 hit 32 banks.
// One F(4,3) tile does not fit the LDS budget that way at chunks of 20, 512 x 80 (175 296 B), and runs UNPADDED rows instead
// (159 360 B): 20 * row mod 32 takes each multiple of 4 once over 8 consecutive rows, rows R and R + 8 collide and always
// differ in bit 3, so the k index is swizzled by that bit (wino_swizzle) and a group reads words {0, 1} of the rows with bit
// 3 clear and {2, 3} of their partners: 32 banks again, whatever the first row.  Tiles that fit padded stay padded (512 x 64
// at chunks of 20 measured 3 - 4 % slower on unpadded rows, profiles/wino4_kc20_ab.txt), and so do those that fit neither way.
constexpr bool wino_unpadded(int m, int units, int bn, int kc) {
    const size_t rows2 = 2 * sizeof(float) * (m * (units + 1) + (m + 2) * bn);          // bytes per float of pitch, two buffers
    return m == 4 && kc == 20 && rows2 * (kc + 2) > kConvLdsBudget && rows2 * kc <= kConvLdsBudget;
}
constexpr int wino_pitch(bool unpadded, int kc) { return unpadded ? kc : kc + 2; }
// XOR on the channel index of `row` (the index inside a plane for input rows, component * bn + n for weight rows; bn is a
// multiple of 16, so that is n's bit 3).  A multiple of 2 below 4: the two 8-byte halves of a 16-byte unit change places.
constexpr int wino_swizzle(bool unpadded, int row) { return unpadded ? 2 * ((row >> 3) & 1) : 0; }
// word of channel c of `row`, from the first row of its plane / of the weight slab
constexpr int wino_word(bool unpadded, int kc, int row, int c) {
    return wino_pitch(unpadded, kc) * row + (c ^ wino_swizzle(unpadded, row));
}

// Staging passes of a tiled kernel of `threads` threads over a slab of m * units + 2 input rows / bn weight rows per
// component: slab rows per pass (a multiple of m: a thread's rows keep their plane) and output channels per pass.  Swizzled
// rows want the swizzle of a thread's units known without arithmetic in the slot loop: rows per pass a multiple of 32 where
// that costs no extra pass (plane index + 8 j per unit: bit 3 is the thread's own, flipped for odd j), channels per pass 16
// (bit 3 of n is the thread's own).
constexpr int wino_stage_rows(bool unpadded, int m, int kc, int threads, int units) {
    const int rows = m * units + 2, any = (threads / (kc / 4)) & ~(m - 1), al = (threads / (kc / 4)) & ~31;
    return (unpadded && al > 0 && (rows + al - 1) / al == (rows + any - 1) / any) ? al : any;
}
constexpr int wino_stage_cols(bool unpadded, int m, int kc, int threads) {
    const int any = threads / ((m + 2) * (kc / 4));
    return (unpadded && any >= 16) ? 16 : any;
}

// floats of one LDS buffer of a tiled kernel: M planes of (units + 1) input rows and M + 2 weight components of bn rows, at
// the row pitch above.  The kernels' BUF and the host's lds_bytes (two buffers) are this one expression.
constexpr int wino_buf_floats(int m, int units, int bn, int kc) {
    return (m * (units + 1) + (m + 2) * bn) * wino_pitch(wino_unpadded(m, units, bn, kc), kc);
}

}  // namespace rs

#ifdef __HIPCC__
#include "device_prelude.hpp"

namespace rs {
namespace {

// The plane layout: a unit (pooled row T for F(2,3), group G of four conv rows for F(4,3)) needs the NC = M + 2 input rows
// M * unit - 1 .. M * unit + M.  Slab row s (the tile's first input row is M * unit0 - 1) lives in plane s % M at index s / M,
// so raw input d_k of unit u is row u + k / M of plane k % M: unit stride across the lanes of a fragment read, and with the
// pitch S = KC + 2 floats (= 2 mod 4) every ds_read_b32 of a 32-lane half hits 32 distinct banks.  (The weights-resident, small
// and streaming kernels keep this pitch at every chunk and tile; the tiled kernels take theirs from wino_pitch: WinoTile.)
template <int M, int KC>
struct WinoGeom {
    static_assert(M == 2 || M == 4, "F(2,3) or F(4,3)");
    static constexpr int NC = M + 2;                   // Winograd components = raw inputs d0 .. d(M+1) of a unit
    static constexpr int NP = M;                       // planes
    static constexpr int S = KC + 2;                   // row pitch (input and weight rows)
    static constexpr int KQ = KC / 4;                  // k-steps per chunk = 16-byte units per row
    static constexpr int PL16 = 17 * S;                // one plane of the 16-unit kernels (wres, small): index s / M <= 16
    static constexpr int IMG16 = NP * PL16;            // ... and their whole input image
};

// A tile of the tiled kernels (BU units x BN output channels, kThreads threads) and its staging passes: a pass of the
// workgroup covers RPT slab rows x KQ 16-byte units of the input slab (RPT a multiple of M, so a thread's rows
// a_row + u * RPT keep their plane), or NPP output channels x NC components x KQ units of the weight slab.
template <int M, int BU, int BN, int KC, int kThreads>
struct WinoTile : WinoGeom<M, KC> {
    using G = WinoGeom<M, KC>;
    static constexpr bool SWZ = wino_unpadded(M, BU, BN, KC);   // unpadded rows, the k index swizzled by bit 3 of the row
    static constexpr int S = wino_pitch(SWZ, KC);
    static constexpr int swz(int row) { return wino_swizzle(SWZ, row); }
    static constexpr int PL = (BU + 1) * S;
    static constexpr int A_ELEMS = M * PL;
    static constexpr int BUF = wino_buf_floats(M, BU, BN, KC);
    static constexpr int RPT = wino_stage_rows(SWZ, M, KC, kThreads, BU);
    static constexpr int A_ROWS = M * BU + 2;
    static constexpr int A_PER = (A_ROWS + RPT - 1) / RPT;
    static constexpr int NPP = wino_stage_cols(SWZ, M, KC, kThreads);
    static constexpr int B_PER = (BN + NPP - 1) / NPP;
    static_assert(BUF == A_ELEMS + G::NC * BN * S, "one buffer: the planes, then the weight components");
};

// V = B^T d.  F(2,3): v0 = d0 - d2, v1 = d1 + d2, v2 = d2 - d1, v3 = d1 - d3.  F(4,3): Lavin & Gray's B^T (conv_wino4.hip).
template <int M>
__device__ __forceinline__ void wino_input_transform(float (&o)[M + 2], const float (&d)[M + 2]) {
#ifdef RS_ABL_NOXFORM                                    // timing experiment only
#pragma unroll
    for (int k = 0; k < M + 2; ++k) o[k] = d[k];
#else
    if constexpr (M == 2) {
        o[0] = d[0] - d[2];
        o[1] = d[1] + d[2];
        o[2] = d[2] - d[1];
        o[3] = d[1] - d[3];
    } else {
        const float p = fmaf(-4.0f, d[2], d[4]), q = fmaf(-4.0f, d[1], d[3]);
        const float s2 = d[4] - d[2], t2 = d[3] - d[1];
        o[0] = fmaf(4.0f, d[0], fmaf(-5.0f, d[2], d[4]));
        o[1] = p + q;
        o[2] = p - q;
        o[3] = fmaf(2.0f, t2, s2);
        o[4] = fmaf(-2.0f, t2, s2);
        o[5] = fmaf(4.0f, d[1], fmaf(-5.0f, d[3], d[5]));
    }
#endif
}

// y = A^T m for ONE accumulator element, then the max over each pooling pair: p[h] = max(y[2h], y[2h+1]), pooled row h of the
// unit.  The caller adds the bias, applies ReLU and the length mask: relu(p[h] + bias), or zero beyond the read's length.
// (The two tiled kernels spell the same lines out in their epilogues: every function form of them moved registers and SGPR
// spills there, profiles/f32_device_checks.txt.  They are held to these by the bit-for-bit tests.)
template <int M>
__device__ __forceinline__ void wino_output_pool(float (&p)[M / 2], const float (&m)[M + 2]) {
    if constexpr (M == 2) {
        const float y0 = (m[0] + m[1]) + m[2];
        const float y1 = (m[1] - m[2]) - m[3];
        p[0] = fmaxf(y0, y1);
    } else {
        const float s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
        const float y0 = (m[0] + s12) + s34;
        const float y1 = fmaf(2.0f, d34, d12);
        const float y2 = fmaf(4.0f, s34, s12);
        const float y3 = fmaf(8.0f, d34, d12) + m[5];
        p[0] = fmaxf(y0, y1);
        p[1] = fmaxf(y2, y3);
    }
}

// Zero fill of a dead tile (every row beyond its read's length: the output is all zeros, no loads, MFMAs or pipeline slots):
// `rows` pooled rows from prow0 by BN columns from col0, in 16-byte pieces, by the whole workgroup.  Pooled row p exists
// while ROW_SCALE * p < row_limit (the Winograd kernels count pooled rows, the direct kernel input rows: ROW_SCALE = 2),
// column c while c < cp_out.
template <int BN, int ROW_SCALE = 1>
__device__ __forceinline__ void zero_fill_tile(float* y, int prow0, int rows, int col0, int row_limit, int cp_out) {
    constexpr int pieces_per_row = BN / 4;
    for (int f = threadIdx.x; f < rows * pieces_per_row; f += blockDim.x) {
        const int rr = f / pieces_per_row, cc = (f - rr * pieces_per_row) * 4;
        const int prow = prow0 + rr, col = col0 + cc;
        if (ROW_SCALE * prow < row_limit && col < cp_out)
            *reinterpret_cast<float4*>(y + (int64_t)prow * cp_out + col) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

}  // namespace
}  // namespace rs
#endif  // __HIPCC__
