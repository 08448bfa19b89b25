// TCN and bottleneck TCN temporal blocks in SPLIT PRECISION on the bf16 MFMA (rs_tcn_set_mode(m, RS_BF16X3)).
//
// The same strided receptive cone as tcn_block_kernel (csrc/tcn.hip): one launch per temporal block, a workgroup of
// four waves takes nb reads x T output positions, stages the block input rows it needs into LDS (zero below position 0 and
// beyond the window), runs the block's convs with LDS-resident intermediates - the convs up to the last k-tap conv over every m
// the tile needs, that conv and what follows it only at m = base * m' - adds the 1x1 shortcut or the identity at the strided
// rows, applies the ReLU and writes only the rows the next block reads.  What changes is the arithmetic of seqnet.hip's
// seq_basic_block_x3_kernel: every activation and weight is a pair hi = bf16(v), lo = bf16(v - hi) (round to nearest even), a
// product is hi*hi + lo*hi + hi*lo on three v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
//   * The LDS buffers (block input X, intermediates P / Q) hold the activations ALREADY SPLIT: two bf16 planes [row][pitch],
//     channels padded to 8 with zeros.  The staging pass splits the block input once; every conv epilogue splits its output
//     once.  A fragment is two ds_read_b128 (8 consecutive channels of one tap row) and converts nothing.  pitch = cp8, or
//     cp8 + 8 where cp8 / 8 is even: an odd number of 16-byte units per row keeps a 16-row group off shared banks.
//   * K of a conv is tap-major over cp8 channels, cut into k-steps of 32: lane (row rl, k-group kq) supplies K elements
//     32 s + 8 kq .. + 7, all of one tap.  K indices behind the last tap read nothing (zero fragment) and meet zero weights.
//   * The weights are split on the host (tcn_x3_pack) and read from global memory (L2) as 16-byte fragments:
//     [hi | lo][step][kq][n][8], so a 16-lane group reads 256 contiguous bytes.
//   * Bias, ReLU, the residual add and the block outputs stay fp32 (HBM layout [read][m][cp4], as in fp32: the head kernel is
//     reused unchanged).  The identity residual reads the fp32 block input from global memory, not its split form.
//   * Block 0's first conv (1 input channel) and its 1 -> n shortcut run on the same path: K = k taps x 8 padded channels in one
//     or two k-steps, a small share of block 0.
// Every output element is a fixed K-ordered sequence of MFMAs from a zero accumulator whatever the tile, the batch or the row
// pitch: a read in a ragged batch gets the bits it gets alone.
#include "tcn_x3.hpp"
#include "seqnet/mfma_split.hpp"

#include <algorithm>
#include <cstring>

namespace rs {
namespace {

inline int x3_pitch(int cp8) { return ((cp8 / 8) % 2 == 0) ? cp8 + 8 : cp8; }

unsigned short bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

float bf16_val(unsigned short h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

__device__ __forceinline__ int read_len(const TcnX3Args& a, int b) {
    int L = as_const_len(a.len)[b];
    return L < 0 ? 0 : (L > a.ld ? a.ld : L);
}

// acc[t] += A (16 rows of S from row offset abase, k-steps of a conv of k taps over cpi channels) x W (columns n0 + 16 t ..)
__device__ __forceinline__ void conv_tile(const unsigned short* S, int plane, int sp, int abase, bool a_ok, int k, int cpi,
                                          int steps, const unsigned short* __restrict__ W, int np, int n0, int rl, int kq,
                                          f32x4 (&acc)[4]) {
    const int wplane = steps * 4 * np * 8;
    for (int s = 0; s < steps; ++s) {
        const int kidx = 32 * s + 8 * kq;
        const int tap = kidx / cpi, ci = kidx - tap * cpi;
        u32x4 ah = {0u, 0u, 0u, 0u}, al = {0u, 0u, 0u, 0u};
        if (a_ok && tap < k) {
            const unsigned short* p = S + abase + tap * sp + ci;
            ah = *reinterpret_cast<const u32x4*>(p);
            al = *reinterpret_cast<const u32x4*>(p + plane);
        }
        const unsigned short* wq = W + ((int64_t)(s * 4 + kq) * np + n0 + rl) * 8;
#pragma unroll
        for (int t = 0; t < 4; ++t)
            if (n0 + 16 * t < np) {
                const u32x4 bh = *reinterpret_cast<const u32x4*>(wq + 128 * t);
                const u32x4 bl = *reinterpret_cast<const u32x4*>(wq + 128 * t + wplane);
                acc[t] = mfma_x3(ah, al, bh, bl, acc[t]);
            }
    }
}

__global__ __launch_bounds__(256) void tcn_block_x3_kernel(const TcnX3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned short lds16[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int tile_b = blockIdx.x / a.tiles_pos, tile_p = blockIdx.x - tile_b * a.tiles_pos;
    const int b0 = tile_b * a.nb, mo0 = tile_p * a.T;      // first read, first output position m'
    const int64_t mbase = (int64_t)a.r * mo0;               // first input / intermediate m of the tile

    // ---- block input rows -> LDS X (split), zero below position 0, beyond the window and in the padded channels
    {
        unsigned short* X = lds16 + a.off[0];
        const int c8n = a.cpi[0] / 8;
        const int n = a.nb * a.rows_in * c8n;
        for (int e = threadIdx.x; e < n; e += 256) {
            const int c8 = e % c8n, rq = e / c8n;
            const int bl = rq / a.rows_in, q = rq - bl * a.rows_in;
            const int b = b0 + bl;
            const int64_t m = mbase + q;
            f32x4 v0 = {0.f, 0.f, 0.f, 0.f}, v1 = {0.f, 0.f, 0.f, 0.f};
            if (b < a.B && m < a.in_rows) {
                const int L = read_len(a, b);
                const int64_t pos = (int64_t)L - 1 - a.dil * m;
                if (pos >= 0) {
                    if (a.first) {
                        if (c8 == 0) v0.x = a.x[(int64_t)b * a.ld + pos];
                    } else {
                        const float* src = a.x + ((int64_t)b * a.in_rows + m) * a.cp_in + 8 * c8;
                        v0 = *reinterpret_cast<const f32x4*>(src);
                        if (8 * c8 + 4 < a.cp_in) v1 = *reinterpret_cast<const f32x4*>(src + 4);
                    }
                }
            }
            u32x4 hi, lo;
            split8(v0, v1, hi, lo);
            unsigned short* d = X + (bl * a.rows_in + q) * a.pitch[0] + 8 * c8;
            *reinterpret_cast<u32x4*>(d) = hi;
            *reinterpret_cast<u32x4*>(d + a.plane[0]) = lo;
        }
    }
    __syncthreads();

    for (int j = 0; j < a.nconv; ++j) {
        const bool last = j == a.nconv - 1;
        const unsigned short* S = lds16 + a.s_off[j];
        const int sp = a.s_pitch[j], srows = a.s_rows[j];
        unsigned short* D = lds16 + a.d_off[j];
        const int dp = a.d_pitch[j], dplane = a.d_plane[j];
        const int R = a.rows[j], M = a.nb * R, np = a.np[j];
        const int mt = (M + 15) / 16, ng = (np + 63) / 64;
        // columns this conv writes: its channels padded to 8 into LDS (what the next conv reads), to 4 into global memory
        const int wcols = last ? a.cp_out : a.cpo[j];
        for (int u = wave; u < mt * ng; u += 4) {
            const int rt = u / ng, cg = u - rt * ng;
            // the output row this lane feeds into the A operand
            const int arow = rt * 16 + rl;
            const bool a_ok = arow < M;
            const int abl = a_ok ? arow / R : 0, aq = a_ok ? arow - abl * R : 0;
            const int n0 = cg * 64;
            f32x4 acc[4], accs[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = accs[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            // pass 1 (last conv of a block with a shortcut): the 1x1 shortcut on the block input at the strided rows, moved to
            // accs; pass 0: the conv.  One instance of the k-loop for both keeps the kernel inside the SGPR file.
            for (int pass = (last && a.sw) ? 1 : 0; pass >= 0; --pass) {
                const bool sc = pass == 1;
                const int p_sp = sc ? a.pitch[0] : sp;
                conv_tile(sc ? lds16 + a.off[0] : S, sc ? a.plane[0] : a.s_plane[j], p_sp,
                          (sc ? abl * a.rows_in + aq * a.r : abl * srows + aq * a.step[j]) * p_sp, a_ok, sc ? 1 : a.k[j],
                          sc ? a.cpi[0] : a.cpi[j], sc ? a.sw_steps : a.steps[j], sc ? a.sw : a.w[j], np, n0, rl, kq, acc);
                if (sc) {
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        accs[t] = acc[t];
                        acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
            // accumulator element e of this lane: row 4 * kq + e of the tile, column rl of each 16-column tile
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = rt * 16 + 4 * kq + e;
                if (row >= M) continue;
                const int bl = row / R, q = row - bl * R;
                const int b = b0 + bl;
                const int64_t m = mbase + (int64_t)q * a.ostride[j];
                int64_t pos = -1;
                if (b < a.B && m <= a.ld) pos = (int64_t)read_len(a, b) - 1 - a.dil * m;
                const bool valid = pos >= 0;
                if (!last) {
                    unsigned short* d = D + (bl * R + q) * dp;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int col = n0 + 16 * t + rl;
                        if (n0 + 16 * t >= np || col >= wcols) continue;
                        const float v = valid ? fmaxf(acc[t][e] + a.b[j][col], 0.0f) : 0.0f;
                        const unsigned h = pack_bf16x2(v, 0.0f) & 0xffffu;
                        d[col] = (unsigned short)h;
                        d[dplane + col] = (unsigned short)pack_bf16x2(v - __builtin_bit_cast(float, h << 16), 0.0f);
                    }
                } else {
                    const int mo = mo0 + q;
                    if (b >= a.B || mo >= a.out_rows) continue;
                    float* y = a.y + ((int64_t)b * a.out_rows + mo) * a.cp_out;
                    // identity residual: the fp32 block input at the same position (block 0: the signal, one channel)
                    const float* xr = nullptr;
                    if (!a.sw && valid && m < a.in_rows)
                        xr = a.first ? a.x + (int64_t)b * a.ld + pos : a.x + ((int64_t)b * a.in_rows + m) * a.cp_in;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int col = n0 + 16 * t + rl;
                        if (n0 + 16 * t >= np || col >= wcols) continue;
                        const float v = fmaxf(acc[t][e] + a.b[j][col], 0.0f);
                        float res = 0.0f;
                        if (a.sw) res = accs[t][e] + a.sb[col];
                        else if (xr && (!a.first || col == 0)) res = xr[a.first ? 0 : col];
                        y[col] = valid ? fmaxf(v + res, 0.0f) : 0.0f;
                    }
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

std::vector<unsigned short> tcn_x3_pack(const float* w, int c_out, int c_in, int k, int* steps_out, int* np_out) {
    const int cp8 = tcn_cp8(c_in), np = (c_out + 15) & ~15;
    const int steps = (k * cp8 + 31) / 32;
    const size_t plane = (size_t)steps * 4 * np * 8;
    std::vector<unsigned short> p(2 * plane, 0);
    for (int s = 0; s < steps; ++s)
        for (int kq = 0; kq < 4; ++kq)
            for (int n = 0; n < c_out; ++n)
                for (int e = 0; e < 8; ++e) {
                    const int K = 32 * s + 8 * kq + e, tap = K / cp8, ci = K - tap * cp8;
                    if (tap >= k || ci >= c_in) continue;
                    const float v = w[((size_t)n * c_in + ci) * k + (k - 1 - tap)];
                    const unsigned short h = bf16_rne(v);
                    const size_t i = (((size_t)s * 4 + kq) * np + n) * 8 + e;
                    p[i] = h;
                    p[plane + i] = bf16_rne(v - bf16_val(h));
                }
    *steps_out = steps;
    *np_out = np;
    return p;
}

TcnX3Plan tcn_x3_plan(int nconv, const int* k, const int* cpi, const int* cpo, int jk, int base, int T, int nb) {
    TcnX3Plan p;
    int64_t need = T;                                       // capped: a tile that large is refused by its LDS size anyway
    for (int j = nconv - 1; j >= 0; --j) {
        p.rows[j] = (int)need;
        need = std::min<int64_t>(1 << 24, (need - 1) * (j == jk ? base : 1) + k[j]);
    }
    p.rows_in = (int)need;
    int rows_buf[3] = {p.rows_in, 0, 0}, pitch_buf[3] = {x3_pitch(cpi[0]), 8, 8};
    for (int j = 0; j + 1 < nconv; ++j) {
        const int d = 1 + (j & 1);
        rows_buf[d] = std::max(rows_buf[d], p.rows[j]);
        pitch_buf[d] = std::max(pitch_buf[d], x3_pitch(cpo[j]));
    }
    size_t off = 0;
    for (int d = 0; d < 3; ++d) {
        const size_t plane = std::min<size_t>((size_t)nb * rows_buf[d] * pitch_buf[d], size_t(1) << 30);
        p.off[d] = (int)std::min<size_t>(off, size_t(1) << 30);
        p.pitch[d] = pitch_buf[d];
        p.plane[d] = (int)plane;
        off += 2 * plane;
    }
    p.lds_bytes = off * 2;
    return p;
}

hipError_t tcn_x3_launch(const TcnX3Args& a, unsigned grid, size_t lds_bytes, hipStream_t st) {
    hipLaunchKernelGGL(tcn_block_x3_kernel, dim3(grid), dim3(256), lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace rs
