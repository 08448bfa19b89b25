// Training of the TCN (riser/nets/tcn.py as riser/train.py builds it: weight-normed causal convs, dropout, two classes)
// through the receptive cone of the last sample alone.  fp32 throughout; a batch is B reads of ONE length L.
//
// The cone is tcn.hip's: block i (dilation d_i) lives on rows m = 0, 1, ... at positions L-1 - d_i m, `need[i]` of them
// (tcn_windows' arithmetic); on those rows its convs are dense k-tap convs, tap j reading row m + j, and block i + 1 reads
// every base-th row.  A block keeps three buffers, position-major [read][row][cp4(F)]:
//     a1  = drop(relu(conv1(x)))   on the R1 = min((Ro - 1) base + k, need[i]) rows conv2 reads,
//     a2  = drop(relu(conv2(a1)))  on the Ro = need[i + 1] rows m = base m',
//     out = relu(a2 + res)         on the same rows; res = x[base m'] or the 1x1 shortcut of it.
// With ONE length per batch every stored row is a position >= 0 (need[i] <= ceil(L / d_i)), so the zero mask of the forward
// cone - a value at a position below 0 is exactly 0 - is "a row beyond a buffer reads as +0", and such a row takes no
// gradient, gives none to a bias or a weight and passes none on, because it is never visited.
//
//   tcn_train_conv_kernel<FWD>    one launch per conv on v_mfma_f32_16x16x4_f32; M = all reads' rows back to back.  conv2's
//                                 launch also runs the shortcut (or reads the identity), and writes a2 and out.
//   tcn_train_head_kernel,        Linear(F, 2) on the one remaining row; train_loss_kernel (train/kernels.hpp); dW_fc, db_fc
//   tcn_train_head_bwd_kernel     and the gradient arriving at the last block's output.
//   tcn_train_conv_kernel<DGRAD>  the transposed convs, taps flipped.  conv2's (stride base) hands dA1[m] the taps j with
//                                 (m - j) % base == 0; conv1's adds the residual's gradient at rows base m' - dOut gated by
//                                 out > 0, or W_sc^T of it - after the taps, in that order, in the one kernel.  Every
//                                 gradient is gated WHILE IT IS LOADED on what the forward wrote: conv2's on out > 0 and
//                                 a2 > 0, conv1's on a1 > 0, times the dropout scale (a dropped element was written as 0, so
//                                 the value gate is the mask).  The buffers hold the raw incoming gradients dA1 and dOut.
//                                 Block 0 computes no input gradient.
//   tcn_train_wgrad_kernel,       dW [c_out][c_in][k] and db of conv1, conv2 and an applied shortcut: train.hip's contraction
//   train_reduce_kernel           (blocked runs of 64 positions, slices of train/plan.hpp, ascending reduction).
//   tcn_train_wn_bwd_kernel       dW -> dg = (dW . v) / ||v||, dv = (g / ||v||) (dW - (dW . v) v / ||v||^2), in double, rounded
//                                 once; a shortcut's dW and every db are copied.  One launch for the whole net.
//   train_adam_kernel             over the flat parameters: per block g1, v1, b1, g2, v2, b2, the shortcut if applied, then the
//                                 Linear.  An unapplied shortcut never reaches the device.
//   tcn_train_fold_kernel         after every update: W = g v / ||v|| (the norm over [c_in][k] summed in double, ascending,
//                                 rounded once) into the two zero-padded forms the MFMA loops read, [k][p16(c_in)][p16(c_out)]
//                                 and its transpose, tap j = reference tap k - 1 - j.  One launch for the whole net.
//
// Dropout: an element of conv c (2 i for conv1, 2 i + 1 for conv2 of block i) of read b at distance q = L-1 - position from
// the end, channel ch, is kept iff tcn_drop_hash(key_c, b, q, ch) >= floor(p 2^32) and then scaled by float(1 / (1 - p));
// include/riser_amd.h states the hash.  No floating-point atomics anywhere; every sum has one fixed order.
#include "device_prelude.hpp"
#include "family/host.hpp"
#include "train/kernels.hpp"
#include "train/plan.hpp"

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace rs {
namespace {

using namespace train;

enum { FWD = 0, DGRAD = 1 };

constexpr int64_t kMaxDil = int64_t(1) << 40;      // dilations beyond any read length behave alike

__host__ __device__ inline int pad16(int c) { return (c + 15) & ~15; }

// lowbias32: the 32-bit integer finaliser the dropout hash chains
__host__ __device__ inline uint32_t mix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

// the key of conv `conv` in the call that has the step counter `counter` (host side of the hash)
inline uint32_t drop_key(uint64_t seed, uint64_t counter, int conv) {
    uint32_t h = mix32((uint32_t)seed + 0x9e3779b9u);
    h = mix32(h + (uint32_t)(seed >> 32));
    h = mix32(h + (uint32_t)counter);
    h = mix32(h + (uint32_t)(counter >> 32));
    return mix32(h + (uint32_t)conv);
}

__device__ __forceinline__ uint32_t tcn_drop_hash(uint32_t key, uint32_t read, uint32_t q, uint32_t ch) {
    return mix32(mix32(mix32(key + read) + q) + ch);
}

// rows of reads: a position-major buffer [B][rows][pitch], or the signals (first: row r of read b is x[b stride + L-1 - r],
// one channel).  A row outside [0, rows) is +0.
struct Rows {
    const float* p;
    int64_t read_stride;
    int rows, pitch, first, L;
};

__device__ __forceinline__ float rows1(const Rows& s, int b, int64_t r, int c) {
    if (r < 0 || r >= s.rows) return 0.0f;
    if (s.first) return s.p[(int64_t)b * s.read_stride + (s.L - 1 - r)];
    return s.p[(int64_t)b * s.read_stride + r * s.pitch + c];
}

// channels ch .. ch + 3 (those below C) as an MFMA A operand
__device__ __forceinline__ f32x4 rows4(const Rows& s, int b, int64_t r, int ch, int C) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ch >= C || r < 0 || r >= s.rows) return v;
    if (s.first) {
        if (ch == 0) v[0] = s.p[(int64_t)b * s.read_stride + (s.L - 1 - r)];
        return v;
    }
    const f32x4 t = *reinterpret_cast<const f32x4*>(s.p + (int64_t)b * s.read_stride + r * s.pitch + ch);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = ch + i < C ? t[i] : 0.0f;            // pad channels are never written
    return v;
}

// a gradient gated while it is loaded: dy where g1 > 0 (and g2 > 0 where there is one), times scale; [B][rows][pitch] all
struct Grad {
    const float* dy;
    const float* g1;
    const float* g2;
    float scale;
    int rows, pitch;
};

__device__ __forceinline__ float grad1(const Grad& g, int b, int64_t r, int c) {
    if (r < 0 || r >= g.rows) return 0.0f;
    const int64_t at = ((int64_t)b * g.rows + r) * g.pitch + c;
    const float d = g.dy[at], a = g.g1[at], c2 = g.g2 ? g.g2[at] : 1.0f;   // three independent loads, then the gates
    return (a > 0.0f && c2 > 0.0f) ? g.scale * d : 0.0f;
}

__device__ __forceinline__ f32x4 grad4(const Grad& g, int b, int64_t r, int ch, int C) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ch >= C || r < 0 || r >= g.rows) return v;
    const int64_t at = ((int64_t)b * g.rows + r) * g.pitch + ch;
    const f32x4 d = *reinterpret_cast<const f32x4*>(g.dy + at);
    const f32x4 a = *reinterpret_cast<const f32x4*>(g.g1 + at);
    f32x4 c = {1.f, 1.f, 1.f, 1.f};
    if (g.g2) c = *reinterpret_cast<const f32x4*>(g.g2 + at);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (ch + i < C && a[i] > 0.0f && c[i] > 0.0f) ? g.scale * d[i] : 0.0f;
    return v;
}

struct ConvArgs {
    Rows x;                     // FWD: the conv's input
    Rows xr;                    // FWD, res: the block's input (the residual's source)
    Grad g;                     // DGRAD: the gradient of the conv's output
    Grad rg;                    // DGRAD, res: the gradient of the block's output, gated on out > 0
    const float* w;             // FWD [k][p16(kc)][np16]; DGRAD the transposed form, [k][p16(c_out)][p16(c_in)]
    const float* bias;          // FWD [nc]
    const float* sw;            // res: the shortcut in the same form as w (one tap), or null: the identity
    const float* sb;
    float* out;                 // FWD: a1 or a2 [B][R][out_pitch]; DGRAD: the raw gradient [B][R][out_pitch]
    float* out2;                // FWD, res: the block's output
    int res;
    int B, R;                   // reads, output rows per read
    int k, s, rs;               // taps; input rows per output row (DGRAD: output rows per input row); the residual's stride
    int kc, nc, np16, out_pitch, skc;       // K channels, output channels, their pad; the shortcut's K channels
    uint32_t thr, key, qstep;   // FWD dropout: thr 0 applies none; q = qstep * row
    float scale;
};

// A workgroup: 4 waves, each 32 output rows (two MFMA row tiles) of all reads' rows back to back times 16 WC columns.
// K runs over taps, then groups of 16 channels; lane (rl, kq) holds channels 16 g + 4 kq + {0..3} of row rl.
template <int MODE, int WC>
__global__ __launch_bounds__(256) void tcn_train_conv_kernel(const ConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int P = a.B * a.R;                                // rows of all reads: inside the 2 GiB window, so below 2^31
    const int p0 = blockIdx.x * 128 + 32 * wave;
    if (p0 >= P) return;                                    // no barrier in this kernel
    const int col0 = blockIdx.y * (16 * WC);
    const int kp16 = pad16(a.kc), G = kp16 / 16;

    int ab[2], au[2];
    bool aok[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = p0 + 16 * i + rl;
        aok[i] = p < P;
        ab[i] = aok[i] ? p / a.R : 0;
        au[i] = aok[i] ? p - ab[i] * a.R : 0;
    }
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // blocked summation: 128 channels of one tap are summed on their own and then added to the element's sum
    f32x4 sum[2][WC], accs[2][WC];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WC; ++j) sum[i][j] = accs[i][j] = zero;

    for (int tap = 0; tap < a.k; ++tap) {
        int64_t row[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (MODE == FWD) {
                row[i] = aok[i] ? (int64_t)a.s * au[i] + tap : -1;
            } else {
                const int t = au[i] - tap;                  // dst row m takes tap j of output row (m - j) / s
                row[i] = (aok[i] && t >= 0 && t % a.s == 0) ? t / a.s : -1;
            }
        }
        for (int g0 = 0; g0 < G; g0 += 8) {
            f32x4 acc[2][WC];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < WC; ++j) acc[i][j] = zero;
            const int g1 = min(g0 + 8, G);
            for (int g = g0; g < g1; ++g) {
                const int ch = 16 * g + 4 * kq;
                f32x4 av[2], bv[WC];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if constexpr (MODE == FWD) av[i] = rows4(a.x, ab[i], row[i], ch, a.kc);
                    else av[i] = grad4(a.g, ab[i], row[i], ch, a.kc);
                }
                const float* wp = a.w + ((int64_t)tap * kp16 + ch) * a.np16 + col0 + rl;
#pragma unroll
                for (int j = 0; j < WC; ++j)
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
                        bv[j][sub] = col0 + 16 * j < a.np16 ? wp[(int64_t)sub * a.np16 + 16 * j] : 0.0f;
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < WC; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][sub], bv[j][sub], acc[i][j], 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < WC; ++j) sum[i][j] += acc[i][j];
        }
    }
    if (a.res && a.sw) {                                    // the 1x1 shortcut (DGRAD: its transpose) at the strided rows
        const int sG = pad16(a.skc) / 16;
        int64_t row[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            if constexpr (MODE == FWD) row[i] = aok[i] ? (int64_t)a.rs * au[i] : -1;
            else row[i] = (aok[i] && au[i] % a.rs == 0) ? au[i] / a.rs : -1;
        }
        for (int g = 0; g < sG; ++g) {
            const int ch = 16 * g + 4 * kq;
            f32x4 av[2], bv[WC];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if constexpr (MODE == FWD) av[i] = rows4(a.xr, ab[i], row[i], ch, a.skc);
                else av[i] = grad4(a.rg, ab[i], row[i], ch, a.skc);
            }
            const float* wp = a.sw + (int64_t)ch * a.np16 + col0 + rl;
#pragma unroll
            for (int j = 0; j < WC; ++j)
#pragma unroll
                for (int sub = 0; sub < 4; ++sub)
                    bv[j][sub] = col0 + 16 * j < a.np16 ? wp[(int64_t)sub * a.np16 + 16 * j] : 0.0f;
#pragma unroll
            for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < WC; ++j)
                        accs[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][sub], bv[j][sub], accs[i][j], 0, 0, 0);
        }
    }
    // lane element e of row tile i: row p0 + 16 i + 4 kq + e, column col0 + 16 j + rl
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        const int col = col0 + 16 * j + rl;
        if (col >= a.nc) continue;
        float bias = 0.0f, sbias = 0.0f;
        if constexpr (MODE == FWD) {
            bias = a.bias[col];
            if (a.res && a.sw) sbias = a.sb[col];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int p = p0 + 16 * i + 4 * kq + e;
                if (p >= P) continue;
                const int b = p / a.R, u = p - b * a.R;
                const int64_t at = (int64_t)p * a.out_pitch + col;
                if constexpr (MODE == FWD) {
                    float v = fmaxf(sum[i][j][e] + bias, 0.0f);
                    if (a.thr) v = tcn_drop_hash(a.key, (uint32_t)b, a.qstep * (uint32_t)u, (uint32_t)col) >= a.thr ? v * a.scale : 0.0f;
                    a.out[at] = v;
                    if (a.res) {
                        const float r = a.sw ? accs[i][j][e] + sbias : rows1(a.xr, b, (int64_t)a.rs * u, col);
                        a.out2[at] = fmaxf(v + r, 0.0f);
                    }
                } else {
                    float v = sum[i][j][e];                 // the taps first, then the residual: one fixed order
                    if (a.res) {
                        if (a.sw) v += accs[i][j][e];
                        else if (u % a.rs == 0) v += grad1(a.rg, b, u / a.rs, col);
                    }
                    a.out[at] = v;
                }
            }
    }
}

struct WgradArgs {
    Grad g;                     // the gradient of the conv's output, [B][g.rows][g.pitch]
    Rows x;                     // the conv's input
    float* partial;             // [n_slices][c_out c_in k + c_out]
    int c_in, c_out, ci_blocks, slice_len, positions;
    int k, s;                   // taps; input rows per output row
};

// train.hip's train_wgrad_kernel on the cone's rows.  One wave: a 32 (c_out) x 3 x 32 (c_in) tile of dW over one slice of
// positions (all reads' output rows back to back) and, in the first c_in block, the matching 32 entries of db.  Lane (rl, kq)
// holds position p0 + kq: channel co0 + 16 m + rl of the gated gradient (A operand), channel ci0 + 16 n + rl of the input rows
// s u + j of the three taps j of tap group blockIdx.z (B operands).  Tap j is the reference's tap k - 1 - j.
__global__ __launch_bounds__(64) void tcn_train_wgrad_kernel(const WgradArgs a) {
    const int lane = threadIdx.x, rl = lane & 15, kq = lane >> 4;
    const int co0 = (blockIdx.x / a.ci_blocks) * 32, ci0 = (blockIdx.x % a.ci_blocks) * 32;
    const int s = blockIdx.y;
    const int p_begin = s * a.slice_len, p_end = min(p_begin + a.slice_len, a.positions);
    const int kt = a.k, tap0 = kTapGroup * (int)blockIdx.z;
    const int nt = min(kTapGroup, kt - tap0);
    const bool with_bias = ci0 == 0 && tap0 == 0;
    const int R = a.g.rows;

    // blocked summation: a run of 64 positions is summed on its own and then added to the slice's sum
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 sum[2][3][2], sumb[2];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        sumb[m] = zero;
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int n = 0; n < 2; ++n) sum[m][k][n] = zero;
    }
    for (int pc = p_begin; pc < p_end; pc += 64) {
        f32x4 acc[2][3][2], accb[2];
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            accb[m] = zero;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int n = 0; n < 2; ++n) acc[m][k][n] = zero;
        }
        for (int p0 = pc; p0 < pc + 64; p0 += 16) {
            float dz[4][2], av[4][3][2];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int p = p0 + 4 * st + kq;
                const bool valid = p < p_end;
                const int b = valid ? p / R : 0, u = valid ? p - b * R : 0;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int co = co0 + 16 * m + rl;
                    dz[st][m] = (valid && co < a.c_out) ? grad1(a.g, b, u, co) : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int64_t r = (int64_t)a.s * u + tap0 + k;
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int ci = ci0 + 16 * n + rl;
                        av[st][k][n] = (k < nt && valid && ci < a.c_in) ? rows1(a.x, b, r, ci) : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int st = 0; st < 4; ++st)
#pragma unroll
                for (int m = 0; m < 2; ++m) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (k >= nt) continue;
#pragma unroll
                        for (int n = 0; n < 2; ++n)
                            acc[m][k][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[st][m], av[st][k][n], acc[m][k][n], 0, 0, 0);
                    }
                    if (with_bias) accb[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[st][m], 1.0f, accb[m], 0, 0, 0);
                }
        }
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            sumb[m] += accb[m];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int n = 0; n < 2; ++n) sum[m][k][n] += acc[m][k][n];
        }
    }
    // element e: c_out row co0 + 16 m + 4 kq + e, c_in column ci0 + 16 n + rl
    const int64_t n_w = (int64_t)a.c_out * a.c_in * kt;
    float* part = a.partial + (int64_t)s * (n_w + a.c_out);
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = co0 + 16 * m + 4 * kq + e;
            if (co >= a.c_out) continue;
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int ci = ci0 + 16 * n + rl;
                if (ci >= a.c_in) continue;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < nt) part[((int64_t)co * a.c_in + ci) * kt + (kt - 1 - tap0 - k)] = sum[m][k][n][e];
            }
            if (with_bias && rl == 0) part[n_w + co] = sumb[m][e];
        }
}

// the two logits of read b from the one remaining row: a c-ordered fmaf chain
__global__ __launch_bounds__(256) void tcn_train_head_kernel(const float* __restrict__ y, int B, int pitch, int C,
                                                             const float* __restrict__ fcw, const float* __restrict__ fcb,
                                                             float* __restrict__ logits) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float l0 = 0.0f, l1 = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float v = y[(int64_t)b * pitch + c];
        l0 = fmaf(v, fcw[c], l0);
        l1 = fmaf(v, fcw[C + c], l1);
    }
    logits[2 * b] = l0 + fcb[0];
    logits[2 * b + 1] = l1 + fcb[1];
}

// dW_fc[j][c] = sum_b dlogits[b][j] y[b][c], db_fc[j] = sum_b dlogits[b][j], ascending b; dy[b][c] = dlogits[b] . W_fc[:, c]
__global__ __launch_bounds__(256) void tcn_train_head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ y,
                                                                 const float* __restrict__ fcw, int B, int pitch, int C,
                                                                 float* __restrict__ gw, float* __restrict__ gb,
                                                                 float* __restrict__ dy) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        const float w0 = fcw[c], w1 = fcw[C + c];
        float s0 = 0.0f, s1 = 0.0f;
        for (int b = 0; b < B; ++b) {
            const float v = y[(int64_t)b * pitch + c], d0 = dlogits[2 * b], d1 = dlogits[2 * b + 1];
            s0 = fmaf(d0, v, s0);
            s1 = fmaf(d1, v, s1);
            dy[(int64_t)b * pitch + c] = fmaf(d1, w1, d0 * w0);
        }
        gw[c] = s0;
        gw[C + c] = s1;
    }
    if (c < 2) {
        float s = 0.0f;
        for (int b = 0; b < B; ++b) s += dlogits[2 * b + c];
        gb[c] = s;
    }
}

// one conv (or applied shortcut) of the net in the flat vectors; g_off < 0: no weight norm (a shortcut)
struct ConvDesc {
    int64_t g_off, v_off, b_off;        // floats into the parameters and their gradients: g [c_out], v [c_out][c_in][k], b
    int64_t wf_off, wt_off;             // floats into the packed vector
    int64_t tile_off;                   // floats into the tiles: dW [c_out][c_in][k], then db
    int c_in, c_out, k, reserved;
};

// ||v[co]||^2 over [c_in][k], in double, ascending
__device__ __forceinline__ double norm2_of(const float* __restrict__ v, int n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)v[i] * (double)v[i];
    return s;
}

// W = g v / ||v|| (tcn._fold_weight_norm's arithmetic) -> wf [k][p16(c_in)][p16(c_out)] and wt [k][p16(c_out)][p16(c_in)],
// zero padded, tap j = reference tap k - 1 - j.  blockIdx.y: the conv.
__global__ __launch_bounds__(256) void tcn_train_fold_kernel(const ConvDesc* __restrict__ table, const float* __restrict__ params,
                                                             float* __restrict__ packed) {
    const ConvDesc d = table[blockIdx.y];
    const int ci16 = pad16(d.c_in), co16 = pad16(d.c_out);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)d.k * ci16 * co16) return;
    const int co = (int)(i % co16), ci = (int)((i / co16) % ci16), j = (int)(i / ((int64_t)co16 * ci16));
    float w = 0.0f;
    if (ci < d.c_in && co < d.c_out) {
        const int n = d.c_in * d.k;
        const float* v = params + d.v_off + (int64_t)co * n;
        const float vi = v[ci * d.k + (d.k - 1 - j)];
        w = d.g_off < 0 ? vi : (float)((double)params[d.g_off + co] * (double)vi / sqrt(norm2_of(v, n)));
    }
    packed[d.wf_off + i] = w;
    packed[d.wt_off + ((int64_t)j * co16 + co) * ci16 + ci] = w;
}

// the tiles (dW, db) -> the gradients of (g, v, b); a shortcut's tile is copied.  blockIdx.y: the conv.
__global__ __launch_bounds__(256) void tcn_train_wn_bwd_kernel(const ConvDesc* __restrict__ table, const float* __restrict__ params,
                                                               const float* __restrict__ tiles, float* __restrict__ grads) {
    const ConvDesc d = table[blockIdx.y];
    const int n = d.c_in * d.k;
    const int64_t n_w = (int64_t)d.c_out * n;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_w + d.c_out) return;
    const float* tile = tiles + d.tile_off;
    if (i >= n_w) {
        grads[d.b_off + (i - n_w)] = tile[i];
        return;
    }
    if (d.g_off < 0) {
        grads[d.v_off + i] = tile[i];
        return;
    }
    const int co = (int)(i / n);
    const float* v = params + d.v_off + (int64_t)co * n;
    const float* dw = tile + (int64_t)co * n;
    double dot = 0.0;
    for (int e = 0; e < n; ++e) dot += (double)dw[e] * (double)v[e];
    const double n2 = norm2_of(v, n), norm = sqrt(n2);
    const double g = (double)params[d.g_off + co];
    const int e = (int)(i - (int64_t)co * n);
    grads[d.v_off + i] = (float)((g / norm) * ((double)dw[e] - dot * (double)v[e] / n2));
    if (e == 0) grads[d.g_off + co] = (float)(dot / norm);
}

struct ConvHost {
    ConvDesc d;
    LayerShape shape() const {          // what train/plan.hpp plans slices on
        LayerShape s;
        s.c_in = d.c_in;
        s.c_out = d.c_out;
        s.k = d.k;
        s.level = 0;
        s.pool = false;
        return s;
    }
    size_t n_w() const { return (size_t)d.c_out * d.c_in * d.k; }
    size_t tile_floats() const { return n_w() + d.c_out; }
    size_t packed_floats() const { return (size_t)d.k * p16(d.c_in) * p16(d.c_out); }
};

struct BlockHost {
    int c_in = 1, F = 1, k = 2, base = 1;
    int64_t dil = 1;
    bool has_sc = false;
    int conv[3] = {-1, -1, -1};         // indices into the conv table: conv1, conv2, shortcut
};

// rows per read of one call: in[i] = need[i], out[i] = need[i + 1], r1[i] = the rows of a1
struct Cone {
    std::vector<int> in, r1, out;
};

}  // namespace
}  // namespace rs

struct rs_tcn_train {
    int device = -1;            // < 0: a handle without device memory (the plans and the argument checks only)
    int n_blocks = 0, F = 1, k = 2;
    std::vector<rs::BlockHost> blocks;
    std::vector<rs::ConvHost> convs;
    std::vector<std::pair<size_t, size_t>> tensors;        // (offset, count) of every tensor of the flat vector, in index order
    std::vector<int> tensor_conv;                           // the conv a tensor belongs to, -1: the Linear
    size_t n_params = 0, fcw_off = 0, fcb_off = 0, n_packed = 0, n_tiles = 0, max_fold = 0, max_tile = 0;
    rs::DevBuf<float> params, grads, m, v, packed, tiles;
    rs::DevBuf<rs::ConvDesc> table;
    int64_t step = 0;
    double drop_p = 0.0;
    uint64_t seed = 0;
    int64_t counter = 0;        // rs_tcn_train_forward_backward calls that returned RS_OK
    void* last_ws = nullptr;    // rs_tcn_train_debug_copy: as rs_train's
    int last_B = 0, last_L = 0;
};

namespace rs {
namespace {

Cone cone_of(const rs_tcn_train* h, int L) {
    const int n = h->n_blocks;
    std::vector<int64_t> need(n + 1, 1);
    for (int i = n - 1; i >= 0; --i) {
        const BlockHost& b = h->blocks[i];
        const int64_t cap = (L + b.dil - 1) / b.dil;
        const int64_t prev = need[i + 1] - 1;
        const int64_t want = prev > (int64_t)L / b.base + 1 ? cap + 1 : prev * b.base + 1 + 2 * (int64_t)(b.k - 1);
        need[i] = std::min(want, cap);
    }
    Cone c;
    for (int i = 0; i < n; ++i) {
        const BlockHost& b = h->blocks[i];
        c.in.push_back((int)need[i]);
        c.out.push_back((int)need[i + 1]);
        // (need - 1) base < need[i] <= L: a stored output row's position is one of the block's input rows
        c.r1.push_back((int)std::min<int64_t>((need[i + 1] - 1) * b.base + b.k, need[i]));
    }
    return c;
}

struct Plan {
    Cone cone;
    std::vector<size_t> a1, out;        // bytes of a block's a1 (and dA1) and of its a2, out, dOut each
    size_t dlogits = 0, flag = 256, partials = 0, largest = 0, total = 0;
};

// slices of conv `c` of block i: it contracts the rows of its OUTPUT gradient
SlicePlan slices_of(const rs_tcn_train* h, const Cone& cone, int i, int which, int B) {
    const ConvHost& c = h->convs[h->blocks[i].conv[which]];
    return plan_slices(c.shape(), 0, B, which == 0 ? cone.r1[i] : cone.out[i]);
}

Plan plan_of(const rs_tcn_train* h, int B, int L) {
    Plan p;
    p.cone = cone_of(h, L);
    const size_t row = (size_t)cp4(h->F) * sizeof(float);
    for (int i = 0; i < h->n_blocks; ++i) {
        p.a1.push_back((size_t)B * p.cone.r1[i] * row);
        p.out.push_back((size_t)B * p.cone.out[i] * row);
        p.total += 2 * round256(p.a1[i]) + 3 * round256(p.out[i]);
        p.largest = std::max({p.largest, p.a1[i], p.out[i]});
        for (int which = 0; which < 3; ++which) {
            if (h->blocks[i].conv[which] < 0) continue;
            const SlicePlan sp = slices_of(h, p.cone, i, which, B);
            p.partials = std::max(p.partials, (size_t)sp.n_slices * h->convs[h->blocks[i].conv[which]].tile_floats() * sizeof(float));
        }
    }
    p.dlogits = (size_t)B * 2 * sizeof(float);
    p.largest = std::max({p.largest, p.partials, (size_t)B * L * sizeof(float)});
    p.total += round256(p.dlogits) + round256(p.flag) + round256(p.partials);
    return p;
}

struct Carved {
    std::vector<float*> a1, a2, out, da1, dout;
    float *dlogits, *partials;
    int32_t* flag;
};

Carved carve(const Plan& p, void* d_ws) {
    Carver ws(d_ws);
    Carved c;
    for (size_t i = 0; i < p.a1.size(); ++i) {
        c.a1.push_back(ws.take(p.a1[i]));
        c.a2.push_back(ws.take(p.out[i]));
        c.out.push_back(ws.take(p.out[i]));
        c.da1.push_back(ws.take(p.a1[i]));
        c.dout.push_back(ws.take(p.out[i]));
    }
    c.dlogits = ws.take(p.dlogits);
    c.flag = ws.take<int32_t>(p.flag);
    c.partials = ws.take(p.partials);
    return c;
}

template <int MODE>
void launch_conv(const ConvArgs& a, hipStream_t st) {
    const int64_t P = (int64_t)a.B * a.R;
    const unsigned gx = (unsigned)((P + 127) / 128);
    const dim3 block(256);
    if (a.nc <= 16) {
        hipLaunchKernelGGL((tcn_train_conv_kernel<MODE, 1>), dim3(gx, (a.np16 + 15) / 16), block, 0, st, a);
    } else if (a.nc <= 32) {
        hipLaunchKernelGGL((tcn_train_conv_kernel<MODE, 2>), dim3(gx, (a.np16 + 31) / 32), block, 0, st, a);
    } else {
        hipLaunchKernelGGL((tcn_train_conv_kernel<MODE, 4>), dim3(gx, (a.np16 + 63) / 64), block, 0, st, a);
    }
}

int fold_all(rs_tcn_train* h, hipStream_t st) {
    hipLaunchKernelGGL(tcn_train_fold_kernel, dim3((unsigned)((h->max_fold + 255) / 256), (unsigned)h->convs.size()), dim3(256), 0,
                       st, h->table.p, h->params.p, h->packed.p);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

int check_call(const char* fn, const rs_tcn_train* h, const void* d_x, const void* d_labels, const void* d_ws, const void* d_out,
               int B, int L, int ld, size_t ws_bytes) {
    if (!h || !d_x || !d_labels || !d_ws || !d_out || B < 1 || L < 1 || ld < L) {
        set_error("%s: bad argument", fn);
        return RS_ERR_ARG;
    }
    if (ws_bytes < rs_tcn_train_workspace_bytes(h, B, L)) {
        set_error("%s: workspace too small", fn);
        return RS_ERR_WORKSPACE;
    }
    if (B > rs_tcn_train_max_batch(h, L) || (int64_t)B * ld * 4 > kWindow) {
        set_error("%s: %d reads of %d samples outgrow the 2 GiB buffer window: split the batch (rs_tcn_train_max_batch)", fn, B, ld);
        return RS_ERR_ARG;
    }
    if (h->device < 0) {
        set_error("%s: the handle was made without a device", fn);
        return RS_ERR_ARG;
    }
    return RS_OK;
}

Rows rows_of(const float* p, int B, int rows, int C) {
    Rows r;
    r.p = p;
    r.rows = rows;
    r.pitch = cp4(C);
    r.read_stride = (int64_t)rows * r.pitch;
    r.first = 0;
    r.L = 0;
    return r;
}

Grad grad_of(const float* dy, const float* g1, const float* g2, float scale, int rows, int C) {
    Grad g;
    g.dy = dy;
    g.g1 = g1;
    g.g2 = g2;
    g.scale = scale;
    g.rows = rows;
    g.pitch = cp4(C);
    return g;
}

int run(rs_tcn_train* h, const char* fn, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
        size_t ws_bytes, float* d_out, void* stream, bool backward) {
    if (h) h->last_ws = nullptr;                            // this call may carve the same workspace at other offsets
    const int rc = check_call(fn, h, d_x, d_labels, d_ws, d_out, B, L, ld, ws_bytes);
    if (rc != RS_OK) return rc;
    DeviceGuard guard(h->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Plan plan = plan_of(h, B, L);
    const Cone& cone = plan.cone;
    const Carved c = carve(plan, d_ws);
    const int n = h->n_blocks, F = h->F;
    const bool drop = backward && h->drop_p > 0.0;          // evaluate is eval mode
    const uint32_t thr = drop ? (uint32_t)std::floor(h->drop_p * 4294967296.0) : 0u;
    const float scale = (drop && thr) ? (float)(1.0 / (1.0 - h->drop_p)) : 1.0f;

    Rows sig;
    sig.p = d_x;
    sig.read_stride = ld;
    sig.rows = cone.in[0];
    sig.pitch = 1;
    sig.first = 1;
    sig.L = L;
    auto input_of = [&](int i) { return i ? rows_of(c.out[i - 1], B, cone.in[i], F) : sig; };

    for (int i = 0; i < n; ++i) {
        const BlockHost& b = h->blocks[i];
        const uint32_t dq = (uint32_t)std::min<int64_t>(b.dil, (int64_t)L);     // a row m > 0 exists only where d m < L
        for (int which = 0; which < 2; ++which) {
            const ConvHost& cv = h->convs[b.conv[which]];
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.x = which ? rows_of(c.a1[i], B, cone.r1[i], F) : input_of(i);
            a.w = h->packed + cv.d.wf_off;
            a.bias = h->params + cv.d.b_off;
            a.out = which ? c.a2[i] : c.a1[i];
            a.B = B;
            a.R = which ? cone.out[i] : cone.r1[i];
            a.k = b.k;
            a.s = which ? b.base : 1;
            a.rs = b.base;
            a.kc = cv.d.c_in;
            a.nc = F;
            a.np16 = p16(F);
            a.out_pitch = cp4(F);
            a.thr = thr;
            a.key = drop_key(h->seed, (uint64_t)h->counter, 2 * i + which);
            a.qstep = which ? (uint32_t)std::min<int64_t>((int64_t)dq * b.base, (int64_t)L) : dq;
            a.scale = scale;
            if (which) {
                a.res = 1;
                a.xr = input_of(i);
                a.out2 = c.out[i];
                a.skc = b.c_in;
                if (b.has_sc) {
                    a.sw = h->packed + h->convs[b.conv[2]].d.wf_off;
                    a.sb = h->params + h->convs[b.conv[2]].d.b_off;
                }
            }
            launch_conv<FWD>(a, st);
            RS_HIP(hipGetLastError());
        }
    }
    const int pitch = cp4(F);
    hipLaunchKernelGGL(tcn_train_head_kernel, dim3((B + 255) / 256), dim3(256), 0, st, c.out[n - 1], B, pitch, F,
                       h->params + h->fcw_off, h->params + h->fcb_off, d_out + 2);
    RS_HIP(hipGetLastError());
    hipLaunchKernelGGL(train_loss_kernel, dim3(1), dim3(64), 0, st, d_out, d_labels, B, c.dlogits, c.flag);
    RS_HIP(hipGetLastError());
    if (backward) {
        hipLaunchKernelGGL(tcn_train_head_bwd_kernel, dim3((std::max(F, 2) + 255) / 256), dim3(256), 0, st, c.dlogits, c.out[n - 1],
                           h->params + h->fcw_off, B, pitch, F, h->grads + h->fcw_off, h->grads + h->fcb_off, c.dout[n - 1]);
        RS_HIP(hipGetLastError());
        for (int i = n - 1; i >= 0; --i) {
            const BlockHost& b = h->blocks[i];
            // the three gated gradients of the block: of conv2's output, of conv1's, and the residual's
            const Grad g2 = grad_of(c.dout[i], c.out[i], c.a2[i], scale, cone.out[i], F);
            const Grad g1 = grad_of(c.da1[i], c.a1[i], nullptr, scale, cone.r1[i], F);
            const Grad gr = grad_of(c.dout[i], c.out[i], nullptr, 1.0f, cone.out[i], F);
            auto wgrad = [&](int which, const Grad& g, const Rows& x, int stride) -> int {
                const ConvHost& cv = h->convs[b.conv[which]];
                const SlicePlan sp = slices_of(h, cone, i, which, B);
                WgradArgs w;
                memset(&w, 0, sizeof(w));
                w.g = g;
                w.x = x;
                w.partial = c.partials;
                w.c_in = cv.d.c_in;
                w.c_out = cv.d.c_out;
                w.ci_blocks = (cv.d.c_in + 31) / 32;
                w.slice_len = sp.slice_len;
                w.positions = B * g.rows;
                w.k = cv.d.k;
                w.s = stride;
                const unsigned tiles = (unsigned)(w.ci_blocks * ((cv.d.c_out + 31) / 32));
                hipLaunchKernelGGL(tcn_train_wgrad_kernel, dim3(tiles, (unsigned)sp.n_slices, (unsigned)tap_groups(cv.d.k)), dim3(64),
                                   0, st, w);
                RS_HIP(hipGetLastError());
                const int64_t n_tile = (int64_t)cv.tile_floats();
                hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)((n_tile + 255) / 256)), dim3(256), 0, st, c.partials,
                                   sp.n_slices, n_tile, h->tiles + cv.d.tile_off);
                RS_HIP(hipGetLastError());
                return RS_OK;
            };
            int rcw = wgrad(1, g2, rows_of(c.a1[i], B, cone.r1[i], F), b.base);
            if (rcw != RS_OK) return rcw;
            if (b.has_sc) {
                rcw = wgrad(2, gr, input_of(i), b.base);
                if (rcw != RS_OK) return rcw;
            }
            {                                               // dA1 = conv2^T of its gated gradient
                const ConvHost& cv = h->convs[b.conv[1]];
                ConvArgs a;
                memset(&a, 0, sizeof(a));
                a.g = g2;
                a.w = h->packed + cv.d.wt_off;
                a.out = c.da1[i];
                a.B = B;
                a.R = cone.r1[i];
                a.k = b.k;
                a.s = b.base;
                a.rs = 1;
                a.kc = F;
                a.nc = F;
                a.np16 = p16(F);
                a.out_pitch = cp4(F);
                launch_conv<DGRAD>(a, st);
                RS_HIP(hipGetLastError());
            }
            rcw = wgrad(0, g1, input_of(i), 1);
            if (rcw != RS_OK) return rcw;
            if (i == 0) break;                              // block 0 computes no input gradient
            {                                               // dOut of block i - 1 = conv1^T of its gated gradient + the residual's
                const ConvHost& cv = h->convs[b.conv[0]];
                ConvArgs a;
                memset(&a, 0, sizeof(a));
                a.g = g1;
                a.rg = gr;
                a.res = 1;
                a.w = h->packed + cv.d.wt_off;
                a.out = c.dout[i - 1];
                a.B = B;
                a.R = cone.in[i];
                a.k = b.k;
                a.s = 1;
                a.rs = b.base;
                a.kc = F;
                a.nc = b.c_in;
                a.np16 = p16(b.c_in);
                a.out_pitch = cp4(b.c_in);
                a.skc = F;
                if (b.has_sc) a.sw = h->packed + h->convs[b.conv[2]].d.wt_off;
                launch_conv<DGRAD>(a, st);
                RS_HIP(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(tcn_train_wn_bwd_kernel, dim3((unsigned)((h->max_tile + 255) / 256), (unsigned)h->convs.size()), dim3(256),
                           0, st, h->table.p, h->params.p, h->tiles.p, h->grads.p);
        RS_HIP(hipGetLastError());
    }
    int32_t bad = 0;                                        // the label check's answer is this call's status
    RS_HIP(hipMemcpyAsync(&bad, c.flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    if (bad) {
        set_error("%s: a label outside {0, 1}", fn);
        return RS_ERR_ARG;
    }
    if (backward) {
        h->counter += 1;
        h->last_ws = d_ws;
        h->last_B = B;
        h->last_L = L;
    }
    return RS_OK;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" {

int rs_tcn_train_destroy(rs_tcn_train* h) {
    if (!h) return RS_OK;
    if (h->device >= 0) {
        DeviceGuard guard(h->device);
        delete h;                       // every device buffer is a DevBuf: freed with its holder
    } else {
        delete h;
    }
    return RS_OK;
}

int rs_tcn_train_create(const rs_tcn_train_config* cfg, const float* const* tensors, int n_tensors, int device, rs_tcn_train** out) {
    if (!out) {
        set_error("rs_tcn_train_create: null output handle");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    if (!cfg) {
        set_error("rs_tcn_train_create: null config");
        return RS_ERR_ARG;
    }
    if (cfg->bottleneck) {
        set_error("rs_tcn_train_create: the bottleneck TCN (tcn-bot) does not train here");
        return RS_ERR_ARG;
    }
    if (cfg->dtype != RS_F32) {
        set_error("rs_tcn_train_create: dtype %d: TCN training is fp32 (RS_F32) only", cfg->dtype);
        return RS_ERR_ARG;
    }
    if (cfg->n_classes != 2 || cfg->in_channels != 1 || cfg->kernel < 2) {
        set_error("rs_tcn_train_create: two classes, one input channel and a kernel >= 2 (got %d, %d, %d)", cfg->n_classes,
                  cfg->in_channels, cfg->kernel);
        return RS_ERR_ARG;
    }
    if (!(cfg->dropout >= 0.0 && cfg->dropout < 1.0)) {
        set_error("rs_tcn_train_create: dropout outside [0, 1)");
        return RS_ERR_ARG;
    }
    if (cfg->n_layers < 1 || cfg->n_layers > 64 || cfg->n_filters < 1 || cfg->n_filters > 4096 || cfg->kernel > 1024 ||
        cfg->dilation < 1) {
        set_error("rs_tcn_train_create: bad shape (n_layers 1-64, n_filters 1-4096, kernel 2-1024, dilation >= 1)");
        return RS_ERR_ARG;
    }
    rs_tcn_train* h = new (std::nothrow) rs_tcn_train();
    if (!h) return RS_ERR_OOM;
    h->device = device < 0 ? -1 : device;
    h->n_blocks = cfg->n_layers;
    h->F = cfg->n_filters;
    h->k = cfg->kernel;
    h->drop_p = cfg->dropout;
    h->seed = cfg->seed;
    size_t off = 0, poff = 0, toff = 0;
    int64_t dil = 1;
    auto add_conv = [&](int c_in, int c_out, int k, bool wn) {
        ConvHost c;
        memset(&c.d, 0, sizeof(c.d));
        c.d.c_in = c_in;
        c.d.c_out = c_out;
        c.d.k = k;
        c.d.g_off = -1;
        if (wn) {
            c.d.g_off = (int64_t)off;
            h->tensors.push_back({off, (size_t)c_out});
            off += c_out;
        }
        c.d.v_off = (int64_t)off;
        h->tensors.push_back({off, c.n_w()});
        off += c.n_w();
        c.d.b_off = (int64_t)off;
        h->tensors.push_back({off, (size_t)c_out});
        off += c_out;
        c.d.wf_off = (int64_t)poff;
        c.d.wt_off = (int64_t)(poff + c.packed_floats());
        poff += 2 * c.packed_floats();
        c.d.tile_off = (int64_t)toff;
        toff += c.tile_floats();
        h->max_fold = std::max(h->max_fold, c.packed_floats());
        h->max_tile = std::max(h->max_tile, c.tile_floats());
        for (int t = 0; t < (wn ? 3 : 2); ++t) h->tensor_conv.push_back((int)h->convs.size());
        h->convs.push_back(c);
        return (int)h->convs.size() - 1;
    };
    for (int i = 0; i < cfg->n_layers; ++i) {
        BlockHost b;
        b.c_in = i == 0 ? 1 : cfg->n_filters;
        b.F = cfg->n_filters;
        b.k = cfg->kernel;
        b.base = cfg->dilation;
        b.dil = dil;
        b.has_sc = b.c_in != b.F;                           // should_apply_shortcut (tcn.py:57-59)
        b.conv[0] = add_conv(b.c_in, b.F, b.k, true);
        b.conv[1] = add_conv(b.F, b.F, b.k, true);
        if (b.has_sc) b.conv[2] = add_conv(b.c_in, b.F, 1, false);
        h->blocks.push_back(b);
        dil = std::min<int64_t>(kMaxDil, dil * cfg->dilation);
    }
    h->fcw_off = off;
    h->tensors.push_back({off, 2 * (size_t)h->F});
    off += 2 * (size_t)h->F;
    h->fcb_off = off;
    h->tensors.push_back({off, 2});
    off += 2;
    h->tensor_conv.push_back(-1);
    h->tensor_conv.push_back(-1);
    h->n_params = off;
    h->n_packed = poff;
    h->n_tiles = toff;
    if (!tensors || n_tensors != (int)h->tensors.size()) {
        set_error("rs_tcn_train_create: %d tensors given, the net has %d (per block g1, v1, b1, g2, v2, b2, an applied shortcut's "
                  "weight and bias; then the Linear's)", tensors ? n_tensors : 0, (int)h->tensors.size());
        delete h;
        return RS_ERR_ARG;
    }
    for (int t = 0; t < n_tensors; ++t)
        if (!tensors[t]) {
            set_error("rs_tcn_train_create: tensor %d is null", t);
            delete h;
            return RS_ERR_ARG;
        }
    if (device < 0) {
        *out = h;
        return RS_OK;
    }
    std::vector<float> flat(h->n_params);
    for (int t = 0; t < n_tensors; ++t) std::copy(tensors[t], tensors[t] + h->tensors[t].second, flat.begin() + h->tensors[t].first);
    std::vector<ConvDesc> table;
    for (const ConvHost& c : h->convs) table.push_back(c.d);
    DeviceGuard guard(device);
    hipError_t e = guard.err;
    const std::vector<float> zeros(h->n_params, 0.0f);
    if (e == hipSuccess) e = upload(h->params, flat);
    if (e == hipSuccess) e = upload(h->grads, zeros);
    if (e == hipSuccess) e = upload(h->m, zeros);
    if (e == hipSuccess) e = upload(h->v, zeros);
    if (e == hipSuccess) e = upload(h->table, table);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->packed.p), h->n_packed * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->tiles.p), h->n_tiles * sizeof(float));
    int rc = RS_OK;
    if (e == hipSuccess) rc = fold_all(h, nullptr);
    if (e == hipSuccess && rc == RS_OK) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess || rc != RS_OK) {
        rs_tcn_train_destroy(h);
        return e != hipSuccess ? hip_fail(e, "rs_tcn_train_create upload") : rc;
    }
    *out = h;
    return RS_OK;
}

size_t rs_tcn_train_workspace_bytes(const rs_tcn_train* h, int B, int L) {
    if (!h || B < 1 || L < 1) return 0;
    return plan_of(h, B, L).total;
}

int rs_tcn_train_max_batch(const rs_tcn_train* h, int L) {
    if (!h || L < 1) return 0;
    const Plan one = plan_of(h, 1, L);
    size_t per = (size_t)L * sizeof(float);
    for (int i = 0; i < h->n_blocks; ++i) per = std::max({per, one.a1[i], one.out[i]});
    return max_batch_of(per);           // every grid's x is rows / 128 of such a buffer; the slices are capped by the plan
}

int rs_tcn_train_slice_plan(const rs_tcn_train* h, int block, int which, int B, int L, int32_t* n_slices, int32_t* slice_len,
                            int32_t* rows) {
    if (!h || block < 0 || block >= h->n_blocks || which < 0 || which > 2 || B < 1 || L < 1 || !n_slices || !slice_len || !rows ||
        h->blocks[block].conv[which] < 0) {
        set_error("rs_tcn_train_slice_plan: bad argument (handle, block, which 0 conv1 / 1 conv2 / 2 an applied shortcut, B, L)");
        return RS_ERR_ARG;
    }
    const Cone cone = cone_of(h, L);
    const SlicePlan p = slices_of(h, cone, block, which, B);
    *n_slices = p.n_slices;
    *slice_len = p.slice_len;
    *rows = which == 0 ? cone.r1[block] : cone.out[block];
    return RS_OK;
}

int rs_tcn_train_forward_backward(rs_tcn_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
                                  size_t ws_bytes, float* d_out, void* stream) {
    return run(h, "rs_tcn_train_forward_backward", d_x, d_labels, B, L, ld, d_ws, ws_bytes, d_out, stream, true);
}

int rs_tcn_train_evaluate(rs_tcn_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
                          size_t ws_bytes, float* d_out, void* stream) {
    return run(h, "rs_tcn_train_evaluate", d_x, d_labels, B, L, ld, d_ws, ws_bytes, d_out, stream, false);
}

int rs_tcn_train_set_dropout(rs_tcn_train* h, double p, uint64_t seed, int64_t counter) {
    if (!h || !(p >= 0.0 && p < 1.0) || counter < 0) {
        set_error("rs_tcn_train_set_dropout: bad argument (handle, p in [0, 1), counter >= 0)");
        return RS_ERR_ARG;
    }
    h->drop_p = p;
    h->seed = seed;
    h->counter = counter;
    return RS_OK;
}

int rs_tcn_train_adam_step(rs_tcn_train* h, float lr, float beta1, float beta2, float eps, void* stream) {
    if (!h || !(lr > 0.0f) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f)) {
        set_error("rs_tcn_train_adam_step: bad argument (handle, lr > 0, betas in [0, 1), eps >= 0)");
        return RS_ERR_ARG;
    }
    if (h->device < 0) {
        set_error("rs_tcn_train_adam_step: the handle was made without a device");
        return RS_ERR_ARG;
    }
    DeviceGuard guard(h->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    h->step += 1;
    const double bc1 = 1.0 - std::pow((double)beta1, (double)h->step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)h->step);
    hipLaunchKernelGGL(train_adam_kernel, dim3((unsigned)((h->n_params + 255) / 256)), dim3(256), 0, st, h->params.p, h->grads.p,
                       h->m.p, h->v.p, (int64_t)h->n_params, beta1, beta2, (float)((double)lr / bc1), (float)std::sqrt(bc2), eps);
    RS_HIP(hipGetLastError());
    return fold_all(h, st);             // the fold runs after every update: the packed forms are W = g v / ||v|| again
}

static int copy_tensor(rs_tcn_train* h, const char* fn, int index, float* get_dst, const float* set_src, size_t count, bool grads) {
    if (!h || (!get_dst && !set_src) || index < 0 || index >= (int)h->tensors.size() || count != h->tensors[index].second) {
        set_error("%s: bad argument (handle, host array, tensor index, its element count)", fn);
        return RS_ERR_ARG;
    }
    if (h->device < 0) {
        set_error("%s: the handle was made without a device", fn);
        return RS_ERR_ARG;
    }
    const size_t off = h->tensors[index].first;
    DeviceGuard guard(h->device);
    RS_HIP(guard.err);
    RS_HIP(hipDeviceSynchronize());
    if (get_dst) {
        RS_HIP(hipMemcpy(get_dst, (grads ? h->grads.p : h->params.p) + off, count * sizeof(float), hipMemcpyDeviceToHost));
        return RS_OK;
    }
    RS_HIP(hipMemcpy(h->params.p + off, set_src, count * sizeof(float), hipMemcpyHostToDevice));
    if (h->tensor_conv[index] >= 0) {
        const int rc = fold_all(h, nullptr);
        if (rc != RS_OK) return rc;
        RS_HIP(hipStreamSynchronize(nullptr));
    }
    return RS_OK;
}

int rs_tcn_train_get_params(rs_tcn_train* h, int index, float* dst, size_t count) {
    return copy_tensor(h, "rs_tcn_train_get_params", index, dst, nullptr, count, false);
}

int rs_tcn_train_get_grads(rs_tcn_train* h, int index, float* dst, size_t count) {
    return copy_tensor(h, "rs_tcn_train_get_grads", index, dst, nullptr, count, true);
}

int rs_tcn_train_set_params(rs_tcn_train* h, int index, const float* src, size_t count) {
    return copy_tensor(h, "rs_tcn_train_set_params", index, nullptr, src, count, false);
}

int rs_tcn_train_debug_copy(rs_tcn_train* h, int block, int what, void* d_dst, size_t bytes) {
    if (!h || block < 0 || block >= h->n_blocks || what < 0 || what > 4 || !d_dst) {
        set_error("rs_tcn_train_debug_copy: bad argument (handle, block, what 0 a1 / 1 a2 / 2 out / 3 dA1 / 4 dOut, destination)");
        return RS_ERR_ARG;
    }
    if (!h->last_ws) {
        set_error("rs_tcn_train_debug_copy: no rs_tcn_train_forward_backward has run on this handle since the last "
                  "rs_tcn_train_evaluate or refused call");
        return RS_ERR_ARG;
    }
    const Plan plan = plan_of(h, h->last_B, h->last_L);
    const size_t need = (what == 0 || what == 3) ? plan.a1[block] : plan.out[block];
    if (bytes < need) {
        set_error("rs_tcn_train_debug_copy: the destination holds %zu bytes, the buffer has %zu", bytes, need);
        return RS_ERR_ARG;
    }
    DeviceGuard guard(h->device);
    RS_HIP(guard.err);
    const Carved c = carve(plan, h->last_ws);
    const float* src[5] = {c.a1[block], c.a2[block], c.out[block], c.da1[block], c.dout[block]};
    RS_HIP(hipDeviceSynchronize());
    RS_HIP(hipMemcpy(d_dst, src[what], need, hipMemcpyDeviceToDevice));
    return RS_OK;
}

}  // extern "C"
