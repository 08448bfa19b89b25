// Training of the ConvNet (riser/nets/cnn.py:12-18,43-65 with `gap_fc`, two classes; riser/train.py:31-80,197-198): forward
// with what the backward pass needs, cross-entropy, backward, Adam.  fp32 throughout.  rs_train_create makes the shipped class
// (depth 1, every kernel 3), rs_train_create_generic any depth and any odd kernels: n_layers x [depth x (conv k_i + ReLU),
// MaxPool(2, 2)], convs numbered j = layer * depth + d.  The last conv of a layer pools; every other is an INNER conv.
//
// Activations are position-major fp32 [read][t][cp4(C)] as in gconv.hip; a batch is B reads of ONE length L, so after l pools
// every read owns L >> l rows.  The kernels (K3: three taps at compile time - the shipped class's instantiations - or the
// conv's k at run time; POOL: the pooling or the inner form):
//
//   train_conv_kernel<FWD>   per conv: conv k + bias + ReLU on v_mfma_f32_16x16x4_f32, tap t reading row q + t - (k - 1) / 2.
//                            POOL: + MaxPool(2, 2).  Writes the pooled rows y and one selector byte per pooled element: 1
//                            where ReLU(row 2j + 1) is strictly larger than ReLU(row 2j) - torch's rule - else 0.  A read's
//                            odd last conv row is computed as its neighbour's right-hand input and dropped by the pool.
//                            Inner: writes all T rows r at full resolution, the odd last one included; no selector - the
//                            backward pass gates on r > 0 of what was written.
//   train_head_kernel,       GAP + Linear(c_last, 2); loss (mean cross-entropy through a stable log-softmax), logits, count of
//   train_loss_kernel,       correct argmax, dlogits = (softmax - onehot) / B; dW_fc, db_fc; dY_last = (dlogits . W_fc) / rows.
//   train_fc_grad_kernel,    Plain C++: they are tiny.
//   train_head_bwd_kernel
//   train_conv_kernel<DGRAD> convs n-1 .. 1: dY_{j-1}[t][ci] = sum_{tap, co} W_j[co][ci][tap] dZ_j[t + (k - 1) / 2 - tap][co],
//                            the forward loop with the taps flipped around the centre and the transposed weight form.  Its
//                            A operand is dZ_j, formed while it is loaded.  POOL: dY_j[u >> 1] where y_j[u >> 1] > 0 and the
//                            selector equals u & 1, else +0; rows u >= 2 (rows >> 1) are +0 - no un-pooled gradient is ever
//                            written.  Inner: dY_j[u] where r_j[u] > 0, else +0, on all T rows.  The output is the gradient
//                            of whatever conv j - 1 wrote: pooled rows or full-resolution rows, T rows either way.
//   train_wgrad_kernel,      every conv: dW_j[co][ci][tap] = sum_{b, u} dZ_j[b][u][co] A_{j-1}[b][u + tap - (k - 1) / 2][ci]
//   train_reduce_kernel      and db_j = sum dZ_j (an MFMA against a column of ones).  M = c_out, N = k c_in, K = all
//                            positions of all reads, cut into the slices of train/plan.hpp.  A wave holds at most three
//                            taps (plan.hpp's tap groups, one per grid z: k = 5 runs 3 + 2, k = 7 3 + 3 + 1), so its
//                            registers do not grow with k; each group writes its own columns of the slice's partial tile,
//                            the first one the bias column; the second kernel adds the partials in ascending slice order.
//                            No floating-point atomics anywhere.  Both dZ forms feed it.
//   train_adam_kernel        one launch over the flat master parameters, torch.optim.Adam's defaults and operation order.
//                            It, train_loss_kernel and train_reduce_kernel live in train/kernels.hpp, shared with tcn_train.hip.
//   train_pack_kernel        per conv, after every update: the two zero-padded forms the MFMA loops read,
//                            [k][p16(c_in)][p16(c_out)] (forward) and [k][p16(c_out)][p16(c_in)] (data gradient).
//
// Every operand fragment is loaded straight from global memory: 16 lanes read 64 contiguous bytes.  Tile shapes depend on
// (c_in, c_out) only.
#include "device_prelude.hpp"
#include "family/host.hpp"
#include "gconv/plan.hpp"
#include "train/kernels.hpp"
#include "train/plan.hpp"

#include <cmath>
#include <new>
#include <vector>

namespace rs {
namespace {

using namespace train;

enum { FWD = 0, DGRAD = 1 };

__host__ __device__ inline int pad16(int c) { return (c + 15) & ~15; }

struct ConvArgs {
    const float* x;             // FWD: the conv's input [B][T][x_pitch] (conv 0: the signals, pitch 1, read stride ld)
                                // DGRAD: dY_j [B][T >> 1][x_pitch], inner conv [B][T][x_pitch]
    const float* yl;            // DGRAD: y_j (inner conv: r_j), same shape
    const uint8_t* sel;         // DGRAD: selectors of a pooling conv, same shape
    float* out;                 // FWD: y_j [B][T >> 1][out_pitch], inner conv r_j [B][T][out_pitch]; DGRAD: dY_{j-1} [B][T][out_pitch]
    uint8_t* sel_out;           // FWD, pooling conv
    const float* w;             // [k][p16(kc)][np16]
    const float* bias;          // FWD: [nc]
    int64_t x_read_stride;
    int x_pitch, T, kc, nc, np16, out_pitch, tiles;
    int k;                      // taps (the K3 instantiations run three whatever this says)
};

// four K channels ch .. ch + 3 of conv row q of read b, as the MFMA's A operand
template <int MODE, bool POOL>
__device__ __forceinline__ f32x4 load_a(const ConvArgs& a, int b, int q, int ch) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ch >= a.kc) return v;
    if constexpr (MODE == FWD) {
        if (q < 0 || q >= a.T) return v;
        const float* p = a.x + (int64_t)b * a.x_read_stride + (int64_t)q * a.x_pitch + ch;
        if ((a.x_pitch & 3) == 0) {
            const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ch + i < a.kc ? t[i] : 0.0f;      // pad channels are never written
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (ch + i < a.kc) v[i] = p[i];
        }
    } else if constexpr (!POOL) {
        if (q < 0 || q >= a.T) return v;                    // every row of an inner conv takes its gradient, an odd last one too
        const int64_t at = ((int64_t)b * a.T + q) * a.x_pitch + ch;
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.x + at);
        const f32x4 r = *reinterpret_cast<const f32x4*>(a.yl + at);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (ch + i < a.kc && r[i] > 0.0f) ? g[i] : 0.0f;
    } else {
        const int Th = a.T >> 1;
        if (q < 0 || q >= 2 * Th) return v;                 // the dropped odd row takes no gradient
        const int64_t at = ((int64_t)b * Th + (q >> 1)) * a.x_pitch + ch;
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.x + at);
        const f32x4 y = *reinterpret_cast<const f32x4*>(a.yl + at);
        const unsigned s = *reinterpret_cast<const unsigned*>(a.sel + at);
        const unsigned odd = q & 1;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            v[i] = (ch + i < a.kc && y[i] > 0.0f && ((s >> (8 * i)) & 0xffu) == odd) ? g[i] : 0.0f;
    }
    return v;
}

// A workgroup: 4 waves, each 32 conv rows (two MFMA row tiles) of ONE read times 16 WC output columns.  K runs over taps,
// then groups of 16 channels; lane (rl, kq) holds channels 16 g + 4 kq + {0..3} of row rl, one MFMA per `sub`.
template <int MODE, int WC, bool POOL, bool K3>
__global__ __launch_bounds__(256) void train_conv_kernel(const ConvArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int q0 = tile * 128 + 32 * wave;
    if (q0 >= a.T) return;                                  // no barrier in this kernel
    const int col0 = blockIdx.y * (16 * WC);
    const int kp16 = pad16(a.kc), G = kp16 / 16;
    const int k = K3 ? 3 : a.k, half = (k - 1) >> 1;

    // blocked summation: 128 channels of one tap are summed on their own and then added to the element's sum, so that a wide
    // layer's rounding error grows with the number of such runs, not with k c_in
    f32x4 sum[2][WC];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < WC; ++j) sum[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int tap = 0; tap < k; ++tap) {
        const int shift = MODE == FWD ? tap - half : half - tap;
        for (int g0 = 0; g0 < G; g0 += 8) {
            f32x4 acc[2][WC];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < WC; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const int g1 = min(g0 + 8, G);
            for (int g = g0; g < g1; ++g) {
                const int ch = 16 * g + 4 * kq;
                f32x4 av[2], bv[WC];
#pragma unroll
                for (int i = 0; i < 2; ++i) av[i] = load_a<MODE, POOL>(a, b, q0 + 16 * i + rl + shift, ch);
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
    // lane element e of row tile i: conv row q0 + 16 i + 4 kq + e, column col0 + 16 j + rl
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        const int col = col0 + 16 * j + rl;
        if (col >= a.nc) continue;
        if constexpr (MODE == FWD && !POOL) {
            const float bias = a.bias[col];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = q0 + 16 * i + 4 * kq + e;
                    if (r < a.T) a.out[((int64_t)b * a.T + r) * a.out_pitch + col] = fmaxf(sum[i][j][e] + bias, 0.0f);
                }
        } else if constexpr (MODE == FWD) {
            const float bias = a.bias[col];
            const int Th = a.T >> 1;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int p = ((q0 + 16 * i + 4 * kq) >> 1) + h;
                    if (p >= Th) continue;
                    const float r0 = fmaxf(sum[i][j][2 * h] + bias, 0.0f), r1 = fmaxf(sum[i][j][2 * h + 1] + bias, 0.0f);
                    const bool second = r1 > r0;            // row 2j wins unless row 2j + 1 is strictly larger
                    const int64_t at = ((int64_t)b * Th + p) * a.out_pitch + col;
                    a.out[at] = second ? r1 : r0;
                    a.sel_out[at] = second ? 1 : 0;
                }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = q0 + 16 * i + 4 * kq + e;
                    if (r < a.T) a.out[((int64_t)b * a.T + r) * a.out_pitch + col] = sum[i][j][e];
                }
        }
    }
}

struct WgradArgs {
    const float* dy;            // dY_j, y_j, selectors: [B][T >> 1][po]; inner conv: dY_j, r_j [B][T][po], no selectors
    const float* yl;
    const uint8_t* sel;
    const float* a;             // A_{j-1}: [B][T][a_pitch] (conv 0: the signals)
    float* partial;             // [n_slices][c_out c_in k + c_out]
    int64_t a_read_stride;
    int a_pitch, T, po, c_in, c_out, ci_blocks, slice_len, positions;
    int k;                      // taps (the K3 instantiation runs three whatever this says)
};

// One wave: a 32 (c_out) x 3 x 32 (c_in) tile of dW over one slice of positions, and - in the first c_in block - the matching
// 32 entries of db.  Lane (rl, kq) holds position p0 + kq: channel co0 + 16 m + rl of dZ (A operand), channel ci0 + 16 n + rl
// of the three input rows around it (B operands).  Positions run over reads back to back; a row outside its own read is +0.
// !K3: the three taps are tap group blockIdx.z of the conv's k, tap0 .. tap0 + nt - 1 with nt <= 3; a tap the group does not
// have loads nothing, issues no MFMA and writes nothing, and only group 0 carries the bias column.
template <bool POOL, bool K3>
__global__ __launch_bounds__(64) void train_wgrad_kernel(const WgradArgs a) {
    const int lane = threadIdx.x, rl = lane & 15, kq = lane >> 4;
    const int co0 = (blockIdx.x / a.ci_blocks) * 32, ci0 = (blockIdx.x % a.ci_blocks) * 32;
    const int s = blockIdx.y;
    const int p_begin = s * a.slice_len, p_end = min(p_begin + a.slice_len, a.positions);
    const int Th = a.T >> 1;
    const int kt = K3 ? 3 : a.k, tap0 = K3 ? 0 : kTapGroup * (int)blockIdx.z;
    const int nt = K3 ? 3 : min(kTapGroup, kt - tap0), half = (kt - 1) >> 1;
    const bool with_bias = ci0 == 0 && tap0 == 0;

    // blocked summation: a run of 64 positions is summed on its own and then added to the slice's sum, so that a long
    // contraction's rounding error grows with the number of runs, not of positions
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
        // sixteen steps whatever is left of the slice (a position at or behind its end is +0 by `valid`), four at a time: the
        // loads of four steps are issued together, then their MFMAs run in step order
        for (int p0 = pc; p0 < pc + 64; p0 += 16) {
            float dz[4][2], av[4][3][2];
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int p = p0 + 4 * st + kq;
                const bool valid = p < p_end;
                const int b = p / a.T, u = p - b * a.T;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const int co = co0 + 16 * m + rl;
                    dz[st][m] = 0.0f;
                    if constexpr (POOL) {
                        if (valid && co < a.c_out && u < 2 * Th) {
                            const int64_t at = ((int64_t)b * Th + (u >> 1)) * a.po + co;
                            if (a.yl[at] > 0.0f && a.sel[at] == (u & 1)) dz[st][m] = a.dy[at];
                        }
                    } else {
                        if (valid && co < a.c_out) {
                            const int64_t at = ((int64_t)b * a.T + u) * a.po + co;
                            if (a.yl[at] > 0.0f) dz[st][m] = a.dy[at];
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int r = u + tap0 + k - half;
#pragma unroll
                    for (int n = 0; n < 2; ++n) {
                        const int ci = ci0 + 16 * n + rl;
                        av[st][k][n] = ((K3 || k < nt) && valid && r >= 0 && r < a.T && ci < a.c_in)
                                           ? a.a[(int64_t)b * a.a_read_stride + (int64_t)r * a.a_pitch + ci] : 0.0f;
                    }
                }
            }
#pragma unroll
            for (int st = 0; st < 4; ++st)
#pragma unroll
                for (int m = 0; m < 2; ++m) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (!K3 && k >= nt) continue;
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
                    if (K3 || k < nt) part[((int64_t)co * a.c_in + ci) * kt + tap0 + k] = sum[m][k][n][e];
            }
            if (with_bias && rl == 0) part[n_w + co] = sumb[m][e];
        }
}

// GAP over the T rows of read b (ascending) and the two logits (a fixed tree over the block)
__global__ __launch_bounds__(256) void train_head_kernel(const float* __restrict__ y, int T, int pitch, int C,
                                                         const float* __restrict__ fcw, const float* __restrict__ fcb,
                                                         float* __restrict__ gap, float* __restrict__ logits) {
    __shared__ float red[2][256];
    const int b = blockIdx.x;
    float p0 = 0.0f, p1 = 0.0f;
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;                                      // thousands of rows: the mean is rounded once
        for (int t = 0; t < T; ++t) s += (double)y[((int64_t)b * T + t) * pitch + c];
        const float g = (float)(s / (double)T);
        gap[(int64_t)b * C + c] = g;
        p0 = fmaf(g, fcw[c], p0);
        p1 = fmaf(g, fcw[C + c], p1);
    }
    red[0][threadIdx.x] = p0;
    red[1][threadIdx.x] = p1;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[0][threadIdx.x] += red[0][threadIdx.x + w];
            red[1][threadIdx.x] += red[1][threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) logits[2 * b + threadIdx.x] = red[threadIdx.x][0] + fcb[threadIdx.x];
}

// dW_fc[j][c] = sum_b dlogits[b][j] gap[b][c], db_fc[j] = sum_b dlogits[b][j], ascending b
__global__ __launch_bounds__(256) void train_fc_grad_kernel(const float* __restrict__ dlogits, const float* __restrict__ gap,
                                                            int B, int C, float* __restrict__ gw, float* __restrict__ gb) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c < C) {
        float s0 = 0.0f, s1 = 0.0f;
        for (int b = 0; b < B; ++b) {
            const float g = gap[(int64_t)b * C + c];
            s0 = fmaf(dlogits[2 * b], g, s0);
            s1 = fmaf(dlogits[2 * b + 1], g, s1);
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

// dY_last[b][t][c] = (dlogits[b] . W_fc[:, c]) / T
__global__ __launch_bounds__(256) void train_head_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ fcw,
                                                             int T, int pitch, int C, float* __restrict__ dy) {
    const int b = blockIdx.y;
    const float d0 = dlogits[2 * b], d1 = dlogits[2 * b + 1];
    for (int c = threadIdx.x; c < C; c += 256) {
        const float v = fmaf(d1, fcw[C + c], d0 * fcw[c]) / (float)T;
        for (int t = blockIdx.x; t < T; t += gridDim.x) dy[((int64_t)b * T + t) * pitch + c] = v;
    }
}

// master W [c_out][c_in][kt] -> wf [kt][p16(c_in)][p16(c_out)] and wt [kt][p16(c_out)][p16(c_in)], zero padded; kt = 3 (K3) or k
template <bool K3>
__global__ __launch_bounds__(256) void train_pack_kernel(const float* __restrict__ w, int c_in, int c_out,
                                                         float* __restrict__ wf, float* __restrict__ wt, int k_taps) {
    const int kt = K3 ? 3 : k_taps;
    const int ci16 = pad16(c_in), co16 = pad16(c_out);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)kt * ci16 * co16) return;
    const int co = (int)(i % co16), ci = (int)((i / co16) % ci16), k = (int)(i / ((int64_t)co16 * ci16));
    const float v = (ci < c_in && co < c_out) ? w[((int64_t)co * c_in + ci) * kt + k] : 0.0f;
    wf[i] = v;
    wt[((int64_t)k * co16 + co) * ci16 + ci] = v;
}

template <int MODE, bool POOL, bool K3>
void launch_conv_form(const ConvArgs& a, int B, hipStream_t st) {
    const dim3 block(256);
    if (a.nc <= 16) {
        hipLaunchKernelGGL((train_conv_kernel<MODE, 1, POOL, K3>), dim3((unsigned)B * a.tiles, (a.np16 + 15) / 16), block, 0, st, a);
    } else if (a.nc <= 32) {
        hipLaunchKernelGGL((train_conv_kernel<MODE, 2, POOL, K3>), dim3((unsigned)B * a.tiles, (a.np16 + 31) / 32), block, 0, st, a);
    } else {
        hipLaunchKernelGGL((train_conv_kernel<MODE, 4, POOL, K3>), dim3((unsigned)B * a.tiles, (a.np16 + 63) / 64), block, 0, st, a);
    }
}

// a pooling conv of three taps takes the shipped class's instantiation, whichever constructor made the handle
template <int MODE>
void launch_conv(const ConvArgs& a, bool pool, int B, hipStream_t st) {
    if (pool && a.k == 3) launch_conv_form<MODE, true, true>(a, B, st);
    else if (pool) launch_conv_form<MODE, true, false>(a, B, st);
    else launch_conv_form<MODE, false, false>(a, B, st);
}

void launch_wgrad(const WgradArgs& g, bool pool, int n_slices, hipStream_t st) {
    const unsigned tiles = (unsigned)(g.ci_blocks * ((g.c_out + 31) / 32));
    const dim3 block(64);
    if (pool && g.k == 3) {
        hipLaunchKernelGGL((train_wgrad_kernel<true, true>), dim3(tiles, (unsigned)n_slices), block, 0, st, g);
    } else if (pool) {
        hipLaunchKernelGGL((train_wgrad_kernel<true, false>), dim3(tiles, (unsigned)n_slices, (unsigned)tap_groups(g.k)), block, 0, st, g);
    } else {
        hipLaunchKernelGGL((train_wgrad_kernel<false, false>), dim3(tiles, (unsigned)n_slices, (unsigned)tap_groups(g.k)), block, 0, st, g);
    }
}

}  // namespace
}  // namespace rs

struct rs_train {
    int device = -1;            // < 0: a handle without device memory (the plan and the argument checks only)
    int n_layers = 0, c_last = 0;       // n_layers: the pools
    int depth = 1, n_convs = 0;         // convs per layer; n_layers * depth
    std::vector<rs::train::LayerShape> layers;      // one per CONV, j = layer * depth + d
    size_t n_params = 0, fcw_off = 0, fcb_off = 0, n_packed = 0;
    rs::DevBuf<float> params, grads, m, v, packed;
    int64_t step = 0;
    void* last_ws = nullptr;    // rs_train_debug_copy: the workspace, batch and length of the last rs_train_forward_backward,
                                // null again once any later training call - an evaluate, a refused one - has begun
    int last_B = 0, last_L = 0;
};

namespace rs {
namespace {

struct Carved {
    std::vector<float*> y, dy;
    std::vector<uint8_t*> sel;
    float *gap, *dlogits, *partials;
    int32_t* flag;
};

Carved carve(const rs_train* h, void* d_ws, int B, int L) {
    const Workspace w = plan_workspace(h->layers, B, L);
    Carver ws(d_ws);
    Carved c;
    for (int j = 0; j < h->n_convs; ++j) {
        c.y.push_back(ws.take(w.act[j]));
        c.dy.push_back(ws.take(w.act[j]));
        c.sel.push_back(w.sel[j] ? ws.take<uint8_t>(w.sel[j]) : nullptr);
    }
    c.gap = ws.take(w.gap);
    c.dlogits = ws.take(w.dlogits);
    c.flag = ws.take<int32_t>(w.flag);
    c.partials = ws.take(w.partials);
    return c;
}

int pack_layer(rs_train* h, int l, hipStream_t st) {
    const LayerShape& s = h->layers[l];
    const int64_t n = (int64_t)s.packed_floats();
    if (s.k == 3)
        hipLaunchKernelGGL(train_pack_kernel<true>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->params + s.w_off,
                           s.c_in, s.c_out, h->packed + s.wf_off, h->packed + s.wt_off, s.k);
    else
        hipLaunchKernelGGL(train_pack_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, h->params + s.w_off,
                           s.c_in, s.c_out, h->packed + s.wf_off, h->packed + s.wt_off, s.k);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

// tensor `index` of the flat parameter vector: 2 j = W_j, 2 j + 1 = b_j of conv j, 2 n = W_fc, 2 n + 1 = b_fc (n convs)
bool tensor_range(const rs_train* h, int index, size_t* off, size_t* count) {
    if (index < 0 || index > 2 * h->n_convs + 1) return false;
    if (index == 2 * h->n_convs) {
        *off = h->fcw_off;
        *count = 2 * (size_t)h->c_last;
    } else if (index == 2 * h->n_convs + 1) {
        *off = h->fcb_off;
        *count = 2;
    } else {
        const LayerShape& s = h->layers[index / 2];
        *off = (index & 1) ? s.b_off : s.w_off;
        *count = (index & 1) ? (size_t)s.c_out : s.n_w();
    }
    return true;
}

// The checks of a training call in the house order: arguments, length, workspace, buffer window, then the handle's device.
int check_train_call(const char* fn, const rs_train* h, const void* d_x, const void* d_labels, const void* d_ws, const void* d_out,
                     int B, int L, int ld, size_t ws_bytes) {
    if (!h || !d_x || !d_labels || !d_ws || !d_out || B < 1 || L < 1 || ld < L) {
        set_error("%s: bad argument", fn);
        return RS_ERR_ARG;
    }
    if ((L >> h->n_layers) < 1) {
        set_error("%s: reads of %d samples are shorter than the network minimum %d", fn, L, 1 << h->n_layers);
        return RS_ERR_LENGTH;
    }
    if (ws_bytes < rs_train_workspace_bytes(h, B, L)) {
        set_error("%s: workspace too small", fn);
        return RS_ERR_WORKSPACE;
    }
    if (B > rs_train_max_batch(h, L)) {
        set_error("%s: %d reads of %d samples outgrow the 2 GiB buffer window: split the batch (rs_train_max_batch)", fn, B, L);
        return RS_ERR_ARG;
    }
    if (h->device < 0) {
        set_error("%s: the handle was made without a device", fn);
        return RS_ERR_ARG;
    }
    return RS_OK;
}

int run(rs_train* h, const char* fn, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
        size_t ws_bytes, float* d_out, void* stream, bool backward) {
    if (h) h->last_ws = nullptr;                            // this call may carve the same workspace at other offsets
    const int rc = check_train_call(fn, h, d_x, d_labels, d_ws, d_out, B, L, ld, ws_bytes);
    if (rc != RS_OK) return rc;
    DeviceGuard guard(h->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Carved c = carve(h, d_ws, B, L);
    const int n = h->n_convs;

    for (int l = 0; l < n; ++l) {
        const LayerShape& s = h->layers[l];
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.x = l ? c.y[l - 1] : d_x;
        a.T = L >> s.level;                                  // conv l - 1 left this many rows, pooled or not
        a.x_pitch = l ? cp4(s.c_in) : 1;
        a.x_read_stride = l ? (int64_t)a.T * a.x_pitch : ld;
        a.out = c.y[l];
        a.sel_out = c.sel[l];
        a.w = h->packed + s.wf_off;
        a.bias = h->params + s.b_off;
        a.kc = s.c_in;
        a.nc = s.c_out;
        a.np16 = p16(s.c_out);
        a.out_pitch = cp4(s.c_out);
        a.tiles = (a.T + 127) / 128;
        a.k = s.k;
        launch_conv<FWD>(a, s.pool, B, st);
        RS_HIP(hipGetLastError());
    }
    const int T_last = L >> h->n_layers, pitch_last = cp4(h->c_last);
    hipLaunchKernelGGL(train_head_kernel, dim3(B), dim3(256), 0, st, c.y[n - 1], T_last, pitch_last, h->c_last,
                       h->params + h->fcw_off, h->params + h->fcb_off, c.gap, d_out + 2);
    RS_HIP(hipGetLastError());
    hipLaunchKernelGGL(train_loss_kernel, dim3(1), dim3(64), 0, st, d_out, d_labels, B, c.dlogits, c.flag);
    RS_HIP(hipGetLastError());
    if (backward) {
        hipLaunchKernelGGL(train_fc_grad_kernel, dim3((h->c_last + 255) / 256), dim3(256), 0, st, c.dlogits, c.gap, B, h->c_last,
                           h->grads + h->fcw_off, h->grads + h->fcb_off);
        RS_HIP(hipGetLastError());
        hipLaunchKernelGGL(train_head_bwd_kernel, dim3(std::min(T_last, 64), B), dim3(256), 0, st, c.dlogits,
                           h->params + h->fcw_off, T_last, pitch_last, h->c_last, c.dy[n - 1]);
        RS_HIP(hipGetLastError());
        for (int l = n - 1; l >= 0; --l) {
            const LayerShape& s = h->layers[l];
            const int T = L >> s.level;
            const SlicePlan sp = plan_slices(s, s.level, B, L);
            WgradArgs g;
            memset(&g, 0, sizeof(g));
            g.dy = c.dy[l];
            g.yl = c.y[l];
            g.sel = c.sel[l];
            g.a = l ? c.y[l - 1] : d_x;
            g.a_pitch = l ? cp4(s.c_in) : 1;
            g.a_read_stride = l ? (int64_t)T * g.a_pitch : ld;
            g.partial = c.partials;
            g.T = T;
            g.po = cp4(s.c_out);
            g.c_in = s.c_in;
            g.c_out = s.c_out;
            g.ci_blocks = (s.c_in + 31) / 32;
            g.slice_len = sp.slice_len;
            g.positions = B * T;
            g.k = s.k;
            launch_wgrad(g, s.pool, sp.n_slices, st);
            RS_HIP(hipGetLastError());
            const int64_t n_tile = (int64_t)s.tile_floats();
            hipLaunchKernelGGL(train_reduce_kernel, dim3((unsigned)((n_tile + 255) / 256)), dim3(256), 0, st, c.partials,
                               sp.n_slices, n_tile, h->grads + s.w_off);
            RS_HIP(hipGetLastError());
            if (l == 0) break;
            ConvArgs a;
            memset(&a, 0, sizeof(a));
            a.x = c.dy[l];
            a.yl = c.y[l];
            a.sel = c.sel[l];
            a.x_pitch = cp4(s.c_out);
            a.T = T;
            a.out = c.dy[l - 1];
            a.w = h->packed + s.wt_off;
            a.kc = s.c_out;
            a.nc = s.c_in;
            a.np16 = p16(s.c_in);
            a.out_pitch = cp4(s.c_in);
            a.tiles = (T + 127) / 128;
            a.k = s.k;
            launch_conv<DGRAD>(a, s.pool, B, st);
            RS_HIP(hipGetLastError());
        }
    }
    int32_t bad = 0;                                        // the label check's answer is this call's status
    RS_HIP(hipMemcpyAsync(&bad, c.flag, sizeof(bad), hipMemcpyDeviceToHost, st));
    RS_HIP(hipStreamSynchronize(st));
    if (bad) {
        set_error("%s: a label outside {0, 1}", fn);
        return RS_ERR_ARG;
    }
    if (backward) {                                         // the buffers rs_train_debug_copy reads are complete and this call's
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

int rs_train_destroy(rs_train* h) {
    if (!h) return RS_OK;
    if (h->device >= 0) {
        DeviceGuard guard(h->device);
        delete h;                       // every device buffer is a DevBuf: freed with its holder
    } else {
        delete h;
    }
    return RS_OK;
}

// the handle of a checked conv table: the flat parameter layout, and on a device the uploads and the first pack
static int make_handle(const char* fn, const rs_gconv_conv* convs, int n_layers, int depth, const float* fc_w, const float* fc_b,
                       int device, rs_train** out) {
    const int n_convs = n_layers * depth;
    rs_train* h = new (std::nothrow) rs_train();
    if (!h) return RS_ERR_OOM;
    h->device = device < 0 ? -1 : device;
    h->n_layers = n_layers;
    h->depth = depth;
    h->n_convs = n_convs;
    h->c_last = convs[n_convs - 1].c_out;
    size_t off = 0, poff = 0;
    for (int i = 0; i < n_convs; ++i) {
        LayerShape s;
        s.c_in = convs[i].c_in;
        s.c_out = convs[i].c_out;
        s.k = convs[i].k;
        s.level = i / depth;
        s.pool = (i % depth) == depth - 1;
        s.w_off = off;
        off += s.n_w();
        s.b_off = off;
        off += s.c_out;
        const size_t np = s.packed_floats();
        s.wf_off = poff;
        s.wt_off = poff + np;
        poff += 2 * np;
        h->layers.push_back(s);
    }
    h->fcw_off = off;
    off += 2 * (size_t)h->c_last;
    h->fcb_off = off;
    off += 2;
    h->n_params = off;
    h->n_packed = poff;
    if (device < 0) {
        *out = h;
        return RS_OK;
    }
    std::vector<float> flat(h->n_params);
    for (int i = 0; i < n_convs; ++i) {
        const LayerShape& s = h->layers[i];
        std::copy(convs[i].w, convs[i].w + s.n_w(), flat.begin() + s.w_off);
        std::copy(convs[i].b, convs[i].b + s.c_out, flat.begin() + s.b_off);
    }
    std::copy(fc_w, fc_w + 2 * (size_t)h->c_last, flat.begin() + h->fcw_off);
    std::copy(fc_b, fc_b + 2, flat.begin() + h->fcb_off);
    DeviceGuard guard(device);
    hipError_t e = guard.err;
    const std::vector<float> zeros(h->n_params, 0.0f);
    if (e == hipSuccess) e = upload(h->params, flat);
    if (e == hipSuccess) e = upload(h->grads, zeros);
    if (e == hipSuccess) e = upload(h->m, zeros);
    if (e == hipSuccess) e = upload(h->v, zeros);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&h->packed.p), h->n_packed * sizeof(float));
    int rc = RS_OK;
    for (int i = 0; i < n_convs && e == hipSuccess && rc == RS_OK; ++i) rc = pack_layer(h, i, nullptr);
    if (e == hipSuccess && rc == RS_OK) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess || rc != RS_OK) {
        rs_train_destroy(h);
        return e != hipSuccess ? hip_fail(e, fn) : rc;
    }
    *out = h;
    return RS_OK;
}

int rs_train_create(const rs_gconv_conv* convs, int n_layers, const float* fc_w, const float* fc_b, int device, rs_train** out) {
    if (!out) {
        set_error("rs_train_create: null output handle");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    if (!convs || n_layers < 1 || n_layers > 30 || !fc_w || !fc_b) {
        set_error("rs_train_create: bad argument (convs, n_layers 1-30, fc weights)");
        return RS_ERR_ARG;
    }
    for (int i = 0; i < n_layers; ++i) {
        const rs_gconv_conv& c = convs[i];
        const int ci = i == 0 ? 1 : convs[i - 1].c_out;
        if (!c.w || !c.b || c.c_in != ci || c.c_out < 1) {
            set_error("rs_train_create: bad conv %d (chained channels from 1, weights and bias)", i);
            return RS_ERR_ARG;
        }
        if (c.k != 3) {
            set_error("rs_train_create: conv %d has the kernel %d: training runs kernels of 3 only", i, c.k);
            return RS_ERR_ARG;
        }
    }
    return make_handle("rs_train_create upload", convs, n_layers, 1, fc_w, fc_b, device, out);
}

// the refusals of rs_gconv_create, in its order: a net that trains is a net the inference family runs
int rs_train_create_generic(const rs_gconv_conv* convs, int n_layers, int depth, const float* fc_w, const float* fc_b, int device,
                            rs_train** out) {
    if (!out) {
        set_error("rs_train_create_generic: null output handle");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    if (!convs || n_layers < 1 || depth < 1 || depth > 64 || !fc_w || !fc_b) {
        set_error("rs_train_create_generic: bad argument (convs, n_layers >= 1, depth 1-64, fc weights)");
        return RS_ERR_ARG;
    }
    if (n_layers > gconv::kMaxPools) {
        set_error("rs_train_create_generic: %d layers: the generic ConvNet family runs %d pools", n_layers, gconv::kMaxPools);
        return RS_ERR_ARG;
    }
    for (int i = 0; i < n_layers * depth; ++i) {
        const rs_gconv_conv& c = convs[i];
        const int ci = i == 0 ? 1 : convs[i - 1].c_out;
        if (!c.w || !c.b || c.c_in != ci || c.c_out < 1 || c.k < 1) {
            set_error("rs_train_create_generic: bad conv %d (chained channels from 1, k >= 1, weights and bias)", i);
            return RS_ERR_ARG;
        }
        if ((c.k & 1) == 0) {
            set_error("rs_train_create_generic: conv %d has the even kernel %d: 'same' pads it asymmetrically", i, c.k);
            return RS_ERR_ARG;
        }
        if (!gconv::plan_conv(c.c_in, c.c_out, c.k, nullptr)) {
            set_error("rs_train_create_generic: conv %d (%d -> %d channels, kernel %d) fits no tile shape of the generic "
                      "ConvNet family, which could not run the trained net", i, c.c_in, c.c_out, c.k);
            return RS_ERR_ARG;
        }
    }
    return make_handle("rs_train_create_generic upload", convs, n_layers, depth, fc_w, fc_b, device, out);
}

size_t rs_train_workspace_bytes(const rs_train* h, int B, int L) {
    if (!h || B < 1 || L < 1 || (L >> h->n_layers) < 1) return 0;
    return plan_workspace(h->layers, B, L).total;
}

int rs_train_max_batch(const rs_train* h, int L) {
    if (!h || L < 1 || (L >> h->n_layers) < 1) return 0;
    return std::min(max_batch_of(per_read_bytes(h->layers, L)), kMaxGridY);   // train_head_bwd_kernel has B in its grid's y
}

int rs_train_slice_plan(const rs_train* h, int layer, int B, int L, int32_t* n_slices, int32_t* slice_len) {
    if (!h || layer < 0 || layer >= h->n_convs || B < 1 || L < 1 || (L >> h->n_layers) < 1 || !n_slices || !slice_len) {
        set_error("rs_train_slice_plan: bad argument");
        return RS_ERR_ARG;
    }
    const SlicePlan p = plan_slices(h->layers[layer], h->layers[layer].level, B, L);
    *n_slices = p.n_slices;
    *slice_len = p.slice_len;
    return RS_OK;
}

int rs_train_forward_backward(rs_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
                              size_t ws_bytes, float* d_out, void* stream) {
    return run(h, "rs_train_forward_backward", d_x, d_labels, B, L, ld, d_ws, ws_bytes, d_out, stream, true);
}

int rs_train_evaluate(rs_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws, size_t ws_bytes,
                      float* d_out, void* stream) {
    return run(h, "rs_train_evaluate", d_x, d_labels, B, L, ld, d_ws, ws_bytes, d_out, stream, false);
}

int rs_train_adam_step(rs_train* h, float lr, float beta1, float beta2, float eps, void* stream) {
    if (!h || !(lr > 0.0f) || !(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f) || !(eps >= 0.0f)) {
        set_error("rs_train_adam_step: bad argument (handle, lr > 0, betas in [0, 1), eps >= 0)");
        return RS_ERR_ARG;
    }
    if (h->device < 0) {
        set_error("rs_train_adam_step: the handle was made without a device");
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
    for (int l = 0; l < h->n_convs; ++l) {
        const int rc = pack_layer(h, l, st);
        if (rc != RS_OK) return rc;
    }
    return RS_OK;
}

static int copy_tensor(rs_train* h, const char* fn, int index, float* get_dst, const float* set_src, size_t count, bool grads) {
    size_t off = 0, n = 0;
    if (!h || (!get_dst && !set_src) || !tensor_range(h, index, &off, &n) || count != n) {
        set_error("%s: bad argument (handle, host array, tensor index 0 .. 2 n_convs + 1, its element count)", fn);
        return RS_ERR_ARG;
    }
    if (h->device < 0) {
        set_error("%s: the handle was made without a device", fn);
        return RS_ERR_ARG;
    }
    DeviceGuard guard(h->device);
    RS_HIP(guard.err);
    RS_HIP(hipDeviceSynchronize());
    if (get_dst) {
        RS_HIP(hipMemcpy(get_dst, (grads ? h->grads.p : h->params.p) + off, n * sizeof(float), hipMemcpyDeviceToHost));
        return RS_OK;
    }
    RS_HIP(hipMemcpy(h->params.p + off, set_src, n * sizeof(float), hipMemcpyHostToDevice));
    if (index < 2 * h->n_convs && (index & 1) == 0) {
        const int rc = pack_layer(h, index / 2, nullptr);
        if (rc != RS_OK) return rc;
        RS_HIP(hipStreamSynchronize(nullptr));
    }
    return RS_OK;
}

int rs_train_get_params(rs_train* h, int index, float* dst, size_t count) {
    return copy_tensor(h, "rs_train_get_params", index, dst, nullptr, count, false);
}

int rs_train_get_grads(rs_train* h, int index, float* dst, size_t count) {
    return copy_tensor(h, "rs_train_get_grads", index, dst, nullptr, count, true);
}

int rs_train_set_params(rs_train* h, int index, const float* src, size_t count) {
    return copy_tensor(h, "rs_train_set_params", index, nullptr, src, count, false);
}

int rs_train_debug_copy(rs_train* h, int layer, int what, void* d_dst, size_t bytes) {
    if (!h || layer < 0 || layer >= h->n_convs || what < 0 || what > 2 || !d_dst) {
        set_error("rs_train_debug_copy: bad argument (handle, layer, what 0 activations / 1 selectors / 2 dY, destination)");
        return RS_ERR_ARG;
    }
    if (what == 1 && !h->layers[layer].pool) {
        set_error("rs_train_debug_copy: conv %d is not the last of its layer: it has no selectors", layer);
        return RS_ERR_ARG;
    }
    if (!h->last_ws) {
        set_error("rs_train_debug_copy: no rs_train_forward_backward has run on this handle since the last rs_train_evaluate "
                  "or refused call");
        return RS_ERR_ARG;
    }
    const Workspace w = plan_workspace(h->layers, h->last_B, h->last_L);
    const size_t need = what == 1 ? w.sel[layer] : w.act[layer];
    if (bytes < need) {
        set_error("rs_train_debug_copy: the destination holds %zu bytes, the buffer has %zu", bytes, need);
        return RS_ERR_ARG;
    }
    DeviceGuard guard(h->device);
    RS_HIP(guard.err);
    const Carved c = carve(h, h->last_ws, h->last_B, h->last_L);
    const void* src = what == 0 ? (const void*)c.y[layer] : what == 1 ? (const void*)c.sel[layer] : (const void*)c.dy[layer];
    RS_HIP(hipDeviceSynchronize());
    RS_HIP(hipMemcpy(d_dst, src, need, hipMemcpyDeviceToDevice));
    return RS_OK;
}

}  // extern "C"
