// CNN-RNN (riser/nets/cnn_rnn.py, ConvRecNet): a valid-conv front, stacked LSTM / GRU layers, Linear + softmax.
//
// Activations are position-major [read][t][channels]: the layout the recurrence reads.  A read's own lengths follow the
// reference: L_{i+1} = (L_i - k_i + 1) // 2 through the conv front, T = L_n recurrent steps.
//
//   crnn_conv_kernel   one launch per conv layer: valid conv + bias + MaxPool1d(2, 2) + ReLU on the f32-input MFMA
//                      (v_mfma_f32_16x16x4_f32).  A workgroup takes 64 conv positions (32 pooled) of one read; the pool
//                      pairs are accumulator elements (0, 1) and (2, 3) of one lane, so pooling costs two fmaxf.
//   crnn_proj_kernel   the input projection W_ih x_t + b of every step of one direction as one parallel GEMM (for the last
//                      layer's backward direction: of each read's last step only).
//   crnn_rec_kernel    one persistent launch per recurrent layer, both directions in it as different workgroups.  A
//                      workgroup (8 waves) owns one direction and 16 reads (the MFMA's M) and loops over t inside the
//                      kernel: gates = xproj_t + h_{t-1} W_hh^T on the MFMA, h_{t-1} passed through LDS (double-buffered,
//                      one barrier per step), c in LDS, the non-linearities in registers.  Wave w owns hidden units
//                      16w .. 16w + 15 and all gates of them.  For hidden <= 128 W_hh stays in VGPRs for the whole loop
//                      (at most 4 gates x 32 k-steps = 128 floats per lane); wider layers read it from the cache.
//                      No workgroup waits for another.
//   last_row_head_kernel (family/head.hpp)   Linear(out_dim -> 2) + softmax on the last step.
//
// Ragged batches: the reads of a tile are aligned so that their recurrences end on the same step; a read that has not
// started keeps h = c = 0 exactly (its update is skipped), the backward direction starts at each read's own last step.
// Every output element comes from a fixed k-ordered MFMA sequence whatever the batch, the tile or ld, so a read gets the
// bits it gets alone.  The K order of the projection and the recurrence: at k-step s lane (r, q) holds
// k = 16 (s / 4) + 4 q + s % 4, so that a lane reads its A operand as one float4 per four steps.
//
// rs_crnn_set_mode(RS_F16X3) switches the gate GEMMs whose input is a hidden state - every recurrence and the input projection
// of every layer but the first - to split precision on the f16 MFMA (crnn/x3.hpp); the kernels above and their launch order
// are the fp32 mode's and do not change with it.
#include "common.hpp"
#include "crnn/shared.hpp"
#include "crnn/x3.hpp"
#include "family/head.hpp"
#include "family/host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

namespace rs {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kConvRows = 64;                       // conv positions per workgroup (32 pooled)
constexpr int kConvLds = 64 * 1024;
constexpr int kResHidden = 128;                     // hidden sizes up to this keep W_hh in VGPRs
constexpr int kMaxHidden = 320;                     // h, h' and c of 16 reads in 64 KB of LDS

// ------------------------------------------------------------------------------------------------ conv front
struct ConvArgs {
    const float* x;             // [B][in_rows][in_pitch] (layer 0: the signal, [B][ld], in_pitch 1)
    const int32_t* len;
    float* y;                   // [B][out_rows][out_pitch]
    int B, ld, layer;
    int in_rows, in_pitch, out_rows, out_pitch;
    int c_in, k, single;        // single: one input channel, K = taps padded to 4
    int cpi, np, ksteps;        // multi-channel: K = k * cpi; weights [K][np]
    int lds_pitch, rows_in, tiles;
    const float* w;
    const float* b;
    Lens ls;
};

__global__ __launch_bounds__(256) void crnn_conv_kernel(const ConvArgs a) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int q0 = tile * kConvRows;
    const int Lin = crnn_len(a.len, b, a.ld, a.ls, a.layer);
    const int Tout = crnn_len(a.len, b, a.ld, a.ls, a.layer + 1);
    const int lim = min(Lin, a.in_rows);
    {
        const int cw = a.single ? 1 : a.cpi;
        const int n = a.rows_in * cw;
        for (int e = threadIdx.x; e < n; e += 256) {
            const int r = e / cw, c = e - r * cw;
            const int q = q0 + r;
            float v = 0.0f;
            if (q < lim && c < a.c_in) v = a.x[((int64_t)b * a.in_rows + q) * a.in_pitch + c];
            lds[r * a.lds_pitch + c] = v;
        }
    }
    __syncthreads();
    const int ng = (a.np + 63) / 64;
    for (int u = wave; u < 4 * ng; u += 4) {
        const int rt = u / ng, cg = u - rt * ng;
        const int arow = rt * 16 + rl;
        const int n0 = cg * 64;
        f32x4 acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (a.single) {
            for (int s = 0; s < a.ksteps; ++s) {
                const int tap = 4 * s + kq;
                const float av = tap < a.k ? lds[(arow + tap) * a.lds_pitch] : 0.0f;
                const float* wr = a.w + (int64_t)(4 * s + kq) * a.np + n0 + rl;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (n0 + 16 * t < a.np) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[16 * t], acc[t], 0, 0, 0);
            }
        } else {
            const int c4n = a.cpi / 4;
            for (int tap = 0; tap < a.k; ++tap) {
                const float* Ar = lds + (arow + tap) * a.lds_pitch + kq;
                const float* wt = a.w + (int64_t)(tap * a.cpi + kq) * a.np + n0 + rl;
                for (int c4 = 0; c4 < c4n; ++c4) {
                    const float av = Ar[4 * c4];
                    const float* wr = wt + (int64_t)(4 * c4) * a.np;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (n0 + 16 * t < a.np) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[16 * t], acc[t], 0, 0, 0);
                }
            }
        }
        // lane element e: conv row rt * 16 + 4 kq + e; pooled rows (q0 / 2) + rt * 8 + 2 kq + {0, 1}
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int col = n0 + 16 * t + rl;
            if (n0 + 16 * t >= a.np || col >= a.out_pitch) continue;
            const float bias = a.b[col];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int p = q0 / 2 + rt * 8 + 2 * kq + h;
                if (p >= a.out_rows) continue;
                // relu(max(conv) + bias) == relu(max(conv + bias)): rounding is monotonic
                const float v = fmaxf(fmaxf(acc[t][2 * h], acc[t][2 * h + 1]) + bias, 0.0f);
                a.y[((int64_t)b * a.out_rows + p) * a.out_pitch + col] = p < Tout ? v : 0.0f;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ input projection
struct ProjArgs {
    const float* a;             // [rows][a_pitch], K = in_dim
    int64_t M;                  // output rows
    int a_pitch, K, KS;         // KS = p16(K) / 4
    int last_only, T_ld, B, ld; // last_only: row b reads row b * T_ld + T_b - 1 of a
    const int32_t* len;
    Lens ls;
    const float* w;             // packed [N / 16][KS][64]
    const float* bias;          // [N]
    float* y;                   // [M][N]
    int N;
};

__global__ __launch_bounds__(256) void crnn_proj_kernel(const ProjArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * 64 + wave * 16;
    const int ct0 = blockIdx.y * 4;
    const int64_t arow = r0 + rl;
    const bool a_ok = arow < a.M;
    int64_t src = arow;
    if (a.last_only && a_ok) {
        const int T = crnn_len(a.len, (int)arow, a.ld, a.ls, a.ls.n);
        src = arow * a.T_ld + (T > 0 ? T - 1 : 0);
    }
    const float* Ar = a.a + (a_ok ? src : 0) * a.a_pitch;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nct = a.N / 16;
    for (int g = 0; g < a.KS / 4; ++g) {
        const int k0 = 16 * g + 4 * kq;
        f32x4 av = {0.f, 0.f, 0.f, 0.f};
        if (a_ok && k0 < a.K) {
            av = *reinterpret_cast<const f32x4*>(Ar + k0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k0 + i >= a.K) av[i] = 0.0f;      // pad columns of the buffer are not written: never read them
        }
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int s = 4 * g + sub;
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (ct0 + t < nct)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[sub], a.w[((int64_t)(ct0 + t) * a.KS + s) * 64 + lane],
                                                                  acc[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (ct0 + t >= nct) continue;
        const int col = (ct0 + t) * 16 + rl;
        const float bias = a.bias[col];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t row = r0 + 4 * kq + e;
            if (row < a.M) a.y[row * a.N + col] = acc[t][e] + bias;
        }
    }
}

// ------------------------------------------------------------------------------------------------ recurrence
struct RecArgs {
    const float* xp[2];         // per direction [B][xp_rows][N]: W_ih x_t + b (LSTM: b_ih + b_hh; GRU: + b_hr, b_hz only)
    int xp_rows[2];             // T_ld, or 1 (one_step)
    int one_step[2];            // the direction runs one step, at each read's last position, from the zero state
    const float* whh[2];        // packed [ng * HT][KS][64]
    const float* bhn[2];        // GRU: b_hn [Hp]
    float* y;                   // sequence output [B][T_ld][y_pitch] (null: not needed)
    float* fin;                 // final output [B][fin_pitch] (null: not needed)
    int T_ld, y_pitch, fin_pitch;
    int B, ld, gru, H, Hp, HT, KS, N, relu, hpitch;
    const int32_t* len;
    Lens ls;
};

template <bool kResident>
__global__ __launch_bounds__(512) void crnn_rec_kernel(const RecArgs a) {
    extern __shared__ float lds[];
    __shared__ int Tb[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * 16;
    const int ng = a.gru ? 3 : 4;
    float* hb0 = lds;
    float* hb1 = lds + 16 * a.hpitch;
    float* cb = lds + 32 * a.hpitch;
    for (int e = threadIdx.x; e < 48 * a.hpitch; e += 512) lds[e] = 0.0f;
    if (threadIdx.x < 16) {
        const int b = b0 + threadIdx.x;
        Tb[threadIdx.x] = b < a.B ? crnn_len(a.len, b, a.ld, a.ls, a.ls.n) : 0;
    }
    __syncthreads();
    int Tmax = 0;
    for (int i = 0; i < 16; ++i) Tmax = max(Tmax, Tb[i]);
    const bool one = a.one_step[dir] != 0;
    const int steps = one ? (Tmax > 0 ? 1 : 0) : Tmax;
    const float* __restrict__ xp = a.xp[dir];
    const int xrows = a.xp_rows[dir];
    const float* __restrict__ W = a.whh[dir];

    float wr[kResident ? 4 : 1][kResident ? 32 : 1];
    if constexpr (kResident) {
        const int j = wave < a.HT ? wave : 0;
#pragma unroll
        for (int gi = 0; gi < 4; ++gi)
#pragma unroll
            for (int s = 0; s < 32; ++s)
                wr[gi][s] = (gi < ng && s < a.KS) ? W[((int64_t)(gi * a.HT + j) * a.KS + s) * 64 + lane] : 0.0f;
    }
    int Trow[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) Trow[e] = Tb[4 * kq + e];

    for (int s = 0; s < steps; ++s) {
        const float* hcur = (s & 1) ? hb1 : hb0;
        float* hnext = (s & 1) ? hb0 : hb1;
        for (int j = wave; j < a.HT; j += 8) {
            const int u = 16 * j + rl;
            // this lane's rows: their step, their projected inputs (issued before the MFMA chain)
            int tr[4];
            bool act[4];
            float xv[4][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = one ? 0 : s - (Tmax - Trow[e]);
                act[e] = q >= 0 && Trow[e] > 0;
                tr[e] = one ? Trow[e] - 1 : (dir == 0 ? q : Trow[e] - 1 - q);
                const int b = b0 + 4 * kq + e;
                const float* xr = xp + ((int64_t)b * xrows + (one ? 0 : tr[e])) * a.N + u;
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) xv[e][gi] = (act[e] && gi < ng) ? xr[gi * a.Hp] : 0.0f;
            }
            f32x4 acc[4];
#pragma unroll
            for (int gi = 0; gi < 4; ++gi) acc[gi] = (f32x4){0.f, 0.f, 0.f, 0.f};
            const float* hr = hcur + rl * a.hpitch + 4 * kq;
            if constexpr (kResident) {
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    if (4 * g < a.KS) {
                        const f32x4 hv = *reinterpret_cast<const f32x4*>(hr + 16 * g);
#pragma unroll
                        for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                            for (int gi = 0; gi < 4; ++gi)
                                if (gi < ng)
                                    acc[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(hv[sub], wr[gi][4 * g + sub], acc[gi], 0, 0, 0);
                    }
                }
            } else {
                for (int g = 0; g < a.KS / 4; ++g) {
                    const f32x4 hv = *reinterpret_cast<const f32x4*>(hr + 16 * g);
#pragma unroll
                    for (int sub = 0; sub < 4; ++sub)
#pragma unroll
                        for (int gi = 0; gi < 4; ++gi)
                            if (gi < ng)
                                acc[gi] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                                    hv[sub], W[((int64_t)(gi * a.HT + j) * a.KS + 4 * g + sub) * 64 + lane], acc[gi], 0, 0, 0);
                }
            }
            const float bhn = a.gru ? a.bhn[dir][u] : 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!act[e]) continue;              // not started (or no read): h = c = 0 stay exact
                const int r = 4 * kq + e;
                const int b = b0 + r;
                float h;
                if (a.gru) {
                    const float rg = sigm(xv[e][0] + acc[0][e]);
                    const float zg = sigm(xv[e][1] + acc[1][e]);
                    const float ng_ = tanhf(xv[e][2] + rg * (acc[2][e] + bhn));
                    h = (1.0f - zg) * ng_ + zg * hcur[r * a.hpitch + u];
                } else {
                    const float ig = sigm(xv[e][0] + acc[0][e]);
                    const float fg = sigm(xv[e][1] + acc[1][e]);
                    const float gg = tanhf(xv[e][2] + acc[2][e]);
                    const float og = sigm(xv[e][3] + acc[3][e]);
                    const float c = fg * cb[r * a.hpitch + u] + ig * gg;
                    cb[r * a.hpitch + u] = c;
                    h = og * tanhf(c);
                }
                hnext[r * a.hpitch + u] = h;
                if (u < a.H) {
                    const float o = a.relu ? fmaxf(h, 0.0f) : h;
                    if (a.y) a.y[((int64_t)b * a.T_ld + tr[e]) * a.y_pitch + dir * a.H + u] = o;
                    if (a.fin && s == steps - 1) a.fin[(int64_t)b * a.fin_pitch + dir * a.H + u] = o;
                }
            }
        }
        __syncthreads();
    }
}

// the head's validity rule: a read too short for the net has no step and gets NaN (the host refuses it first)
struct HasStep {
    const int32_t* len;
    int ld;
    Lens ls;
    __device__ bool operator()(int b) const { return !(crnn_len(len, b, ld, ls, ls.n) < 1); }
};

struct ConvDev {
    int c_in = 0, c_out = 0, k = 0, single = 0, cpi = 0, np = 0, ksteps = 0;
    DevBuf<float> w, b;
};

struct LayerDev {
    int gru = 0, in_dim = 0, H = 0, Hp = 0, HT = 0, ndir = 1, relu = 0, N = 0, KSi = 0, KSh = 0;
    DevBuf<float> wih[2];       // packed [N / 16][KSi][64]
    DevBuf<float> bias[2];      // [N]
    DevBuf<float> whh[2];       // packed [N / 16][KSh][64]
    DevBuf<float> bhn[2];       // [Hp]
    // f16x3 mode: the host weights and their f16 hi / lo fragments.  The host copies (W_hh, and W_ih of every layer but the
    // first: 4 bytes per weight, 1.6 MB for the bench LSTM) wait for the first rs_crnn_set_mode(RS_F16X3), which packs and
    // releases them; a handle that never leaves fp32 keeps them until rs_crnn_destroy
    std::vector<float> h_wih[2], h_whh[2];
    DevBuf<uint32_t> wih3[2];   // u32x4 [N / 16][KSi3][hi, lo][64]; null for the first layer (fp32 projection)
    DevBuf<uint32_t> whh3[2];   // u32x4 [N / 16][KSh3][hi, lo][64]
    float inv_si[2] = {1.0f, 1.0f}, inv_sh[2] = {1.0f, 1.0f};
    int KSi3 = 0, KSh3 = 0;
};

// w [rows = ng * H][K] (gate-major, as torch stores weight_ih / weight_hh) -> the MFMA B operand of every 16-column tile
// of the padded gate layout (column gi * Hp + u) in the k order of the kernels: [N / 16][p16(K) / 4][64]
std::vector<float> pack_gates(const float* w, int ng, int H, int Hp, int K) {
    const int N = ng * Hp, KS = p16(K) / 4;
    std::vector<float> out((size_t)(N / 16) * KS * 64, 0.0f);
    for (int ct = 0; ct < N / 16; ++ct)
        for (int s = 0; s < KS; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int col = ct * 16 + (lane & 15), gi = col / Hp, u = col - gi * Hp;
                const int k = 16 * (s >> 2) + 4 * (lane >> 4) + (s & 3);
                if (u < H && k < K) out[((size_t)ct * KS + s) * 64 + lane] = w[(size_t)(gi * H + u) * K + k];
            }
    return out;
}

}  // namespace
}  // namespace rs

struct rs_crnn {
    int device = 0;
    std::vector<rs::ConvDev> convs;
    std::vector<rs::LayerDev> layers;
    rs::Lens ls{};
    rs::DevBuf<float> d_fcw, d_fcb;
    int out_dim = 0;
    int min_len = 1;
    int x3 = 0;                 // 1: RS_F16X3
    bool x3_packed = false;
};

namespace rs {
namespace {

// rows per read of conv layer i's output for reads of pitch ld (rows[0] = ld); 0 where ld is too short
void conv_rows(const rs_crnn* m, int ld, std::vector<int>& rows) {
    rows.assign(m->convs.size() + 1, ld);
    for (size_t i = 0; i < m->convs.size(); ++i) {
        const int L = rows[i], k = m->convs[i].k;
        rows[i + 1] = L >= k + 1 ? (L - k + 1) / 2 : 0;
    }
}

struct Plan {
    int T = 0;
    size_t conv = 0, xp = 0, y = 0, fin = 0;      // bytes of one buffer per read
};

Plan plan(const rs_crnn* m, int ld) {
    Plan p;
    std::vector<int> rows;
    conv_rows(m, ld, rows);
    p.T = rows.back();
    for (size_t i = 0; i < m->convs.size(); ++i)
        p.conv = std::max(p.conv, (size_t)rows[i + 1] * cp4(m->convs[i].c_out) * 4);
    for (const LayerDev& l : m->layers) {
        p.xp = std::max(p.xp, (size_t)p.T * l.N * 4);
        p.y = std::max(p.y, (size_t)p.T * cp4(l.ndir * l.H) * 4);
    }
    p.fin = (size_t)cp4(m->out_dim) * 4;
    return p;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" {

int rs_crnn_destroy(rs_crnn* m) {
    if (!m) return RS_OK;
    DeviceGuard guard(m->device);
    delete m;                           // every device buffer is a DevBuf: freed with its holder
    return RS_OK;
}

int rs_crnn_create(const rs_crnn_conv* convs, int n_conv, const rs_crnn_layer* layers, int n_layers, const float* fc_w,
                   const float* fc_b, int out_dim, int device, rs_crnn** out) {
    if (!out) {
        set_error("rs_crnn_create: null output handle");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    if (!convs || n_conv < 1 || n_conv > kMaxConv || !layers || n_layers < 1 || !fc_w || !fc_b || out_dim < 1) {
        set_error("rs_crnn_create: bad argument (1-%d conv layers, >= 1 recurrent layer, fc weights, out_dim >= 1)", kMaxConv);
        return RS_ERR_ARG;
    }
    for (int i = 0; i < n_conv; ++i) {
        const rs_crnn_conv& c = convs[i];
        const int ci = i == 0 ? 1 : convs[i - 1].c_out;
        if (!c.w || !c.b || c.c_in != ci || c.c_out < 1 || c.k < 1 ||
            (size_t)(kConvRows + c.k - 1) * (c.c_in == 1 ? 1 : lds_pitch(cp4(c.c_in))) * 4 > (size_t)kConvLds) {
            set_error("rs_crnn_create: bad conv layer %d (chained channels from 1, k >= 1, weights and bias, a tile inside "
                      "64 KB of LDS)", i);
            return RS_ERR_ARG;
        }
    }
    for (int l = 0; l < n_layers; ++l) {
        const rs_crnn_layer& s = layers[l];
        const int want_in = l == 0 ? convs[n_conv - 1].c_out : layers[l - 1].hidden * (layers[l - 1].bidirectional ? 2 : 1);
        bool ok = (s.cell == 0 || s.cell == 1) && s.hidden >= 1 && s.hidden <= kMaxHidden && s.in_dim == want_in &&
                  (s.bidirectional == 0 || s.bidirectional == 1);
        for (int d = 0; ok && d <= s.bidirectional; ++d) ok = s.w_ih[d] && s.w_hh[d] && s.b_ih[d] && s.b_hh[d];
        if (!ok) {
            set_error("rs_crnn_create: bad recurrent layer %d (cell 0 = LSTM / 1 = GRU, hidden 1-%d, in_dim the previous "
                      "output, both directions' weights)", l, kMaxHidden);
            return RS_ERR_ARG;
        }
    }
    const rs_crnn_layer& last = layers[n_layers - 1];
    if (out_dim != last.hidden * (last.bidirectional ? 2 : 1)) {
        set_error("rs_crnn_create: out_dim %d is not the last layer's output", out_dim);
        return RS_ERR_ARG;
    }
    DeviceGuard guard(device);
    RS_HIP(guard.err);
    rs_crnn* m = new (std::nothrow) rs_crnn();
    if (!m) return RS_ERR_OOM;
    m->device = device;
    m->out_dim = out_dim;
    m->ls.n = n_conv;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_conv && e == hipSuccess; ++i) {
        const rs_crnn_conv& c = convs[i];
        ConvDev cd;
        cd.c_in = c.c_in; cd.c_out = c.c_out; cd.k = c.k;
        cd.single = c.c_in == 1;
        cd.cpi = cd.single ? 1 : cp4(c.c_in);
        cd.np = p16(c.c_out);
        const int K = cd.single ? cp4(c.k) : c.k * cd.cpi;
        cd.ksteps = K / 4;
        std::vector<float> w((size_t)K * cd.np, 0.0f), b(cd.np, 0.0f);
        for (int co = 0; co < c.c_out; ++co) {
            b[co] = c.b[co];
            for (int ci = 0; ci < c.c_in; ++ci)
                for (int t = 0; t < c.k; ++t)
                    w[((size_t)t * cd.cpi + ci) * cd.np + co] = c.w[((size_t)co * c.c_in + ci) * c.k + t];
        }
        e = upload(cd.w, w);
        if (e == hipSuccess) e = upload(cd.b, b);
        m->convs.push_back(std::move(cd));
        m->ls.k[i] = c.k;
    }
    for (int l = 0; l < n_layers && e == hipSuccess; ++l) {
        const rs_crnn_layer& s = layers[l];
        LayerDev ld;
        ld.gru = s.cell;
        ld.in_dim = s.in_dim;
        ld.H = s.hidden;
        ld.Hp = p16(s.hidden);
        ld.HT = ld.Hp / 16;
        ld.ndir = s.bidirectional ? 2 : 1;
        ld.relu = s.relu_after != 0 || l == n_layers - 1;
        const int ng = ld.gru ? 3 : 4;
        ld.N = ng * ld.Hp;
        ld.KSi = p16(s.in_dim) / 4;
        ld.KSh = ld.Hp / 4;
        ld.KSi3 = p32(s.in_dim) / 32;
        ld.KSh3 = p32(ld.Hp) / 32;
        m->layers.push_back(std::move(ld));
        LayerDev& L = m->layers.back();
        for (int d = 0; d < L.ndir && e == hipSuccess; ++d) {
            std::vector<float> bias(L.N, 0.0f), bhn(L.Hp, 0.0f);
            for (int gi = 0; gi < ng; ++gi)
                for (int u = 0; u < L.H; ++u) {
                    const float bi = s.b_ih[d][gi * L.H + u], bh = s.b_hh[d][gi * L.H + u];
                    bias[gi * L.Hp + u] = (L.gru && gi == 2) ? bi : bi + bh;     // GRU: r multiplies (W_hn h + b_hn)
                    if (L.gru && gi == 2) bhn[u] = bh;
                }
            e = upload(L.wih[d], pack_gates(s.w_ih[d], ng, L.H, L.Hp, L.in_dim));
            if (e == hipSuccess) e = upload(L.whh[d], pack_gates(s.w_hh[d], ng, L.H, L.Hp, L.H));
            if (e == hipSuccess) e = upload(L.bias[d], bias);
            if (e == hipSuccess) e = upload(L.bhn[d], bhn);
            if (l > 0) L.h_wih[d].assign(s.w_ih[d], s.w_ih[d] + (size_t)ng * L.H * L.in_dim);
            L.h_whh[d].assign(s.w_hh[d], s.w_hh[d] + (size_t)ng * L.H * L.H);
        }
    }
    if (e == hipSuccess) e = upload(m->d_fcw, std::vector<float>(fc_w, fc_w + 2 * (size_t)out_dim));
    if (e == hipSuccess) e = upload(m->d_fcb, std::vector<float>(fc_b, fc_b + 2));
    if (e != hipSuccess) {
        rs_crnn_destroy(m);
        return hip_fail(e, "rs_crnn_create upload");
    }
    // shortest read with one step: every conv needs k_i + 1 samples so that its pool has an output
    int64_t need = 1;
    for (int i = n_conv - 1; i >= 0; --i) need = 2 * need + m->convs[i].k - 1;
    m->min_len = (int)std::min<int64_t>(need, INT32_MAX);
    *out = m;
    return RS_OK;
}

int rs_crnn_set_mode(rs_crnn* m, int dtype) {
    if (!m) {
        set_error("rs_crnn_set_mode: null handle");
        return RS_ERR_ARG;
    }
    if (dtype == RS_F32 || dtype == RS_F32W) {
        m->x3 = 0;
        return RS_OK;
    }
    if (dtype != RS_F16X3) {
        set_error("rs_crnn_set_mode: dtype %d: a CNN-RNN runs in RS_F32 / RS_F32W or RS_F16X3", dtype);
        return RS_ERR_ARG;
    }
    if (!m->x3_packed) {
        DeviceGuard guard(m->device);
        RS_HIP(guard.err);
        // pack everything on the host first: a refusal leaves the handle as it was
        struct Packed {
            std::vector<uint32_t> wih[2], whh[2];
            float inv_si[2], inv_sh[2];
        };
        std::vector<Packed> pk(m->layers.size());
        for (size_t l = 0; l < m->layers.size(); ++l) {
            const LayerDev& L = m->layers[l];
            const int ng = L.gru ? 3 : 4;
            for (int d = 0; d < L.ndir; ++d) {
                bool ok = pack_gates_x3(L.h_whh[d].data(), ng, L.H, L.Hp, L.H, pk[l].whh[d], pk[l].inv_sh[d]);
                if (ok && l > 0) ok = pack_gates_x3(L.h_wih[d].data(), ng, L.H, L.Hp, L.in_dim, pk[l].wih[d], pk[l].inv_si[d]);
                if (!ok) {
                    set_error("rs_crnn_set_mode: recurrent layer %d has a weight that is not finite", (int)l);
                    return RS_ERR_ARG;
                }
            }
        }
        hipError_t e = hipSuccess;
        for (size_t l = 0; l < m->layers.size() && e == hipSuccess; ++l) {
            LayerDev& L = m->layers[l];
            for (int d = 0; d < L.ndir && e == hipSuccess; ++d) {
                if (!L.whh3[d]) e = upload(L.whh3[d], pk[l].whh[d]);
                if (e == hipSuccess && l > 0 && !L.wih3[d]) e = upload(L.wih3[d], pk[l].wih[d]);
                L.inv_sh[d] = pk[l].inv_sh[d];
                if (l > 0) L.inv_si[d] = pk[l].inv_si[d];
            }
        }
        if (e != hipSuccess) return hip_fail(e, "rs_crnn_set_mode upload");
        m->x3_packed = true;
        for (LayerDev& L : m->layers)               // the host copies have served
            for (int d = 0; d < 2; ++d) {
                std::vector<float>().swap(L.h_wih[d]);
                std::vector<float>().swap(L.h_whh[d]);
            }
    }
    m->x3 = 1;
    return RS_OK;
}

int rs_crnn_min_length(const rs_crnn* m) {
    if (!m) {
        set_error("rs_crnn_min_length: null program");
        return RS_ERR_ARG;
    }
    return m->min_len;
}

int rs_crnn_steps(const rs_crnn* m, int len) {
    if (!m || len < 0) {
        set_error("rs_crnn_steps: bad argument");
        return RS_ERR_ARG;
    }
    std::vector<int> rows;
    conv_rows(m, len, rows);
    return rows.back();
}

size_t rs_crnn_workspace_bytes(const rs_crnn* m, int B, int ld) {
    if (!m || B < 1 || ld < m->min_len) return 0;
    const Plan p = plan(m, ld);
    return 2 * round256(B * p.conv) + 2 * round256(B * p.xp) + 2 * round256(B * p.y) + round256(B * p.fin);
}

int rs_crnn_max_batch(const rs_crnn* m, int ld) {
    if (!m || ld < m->min_len) return 0;
    const Plan p = plan(m, ld);
    return max_batch_of(std::max(std::max(p.conv, p.xp), std::max(p.y, p.fin)));
}

int rs_crnn_forward_ragged(rs_crnn* m, const float* d_x, const int32_t* d_len, int B, int ld, void* d_ws, size_t ws_bytes,
                           float* d_probs, float* d_logits, void* stream) {
    const int rc = check_ragged_call("rs_crnn_forward_ragged", "rs_crnn_max_batch", m, d_x, d_len, d_ws, d_probs, B, ld, ws_bytes, [&] {
        return RaggedLimits{m->min_len, rs_crnn_workspace_bytes(m, B, ld), B <= rs_crnn_max_batch(m, ld)};
    });
    if (rc != RS_OK) return rc;
    DeviceGuard guard(m->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const Plan p = plan(m, ld);
    std::vector<int> rows;
    conv_rows(m, ld, rows);
    Carver ws(d_ws);
    float* cbuf[2] = {ws.take(B * p.conv), ws.take(B * p.conv)};
    float* xp[2] = {ws.take(B * p.xp), ws.take(B * p.xp)};
    float* ybuf[2] = {ws.take(B * p.y), ws.take(B * p.y)};
    float* fin = ws.take(B * p.fin);

    // conv front
    const float* in = d_x;
    int in_pitch = 1;
    const int nc = (int)m->convs.size();
    for (int i = 0; i < nc; ++i) {
        const ConvDev& c = m->convs[i];
        ConvArgs a;
        memset(&a, 0, sizeof(a));
        a.x = in;
        a.len = d_len;
        a.y = cbuf[i & 1];
        a.B = B;
        a.ld = ld;
        a.layer = i;
        a.in_rows = rows[i];
        a.in_pitch = in_pitch;
        a.out_rows = rows[i + 1];
        a.out_pitch = cp4(c.c_out);
        a.c_in = c.c_in;
        a.k = c.k;
        a.single = c.single;
        a.cpi = c.cpi;
        a.np = c.np;
        a.ksteps = c.ksteps;
        a.lds_pitch = c.single ? 1 : lds_pitch(c.cpi);
        a.rows_in = kConvRows + c.k - 1;
        a.tiles = (2 * rows[i + 1] + kConvRows - 1) / kConvRows;
        a.w = c.w;
        a.b = c.b;
        a.ls = m->ls;
        const int64_t grid = (int64_t)B * a.tiles;
        if (grid > INT32_MAX) {
            set_error("rs_crnn_forward_ragged: grid too large: split the batch");
            return RS_ERR_ARG;
        }
        hipLaunchKernelGGL(crnn_conv_kernel, dim3((unsigned)grid), dim3(256), (size_t)a.rows_in * a.lds_pitch * 4, st, a);
        RS_HIP(hipGetLastError());
        in = a.y;
        in_pitch = a.out_pitch;
    }

    // recurrent stack
    const int T = p.T;
    const int nl = (int)m->layers.size();
    int in_dim_pitch = in_pitch;
    for (int l = 0; l < nl; ++l) {
        const LayerDev& L = m->layers[l];
        const bool last = l == nl - 1;
        RecArgs r;
        memset(&r, 0, sizeof(r));
        for (int d = 0; d < L.ndir; ++d) {
            const bool one = last && d == 1;        // the head reads the backward half at T - 1: its first step
            ProjArgs a;
            memset(&a, 0, sizeof(a));
            a.a = in;
            a.M = one ? B : (int64_t)B * T;
            a.a_pitch = in_dim_pitch;
            a.K = L.in_dim;
            a.KS = L.KSi;
            a.last_only = one;
            a.T_ld = T;
            a.B = B;
            a.ld = ld;
            a.len = d_len;
            a.ls = m->ls;
            a.w = L.wih[d];
            a.bias = L.bias[d];
            a.y = xp[d];
            a.N = L.N;
            const int64_t gx = (a.M + 63) / 64;
            if (gx > INT32_MAX) {
                set_error("rs_crnn_forward_ragged: grid too large: split the batch");
                return RS_ERR_ARG;
            }
            if (m->x3 && l > 0) {                   // the input is a previous layer's h
                ProjX3Args x;
                memset(&x, 0, sizeof(x));
                x.a = a.a;
                x.M = a.M;
                x.a_pitch = a.a_pitch;
                x.K = a.K;
                x.KS = L.KSi3;
                x.last_only = a.last_only;
                x.T_ld = T;
                x.B = B;
                x.ld = ld;
                x.len = d_len;
                x.ls = m->ls;
                x.w = reinterpret_cast<const u32x4*>(L.wih3[d].p);
                x.bias = L.bias[d];
                x.inv_s = L.inv_si[d];
                x.y = xp[d];
                x.N = L.N;
                hipLaunchKernelGGL(crnn_proj_x3_kernel, dim3((unsigned)gx, (unsigned)((L.N / 16 + 15) / 16)), dim3(256), 0, st, x);
            } else {
                hipLaunchKernelGGL(crnn_proj_kernel, dim3((unsigned)gx, (unsigned)((L.N / 16 + 3) / 4)), dim3(256), 0, st, a);
            }
            RS_HIP(hipGetLastError());
            r.xp[d] = xp[d];
            r.xp_rows[d] = one ? 1 : T;
            r.one_step[d] = one;
            r.whh[d] = L.whh[d];
            r.bhn[d] = L.bhn[d];
        }
        r.y = last ? nullptr : ybuf[l & 1];
        r.fin = last ? fin : nullptr;
        r.T_ld = T;
        r.y_pitch = cp4(L.ndir * L.H);
        r.fin_pitch = cp4(m->out_dim);
        r.B = B;
        r.ld = ld;
        r.gru = L.gru;
        r.H = L.H;
        r.Hp = L.Hp;
        r.HT = L.HT;
        r.KS = L.KSh;
        r.N = L.N;
        r.relu = L.relu;
        r.hpitch = L.Hp + 4;
        r.len = d_len;
        r.ls = m->ls;
        const dim3 grid((unsigned)((B + 15) / 16), (unsigned)L.ndir);
        const size_t lds = (size_t)48 * r.hpitch * 4;
        if (m->x3) {
            RecX3Args x;
            memset(&x, 0, sizeof(x));
            for (int d = 0; d < L.ndir; ++d) {
                x.xp[d] = r.xp[d];
                x.xp_rows[d] = r.xp_rows[d];
                x.one_step[d] = r.one_step[d];
                x.whh[d] = reinterpret_cast<const u32x4*>(L.whh3[d].p);
                x.inv_s[d] = L.inv_sh[d];
                x.bhn[d] = L.bhn[d];
            }
            x.y = r.y;
            x.fin = r.fin;
            x.T_ld = T;
            x.y_pitch = r.y_pitch;
            x.fin_pitch = r.fin_pitch;
            x.B = B;
            x.ld = ld;
            x.gru = L.gru;
            x.H = L.H;
            x.Hp = L.Hp;
            x.HT = L.HT;
            x.KS = L.KSh3;
            x.N = L.N;
            x.relu = L.relu;
            x.hp = 32 * L.KSh3 + 8;
            x.len = d_len;
            x.ls = m->ls;
            const size_t lds3 = (size_t)4 * 16 * x.hp * 2;      // two buffers of an f16 hi and an f16 lo plane
            if (L.H <= kResHidden)
                hipLaunchKernelGGL(crnn_rec_x3_kernel<true>, grid, dim3(512), lds3, st, x);
            else
                hipLaunchKernelGGL(crnn_rec_x3_kernel<false>, grid, dim3(512), lds3, st, x);
        } else if (L.H <= kResHidden)
            hipLaunchKernelGGL(crnn_rec_kernel<true>, grid, dim3(512), lds, st, r);
        else
            hipLaunchKernelGGL(crnn_rec_kernel<false>, grid, dim3(512), lds, st, r);
        RS_HIP(hipGetLastError());
        if (!last) {
            in = r.y;
            in_dim_pitch = r.y_pitch;
        }
    }
    hipLaunchKernelGGL(last_row_head_kernel<HasStep>, dim3((B + 255) / 256), dim3(256), 0, st, fin, B, cp4(m->out_dim), m->out_dim,
                       m->d_fcw, m->d_fcb, HasStep{d_len, ld, m->ls}, d_probs, d_logits);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

}  // extern "C"
