// The CNN-RNN's f16x3 mode (RS_F16X3): every gate GEMM whose A operand is a hidden state runs as hi*hi + lo*hi + hi*lo on
// v_mfma_f32_16x16x32_f16 with fp32 accumulation (hi = f16(v), lo = f16(v - hi)).  Kernels, the host's f16 conversion and the
// weight packer; crnn.hip launches them.
//
//   crnn_proj_x3_kernel   the input projection of every layer but the first (their input is a previous layer's h, in (-1, 1)).
//                         A workgroup (4 waves) takes 64 rows x 256 gate columns; per 64-wide k-chunk the 256 threads load the
//                         fp32 rows once, split them and stage the f16 hi / lo planes in LDS (A is split once per tile); wave w
//                         owns 4 column tiles and all 4 row tiles, so a weight fragment read from the cache meets 4 row tiles.
//   crnn_rec_x3_kernel    the persistent recurrence with crnn_rec_kernel's ownership (16 reads x one direction per workgroup,
//                         8 waves, wave w owns hidden units 16 w .. and all their gates, one barrier per step).  h lives in LDS
//                         as two f16 planes (hi, lo), double-buffered, written by the lane that produces h: every wave reads
//                         ready-made A fragments, one 16-byte read per plane and k-step.  The fp32 state a lane needs again (the
//                         LSTM's c, the GRU's h) stays in that lane's registers: a lane owns the same (read, unit) every step.
//                         For hidden <= 128 the packed W_hh halves stay in VGPRs (4 gates x 4 k-steps x 4 VGPRs x 2 halves).
//
// Scales: h is stored as f16 halves of 1024 h (|1024 h| < 1024: the lo half of a typical h is a normal f16); a weight matrix
// as halves of s w with s the power of two that puts max |w| into [2^13, 2^14).  Both are undone exactly on the accumulator
// (inv_s = 1 / (1024 s), a power of two).  No operand can reach f16's 65504, so the mode has no range check and no flag.
// The k order: at k-step ks lane (r, q) holds k = 32 ks + 8 q + j, j = 0..7; a chain is ks ascending, hi*hi, lo*hi, hi*lo in
// each step, whatever the batch, the tile or ld: a read gets the bits it gets alone.
#pragma once
#include "../seqnet/mfma_split.hpp"
#include "shared.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace rs {
namespace {

constexpr float kHScale = 1024.0f;
constexpr int kProjRows = 64;                       // rows of A per workgroup
constexpr int kProjKc = 64;                         // k per staged chunk
constexpr int kProjPitch = kProjKc + 8;             // halves per LDS row: 16-byte row reads of 16 rows hit 64 distinct banks

inline int p32(int c) { return (c + 31) & ~31; }

struct ProjX3Args {
    const float* a;             // [rows][a_pitch] fp32, K = in_dim, values in (-1, 1)
    int64_t M;
    int a_pitch, K, KS;         // KS = p32(K) / 32
    int last_only, T_ld, B, ld;
    const int32_t* len;
    Lens ls;
    const u32x4* w;             // packed [N / 16][KS][hi, lo][64]
    const float* bias;          // [N]
    float inv_s;
    float* y;                   // [M][N]
    int N;
};

__global__ __launch_bounds__(256) void crnn_proj_x3_kernel(const ProjX3Args a) {
    __shared__ __attribute__((aligned(16))) unsigned short pl[2][kProjRows * kProjPitch];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * kProjRows;
    const int ct0 = blockIdx.y * 16 + wave * 4;
    const int nct = a.N / 16;
    // staging: thread t takes float4 column c4 = t % 16 of rows t / 16 + 16 i
    const int c4 = threadIdx.x & 15, srow = threadIdx.x >> 4;
    const float* Ar[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t grow = r0 + srow + 16 * i;
        ok[i] = grow < a.M;
        int64_t src = grow;
        if (a.last_only && ok[i]) {
            const int T = crnn_len(a.len, (int)grow, a.ld, a.ls, a.ls.n);
            src = grow * a.T_ld + (T > 0 ? T - 1 : 0);
        }
        Ar[i] = a.a + (ok[i] ? src : 0) * a.a_pitch;
    }
    f32x4 acc[4][4];
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[rt][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int Kp = a.KS * 32;
    for (int kc = 0; kc < Kp; kc += kProjKc) {
        __syncthreads();
        const int k0 = kc + 4 * c4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (ok[i] && k0 < a.K) {
                v = *reinterpret_cast<const f32x4*>(Ar[i] + k0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k0 + e >= a.K) v[e] = 0.0f;     // pad columns of the buffer are not written: never read them
            }
            unsigned hi[2], lo[2];
            split2_f16(v[0] * kHScale, v[1] * kHScale, hi[0], lo[0]);
            split2_f16(v[2] * kHScale, v[3] * kHScale, hi[1], lo[1]);
            const int o = (srow + 16 * i) * kProjPitch + 4 * c4;
            *reinterpret_cast<uint2*>(&pl[0][o]) = make_uint2(hi[0], hi[1]);
            *reinterpret_cast<uint2*>(&pl[1][o]) = make_uint2(lo[0], lo[1]);
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < kProjKc / 32; ++sub) {
            const int ks = kc / 32 + sub;
            if (ks >= a.KS) break;
            u32x4 bh[4], bl[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bool on = ct0 + t < nct;
                const u32x4* wp = a.w + ((int64_t)((on ? ct0 + t : 0) * a.KS + ks) * 2) * 64 + lane;
                bh[t] = wp[0];
                bl[t] = wp[64];
            }
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) {
                const int o = (rt * 16 + rl) * kProjPitch + 32 * sub + 8 * kq;
                const u32x4 ah = *reinterpret_cast<const u32x4*>(&pl[0][o]);
                const u32x4 al = *reinterpret_cast<const u32x4*>(&pl[1][o]);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (ct0 + t < nct) acc[rt][t] = mfma_x3_f16(ah, al, bh[t], bl[t], acc[rt][t]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (ct0 + t >= nct) continue;
        const int col = (ct0 + t) * 16 + rl;
        const float bias = a.bias[col];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t row = r0 + rt * 16 + 4 * kq + e;
                if (row < a.M) a.y[row * a.N + col] = acc[rt][t][e] * a.inv_s + bias;
            }
    }
}

struct RecX3Args {
    const float* xp[2];         // as RecArgs
    int xp_rows[2];
    int one_step[2];
    const u32x4* whh[2];        // packed [ng * HT][KS][hi, lo][64]
    float inv_s[2];
    const float* bhn[2];
    float* y;
    float* fin;
    int T_ld, y_pitch, fin_pitch;
    int B, ld, gru, H, Hp, HT, KS, N, relu, hp;     // KS = p32(Hp) / 32; hp = 32 KS + 8: halves per row of a plane
    const int32_t* len;
    Lens ls;
};

template <bool kResident>
__global__ __launch_bounds__(512) void crnn_rec_x3_kernel(const RecX3Args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned short hpl[];     // [buffer][hi, lo][16][hp]
    __shared__ int Tb[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int dir = blockIdx.y;
    const int b0 = blockIdx.x * 16;
    const int ng = a.gru ? 3 : 4;
    const int plane = 16 * a.hp;
    for (int e = threadIdx.x; e < 2 * plane; e += 512) reinterpret_cast<unsigned*>(hpl)[e] = 0u;
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
    const u32x4* __restrict__ W = a.whh[dir];
    const float inv_s = a.inv_s[dir];

    u32x4 wh[kResident ? 4 : 1][kResident ? 4 : 1], wl[kResident ? 4 : 1][kResident ? 4 : 1];
    if constexpr (kResident) {
        const int j = wave < a.HT ? wave : 0;
#pragma unroll
        for (int gi = 0; gi < 4; ++gi)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bool on = gi < ng && ks < a.KS;
                const u32x4* wp = W + ((int64_t)((on ? gi * a.HT + j : 0) * a.KS + (on ? ks : 0)) * 2) * 64 + lane;
                wh[gi][ks] = on ? wp[0] : (u32x4){0u, 0u, 0u, 0u};
                wl[gi][ks] = on ? wp[64] : (u32x4){0u, 0u, 0u, 0u};
            }
    }
    constexpr int JN = kResident ? 1 : 3;       // tiles of a wave: HT <= 8 resident, <= 20 (hidden 320) otherwise
    float st[JN][4];                            // this lane's fp32 state: the LSTM's c, the GRU's h
#pragma unroll
    for (int jj = 0; jj < JN; ++jj)
#pragma unroll
        for (int e = 0; e < 4; ++e) st[jj][e] = 0.0f;
    int Trow[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) Trow[e] = Tb[4 * kq + e];

    for (int s = 0; s < steps; ++s) {
        const unsigned short* cur = hpl + (s & 1) * 2 * plane;
        unsigned short* nxt = hpl + ((s & 1) ^ 1) * 2 * plane;
#pragma unroll
        for (int jj = 0; jj < JN; ++jj) {
            const int j = wave + 8 * jj;
            if (j >= a.HT) continue;
            const int u = 16 * j + rl;
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
            const unsigned short* hr = cur + rl * a.hp + 8 * kq;
            if constexpr (kResident) {
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) {
                    if (ks < a.KS) {
                        const u32x4 ah = *reinterpret_cast<const u32x4*>(hr + 32 * ks);
                        const u32x4 al = *reinterpret_cast<const u32x4*>(hr + plane + 32 * ks);
#pragma unroll
                        for (int gi = 0; gi < 4; ++gi)
                            if (gi < ng) acc[gi] = mfma_f16(ah, wh[gi][ks], acc[gi]);
#pragma unroll
                        for (int gi = 0; gi < 4; ++gi)
                            if (gi < ng) acc[gi] = mfma_f16(al, wh[gi][ks], acc[gi]);
#pragma unroll
                        for (int gi = 0; gi < 4; ++gi)
                            if (gi < ng) acc[gi] = mfma_f16(ah, wl[gi][ks], acc[gi]);
                    }
                }
            } else {
                for (int ks = 0; ks < a.KS; ++ks) {
                    const u32x4 ah = *reinterpret_cast<const u32x4*>(hr + 32 * ks);
                    const u32x4 al = *reinterpret_cast<const u32x4*>(hr + plane + 32 * ks);
                    u32x4 bh[4], bl[4];
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi) {
                        const u32x4* wp = W + ((int64_t)((gi < ng ? gi * a.HT + j : 0) * a.KS + ks) * 2) * 64 + lane;
                        bh[gi] = wp[0];
                        bl[gi] = wp[64];
                    }
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi)
                        if (gi < ng) acc[gi] = mfma_f16(ah, bh[gi], acc[gi]);
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi)
                        if (gi < ng) acc[gi] = mfma_f16(al, bh[gi], acc[gi]);
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi)
                        if (gi < ng) acc[gi] = mfma_f16(ah, bl[gi], acc[gi]);
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
                    const float rg = sigm(xv[e][0] + acc[0][e] * inv_s);
                    const float zg = sigm(xv[e][1] + acc[1][e] * inv_s);
                    const float ng_ = tanhf(xv[e][2] + rg * (acc[2][e] * inv_s + bhn));
                    h = (1.0f - zg) * ng_ + zg * st[jj][e];
                    st[jj][e] = h;
                } else {
                    const float ig = sigm(xv[e][0] + acc[0][e] * inv_s);
                    const float fg = sigm(xv[e][1] + acc[1][e] * inv_s);
                    const float gg = tanhf(xv[e][2] + acc[2][e] * inv_s);
                    const float og = sigm(xv[e][3] + acc[3][e] * inv_s);
                    const float c = fg * st[jj][e] + ig * gg;
                    st[jj][e] = c;
                    h = og * tanhf(c);
                }
                const float hs = h * kHScale;
                const _Float16 hh = (_Float16)hs;
                const _Float16 hlo = (_Float16)(hs - (float)hh);
                nxt[r * a.hp + u] = __builtin_bit_cast(unsigned short, hh);
                nxt[plane + r * a.hp + u] = __builtin_bit_cast(unsigned short, hlo);
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

// fp32 -> f16 bits, round to nearest even, subnormals kept: the device's conversion, on the host
inline uint16_t f16_bits(float f) {
    uint32_t x;
    memcpy(&x, &f, 4);
    const uint16_t sign = (uint16_t)((x >> 16) & 0x8000u);
    x &= 0x7fffffffu;
    if (x >= 0x7f800000u) return sign | (x > 0x7f800000u ? 0x7e00u : 0x7c00u);
    if (x >= 0x477ff000u) return sign | 0x7c00u;                   // 65520 and above round to infinity
    if (x < 0x38800000u) {                                          // below 2^-14: a subnormal, unit 2^-24
        if (x < 0x33000000u) return sign;                           // below 2^-25
        const int shift = 126 - (int)(x >> 23);
        const uint32_t m = (x & 0x7fffffu) | 0x800000u;
        uint32_t r = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (r & 1u))) ++r;
        return sign | (uint16_t)r;
    }
    uint32_t r = (x - 0x38000000u) >> 13;
    const uint32_t rem = x & 0x1fffu;
    if (rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ++r;
    return sign | (uint16_t)r;
}

inline float f16_value(uint16_t h) {
    const int e = (h >> 10) & 31, m = h & 0x3ff;
    const float v = e == 0 ? ldexpf((float)m, -24) : ldexpf((float)(m | 0x400), e - 25);
    return (h & 0x8000) ? -v : v;
}

// w [ng * H][K] (gate-major) -> the f16 hi / lo B fragments of every 16-column tile of the padded gate layout in the k order
// of the kernels above, [N / 16][p32(K) / 32][hi, lo][64] x 4 dwords, of s w with s = 2^e, max |s w| in [2^13, 2^14);
// inv_s = 1 / (kHScale s).  False for a weight that is not finite.
bool pack_gates_x3(const float* w, int ng, int H, int Hp, int K, std::vector<uint32_t>& out, float& inv_s) {
    float mx = 0.0f;
    for (size_t i = 0; i < (size_t)ng * H * K; ++i) {
        if (!std::isfinite(w[i])) return false;
        mx = std::max(mx, std::fabs(w[i]));
    }
    int ex = 0, sh = 0;
    if (mx > 0.0f) {
        (void)frexpf(mx, &ex);                      // mx = f 2^ex, f in [0.5, 1)
        sh = std::min(14 - ex, 110);
    }
    const float s = ldexpf(1.0f, sh);
    inv_s = ldexpf(1.0f, -sh) / kHScale;
    const int N = ng * Hp, KS = p32(K) / 32;
    out.assign((size_t)(N / 16) * KS * 2 * 64 * 4, 0u);
    for (int ct = 0; ct < N / 16; ++ct)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane) {
                const int col = ct * 16 + (lane & 15), gi = col / Hp, u = col - gi * Hp;
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * ks + 8 * (lane >> 4) + j;
                    if (u >= H || k >= K) continue;
                    const float v = w[(size_t)(gi * H + u) * K + k] * s;
                    const uint16_t hi = f16_bits(v), lo = f16_bits(v - f16_value(hi));
                    const size_t base = (((size_t)ct * KS + ks) * 2 * 64 + lane) * 4 + j / 2;
                    out[base] |= (uint32_t)hi << (16 * (j & 1));
                    out[base + 64 * 4] |= (uint32_t)lo << (16 * (j & 1));
                }
            }
    return true;
}

}  // namespace
}  // namespace rs
