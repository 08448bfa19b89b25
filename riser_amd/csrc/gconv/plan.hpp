// Generic ConvNets (gconv.hip): the tile shape a conv takes and the order its weights are packed in.  Host only, no device
// call: rs_gconv_create refuses a net through plan_conv before it touches a device, and tests/gconv_ref.py mirrors the
// arithmetic below.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../family/host.hpp"      // cp4, p16

namespace rs {
namespace gconv {

constexpr int kMaxPools = 16;                       // rows of the length table - 1
constexpr int kLdsPrefer = 52 * 1024;               // three workgroups per CU
constexpr int kLdsMax = 160 * 1024;                 // one workgroup per CU
constexpr int kDeepFrom = 256;                      // p16(c_out) beyond this: 16-row tiles (wide layers sit deep, where reads are short)

// (row tiles, wave columns, column tiles per wave) of gconv_tile_kernel; a workgroup is 4 waves laid out (4 / wgc) x wgc
struct Shape {
    int rt, wgc, wc;
    int rows() const { return 16 * rt; }
    int cols() const { return 16 * wc * wgc; }
};
constexpr Shape kShapes[5] = {{4, 1, 2}, {4, 2, 2}, {4, 4, 2}, {1, 4, 1}, {1, 4, 2}};

struct TilePlan {
    int shape;                  // index into kShapes
    int vec;                    // 4: K groups of 16 channels, a lane's operand one float4; 1: groups of 4 (c_in <= 4)
    int kc, nchunk;             // channels per K chunk (a multiple of 4 vec), chunks
    int lpitch;                 // floats per slab row
    int slab_floats, panel_floats;
    int lds_bytes;
    int ncb;                    // column blocks
};

inline int slab_pitch(int kc) { return ((kc / 4) % 2 == 0) ? kc + 4 : kc; }

inline int lds_bytes_of(const Shape& s, int k, int kc) {
    return ((s.rows() + k - 1) * slab_pitch(kc) + s.cols() * k * kc) * 4;
}

// false: no shape holds the slab and the panel of even the smallest chunk
inline bool plan_conv(int c_in, int c_out, int k, TilePlan* out) {
    TilePlan p{};
    p.vec = c_in <= 4 ? 1 : 4;
    const int kg = 4 * p.vec;
    const int np = p16(c_out);
    const int deep[2] = {4, 3}, flat[3] = {2, 1, 0};
    const bool is_deep = np > kDeepFrom;
    const int* cand = is_deep ? deep : flat;
    const int ncand = is_deep ? 2 : 3;
    int pick = -1;
    for (int i = 0; i < ncand; ++i) {
        const Shape& s = kShapes[cand[i]];
        if (i + 1 < ncand && kShapes[cand[i + 1]].cols() >= np) continue;      // a narrower shape holds every column
        if (lds_bytes_of(s, k, kg) <= kLdsPrefer) {
            pick = cand[i];
            break;
        }
    }
    if (pick < 0) {
        pick = cand[ncand - 1];
        if (lds_bytes_of(kShapes[pick], k, kg) > kLdsMax) return false;
    }
    p.shape = pick;
    const Shape& s = kShapes[pick];
    const int cpad = (c_in + kg - 1) / kg * kg;
    p.kc = kg;
    if (p.vec == 4)
        for (int kc = 64; kc > 16; kc >>= 1)
            if (kc <= cpad && lds_bytes_of(s, k, kc) <= kLdsPrefer) {
                p.kc = kc;
                break;
            }
    p.nchunk = (c_in + p.kc - 1) / p.kc;
    p.lpitch = slab_pitch(p.kc);
    p.slab_floats = (s.rows() + k - 1) * p.lpitch;
    p.panel_floats = s.cols() * k * p.kc;
    p.lds_bytes = (p.slab_floats + p.panel_floats) * 4;
    p.ncb = (c_out + s.cols() - 1) / s.cols();
    if (out) *out = p;
    return true;
}

// w [c_out][c_in][k] -> [column block][chunk][column tile][tap][group][lane][vec]: the panel of one workgroup and one chunk is
// contiguous, and inside it a lane's B operands of one group are one vector.  Lane (rl, kq), element sub: column
// block * cols + 16 tile + rl, channel chunk * kc + 4 vec group + vec kq + sub.  Pads are zero.
inline std::vector<float> pack_weights(const float* w, int c_in, int c_out, int k, const TilePlan& p) {
    const Shape& s = kShapes[p.shape];
    const int G = p.kc / (4 * p.vec), nct = s.cols() / 16;
    std::vector<float> out((size_t)p.ncb * p.nchunk * p.panel_floats, 0.0f);
    size_t o = 0;
    for (int nb = 0; nb < p.ncb; ++nb)
        for (int ch = 0; ch < p.nchunk; ++ch)
            for (int ct = 0; ct < nct; ++ct)
                for (int tap = 0; tap < k; ++tap)
                    for (int g = 0; g < G; ++g)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int sub = 0; sub < p.vec; ++sub, ++o) {
                                const int col = nb * s.cols() + 16 * ct + (lane & 15);
                                const int ci = ch * p.kc + 4 * p.vec * g + p.vec * (lane >> 4) + sub;
                                if (col < c_out && ci < c_in) out[o] = w[((size_t)col * c_in + ci) * k + tap];
                            }
    return out;
}

// ---- split precision on the bf16 MFMA (gconv_x3.hip): the fp32 plan's shape, kc and nchunk, its own slab and packing ----
// K of a chunk is tap-major over the chunk's kc channels, cut into k-steps of 32: lane (rl, kq) of step s takes pair
// p = 4 s + kq, i.e. tap p / (kc / 8) and the 8 channels 8 (p % (kc / 8)) ..  Pairs behind the last tap (kc = 16 only: two
// taps per step, k odd) meet zero weights and read a zeroed spare slab row.
struct X3Plan {
    int steps;                  // ceil(k kc / 32)
    int xpitch;                 // bf16 per slab row: kc + 8, an odd number of 16-byte units
    int slab_rows;              // tile rows + the last tap any pair addresses (k - 1, or k with a spare row)
    int slab_half, panel_half;  // bf16 per plane: the slab; one chunk's panel of one column block
    int lds_bytes;              // both planes of both
};

inline X3Plan plan_x3(const TilePlan& p, int k) {
    const Shape& s = kShapes[p.shape];
    const int c8n = p.kc / 8;
    X3Plan x{};
    x.steps = (k * p.kc + 31) / 32;
    x.xpitch = (c8n % 2 == 0) ? p.kc + 8 : p.kc;
    x.slab_rows = s.rows() + (4 * x.steps - 1) / c8n;
    x.slab_half = x.slab_rows * x.xpitch;
    x.panel_half = s.cols() * x.steps * 32;
    x.lds_bytes = (x.slab_half + x.panel_half) * 4;
    return x;
}

inline uint16_t bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

inline float bf16_val(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// pack_weights undone: [c_out][c_in][k] from the packed fp32 panels (rs_gconv_set_mode reads them back from the device, so a
// handle keeps no host copy of its weights)
inline std::vector<float> unpack_weights(const float* packed, int c_in, int c_out, int k, const TilePlan& p) {
    const Shape& s = kShapes[p.shape];
    const int G = p.kc / (4 * p.vec), nct = s.cols() / 16;
    std::vector<float> w((size_t)c_out * c_in * k, 0.0f);
    size_t o = 0;
    for (int nb = 0; nb < p.ncb; ++nb)
        for (int ch = 0; ch < p.nchunk; ++ch)
            for (int ct = 0; ct < nct; ++ct)
                for (int tap = 0; tap < k; ++tap)
                    for (int g = 0; g < G; ++g)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int sub = 0; sub < p.vec; ++sub, ++o) {
                                const int col = nb * s.cols() + 16 * ct + (lane & 15);
                                const int ci = ch * p.kc + 4 * p.vec * g + p.vec * (lane >> 4) + sub;
                                if (col < c_out && ci < c_in) w[((size_t)col * c_in + ci) * k + tap] = packed[o];
                            }
    return w;
}

// w [c_out][c_in][k] -> two planes [hi | lo] of bf16 bit patterns, each [column block][chunk][column tile][step][lane][8]: hi =
// bf16(w), lo = bf16(w - hi), round to nearest even.  Lane (rl, kq), element e of step s: column block * cols + 16 tile + rl,
// pair p = 4 s + kq, tap p / (kc / 8), channel chunk * kc + 8 (p % (kc / 8)) + e.  Zero where tap >= k, the channel >= c_in
// or the column >= c_out.
inline std::vector<uint16_t> pack_weights_x3(const float* w, int c_in, int c_out, int k, const TilePlan& p) {
    const Shape& s = kShapes[p.shape];
    const X3Plan x = plan_x3(p, k);
    const int c8n = p.kc / 8, nct = s.cols() / 16;
    const size_t plane = (size_t)p.ncb * p.nchunk * x.panel_half;
    std::vector<uint16_t> out(2 * plane, 0);
    size_t o = 0;
    for (int nb = 0; nb < p.ncb; ++nb)
        for (int ch = 0; ch < p.nchunk; ++ch)
            for (int ct = 0; ct < nct; ++ct)
                for (int st = 0; st < x.steps; ++st)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 8; ++e, ++o) {
                            const int pr = 4 * st + (lane >> 4);
                            const int tap = pr / c8n, ci = ch * p.kc + 8 * (pr % c8n) + e;
                            const int col = nb * s.cols() + 16 * ct + (lane & 15);
                            if (tap >= k || ci >= c_in || col >= c_out) continue;
                            const float v = w[((size_t)col * c_in + ci) * k + tap];
                            const uint16_t h = bf16_rne(v);
                            out[o] = h;
                            out[plane + o] = bf16_rne(v - bf16_val(h));
                        }
    return out;
}

}  // namespace gconv
}  // namespace rs
