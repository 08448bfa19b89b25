// ConvNet weight packing, host side only: the number formats, the sizing rules and the layouts of the packed weight tables,
// and the one loop that fills any of them from a layer's [c_out][c_in][3] weights.
#pragma once
#include <math.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "common.hpp"

namespace rs {
namespace {

// ---- number formats ---------------------------------------------------------------------------
// 16-bit storage type of a mode (RS_BF16 or RS_F16), also for the split-precision modes
int base16(int dtype) { return is_f16_family(dtype) ? RS_F16 : RS_BF16; }

// fp32 -> bf16 / f16 bits, round to nearest even (host side, weight packing)
float from_h16(unsigned short u, int dtype) {
    if (dtype == RS_F16) return (float)__builtin_bit_cast(_Float16, u);
    return __builtin_bit_cast(float, (unsigned)u << 16);
}

unsigned short to_h16(float f, int dtype) {
    if (dtype == RS_F16) return __builtin_bit_cast(unsigned short, (_Float16)f);
    unsigned u = __builtin_bit_cast(unsigned, f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}

// fp32 -> OCP e4m3 (bias 7, largest finite 448, subnormals of 2^-9), round to nearest even, saturating
unsigned char to_e4m3(float f) {
    const unsigned char sign = std::signbit(f) ? 0x80 : 0x00;
    float a = fabsf(f);
    if (!(a == a)) return (unsigned char)(sign | 0x7f);
    if (a >= 448.0f) return (unsigned char)(sign | 0x7e);
    int e = a > 0.0f ? ilogbf(a) : -127;
    if (e < -6) e = -6;                                       // subnormal quantum 2^-9
    const float q = ldexpf(1.0f, e - 3);
    const float n = nearbyintf(a / q);                        // half to even (default rounding mode); n <= 16
    if (n == 0.0f) return sign;
    int m = (int)n, ee = e;
    if (m == 16) {                                            // rounded up into the next binade
        m = 8;
        ++ee;
    }
    if (m < 8) return (unsigned char)(sign | m);              // subnormal: exponent field 0
    return (unsigned char)(sign | ((ee + 7) << 3) | (m - 8));
}

// power-of-two scale 2^k of a half-precision layer's packed weights (ConvLayerDev::w_unscale = 2^-k): max |w| 2^k in
// [8192, 16384).  1 for the bf16 modes and for weights that are all zero or not finite.
float weight_scale(const float* w, size_t count, int dtype) {
    if (!is_f16_family(dtype)) return 1.0f;
    float wmax = 0.0f;
    for (size_t k = 0; k < count; ++k) wmax = std::max(wmax, fabsf(w[k]));
    if (wmax > 0.0f && std::isfinite(wmax)) return ldexpf(1.0f, std::min(60, std::max(-60, 13 - ilogbf(wmax))));
    return 1.0f;
}

// ---- which layers, which row widths -----------------------------------------------------------
// RS_F16XF8: layer i can take part in a run of F8 rows (conv_ring_f8.hip).  Wide layers only (RS_F8_MIN_CIN input channels,
// default 200: layers 7-11 of the shipped net): with 2/3 of the matrix-pipe time a tile of this kernel is bound three ways at
// once - MFMA, L2 -> LDS staging (~24 B/clk/CU) and LDS fragment reads are each ~1 500 cycles per sub-stage at 256 x 192 - and
// its even-NT tile shapes cover the narrow layers' columns worse than the split-precision kernel's (measured, 512 x 16000:
// layers 4, 5 +20 ... +30 %, layer 6 +-0, layers 7 / 8 / 9 / 11 -5 / -11 / -10 / -18 %)
bool f8_eligible(const Hooks& h, int dtype, int i, int n_layers, const int32_t* channels) {
    return dtype == RS_F16XF8 && i >= 3 && i < n_layers && channels[i - 1] >= std::max(64, h.f8_min_cin);
}
// ... once per layer: f8[0 .. n_layers], the last entry (the layer behind the net) false.  The rows BETWEEN two eligible
// layers are F8 rows: layer i reads them if f8[i - 1] && f8[i], writes them if f8[i] && f8[i + 1].
void f8_layers(const Hooks& h, int dtype, int n_layers, const int32_t* channels, bool f8[kMaxLayers + 1]) {
    for (int i = 0; i <= n_layers; ++i) f8[i] = f8_eligible(h, dtype, i, n_layers, channels);
}

// row width of a layer's output buffer: channels padded to 16 bytes; split precision: 32-channel panels laid out as
// [hi x 32 | lo x 32] (conv_ring_h16.hip); F8 rows: 128 elements (an H and an F panel) per 64 channels
int row_pitch(int dtype, int channels, bool f8_rows) {
    if (f8_rows) return 128 * ((channels + 63) / 64);
    return is_x3(dtype) ? 64 * ((channels + 31) / 32) : round_up(channels, (dtype == RS_F32 || dtype == RS_F32W) ? 4 : 8);
}

// ---- layouts ----------------------------------------------------------------------------------
// A layout names its element type T, sizes its table (elems) and stores row kw < kRows of the (output channel n, input
// channel ci) pair, whose three taps are g[0 .. 2] (put).  What put() never touches stays zero.

// layer 0 (one input channel): [cp][4] = (w0, w1, w2, bias); pack_layer0 adds the bias
struct Layer0Layout {
    typedef float T;
    static constexpr int kRows = 3;
    int cp;
    size_t elems() const { return (size_t)cp * 4; }
    void put(std::vector<float>& dst, int n, int, int kw, const float* g) const { dst[(size_t)n * 4 + kw] = g[kw]; }
};

// fp32 kernels: [n_alloc][nch][R][kc], chunks of plan.kc input channels (convnet_model.hpp: plan_static_*).  The R rows of a
// channel pair are its three taps (direct, conv_f32.hip) or its Winograd filter transform U = G g, computed in fp64 and
// rounded once: F(2,3) (conv_wino.hip) U0 = g0, U1 = (g0+g1+g2)/2, U2 = (g0-g1+g2)/2, U3 = g2; F(4,3) (conv_wino4.hip) below
template <int R>
double filter_row(int j, const float* g);
template <>
double filter_row<3>(int j, const float* g) { return g[j]; }
template <>
double filter_row<4>(int j, const float* g) {
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    const double u[4] = {g0, (g0 + g1 + g2) * 0.5, (g0 - g1 + g2) * 0.5, g2};
    return u[j];
}
template <>
double filter_row<6>(int j, const float* g) {
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    const double u[6] = {g0 / 4.0, -(g0 + g1 + g2) / 6.0, -(g0 - g1 + g2) / 6.0,
                         g0 / 24.0 + g1 / 12.0 + g2 / 6.0, g0 / 24.0 - g1 / 12.0 + g2 / 6.0, g2};
    return u[j];
}
template <int R>
struct ChunkedF32 {
    typedef float T;
    static constexpr int kRows = R;
    ConvPlan p;
    size_t elems() const { return (size_t)p.n_alloc * p.nch * R * p.kc; }
    void put(std::vector<float>& dst, int n, int ci, int j, const float* g) const {
        const int c = ci / p.kc, cc = ci - c * p.kc;
        dst[(((size_t)n * p.nch + c) * R + j) * p.kc + cc] = (float)filter_row<R>(j, g);
    }
};

// 16-bit modes.  Every packing is [panel][tap][n_alloc][width] of weights x ws (weight_scale) in the mode's storage type st16.
struct Panels16 {
    int panels, n_alloc, width;
    float ws;
    int st16;
    size_t elems() const { return (size_t)panels * 3 * n_alloc * width; }
    size_t at(int pn, int kw, int n) const { return (((size_t)pn * 3 + kw) * n_alloc + n) * width; }
};
// plain 16-bit: panels of `width` input channels - 32 for the streaming kernel of layers 1-2 (conv_stream_h16.hip, d_w), 64
// for the ring kernel (conv_ring_h16.hip, d_w2)
struct PlainLayout : Panels16 {
    typedef unsigned short T;
    static constexpr int kRows = 3;
    void put(std::vector<T>& dst, int n, int ci, int kw, const float* g) const {
        dst[at(ci / width, kw, n) + ci % width] = to_h16(g[kw] * ws, st16);
    }
};
// split precision (ring kernel): a panel is 32 input channels as [hi x 32 | lo x 32] with lo = round(w - hi).  tail: the
// merged tail slab sits in the last panel's tap-0 place, K group kw = tap kw's 8 channel slots
struct SplitLayout : Panels16 {
    typedef unsigned short T;
    static constexpr int kRows = 3;
    bool tail;
    void put(std::vector<T>& dst, int n, int ci, int kw, const float* g) const {
        const float wv = g[kw] * ws;
        const unsigned short hi = to_h16(wv, st16);
        const int pn = ci / 32, cc = ci - pn * 32;
        const size_t a = tail && pn == panels - 1 ? at(pn, 0, n) + 8 * kw + cc : at(pn, kw, n) + cc;
        dst[a] = hi;
        dst[a + 32] = to_h16(wv - from_h16(hi, st16), st16);
    }
};
// F8 rows (conv_ring_f8.hip): per 64 input channels an H panel (hi16 x 64) and an F panel of e4m3 bytes
// [lo8 c0-31 | hi8 c0-31 | lo8 c32-63 | hi8 c32-63], hi8 = e4m3(hi 2^-6), lo8 = e4m3((w - hi) 2^5)
struct F8Layout : Panels16 {
    typedef unsigned short T;
    static constexpr int kRows = 3;
    void put(std::vector<T>& dst, int n, int ci, int kw, const float* g) const {
        const float wv = g[kw] * ws;
        const unsigned short hi = to_h16(wv, st16);
        const float hf = from_h16(hi, st16);
        const int pn = ci / 64, cc = ci - pn * 64;
        dst[at(2 * pn, kw, n) + cc] = hi;
        unsigned char* fb = reinterpret_cast<unsigned char*>(dst.data()) + at(2 * pn + 1, kw, n) * 2 + (cc >> 5) * 64 + (cc & 31);
        fb[0] = to_e4m3(ldexpf(wv - hf, 5));
        fb[32] = to_e4m3(ldexpf(hf, -6));
    }
};

// Sizes of a 16-bit layer's tables (L's channels, pitches and f8_in / f8_out are set): plan.kc / nch for the 32-channel
// panels of d_w, ring_panels / ring_tail for d_w2
void plan_h16(ConvLayerDev& L, bool x3, bool x3_tail) {
    L.plan.kc = 32;
    L.plan.nch = x3 ? (L.c_in + 31) / 32 : (L.cp_in + 31) / 32;
    // rows of the packed weight / bias tables: the channels (split precision: all 32 slots of the last panel,
    // every one of which a tile covers) plus zero rows for the widest tile's overhang
    L.plan.n_alloc = (L.f8_out ? 64 * ((L.c_out + 63) / 64) : x3 ? 32 * ((L.c_out + 31) / 32) : round_up(L.c_out, 16)) + conv_ring_max_bn();
    // a panel is 64 input channels, or 32 input channels as hi | lo in split precision, or - F8 rows - an H and an F panel
    // per 64 input channels
    L.ring_panels = L.f8_in ? 2 * ((L.c_in + 63) / 64) : x3 ? (L.c_in + 31) / 32 : (L.cp_in + 63) / 64;
    // split precision, a last panel of at most 8 channels behind 2 ... 4 full ones (67 = 64 + 3, 100 = 96 + 4): its three
    // taps become one K step (conv_ring_h16.hip: TAIL).  Not where another kernel reads the same packing (the 8-bit
    // kernel's split-precision input, the weights-resident kernel): a layer's bits must not depend on who runs it.
    const int x3_panels = (L.c_in + 31) / 32;
    L.ring_tail = x3 && x3_tail && !L.f8_in && !L.f8_out && L.c_in % 32 >= 1 && L.c_in % 32 <= 8 && x3_panels >= 3 && x3_panels <= 5;
}

// ---- the packer -------------------------------------------------------------------------------
// w = [c_out][c_in][3]
template <class Layout>
std::vector<typename Layout::T> pack_conv3(const Layout& lay, const float* w, int c_out, int c_in) {
    std::vector<typename Layout::T> dst(lay.elems(), 0);
    for (int n = 0; n < c_out; ++n)
        for (int ci = 0; ci < c_in; ++ci)
            for (int kw = 0; kw < Layout::kRows; ++kw) lay.put(dst, n, ci, kw, &w[((size_t)n * c_in + ci) * 3]);
    return dst;
}

std::vector<float> pack_layer0(int cp, int c_out, const float* w, const float* b) {
    std::vector<float> w4 = pack_conv3(Layer0Layout{cp}, w, c_out, 1);
    for (int c = 0; c < c_out; ++c) w4[(size_t)c * 4 + 3] = b[c];
    return w4;
}

}  // namespace
}  // namespace rs
