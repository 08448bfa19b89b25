// Sequential conv programs (seqnet.hip), host side: the two weight layouts of the MFMA kernels and one packer over them; the
// packed matrices are uploaded into the device buffers of devbuf.hpp.
#pragma once
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "../common.hpp"
#include "../devbuf.hpp"

namespace rs {
namespace {
// float -> bf16, round to nearest even (what v_cvt_pk_bf16_f32 does for finite values)
unsigned short bf16_rne(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (unsigned short)(u >> 16);       // inf / nan: truncate
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
float bf16_widen(unsigned short h) {
    const unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// Where element (kidx, n) of a GEMM's B matrix of column pitch NP lives.
// fp32: [K16 / 4][NP][4] - lane (column, k-group) reads the B operands of four k-steps with one ds_read_b128
struct PackF32 {
    typedef float T;
    static void put(std::vector<float>& dst, int NP, int kidx, int n, float w) { dst[((size_t)(kidx / 4) * NP + n) * 4 + kidx % 4] = w; }
};
// split precision: two planes [hi | lo] (each half of dst) of [k-step of 32][kq][NP][8 x bf16]
struct PackSplit {
    typedef unsigned short T;
    static void put(std::vector<unsigned short>& dst, int NP, int kidx, int n, float w) {
        const size_t at = (((size_t)(kidx / 32) * 4 + (kidx % 32) / 8) * NP + n) * 8 + kidx % 8;
        const unsigned short h = bf16_rne(w);
        dst[at] = h;
        dst[dst.size() / 2 + at] = bf16_rne(w - bf16_widen(h));
    }
};

// A conv of k taps, host weights w = [c_out][c_in][k] (null: no such conv), as GEMM columns co, K index k0 + tap * pitch + c.
// A 1x1 shortcut conv behind another conv's K range is k = 1 at that k0.
struct ConvSrc {
    const float* w;
    int c_in, k, pitch, k0;
};
template <class Layout>
void pack_conv(std::vector<typename Layout::T>& dst, int NP, int c_out, const ConvSrc& c) {
    for (int co = 0; c.w && co < c_out; ++co)
        for (int ci = 0; ci < c.c_in; ++ci)
            for (int kk = 0; kk < c.k; ++kk)
                Layout::put(dst, NP, c.k0 + kk * c.pitch + ci, co, c.w[((size_t)co * c.c_in + ci) * c.k + kk]);
}

// one weight matrix of `elems` elements (its zero padding is part of the layout: the kernels copy all of it to LDS), column pitch
// NP, holding the given convs, on the device
template <class Layout>
hipError_t pack_upload(DevBuf<typename Layout::T>& d, size_t elems, int NP, int c_out, std::initializer_list<ConvSrc> convs) {
    std::vector<typename Layout::T> v(elems, 0);
    for (const ConvSrc& c : convs) pack_conv<Layout>(v, NP, c_out, c);
    return upload(d, v);
}
}  // namespace
}  // namespace rs
