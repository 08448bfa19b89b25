// Generic ConvNets in split precision on the bf16 MFMA (rs_gconv_set_mode(m, RS_BF16X3)): the interface between the host
// program of csrc/gconv.hip and the kernel of csrc/gconv_x3.hip.  The plan and the weight packing are gconv/plan.hpp's
// (plan_x3, pack_weights_x3).
#pragma once
#include "common.hpp"

namespace rs {

struct GconvX3Args {
    const float* x;             // [B][in_rows][in_pitch] fp32, in_pitch a multiple of 4
    float* y;                   // [B][out_rows][out_pitch] fp32
    const int32_t* rows;        // [B] rows of each read at this conv's input
    const unsigned short* w;    // pack_weights_x3: the hi plane; the lo plane w_plane bf16 behind it
    const float* b;             // [cols of every block], zero padded
    int64_t w_plane;
    int in_rows, in_pitch, out_rows, out_pitch;
    int c_in, c_out, k, kc, nchunk, tiles;
    int c8_shift;               // log2(kc / 8)
    int steps, xpitch, slab_rows, slab_half, panel_half;    // gconv/plan.hpp: X3Plan
};

// shape: index into gconv::kShapes.  allow_lds: once per handle for a conv beyond 64 KB of dynamic LDS.
hipError_t gconv_x3_allow_lds(int shape, bool pool, int bytes);
hipError_t gconv_x3_launch(int shape, bool pool, const GconvX3Args& a, dim3 grid, size_t lds_bytes, hipStream_t st);

}  // namespace rs
