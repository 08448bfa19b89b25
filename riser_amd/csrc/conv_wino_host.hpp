// Host side of the two tiled fp32 Winograd kernels (conv_wino.hip: F(2,3), conv_wino4.hip: F(4,3)), parameterised by the
// transform size M: the F(2,3) kernel-argument record, the LDS and cost formulas behind the tile planner (tile_plan.hpp), and the
// launcher.  A kernel file keeps its shape table, its cost coefficients and the functions common.hpp declares, which forward
// here.  Row unit of a family: pooled rows (M = 2) or groups of four conv rows (M = 4).
#pragma once
#include "conv_wino_device.hpp"
#include "tile_plan.hpp"
#include "tile_walk.hpp"

#include <stdio.h>

#include <algorithm>

namespace rs {

// the F(2,3) kernel's arguments (the F(4,3) kernel keeps a record of its own, conv_wino4.hip: Wino4Args)
struct WinoArgs {
    const float* x;
    const float* w;        // packed [n_alloc][nch][4][kc] (U0..U3), zero rows beyond c_out
    const float* bias;     // [n_alloc]
    float* y;
    const int32_t* len;
    unsigned x_bytes;      // size of the activation buffer x (rows_in * cp_in floats), < 2^31
    unsigned w_bytes;      // size of the packed weights, < 2^31
    unsigned y_bytes;      // size of the output buffer (rows_out * cp_out floats), < 2^31
    unsigned y_row_bytes;  // cp_out * 4
    unsigned len_bytes;    // B * 4
    unsigned bias_bytes;   // n_alloc * 4
    int rows_in;           // B * P_in
    int rows_out;          // B * P_out (pooled rows)
    int P_out;
    float inv_P_out;
    int cp_in, cp_out;
    int nch;
    int shift_out;         // valid output rows of read b: len[b] >> shift_out
    WalkArgs walk;         // tile grid, order and dead-tile flag (tile_walk.hpp)
    // FUSE0 (F(2,3), layer 1 only): the input rows are not read from x but computed on the fly from the
    // normalised signal - ConvNet layer 0 (C_in = 1: 3 FMAs per output) folded into the staging
    const float* xs;       // normalised signals, flat [B * P0] (row pitch == P0, zero beyond each read's length),
                           // preceded by >= 16 readable bytes of zeros
    unsigned xs_bytes;
    const float* w0;       // layer 0: [cp_in][4] = (w0, w1, w2, bias)
    int n_reads;
};

namespace {

// a shape-table entry: the tile and its instantiations per channel chunk 16, 20, ... (NK of them)
template <class Args, int NK_>
struct WinoShape : TileGeom {
    using KernelFn = void (*)(const Args);
    using ArgsT = Args;
    static constexpr int NK = NK_;
    KernelFn fn[NK_];      // by chunk
    KernelFn deep[NK_];    // the same tile with staging loads one item ahead (thin launches), or null
};

template <int M>
size_t wino_lds_bytes(const TileGeom& s, int kc) {
    return 2 * (size_t)wino_buf_floats(M, s.bm(), s.bn(), kc) * sizeof(float);      // two buffers
}

// Cost model of a family, in SIMD cycles.  One persistent workgroup per CU; time = rounds x (MFMA issue of a tile + per-item
// staging and barrier + per-tile epilogue).
struct WinoCost {
    // FULL launches (at least one tile per CU), eight-wave shapes; calibrated on tools/shape_sweep.py at B = 512.  Per slot:
    // the MFMAs of the two waves of a SIMD, `frag` per fragment read, `xform` per MT for the share of the input transform that
    // does not hide behind the MFMAs; per item: fixed cost, staging, `xslab` per byte of the activation slab's trip from L2 /
    // Infinity Cache (the weight slab is an L2 hit); per tile: 1500 + tile_mn per accumulator tile
    double frag, xform, xslab, tile_mn;
    // THIN launches (fewer tiles than CUs): a least-squares fit over tools/shape_sweep.py at 16 ... 512 reads, every shape.
    // Per slot the MFMAs of a SIMD's waves add up; the other instructions of a slot do not depend on the waves per SIMD;
    // staged bytes cost more the more CUs stream (fill).  thin_launch: launch + first / last tile effects of the same fit
    // (for the comparison with conv_small_f32)
    double thin_launch, thin_slot, thin_slot_mn, thin_item, thin_byte, thin_byte_fill, thin_tile, thin_tile_mn;
};

template <int M>
double wino_tile_cost(const TileGeom& s, int kc, int nch, const WinoCost& k) {
    constexpr int NC = M + 2;
    if (wino_lds_bytes<M>(s, kc) > kConvLdsBudget || s.waves() != 8) return -1.0;
    const int bu = s.bm(), bnt = s.bnt();
    const double slots = (double)NC * kc / 4.0;                 // NC components x kc / 4 k-steps
    const double staged = (((double)M * bu + 2) + (double)NC * bnt * 16) * kc * 4.0;   // bytes per item
    const double xslab = ((double)M * bu + 2) * kc * 4.0;
    const double item = slots * (2.0 * s.mt * s.nt * 32.0 + k.frag * (s.mt + s.nt) + k.xform * s.mt) + 900.0 +
                        0.06 * staged + k.xslab * xslab;
    return nch * item + 1500.0 + k.tile_mn * s.mt * s.nt;
}

// per_cu: workgroups of a four-wave shape resident on one CU (two: their waves share the SIMDs like an eight-wave workgroup's)
template <int M>
double wino_thin_tile_cost(const TileGeom& s, int kc, int nch, int per_cu, double fill, const WinoCost& k) {
    constexpr int NC = M + 2;
    if (wino_lds_bytes<M>(s, kc) * per_cu > kConvLdsBudget) return -1.0;
    const int bu = s.bm(), bnt = s.bnt();
    const double slots = (double)NC * kc / 4.0;
    const double staged = (((double)M * bu + 2) + (double)NC * bnt * 16) * kc * 4.0 * per_cu;
    const double wps = s.waves() * per_cu / 4.0;
    const double item = slots * (wps * s.mt * s.nt * 32.0 + k.thin_slot + k.thin_slot_mn * (s.mt + s.nt)) + k.thin_item +
                        staged * (k.thin_byte + k.thin_byte_fill * fill);
    return nch * item + k.thin_tile + k.thin_tile_mn * s.mt * s.nt;
}

// the family as plan_tiles sees it (tile_plan.hpp), for a layer of nch chunks of kc channels.  A forced or tuned shape need
// only fit the LDS: the four-wave entries, which no full-launch search picks, can be pinned.  unpadded (ConvPlan): whether the
// layer takes the tiles that fit on unpadded rows only; without it they are out of reach like the ones that do not fit.
template <int M, class Shape>
auto wino_family(const Shape* shapes, int n_shapes, const WinoCost& k, int kc, int nch, bool unpadded = false) {
    auto open = [=](int i) { return unpadded || !wino_unpadded(M, shapes[i].bm(), shapes[i].bn(), kc); };
    return tile_family(
        n_shapes, [=](int i) -> const TileGeom& { return shapes[i]; },
        [=](int i) { return open(i) ? wino_tile_cost<M>(shapes[i], kc, nch, k) : -1.0; },
        [=](int i, int per_cu, double fill) { return open(i) ? wino_thin_tile_cost<M>(shapes[i], kc, nch, per_cu, fill, k) : -1.0; },
        [=](int i) { return open(i) && wino_lds_bytes<M>(shapes[i], kc) <= kConvLdsBudget; });
}

// index of channel chunk kc in a shape's instantiations (16, 20, ...), or -1
template <class Shape>
int wino_chunk_index(int kc) {
    return (kc >= 16 && kc % 4 == 0 && (kc - 16) / 4 < Shape::NK) ? (kc - 16) / 4 : -1;
}

// estimate of one launch INCLUDING its launch cost where the thin-launch fit applies (*thin_out), for the choice between
// a tiled kernel and conv_small_f32 (whose fit includes its launch as well)
template <class Family>
double wino_launch_cost(const Family& f, int64_t units, int n16, int num_cu, const WinoCost& k, bool* thin_out) {
    const TileChoice c = choose_tile(f, units, n16, num_cu);
    if (thin_out) *thin_out = c.thin;
    return c.thin ? c.cost + k.thin_launch : c.cost;
}

// the F(2,3) kernel's one extra form: layer 0 folded into layer 1's staging.  It exists as ONE instantiation, so it pins the
// shape; a tuned shape behind it changes the tile walk, not the kernel
template <class Shape>
struct WinoFuse0 {
    const float* xs;       // null: not fused
    const float* w0;
    typename Shape::KernelFn fn;
    const TileGeom* geom;
};

// One layer: the buffer-window checks, the plan (head + tail launches), the argument record, the launches.
template <int M, class Shape>
int launch_wino(const char* name, const Shape* shapes, int n_shapes, const WinoCost& cost, const char* force,
                const ConvLayerDev& L, const float* d_x, float* d_y, const int32_t* d_len, int B, int P_in, int layer_index,
                int num_cu, int check_dead, hipStream_t st, int* bm_out, int* bn_out, const WinoFuse0<Shape>& fuse = {}) {
    constexpr int NC = M + 2;
    const ConvPlan& p = L.plan;
    const int ki = wino_chunk_index<Shape>(p.kc);
    if (ki < 0) {
        set_error("%s: unsupported channel chunk %d", name, p.kc);
        return RS_ERR_ARG;
    }
    const bool fused = fuse.xs != nullptr;
    const int64_t rows64 = (int64_t)B * P_in;
    const int64_t xb = fused ? rows64 * 2 * 4 : rows64 * L.cp_in * 4;      // fused: the signals, B * P0 floats (P0 = 2 * P_in)
    const int64_t wb = (int64_t)p.n_alloc * p.nch * NC * p.kc * 4, yb = rows64 / 2 * L.cp_out * 4;
    if (rows64 > 0x7fffffff || xb >= 0x80000000LL || wb >= 0x80000000LL || yb >= 0x80000000LL) {
        set_error("%s: batch too large for the 2 GiB buffer window, split it", name);
        return RS_ERR_ARG;
    }
    const int n16 = round_up(L.c_out, 16) / 16;
    const int64_t units = M == 2 ? rows64 / 2 : (rows64 + 3) / 4;
    const TilePlan plan = plan_tiles(wino_family<M>(shapes, n_shapes, cost, p.kc, p.nch, p.unpadded), units, n16, num_cu,
                                     {force, layer_index, tuned_pick(L.force_shape, L.tuned, rows64), fused ? fuse.geom : nullptr},
                                     {!L.hooks->no_tail_split, L.hooks->tail_margin > 0 ? L.hooks->tail_margin : 0.97, true});
    if (!plan.n_parts) {
        set_error("%s: no tile shape fits (kc=%d)", name, p.kc);
        return RS_ERR_ARG;
    }
    typename Shape::ArgsT a;
    a.x = d_x;
    a.w = static_cast<const float*>(L.d_w);
    a.bias = L.d_bias;
    a.y = d_y;
    a.len = d_len;
    a.x_bytes = fused ? 0u : (unsigned)xb;
    a.w_bytes = (unsigned)wb;
    a.y_bytes = (unsigned)yb;
    a.y_row_bytes = (unsigned)L.cp_out * 4u;
    a.len_bytes = (unsigned)B * 4u;
    a.bias_bytes = (unsigned)p.n_alloc * 4u;
    a.rows_in = (int)rows64;
    a.rows_out = (int)(rows64 / 2);
    a.P_out = P_in / 2;
    a.inv_P_out = 1.0f / (float)a.P_out;
    a.cp_in = L.cp_in;
    a.cp_out = L.cp_out;
    a.nch = p.nch;
    a.shift_out = layer_index + 1;
    if constexpr (M == 2) {
        a.xs = fuse.xs;
        a.xs_bytes = (unsigned)std::min<int64_t>(rows64 * 2 * 4, 0x7fffffffLL);
        a.w0 = fuse.w0;
        a.n_reads = B;
    } else {
        a.n_groups = (int)units;
    }
    // one launch over the row tiles [m_base, m_base + n_mtiles x bm) of shape sh
    auto launch_part = [&](const Shape& sh, int m_base, int n_mtiles, int wg_per_cu) -> int {
        const int BN = sh.bn();
        typename Shape::KernelFn fn = fused ? fuse.fn : sh.fn[ki];
        if (auto d = sh.deep[ki]; d && !fused && !L.hooks->no_deep_staging) fn = d;
        RS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)kConvLdsBudget));
        const int n_ntiles = (n16 * 16 + BN - 1) / BN;
        const int64_t tiles = (int64_t)n_mtiles * n_ntiles;
        const int slots_ = num_cu * wg_per_cu;
        const unsigned grid = (unsigned)std::min<int64_t>(tiles, slots_);
        a.walk = plan_walk(n_mtiles, n_ntiles, grid, slots_, (double)M * sh.bm(), (double)NC * BN, check_dead,
                           !L.hooks->no_rect_order);
        a.walk.m_base = m_base;
        hipLaunchKernelGGL(fn, dim3(grid), dim3(fused ? 512 : 64 * sh.waves()), wino_lds_bytes<M>(sh, p.kc), st, a);
        RS_HIP(hipGetLastError());
        return RS_OK;
    };
    const Shape& h = shapes[plan.part[0].shape];
    if (plan.n_parts == 2 && L.hooks->tail_debug) {
        const Shape& t = shapes[plan.part[1].shape];
        fprintf(stderr, "[tail-split] layer %d: head %dx%dx%dx%d x %d row tiles, tail %dx%dx%dx%d (%d per CU); planned %.0f vs %.0f cycles\n",
                layer_index, h.wm, h.wn, h.mt, h.nt, plan.part[0].n_mtiles, t.wm, t.wn, t.mt, t.nt, plan.part[1].per_cu, plan.cost,
                plan.single_cost);
    }
    for (int i = 0; i < plan.n_parts; ++i) {
        const TilePart& part = plan.part[i];
        const int rc = launch_part(shapes[part.shape], part.m_base, part.n_mtiles, part.per_cu);
        if (rc != RS_OK) return rc;
    }
    if (bm_out) *bm_out = M * h.bm();       // reported in conv rows, like the direct kernels; a split reports the head's shape
    if (bn_out) *bn_out = h.bn();
    return RS_OK;
}

}  // namespace
}  // namespace rs
