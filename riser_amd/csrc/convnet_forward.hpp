// One forward pass of the ConvNet on a planned batch: which kernel every layer runs (Kernel, select_kernel), the launch
// sequence, and rs_autotune's timing of a tiled layer's shapes in place.
#pragma once
#include <stdio.h>

#include <algorithm>

#include "common.hpp"
#include "convnet_model.hpp"
#include "convnet_workspace.hpp"
#include "tile_plan.hpp"

namespace rs {
namespace {

// record an event tagged `stage` (-1 opens a call) on the stream, if profiling is on
void prof_mark(rs_model* m, int stage, hipStream_t st) {
    if (!m->prof_on) return;
    // coarse level: an event costs ~4.5 us on the stream; only the boundaries of the conv stack are kept, a skipped
    // stage's time is added to the next recorded one (normalise -> stage 1, conv layers 1..n-2 -> stage n-1)
    if (m->prof_level == 2 && (stage == 0 || (stage >= 2 && stage < m->n_layers))) return;
    if (m->ev_used == m->ev_pool.size()) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        m->ev_pool.push_back(e);
        m->ev_stage.push_back(0);
    }
    m->ev_stage[m->ev_used] = stage;
    (void)hipEventRecord(m->ev_pool[m->ev_used], st);
    ++m->ev_used;
    if (stage < 0) {
        ++m->prof_calls;
        m->prof_open = true;
    }
    if (stage == m->n_layers + 1) m->prof_open = false;     // the head closes the call
}

// The kernels a conv layer i >= 1 can run
enum class Kernel {
    StreamF32,      // fp32 Winograd: layers 0 + 1 as one LDS-free streaming launch (conv_stream_f32.hip)
    SmallF32,       // fp32 Winograd on a launch of a few rows: a wave per 16 x 16 tile (conv_small_f32.hip)
    WresF32,        // fp32 Winograd, narrow layers of a full launch: weights resident in LDS, a run of steps per wave (conv_wres_f32.hip)
    Wino4,          // F(4,3) (conv_wino4.hip)
    Wino2,          // F(2,3) (conv_wino.hip), optionally with layer 0 folded into layer 1's staging
    DirectF32,      // RS_F32 (conv_f32.hip)
    StreamH16,      // 16-bit: per-wave streaming kernel of the narrow layers 1 and 2, optionally with layer 0 folded in (conv_stream_h16.hip)
    Stream012H16,   // 16-bit: layers 0 + 1 + 2 in one streaming launch; chosen at layer 1, its output takes the place of layer 2's
    ThinH16,        // split precision on a launch of a few rows (conv_thin_h16.hip)
    RingF8,         // RS_F16XF8: the layer reads and / or writes F8 rows (conv_ring_f8.hip)
    WresH16,        // narrow tiled 16-bit layers: the whole weight tensor resident in LDS (conv_wres_h16.hip)
    RingH16,        // every other tiled 16-bit layer: the LDS-DMA ring kernel (conv_ring_h16.hip)
};
// the kernels that read the ring packing d_w2 (rs_model_layer_info reports its K padding for them)
inline bool reads_ring_packing(Kernel k) {
    return k == Kernel::ThinH16 || k == Kernel::RingF8 || k == Kernel::WresH16 || k == Kernel::RingH16;
}
// the tile-shape table of a tiled kernel whose launcher consults rs_autotune's picks (tile_plan.hpp: tuned_pick): its size, and whether entry k can run layer L
struct ShapeTable {
    int (*num_shapes)();
    bool (*shape_ok)(const ConvLayerDev& L, int k);
};
inline ShapeTable shape_table(Kernel k) {
    switch (k) {
        case Kernel::Wino4: return {conv_wino4_num_shapes, conv_wino4_shape_ok};
        case Kernel::Wino2: return {conv_wino_num_shapes, conv_wino_shape_ok};
        case Kernel::RingF8: return {conv_ring_f8_num_shapes, conv_ring_f8_shape_ok};
        case Kernel::RingH16: return {conv_ring_num_shapes, conv_ring_shape_ok};
        default: return {nullptr, nullptr};
    }
}
// the kernels that rs_autotune times
inline bool tunable(Kernel k) { return shape_table(k).num_shapes != nullptr; }

// How layer 0 (one input channel) runs in this call: as its own launch, or folded into layer 1's kernel, which needs the
// signal rows in the packed layout (always true via rs_classify)
struct Fuse0 {
    bool stream_f32;    // fp32 Winograd: the streaming kernel of layers 0 + 1, which only needs 64-row blocks
    bool wino;          // ... or - RS_NO_STREAM_F32 - the tiled kernel's staging, which needs a tile to span at most two blocks
    bool h16;           // 16-bit: the streaming kernel of layer 1 ("fused preprocess + conv")
    bool any() const { return stream_f32 || wino || h16; }
};
Fuse0 fuse0_of(const rs_model* m, bool packed_x, int U0) {
    Fuse0 f{};
    f.stream_f32 = packed_x && m->dtype == RS_F32W && !m->hooks.no_fuse0 && conv_stream_f32_ok(m->layers[1], m->channels[0], U0 >> 1);
    f.wino = !f.stream_f32 && packed_x && m->dtype == RS_F32W && conv_wino_can_fuse0(m->layers[1], U0 >> 1);
    f.h16 = is_16bit(m->dtype) && packed_x && m->channels[0] <= 32 && conv_stream_h16_ok(m->layers[1], U0 >> 1);
    return f;
}

// The kernel of layer i >= 1 on a launch of NB blocks of P_in input rows.  The order of the questions is the precedence:
//   RS_F32W:  streaming 0 + 1  >  weights-resident (full launches of narrow layers)  >  small-batch  >  F(4,3) / F(2,3) by the layer's packing
//   RS_F32:   direct
//   16-bit:   streaming 0 + 1 + 2  >  streaming  >  F8 rows  >  thin (split precision)  >  weights-resident  >  ring
// (rs_autotune runs no small-batch and no thin launch: it times the tiled kernels' shapes)
Kernel select_kernel(const rs_model* m, int i, int NB, int P_in, const Fuse0& fuse0) {
    const ConvLayerDev& L = m->layers[i];
    const int64_t rows_in = (int64_t)NB * P_in;
    if (m->dtype == RS_F32) return Kernel::DirectF32;
    if (m->dtype == RS_F32W) {
        if (i == 1 && fuse0.stream_f32) return Kernel::StreamF32;
        const Kernel tiled = L.wino_m == 4 ? Kernel::Wino4 : Kernel::Wino2;
        // narrow layers whose whole weight tensor fits LDS next to a private activation image per wave (layers 2 and 3 of the
        // shipped net), on launches that give every wave slot a run of steps (RS_WRES_F32=1: whatever the launch size).  It
        // steps aside for everything that asks for the tiled or the small kernel by name: a forced small kernel, rs_autotune,
        // RS_NO_STREAM_F32 ("tiled kernels on every layer"), a forced tile shape of this layer - and for layer 1 while
        // layer 0 is folded into its staging
        if (!(i == 1 && fuse0.wino) && m->hooks.small_f32_waves <= 0 && !m->tuning && !m->hooks.no_stream_f32 && conv_wres_f32_ok(L)) {
            int wm, wn, mt, nt;
            const bool pinned = next_layer_shape(L.wino_m == 4 ? m->hooks.force_wino4 : m->hooks.force_wino, i, &wm, &wn, &mt, &nt) != nullptr;
            if (!pinned && (m->hooks.wres_f32 > 0 || conv_wres_f32_fills(L, rows_in, m->num_cu))) return Kernel::WresF32;
        }
        // fp32 Winograd layers of a launch with only a handful of rows (Model.classify at batch 1, a thin ReadUntil batch):
        // one wave per 16 x 16 tile instead of 256-row tiles that are mostly padding (conv_small_f32.hip; same bits)
        // (not layer 1 when layer 0 is folded into its staging: nothing has written that layer's input)
        if ((i == 1 && fuse0.wino) || m->tuning || m->hooks.small_f32_waves == 0 || !conv_small_f32_ok(L)) return tiled;
        if (m->hooks.small_f32_waves > 0)                           // forced limit (tests, A/B runs)
            return conv_small_f32_waves(L, rows_in) <= m->hooks.small_f32_waves ? Kernel::SmallF32 : tiled;
        // the launch planner's own estimate of the tiled kernel against the small kernel's (both in cycles, both
        // rough): take the small kernel where it is clearly ahead
        const int n16 = round_up(L.c_out, 16) / 16;
        bool thin_fit = false;                               // the tiled estimate is the thin-launch fit (with its launch cost: like the small kernel's)
        const double cost = L.wino_m == 4
            ? conv_wino4_launch_cost((rows_in + 3) / 4, n16, L.plan.kc, L.plan.nch, L.plan.unpadded, m->num_cu, &thin_fit)
            : conv_wino_launch_cost(rows_in / 2, n16, L.plan.kc, L.plan.nch, m->num_cu, &thin_fit);
        const bool small32 = conv_small_f32_waves(L, rows_in) <= 4096 &&
                             conv_small_f32_cost(L, rows_in, m->num_cu) < (thin_fit ? 1.0 : 0.8) * cost;
        if (m->hooks.tail_debug)
            fprintf(stderr, "[small-or-tiled] layer %d: rows %lld, small %.0f (%lld workgroups), tiled %.0f (%s) -> %s\n", i,
                    (long long)rows_in, conv_small_f32_cost(L, rows_in, m->num_cu), (long long)conv_small_f32_waves(L, rows_in),
                    cost, thin_fit ? "thin fit + launch" : "full-launch model", small32 ? "small" : "tiled");
        return small32 ? Kernel::SmallF32 : tiled;
    }
    // 16-bit paths: the narrow layers 1 and 2 run the per-wave streaming kernel; on the rs_classify path
    // layer 0 is folded into layer 1 there as well ("fused preprocess + conv"), or layers 0 + 1 + 2 are one streaming
    // kernel (not while a test captures the output of layer 1 or 2, which that kernel never writes)
    const bool x3 = is_x3(m->dtype);
    if (i == 1 && fuse0.h16 && m->n_layers > 2 && !(m->dbg_dst && m->dbg_layer <= 2) &&
        conv_stream012_h16_ok(L, m->layers[2], m->channels[0], P_in))
        return Kernel::Stream012H16;
    if (i <= 2 && conv_stream_h16_ok(L, P_in)) return Kernel::StreamH16;
    // every tiled 16-bit layer runs the LDS-DMA ring kernel (the register-staged kernel of round 1, conv_h16.hip, was its
    // bit-for-bit cross-check through round 3 and has been removed)
    // RS_F16XF8: the wide layers read and / or write F8 rows (cross terms on the 8-bit MFMA: conv_ring_f8.hip)
    if (L.f8_in || L.f8_out) return Kernel::RingF8;
    // split precision on a launch of a few rows (Model.classify at batch 1, a thin ReadUntil batch): 64 x 32 tiles that take a
    // WHOLE PANEL per barrier instead of the ring's (panel, tap) sub-stages, each as long as a staging round trip whatever
    // the tile holds (conv_thin_h16.hip; same bits)
    if (x3 && !m->tuning && m->hooks.thin_h16_rows != 0 && conv_thin_h16_ok(L)) {
        const bool thin16 = m->hooks.thin_h16_rows > 0
                                ? rows_in <= m->hooks.thin_h16_rows
                                : conv_thin_h16_cost(L, rows_in, m->num_cu) < conv_ring_plan_cost(L, rows_in, m->num_cu, x3);
        if (m->hooks.tail_debug)
            fprintf(stderr, "[thin-or-ring] layer %d: rows %lld, thin %.0f (%lld tiles), ring %.0f -> %s\n", i, (long long)rows_in,
                    conv_thin_h16_cost(L, rows_in, m->num_cu), (long long)conv_thin_h16_tiles(L, rows_in),
                    conv_ring_plan_cost(L, rows_in, m->num_cu, x3), thin16 ? "thin" : "ring");
        if (thin16) return Kernel::ThinH16;
    }
    // ... and narrow layers whose whole weight tensor fits LDS next to two activation slabs on the weights-resident kernel
    return conv_wres_h16_ok(L, x3) ? Kernel::WresH16 : Kernel::RingH16;
}

// rs_autotune: every feasible entry of the kernel's shape table on THIS layer's real input (the buffers hold the
// activations of the batch; re-running a layer rewrites the same output), 1 warm + 3 timed launches each;
// a shape replaces the planner's choice for launches of `rows` GEMM rows only if it is > 3 % faster
template <class Launch>
int autotune_layer(rs_model* m, ConvLayerDev& L, Kernel kernel, int64_t rows, hipStream_t st, Launch launch_layer) {
    const ShapeTable table = shape_table(kernel);
    const int n = table.num_shapes();
    auto ok = [&](int k) { return table.shape_ok(L, k); };
    hipEvent_t e0, e1;
    RS_HIP(hipEventCreate(&e0));
    RS_HIP(hipEventCreate(&e1));
    auto timed = [&](int k, float* ms) -> int {
        L.force_shape = k;
        int r = launch_layer();
        if (r == RS_OK) r = hipEventRecord(e0, st) == hipSuccess ? RS_OK : RS_ERR_HIP;
        for (int rep = 0; rep < 3 && r == RS_OK; ++rep) r = launch_layer();
        if (r == RS_OK) r = hipEventRecord(e1, st) == hipSuccess && hipEventSynchronize(e1) == hipSuccess ? RS_OK : RS_ERR_HIP;
        if (r == RS_OK) r = hipEventElapsedTime(ms, e0, e1) == hipSuccess ? RS_OK : RS_ERR_HIP;
        L.force_shape = -1;
        return r;
    };
    for (size_t t = 0; t < L.tuned.size(); ++t)                       // re-tuning a geometry: forget the old entry
        if (L.tuned[t].first == rows) L.tuned.erase(L.tuned.begin() + t--);
    float base_ms = 0.f, best_ms = 1e30f;
    int best_k = -1;
    int rc = timed(-1, &base_ms);                                      // the planner's own choice
    for (int k = 0; k < n && rc == RS_OK; ++k) {
        if (!ok(k)) continue;
        float ms = 0.f;
        rc = timed(k, &ms);
        if (rc == RS_OK && ms < best_ms) {
            best_ms = ms;
            best_k = k;
        }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc != RS_OK) return rc;
    if (best_k >= 0 && best_ms < 0.97f * base_ms) {
        L.tuned.emplace_back(rows, best_k);
        ++m->tuned_changed;
    }
    return RS_OK;
}

// The conv stack + head on a planned batch.  packed_x: d_x is the workspace's own normalised-signal region in the packed
// block layout behind 16 zero bytes (rs_classify); otherwise rows of ldx floats, one per read (rs_forward).
int forward_impl(rs_model* m, const float* d_x, int64_t ldx, const int32_t* d_len, int B, const Batch& bt, const WsLayout& w,
                 void* d_ws, float* d_probs, float* d_logits, void* stream, bool packed_x) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(d_ws);
    void* buf[2] = {ws + w.bufa_off, ws + w.bufb_off};
    // from here on the kernels see NB blocks of U samples as NB reads in slots of U (common.hpp: BlockPlan)
    // the layout a conv layer reads: fine blocks below the split, coarse ones from it on (one level: the same table)
    const bool two = two_level(m);
    const Fuse0 fuse0 = fuse0_of(m, packed_x, w.Uf);              // w.Uf: block size of the normalised rows and of layers 0, 1
    const bool x3 = is_x3(m->dtype);
    const bool f16 = is_f16_family(m->dtype);
    int rc = RS_OK;
    // unfused layer 0: ldx < 0 tells the kernel that read b's samples start at block rbase[b] of d_x
    if (!fuse0.any())
        rc = launch_conv0(d_x, packed_x ? -1 : ldx, d_len, bt.fine, bt.NBf, m->d_w0, m->cp[0], buf[0], act_dtype(m), st, m->d_sat);
    if (rc != RS_OK) return rc;
    prof_mark(m, 1, st);
    int cur = 0;
    for (int i = 1; i < m->n_layers; ++i) {
        ConvLayerDev& L = m->layers[i];
        // layer split - 1 wrote its rows on fine blocks; the late layers read coarse ones: a re-pack of that (small) buffer -
        // per read, its rows in order, zero rows up to the end of its coarse blocks - into the other buffer.  Not needed when
        // every read fills its coarse blocks with fine ones (16000, 12000, 8000 samples: 16 / 12 / 8 blocks of 1024 = 4 / 3 / 2
        // of 4096): then the two layouts put every row in the same place.
        if (two && i == m->split && (int64_t)bt.NBf * w.Uf != (int64_t)bt.NB * w.U) {
            const size_t row_bytes = (size_t)m->cp[i - 1] * esize(m);
            rc = launch_repack_rows(buf[cur], buf[cur ^ 1], bt.fine, bt.plan, bt.NB, w.Uf >> i, w.U >> i, row_bytes, st);
            if (rc != RS_OK) return rc;
            if (L.f8_in) {                                            // F8 rows: their scale plane moves with them
                const int64_t rows_f = (int64_t)bt.NBf * (w.Uf >> i), rows_c = (int64_t)bt.NB * (w.U >> i);
                rc = launch_repack_scales(static_cast<const char*>(buf[cur]) + f8_scale_offset(rows_f, L.cp_in),
                                          static_cast<char*>(buf[cur ^ 1]) + f8_scale_offset(rows_c, L.cp_in), bt.fine, bt.plan, bt.NB,
                                          w.Uf >> i, w.U >> i, L.cp_in / 128, f8_scale_stride(rows_f), f8_scale_stride(rows_c), st);
                if (rc != RS_OK) return rc;
            }
            cur ^= 1;
        }
        const bool fine = two && i < m->split;
        const int U = fine ? w.Uf : w.U;
        const int NB_all = fine ? bt.NBf : bt.NB;
        const int32_t* d_blen = fine ? bt.fine.blen : bt.plan.blen;
        const int Lmin = fine ? bt.Lmin_blk_f : bt.Lmin_blk;
        const int P_in = U >> i;
        // RS_EMU_ROWS (timing experiments only, results WRONG): run this layer on a share of the blocks, to price a layout
        // with fewer rows before building it (compact rows)
        int NB = NB_all, pm;
        for (const char* q = m->hooks.emu_rows; (q = next_layer_value(q, i, &pm));) NB = std::max(1, (int)((int64_t)NB_all * pm / 1000));
        // a tile of >= 64 rows can only be all padding if some block leaves >= 64 rows unused at this layer;
        // Lmin == 0 means "unknown": keep the test
        const int check_dead = (Lmin <= 0 || (U >> i) - (Lmin >> i) >= 64) ? 1 : 0;
        const Kernel kernel = select_kernel(m, i, NB, P_in, fuse0);
        const void* x = buf[cur];
        void* y = buf[cur ^ 1];
        int* bm = &m->last_bm[i];
        int* bn = &m->last_bn[i];
        auto launch_layer = [&]() -> int {
            switch (kernel) {
            case Kernel::StreamF32:
                *bm = 32;
                *bn = round_up(L.c_out, 16);
                return launch_conv_stream_f32(L, d_x, m->d_w0, m->channels[0], static_cast<float*>(y), d_blen, NB, P_in, m->num_cu, st);
            case Kernel::SmallF32:
                return launch_conv_small_f32(L, static_cast<const float*>(x), static_cast<float*>(y), d_blen, NB, P_in, i, m->num_cu,
                                             st, bm, bn);
            case Kernel::WresF32:
                return launch_conv_wres_f32(L, static_cast<const float*>(x), static_cast<float*>(y), d_blen, NB, P_in, i, m->num_cu, st,
                                            bm, bn);
            case Kernel::Wino4:
                return launch_conv_wino4(L, static_cast<const float*>(x), static_cast<float*>(y), d_blen, NB, P_in, i, m->num_cu,
                                         check_dead, st, bm, bn);
            case Kernel::Wino2:
                return launch_conv_wino(L, static_cast<const float*>(x), static_cast<float*>(y), d_blen, NB, P_in, i, m->num_cu,
                                        m->d_zero, check_dead, st, bm, bn, (fuse0.wino && i == 1) ? d_x : nullptr, m->d_w0);
            case Kernel::DirectF32:
                return launch_conv_f32(L, static_cast<const float*>(x), static_cast<float*>(y), d_blen, NB, P_in, i, m->num_cu,
                                       m->d_zero, check_dead, st, bm, bn);
            case Kernel::StreamH16:
                *bm = 16;
                *bn = round_up(L.c_out, 16);
                return launch_conv_stream_h16(L, x, y, d_blen, NB, P_in, i, m->num_cu, f16, st, (fuse0.h16 && i == 1) ? d_x : nullptr,
                                              m->d_w0, m->channels[0], x3);
            case Kernel::Stream012H16:                                  // writes layer 2's output where layer 1 would read its input
                return launch_conv_stream012_h16(L, m->layers[2], d_x, m->d_w0, m->channels[0], buf[cur], d_blen, NB, P_in, m->num_cu,
                                                 f16, x3, st);
            case Kernel::ThinH16:
                return launch_conv_thin_h16(L, x, y, d_blen, NB, P_in, i, m->num_cu, f16, st, bm, bn);
            case Kernel::RingF8:
                return launch_conv_ring_f8(L, x, y, d_blen, NB, P_in, i, m->num_cu, check_dead, st, bm, bn);
            case Kernel::WresH16:
                return launch_conv_wres_h16(L, x, y, d_blen, NB, P_in, i, m->num_cu, f16, x3, check_dead, st, bm, bn);
            case Kernel::RingH16:
                return launch_conv_ring_h16(L, x, y, d_blen, NB, P_in, i, m->num_cu, f16, x3, check_dead, st, bm, bn);
            default:
                set_error("no kernel for layer %d in this mode", i);
                return RS_ERR_ARG;
            }
        };
        if (kernel == Kernel::Stream012H16) {
            rc = launch_layer();
            if (rc != RS_OK) return rc;
            for (int k = 1; k <= 2; ++k) {
                m->last_ring[k] = false;
                m->last_bm[k] = 16;
                m->last_bn[k] = round_up(m->layers[k].c_out, 16);
                prof_mark(m, 1 + k, st);
            }
            i = 2;
            continue;
        }
        m->last_ring[i] = reads_ring_packing(kernel);
        if (m->tuning && tunable(kernel)) {
            rc = autotune_layer(m, L, kernel, (int64_t)NB * P_in, st, launch_layer);
            if (rc != RS_OK) return rc;
        }
        rc = launch_layer();
        if (rc != RS_OK) return rc;
        prof_mark(m, 1 + i, st);
        if (m->dbg_dst && m->dbg_layer == i) {
            const int64_t rows_out = (int64_t)NB * (P_in / 2);          // F8 rows: with the scale plane behind them
            const size_t all = L.f8_out ? f8_scale_offset(rows_out, L.cp_out) + f8_scale_bytes(rows_out, L.cp_out)
                                        : (size_t)rows_out * L.cp_out * esize(m);
            const size_t nb = std::min(m->dbg_bytes, all);
            RS_HIP(hipMemcpyAsync(m->dbg_dst, buf[cur ^ 1], nb, hipMemcpyDeviceToDevice, st));
        }
        cur ^= 1;
    }
    if (m->fc.H)
        rc = launch_fc_head(static_cast<const float*>(buf[cur]), m->cp[m->n_layers - 1], w.U >> m->n_layers, m->n_layers, d_len,
                            B, bt.plan, m->fc, reinterpret_cast<float*>(static_cast<char*>(d_ws) + w.fc_part_off), d_probs,
                            d_logits, st);
    else
        rc = launch_head(buf[cur], act_dtype(m), m->cp[m->n_layers - 1], m->channels[m->n_layers - 1],
                         w.U >> m->n_layers, m->n_layers, d_len, B, bt.plan, two ? &bt.fine : nullptr, m->d_fcw, m->d_fcb,
                         d_probs, d_logits, st);
    if (rc == RS_OK) prof_mark(m, m->n_layers + 1, st);
    return rc;
}

// normalise + block plan of one batch into the workspace (the first launch of rs_classify / rs_classify_ensemble)
int normalise_packed(rs_model* m, const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B, int Lmax,
                     const WsLayout& w, const Batch& bt, void* d_ws, hipStream_t st) {
    float* xn = reinterpret_cast<float*>(static_cast<char*>(d_ws) + w.xnorm_off);
    return launch_normalise(d_sig, d_off, d_len, B, Lmax, xn, 0, 0, nullptr, 0, nullptr, st, /*zero_prefix=*/1, &bt.fine,
                            two_level(m) ? &bt.plan : nullptr);
}

}  // namespace
}  // namespace rs
