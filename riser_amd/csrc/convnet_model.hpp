// The ConvNet model behind the C ABI: what an rs_model holds and owns, the static part of every layer's plan (the K chunking,
// which fixes the weight packing), and its construction from the host weights.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "convnet_pack.hpp"
#include "devbuf.hpp"

struct rs_model {
    // test hook (rs_debug_capture_layer): copy the output buffer of conv layer dbg_layer to dbg_dst
    void* dbg_dst = nullptr;
    size_t dbg_bytes = 0;
    int dbg_layer = -1;
    rs::Hooks hooks;                      // RS_* switches, read once in rs_model_create
    int device = 0;
    int dtype = RS_F32;
    int n_layers = 0;
    int pad_shift = 0;                    // log2 of the block size of the (late layers') packed layout (>= n_layers)
    // two-level packed layout: conv layers 0 .. split - 1 run on FINE blocks of 1 << fine_shift samples, a
    // re-pack of layer split - 1's (small) output moves the batch to the blocks of 1 << pad_shift samples the late layers and
    // the head need.  split == n_layers / fine_shift == pad_shift: one level.
    int fine_shift = 0;
    int split = 0;
    int n_classes = 2;
    int channels[rs::kMaxLayers] = {0};
    int cp[rs::kMaxLayers] = {0};         // padded row width of layer i's OUTPUT buffer
    // Every device allocation of the model has its owner here and goes with the model; ConvLayerDev and FcHead, which
    // the launchers read, point into them.
    rs::DevBuf<float> d_w0;               // layer 0: [cp[0]][4] = (w0, w1, w2, bias)
    struct LayerBufs {
        rs::DevBuf<float> w32, bias;      // d_w of the fp32 modes, d_bias
        rs::DevBuf<unsigned short> w16, ring;   // d_w and d_w2 of the 16-bit modes
    } own[rs::kMaxLayers];
    rs::ConvLayerDev layers[rs::kMaxLayers];   // i >= 1
    rs::DevBuf<float> d_fcw;              // [2][c_last]
    rs::DevBuf<float> d_fcb;
    rs::FcHead fc;                        // fc.H > 0: the `fc` classifier replaces the gap_fc head (rs_model_set_fc_classifier)
    rs::DevBuf<float> fc_w1p, fc_b1, fc_w2, fc_b2;
    rs::DevBuf<float> d_zero;             // 256 zero bytes: target of masked-off staging loads
    rs::DevBuf<unsigned> d_sat;           // half-precision modes: sticky word, non-zero once an activation overflowed f16 (rs_model_saturated)
    rs::PinnedWord h_sat;                 // ... and the pinned host word rs_model_saturated's kernel stores the flag's value into
    int num_cu = 256;
    int last_bm[rs::kMaxLayers] = {0};
    int last_bn[rs::kMaxLayers] = {0};
    bool last_ring[rs::kMaxLayers] = {false};  // the layer's last launch read the ring packing (convnet_forward.hpp: reads_ring_packing)
    // stage profiling (rs_profile_*): events recorded on the launch stream
    bool prof_on = false;
    bool prof_open = false;      // a profiled call has recorded its opening event (rs_classify opens before normalise)
    int prof_level = 1;          // 1: one event per launch; 2: call start, end of normalise + layer 0, end of the conv stack, head
    std::vector<hipEvent_t> ev_pool;
    std::vector<int> ev_stage;            // stage of event k (-1 = start of a call)
    size_t ev_used = 0;
    int prof_calls = 0;
    bool tuning = false;                  // rs_autotune: time every feasible tile shape of each tiled layer in place
    int tuned_changed = 0;                // layers whose measured best differs from the planner's choice
    // rs_classify_ensemble: the forwards of models 1.. run on library-owned side streams next to model 0's on the
    // caller's stream (created on first use)
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};

namespace rs {
namespace {

// storage type of the activations: the Winograd fp32 path shares every non-conv kernel with RS_F32
// (RS_F16XF8 is RS_F16X3 everywhere but in the wide layers' conv kernel and their rows)
int act_dtype(const rs_model* m) { return m->dtype == RS_F32W ? RS_F32 : m->dtype == RS_F16XF8 ? RS_F16X3 : m->dtype; }
int esize(const rs_model* m) { return act_dtype(m) == RS_F32 ? 4 : 2; }

inline bool two_level(const rs_model* m) { return m->split < m->n_layers && m->fine_shift < m->pad_shift; }
// block size (log2) of the layout conv layer i READS (i = 0: the normalised signal); its output is in the same layout, except
// that layer split - 1's output is re-packed to the coarse layout before layer `split` reads it
inline int layer_shift(const rs_model* m, int i) { return (two_level(m) && i < m->split) ? m->fine_shift : m->pad_shift; }

// ---- static part of the plan: the K chunking (fixes the weight packing) -------------------------
// kc minimises nch * (3*kc/4 + 0.75) k-steps (0.75 step ~ the per-item barrier + LDS write);
// the tile shape is chosen per launch from the batch's row count (conv_f32.hip).
ConvPlan plan_static_f32(int cp_in, int c_out) {
    ConvPlan p{};
    double best_cost = -1;
    for (int kc = 4; kc <= conv_f32_kc_max(); kc += 4) {
        // chunks of 16 / 20 / 24 channels have fully unrolled kernels (immediate LDS offsets);
        // other sizes run the generic kernel and are only worth it for very narrow layers
        if (cp_in >= 16 && kc != 16 && kc != 20 && kc != 24) continue;
        const int nch = (cp_in + kc - 1) / kc;
        const double cost = nch * (3.0 * kc / 4.0 + 0.75);
        if (best_cost < 0 || cost < best_cost - 1e-9 || (cost < best_cost + 1e-9 && kc > p.kc)) {
            best_cost = cost;
            p.kc = kc;
            p.nch = nch;
        }
    }
    p.n_alloc = round_up(c_out, 16) + conv_f32_max_bn();
    return p;
}

// Winograd F(2,3): a chunk of kc channels is 4 * kc / 4 = kc MFMA slots; ~1.5 slots per item for
// the barrier and the staging writes
ConvPlan plan_static_wino(int cp_in, int c_out) {
    ConvPlan p{};
    double best_cost = -1;
    for (int kc = 16; kc <= 24; kc += 4) {
        const int nch = (cp_in + kc - 1) / kc;
        const double cost = nch * (kc + 1.5);
        if (best_cost < 0 || cost < best_cost - 1e-9) {
            best_cost = cost;
            p.kc = kc;
            p.nch = nch;
        }
    }
    p.n_alloc = round_up(c_out, 16) + conv_wino_max_bn();
    return p;
}

// F(4,3): chunks of 16 or 20 channels (LDS capacity); 6 * kc / 4 slots per chunk
// The chunk (16 or 20 channels; LDS capacity) fixes the weight packing, but also which tile shapes fit in LDS
// (96-channel-wide tiles need chunks of 16), so it is chosen with the launch planner's own cost estimate at a
// nominal batch (512 reads of 16000 samples, BASELINE config 2).
// Chunks of 20 come with the tiles that fit the LDS on unpadded rows only (512 x 80; ConvPlan::unpadded), which is what makes
// them the cheaper chunk for 80-column layers.
// tuning aid: RS_PLAN_KC = "layer:kc;layer:kc" forces the channel chunk of a layer when the model is created.  "layer:20" means
// what it always has, the tiles at the row pitch of kc + 2 (the set tools/shape_sweep.py and the shape sweep of the tests walk,
// by that footprint); "layer:20u" is the chunk as the planner takes it, unpadded tiles included.
ConvPlan plan_static_wino4(const Hooks& h, int cp_in, int c_out, int layer, int num_cu) {
    ConvPlan p{};
    double best_cost = -1;
    const int64_t groups = (int64_t)512 * (16384 >> layer) / 4;
    int forced_kc = 0;
    bool forced_unpadded = false;
    if (const char* end = next_layer_value(h.plan_kc, layer, &forced_kc)) {  // the layer's first entry, if it has one
        const char* q = end;                                                 // its last character: before the ';' or the end
        while (q > h.plan_kc && (q[-1] == ';' || q[-1] == ' ')) --q;
        forced_unpadded = q > h.plan_kc && q[-1] == 'u';
    }
    for (int kc = 16; kc <= 20; kc += 4) {
        if (forced_kc && kc != forced_kc) continue;
        const bool unpadded = kc == 20 && (!forced_kc || forced_unpadded);
        const int nch = (cp_in + kc - 1) / kc;
        const double cost = conv_wino4_plan_cost(groups, round_up(c_out, 16) / 16, kc, nch, unpadded, num_cu);
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            p.kc = kc;
            p.nch = nch;
            p.unpadded = unpadded;
        }
    }
    p.n_alloc = round_up(c_out, 16) + conv_wino4_max_bn();
    return p;
}

// measurement aid (libraries built with -DRS_X3_MASK only): RS_X3_TERMS = "layer:mask;layer:mask" picks the products a
// split-precision layer of the ring kernel executes (1 = hi*hi, 2 = x lo * w hi, 4 = x hi * w lo; 7 = all, the shipped mode)
int x3_terms_of(const Hooks& h, int layer) {
    int t;
    return next_layer_value(h.x3_terms, layer, &t) ? (t & 7) | 1 : 7;
}

// which layers of an RS_F32W model run F(4,3) instead of F(2,3): by default the wide ones (>= 96 input
// channels: layers 5-11 of the shipped net, where the matrix pipe is the bound: measured -8 % on layer 5,
// -12 ... -20 % on layers 6-10, -5 % on layer 11; +15 % on layer 4, whose tiles are dominated by staging and
// epilogue), plus narrower layers whose output channels fill the 80-wide F(4,3) tile exactly (16 * 5 | padded
// C_out: layer 3 of the shipped net, 45 -> 67 channels, measured -8 %).  RS_WINO4 = comma list of layer indices
// overrides it when the model is created ("none" = F(2,3) everywhere).
bool use_wino4(const Hooks& h, int layer, int n_layers, int c_in, int c_out) {
    if (h.wino4_set) {
        for (const char* q = h.wino4; *q;) {
            char* end = nullptr;
            const long v = strtol(q, &end, 10);
            if (end == q) break;
            if (v == layer) return true;
            q = *end ? end + 1 : end;
        }
        return false;
    }
    // F(4,3) groups four input rows: every read must start on a group boundary in such a layer (see pad_shift in
    // model_build), i.e. blocks of 2^(layer + 2) samples.  The last layer would double the block size of the packed
    // layout (2^13 samples for the 12-layer net: an 8615-sample read would occupy 16384) for ~5 % of that layer's time,
    // so it stays on F(2,3) unless RS_WINO4 names it.
    if (layer + 2 > n_layers) return false;
    return c_in >= 96 || (c_in >= 32 && (round_up(c_out, 16) / 16) % 5 == 0);
}

// upload into a buffer the model owns; a failure is reported in the words it has always had
template <class T>
int upload_owned(DevBuf<T>& d, const std::vector<T>& h) {
    const hipError_t e = upload(d, h);
    if (e == hipSuccess) return RS_OK;
    return hip_fail(e, d.p ? "hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)"
                           : "hipMalloc(reinterpret_cast<void**>(dptr), std::max<size_t>(h.size(), 1) * sizeof(T))");
}

// Layer i >= 1: the static plan of the mode's kernel, the weights packed for it, the bias table
int layer_build(rs_model* m, int i, const float* w, const float* b) {
    ConvLayerDev& L = m->layers[i];
    rs_model::LayerBufs& own = m->own[i];
    const int dtype = m->dtype;
    int rc = RS_OK;
    if (dtype == RS_F32) {
        L.plan = plan_static_f32(L.cp_in, L.c_out);
        rc = upload_owned(own.w32, pack_conv3(ChunkedF32<3>{L.plan}, w, L.c_out, L.c_in));
    } else if (dtype == RS_F32W && use_wino4(m->hooks, i, m->n_layers, L.c_in, L.c_out)) {
        L.wino_m = 4;
        L.plan = plan_static_wino4(m->hooks, L.cp_in, L.c_out, i, m->num_cu);
        rc = upload_owned(own.w32, pack_conv3(ChunkedF32<6>{L.plan}, w, L.c_out, L.c_in));
    } else if (dtype == RS_F32W) {
        L.plan = plan_static_wino(L.cp_in, L.c_out);
        rc = upload_owned(own.w32, pack_conv3(ChunkedF32<4>{L.plan}, w, L.c_out, L.c_in));
    } else {
        const bool x3 = is_x3(dtype);
        const float ws = weight_scale(w, (size_t)L.c_out * L.c_in * 3, dtype);
        L.w_unscale = 1.0f / ws;
        plan_h16(L, x3, m->hooks.x3_tail);
        const Panels16 ring{L.ring_panels, L.plan.n_alloc, 64, ws, base16(dtype)};
        if (!x3) {
            Panels16 narrow = ring;                                   // conv_stream_h16.hip: layers 1-2
            narrow.panels = L.plan.nch;
            narrow.width = 32;
            rc = upload_owned(own.w16, pack_conv3(PlainLayout{narrow}, w, L.c_out, L.c_in));
        }
        if (rc != RS_OK) return rc;
        rc = upload_owned(own.ring, L.f8_in ? pack_conv3(F8Layout{ring}, w, L.c_out, L.c_in)
                                    : x3    ? pack_conv3(SplitLayout{ring, L.ring_tail}, w, L.c_out, L.c_in)
                                            : pack_conv3(PlainLayout{ring}, w, L.c_out, L.c_in));
    }
    L.d_w = own.w32 ? static_cast<void*>(own.w32.p) : own.w16.p;
    L.d_w2 = own.ring;
    if (rc != RS_OK) return rc;
    std::vector<float> bp((size_t)L.plan.n_alloc, 0.0f);
    for (int n = 0; n < L.c_out; ++n) bp[n] = b[n];
    rc = upload_owned(own.bias, bp);
    L.d_bias = own.bias;
    return rc;
}

// rs_model_create behind its argument checks, on the model's device.  A model that fails half-way frees what it holds when
// the caller deletes it.
int model_build(rs_model* m, int n_layers, const int32_t* channels, const float* const* conv_w, const float* const* conv_b,
                const float* fc_w, const float* fc_b, int dtype, int device) {
    m->device = device;
    m->hooks = Hooks::from_env();
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
            m->num_cu = cus;
    }
    m->dtype = dtype;
    m->n_layers = n_layers;
    bool f8[kMaxLayers + 1];
    f8_layers(m->hooks, dtype, n_layers, channels, f8);
    for (int i = 0; i < n_layers; ++i) {
        m->channels[i] = channels[i];
        m->cp[i] = row_pitch(dtype, channels[i], f8[i] && f8[i + 1]);
    }
    int rc = RS_OK;
    if (is_f16_family(dtype)) {
        rc = upload_owned(m->d_sat, std::vector<unsigned>(1, 0u));
        if (rc == RS_OK) {
            const hipError_t e = m->h_sat.alloc();
            if (e != hipSuccess) rc = hip_fail(e, "hipHostMalloc(&h_sat, sizeof(unsigned))");
        }
    }
    if (rc == RS_OK) rc = upload_owned(m->d_w0, pack_layer0(m->cp[0], channels[0], conv_w[0], conv_b[0]));
    for (int i = 1; i < n_layers && rc == RS_OK; ++i) {
        ConvLayerDev& L = m->layers[i];
        L.hooks = &m->hooks;
        L.d_sat = m->d_sat;
        L.c_in = channels[i - 1];
        L.c_out = channels[i];
        L.cp_in = m->cp[i - 1];
        L.cp_out = m->cp[i];
        L.x3_terms = x3_terms_of(m->hooks, i);
        L.f8_in = f8[i] && f8[i - 1];
        L.f8_out = f8[i] && f8[i + 1];
        rc = layer_build(m, i, conv_w[i], conv_b[i]);
    }
    // every read's slot must start on a Winograd group boundary in every F(4,3) layer (P0 >> i divisible by 4):
    // then the grouping of a read's rows - and with it every rounding - is the same wherever the read sits in a
    // batch and whatever the batch's longest read is (results are bit-identical across batch compositions)
    // ... and the packed layout's block is never smaller than 4096 samples (shallow nets: several rows of the last
    // buffer per block), so a read spans a handful of blocks whatever the depth
    m->pad_shift = std::max(n_layers, 12);
    for (int i = 1; i < n_layers; ++i)
        if (m->layers[i].wino_m == 4) m->pad_shift = std::max(m->pad_shift, i + 2);
    // Two-level layout: the last three layers (and the head) need the coarse blocks - their launches are one round of
    // tiles at a ReadUntil batch whatever the row count - everything before them runs on blocks a quarter the size (1024
    // samples for the shipped net: a live 8615-sample read occupies 9216 samples of rows there instead of 12288).  The
    // fine block must give layer split - 1 a whole output row per block, every F(4,3) layer below the split its group
    // alignment, and the streaming kernels of layers 0-2 their 32-row steps.
    m->split = n_layers;
    m->fine_shift = m->pad_shift;
    if (!m->hooks.one_level && n_layers >= 6) {
        const int split = n_layers - 3;
        int fs = std::max(split + 1, 8);
        for (int i = 1; i < split; ++i)
            if (m->layers[i].wino_m == 4) fs = std::max(fs, i + 2);
        if (fs < m->pad_shift) {
            m->split = split;
            m->fine_shift = fs;
        }
    }
    if (rc == RS_OK) rc = upload_owned(m->d_zero, std::vector<float>(64, 0.0f));
    if (rc == RS_OK) rc = upload_owned(m->d_fcw, std::vector<float>(fc_w, fc_w + 2 * (size_t)channels[n_layers - 1]));
    if (rc == RS_OK) rc = upload_owned(m->d_fcb, std::vector<float>(fc_b, fc_b + 2));
    return rc;
}

}  // namespace
}  // namespace rs
