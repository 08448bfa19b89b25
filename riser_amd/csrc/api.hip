// C ABI of libriser_amd (see include/riser_amd.h): the error text, the RS_* switches and the entry points with their argument
// checks.  What they call: convnet_pack.hpp (weight layouts and the packer), convnet_model.hpp (rs_model, static plans,
// construction), convnet_workspace.hpp (workspace layout, the batch of a call), convnet_forward.hpp (kernel selection, the launch
// sequence of one forward pass, autotune).
#include "common.hpp"
#include "convnet_forward.hpp"
#include "convnet_model.hpp"
#include "convnet_workspace.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

namespace rs {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
    set_error("HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
    return RS_ERR_HIP;
}

Hooks Hooks::from_env() {
    Hooks h;
    auto flag = [](const char* n) { return getenv(n) != nullptr; };
    auto text = [](const char* n, char* dst, size_t cap) {
        if (const char* e = getenv(n)) {
            strncpy(dst, e, cap - 1);
            dst[cap - 1] = 0;
        }
    };
    h.no_rect_order = flag("RS_NO_RECT_ORDER");
    h.no_tail_split = flag("RS_NO_TAIL_SPLIT");
    h.tail_debug = flag("RS_TAIL_DEBUG");
    if (const char* e = getenv("RS_TAIL_MARGIN")) h.tail_margin = atof(e);
    h.no_deep_staging = flag("RS_NO_DEEP_STAGING");
    if (const char* e = getenv("RS_SMALL_SHARED")) h.small_shared = atoi(e);
    if (const char* e = getenv("RS_SMALL_NW")) h.small_nw = atoi(e);
    if (const char* e = getenv("RS_SF32_MIN_RUN")) h.sf32_min_run = atoi(e) > 0 ? atoi(e) : 1;
    h.ring_tail_split = flag("RS_RING_TAIL_SPLIT");
    h.no_fuse0 = flag("RS_NO_FUSE0");
    h.no_stream_f32 = flag("RS_NO_STREAM_F32");
    h.no_stream_h16 = flag("RS_NO_STREAM_H16");
    h.no_stream012 = flag("RS_NO_STREAM012");
    h.ensemble_serial = flag("RS_ENSEMBLE_SERIAL");
    h.one_level = flag("RS_ONE_LEVEL");
    h.conv_stamps = flag("RS_CONV_STAMPS");
    text("RS_FORCE_SHAPE_F32", h.force_f32, sizeof(h.force_f32));
    text("RS_FORCE_SHAPE_WINO", h.force_wino, sizeof(h.force_wino));
    text("RS_FORCE_SHAPE_WINO4", h.force_wino4, sizeof(h.force_wino4));
    text("RS_FORCE_SHAPE_RING", h.force_ring, sizeof(h.force_ring));
    text("RS_EMU_ROWS", h.emu_rows, sizeof(h.emu_rows));
    if (const char* e = getenv("RS_SMALL_F32_WAVES")) h.small_f32_waves = atoi(e);
    if (const char* e = getenv("RS_H16_WRES")) h.h16_wres = atoi(e) != 0;
    if (const char* e = getenv("RS_WRES_F32")) h.wres_f32 = atoi(e) != 0;
    if (const char* e = getenv("RS_THIN_H16_ROWS")) h.thin_h16_rows = atoi(e);
    if (const char* e = getenv("RS_F8_MIN_CIN")) h.f8_min_cin = atoi(e);
    if (const char* e = getenv("RS_X3_TAIL")) h.x3_tail = atoi(e) != 0;
    text("RS_PLAN_KC", h.plan_kc, sizeof(h.plan_kc));
    text("RS_X3_TERMS", h.x3_terms, sizeof(h.x3_terms));
    h.wino4_set = flag("RS_WINO4");
    text("RS_WINO4", h.wino4, sizeof(h.wino4));
    return h;
}

const Hooks& default_hooks() {
    static const Hooks h;
    return h;
}

namespace {
// rs_model_saturated: one thread moves the model's sticky overflow word to a pinned host word; with `reset` the read and the
// clear are one atomic exchange, so nothing raised between them can be lost
__global__ void read_flag_kernel(unsigned* __restrict__ flag, unsigned* __restrict__ host_word, int reset) {
    const unsigned old = reset ? atomicExch(flag, 0u) : __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(host_word, old, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
}  // namespace

}  // namespace rs

using namespace rs;

extern "C" {

const char* rs_last_error(void) { return g_err; }

int rs_version(void) { return (2 << 16) | 9; }

int rs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rs_model_create(int n_layers, const int32_t* channels, int n_classes, const float* const* conv_w,
                    const float* const* conv_b, const float* fc_w, const float* fc_b, int dtype, int device,
                    rs_model** out) {
    if (!out || !channels || !conv_w || !conv_b || !fc_w || !fc_b) {
        set_error("rs_model_create: null argument");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    if (n_layers < 2 || n_layers > kMaxLayers) {
        set_error("rs_model_create: n_layers %d outside [2, %d]", n_layers, kMaxLayers);
        return RS_ERR_ARG;
    }
    if (n_classes != 2) {
        set_error("rs_model_create: n_classes must be 2 (got %d)", n_classes);
        return RS_ERR_ARG;
    }
    if (dtype != RS_F32 && dtype != RS_BF16 && dtype != RS_F16 && dtype != RS_F32W && !is_x3(dtype)) {      // is_x3: RS_F16XF8 too
        set_error("rs_model_create: unknown dtype %d", dtype);
        return RS_ERR_ARG;
    }
    for (int i = 0; i < n_layers; ++i)
        if (channels[i] < 1 || !conv_w[i] || !conv_b[i]) {
            set_error("rs_model_create: bad layer %d", i);
            return RS_ERR_ARG;
        }
    DeviceGuard guard(device);            // the caller's current device is restored on return
    RS_HIP(guard.err);
    rs_model* m = new (std::nothrow) rs_model();
    if (!m) {
        set_error("rs_model_create: out of host memory");
        return RS_ERR_OOM;
    }
    const int rc = model_build(m, n_layers, channels, conv_w, conv_b, fc_w, fc_b, dtype, device);
    if (rc != RS_OK) {
        delete m;                         // (frees what was uploaded; the error text stays that of the failure)
        return rc;
    }
    *out = m;
    return RS_OK;
}

int rs_model_set_fc_classifier(rs_model* m, int positions, int hidden, const float* w1, const float* b1, const float* w2,
                               const float* b2) {
    if (!m || !w1 || !b1 || !w2 || !b2) {
        set_error("rs_model_set_fc_classifier: null argument");
        return RS_ERR_ARG;
    }
    if (m->dtype != RS_F32 && m->dtype != RS_F32W) {
        set_error("rs_model_set_fc_classifier: fp32 models only (RS_F32 / RS_F32W)");
        return RS_ERR_ARG;
    }
    if (m->fc.H) {
        set_error("rs_model_set_fc_classifier: already set");
        return RS_ERR_ARG;
    }
    const int C = m->channels[m->n_layers - 1], C4 = round_up(C, 4);
    if (positions < 1 || hidden < 64 || hidden % 64 != 0 || C4 > m->cp[m->n_layers - 1] ||
        (int64_t)positions << m->n_layers > kMaxNormLen) {
        set_error("rs_model_set_fc_classifier: positions %d / hidden %d not supported (hidden: a multiple of 64)", positions, hidden);
        return RS_ERR_ARG;
    }
    DeviceGuard guard(m->device);
    const size_t F = (size_t)C * positions;
    DevBuf<float> raw, d_w1p, d_b1, d_w2, d_b2;   // w1 as given, and the head's four tables, which go to the model on success
    float*& d_raw = raw.p;
    RS_HIP(hipMalloc(reinterpret_cast<void**>(&d_raw), F * hidden * sizeof(float)));
    int rc = RS_OK;
    auto fail = [&](hipError_t e) {
        set_error("rs_model_set_fc_classifier: %s", hipGetErrorString(e));
        rc = RS_ERR_HIP;
    };
    hipError_t e = hipMemcpy(d_raw, w1, F * hidden * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) fail(e);
    if (rc == RS_OK && (e = hipMalloc(reinterpret_cast<void**>(&d_w1p.p), (size_t)positions * C4 * hidden * sizeof(float))) != hipSuccess)
        fail(e);
    if (rc == RS_OK) rc = launch_fc_pack(d_raw, d_w1p, C, C4, positions, hidden, nullptr);
    if (rc == RS_OK && (e = hipDeviceSynchronize()) != hipSuccess) fail(e);
    if (rc == RS_OK) rc = upload_owned(d_b1, std::vector<float>(b1, b1 + hidden));
    if (rc == RS_OK) rc = upload_owned(d_w2, std::vector<float>(w2, w2 + 2 * (size_t)hidden));
    if (rc == RS_OK) rc = upload_owned(d_b2, std::vector<float>(b2, b2 + 2));
    if (rc != RS_OK) return rc;
    m->fc.d_w1p = m->fc_w1p = std::move(d_w1p);
    m->fc.d_b1 = m->fc_b1 = std::move(d_b1);
    m->fc.d_w2 = m->fc_w2 = std::move(d_w2);
    m->fc.d_b2 = m->fc_b2 = std::move(d_b2);
    m->fc.C = C;
    m->fc.C4 = C4;
    m->fc.P = positions;
    m->fc.H = hidden;
    return RS_OK;
}

int rs_model_destroy(rs_model* m) {
    if (!m) return RS_OK;
    DeviceGuard guard(m->device);
    if (m->side_stream) (void)hipStreamDestroy(m->side_stream);
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_join) (void)hipEventDestroy(m->ev_join);
    for (hipEvent_t e : m->ev_pool) (void)hipEventDestroy(e);
    delete m;                             // the device buffers go with their owners (convnet_model.hpp)
    return RS_OK;
}

int rs_padded_length(const rs_model* m, int Lmax) {
    if (!m || Lmax < 1) return 0;
    return ((Lmax >> m->pad_shift) + 1) << m->pad_shift;
}

int rs_block_samples(const rs_model* m) { return m ? 1 << m->pad_shift : 0; }

int rs_max_batch(const rs_model* m, int Lmax) {
    if (!m || Lmax < 1) return 0;
    // every activation buffer (and the normalised signals) is addressed through a 2 GiB buffer-resource window
    const WsLayout w1 = ws_layout(m, 1, Lmax);
    const int64_t per_read = std::max<int64_t>((int64_t)(w1.bufb_off - w1.bufa_off), (int64_t)w1.nb_f_max * w1.Uf * 4);
    return (int)std::max<int64_t>(1, ((1LL << 31) - (1 << 20)) / per_read);
}

size_t rs_workspace_bytes(const rs_model* m, int B, int Lmax) {
    if (!m || B < 1 || Lmax < 1) return 0;
    return ws_layout(m, B, Lmax).total;
}

int rs_normalise(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B, int Lmax, float* d_out32,
                 int64_t ld32, int32_t pad_to, double* d_out64, int64_t ld64, double* d_stats, void* stream) {
    if (B < 0 || (B > 0 && (!d_sig || !d_off || !d_len))) {
        set_error("rs_normalise: null argument");
        return RS_ERR_ARG;
    }
    if (!d_out32 && !d_out64 && !d_stats) {
        set_error("rs_normalise: no output requested");
        return RS_ERR_ARG;
    }
    if ((d_out32 && (ld32 < Lmax || pad_to > ld32)) || (d_out64 && ld64 < Lmax)) {
        set_error("rs_normalise: output pitch smaller than Lmax / pad_to");
        return RS_ERR_ARG;
    }
    return launch_normalise(d_sig, d_off, d_len, B, Lmax, d_out32, ld32, pad_to, d_out64, ld64, d_stats,
                            static_cast<hipStream_t>(stream));
}

int rs_normalise_float(const void* d_sig, int elem_bytes, const int64_t* d_off, const int32_t* d_len, int B, void* d_out,
                       int64_t ld, double* d_stats, void* stream) {
    if (B < 0 || (B > 0 && (!d_sig || !d_off || !d_len || !d_out)) || (elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)) {
        set_error("rs_normalise_float: null argument or element size %d not 2 / 4 / 8", elem_bytes);
        return RS_ERR_ARG;
    }
    return launch_normalise_float(d_sig, elem_bytes, d_off, d_len, B, d_out, ld, d_stats, static_cast<hipStream_t>(stream));
}

int rs_forward(rs_model* m, const float* d_x, int64_t ldx, const int32_t* d_len, const int32_t* h_len, int B, int Lmin,
               int Lmax, void* d_ws, size_t ws_bytes, float* d_probs, float* d_logits, void* stream) {
    if (!m || !d_x || !d_len || !d_ws || !d_probs || B < 1) {
        set_error("rs_forward: null argument or empty batch");
        return RS_ERR_ARG;
    }
    if (Lmax < (1 << m->n_layers)) {
        set_error("rs_forward: Lmax %d shorter than the network minimum %d", Lmax, 1 << m->n_layers);
        return RS_ERR_LENGTH;
    }
    if (ldx < Lmax) {
        set_error("rs_forward: ldx %lld < Lmax %d", (long long)ldx, Lmax);
        return RS_ERR_ARG;
    }
    const WsLayout w = ws_layout(m, B, Lmax);
    int rc = check_call("rs_forward", m, B, Lmax, w, ws_bytes);
    if (rc != RS_OK) return rc;
    Batch bt;
    rc = make_batch(m, w, d_ws, h_len, B, Lmin, Lmax, &bt);
    if (rc != RS_OK) return rc;
    DeviceGuard guard(m->device);         // launches go to the model's device whatever the caller's current one is
    RS_HIP(guard.err);
    if (!m->prof_open) prof_mark(m, -1, static_cast<hipStream_t>(stream));
    rc = launch_plan(d_len, B, Lmax, bt.plan, static_cast<hipStream_t>(stream));
    if (rc == RS_OK && two_level(m)) rc = launch_plan(d_len, B, Lmax, bt.fine, static_cast<hipStream_t>(stream));
    if (rc != RS_OK) return rc;
    return forward_impl(m, d_x, ldx, d_len, B, bt, w, d_ws, d_probs, d_logits, stream, false);
}

int rs_classify(rs_model* m, const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, const int32_t* h_len, int B,
                int Lmin, int Lmax, void* d_ws, size_t ws_bytes, float* d_probs, float* d_logits, void* stream) {
    if (!m || !d_sig || !d_off || !d_len || !d_ws || !d_probs || B < 1) {
        set_error("rs_classify: null argument or empty batch");
        return RS_ERR_ARG;
    }
    if (Lmax < (1 << m->n_layers) || Lmax > kMaxNormLen) {
        set_error("rs_classify: Lmax %d outside [%d, %d]", Lmax, 1 << m->n_layers, kMaxNormLen);
        return RS_ERR_LENGTH;
    }
    const WsLayout w = ws_layout(m, B, Lmax);
    int rc = check_call("rs_classify", m, B, Lmax, w, ws_bytes);
    if (rc != RS_OK) return rc;
    Batch bt;
    rc = make_batch(m, w, d_ws, h_len, B, Lmin, Lmax, &bt);
    if (rc != RS_OK) return rc;
    DeviceGuard guard(m->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    prof_mark(m, -1, st);
    rc = normalise_packed(m, d_sig, d_off, d_len, B, Lmax, w, bt, d_ws, st);
    if (rc != RS_OK) return rc;
    prof_mark(m, 0, st);
    const float* xn = reinterpret_cast<const float*>(static_cast<char*>(d_ws) + w.xnorm_off);
    return forward_impl(m, xn, w.Uf, d_len, B, bt, w, d_ws, d_probs, d_logits, stream, true);
}

int rs_autotune(rs_model* m, const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, const int32_t* h_len, int B,
                int Lmin, int Lmax, void* d_ws, size_t ws_bytes, float* d_probs, int32_t* n_changed, void* stream) {
    if (!m) {
        set_error("rs_autotune: null model");
        return RS_ERR_ARG;
    }
    const bool prof = m->prof_on;
    m->prof_on = false;
    m->tuning = true;
    m->tuned_changed = 0;
    const int rc = rs_classify(m, d_sig, d_off, d_len, h_len, B, Lmin, Lmax, d_ws, ws_bytes, d_probs, nullptr, stream);
    m->tuning = false;
    m->prof_on = prof;
    if (n_changed) *n_changed = m->tuned_changed;
    return rc;
}

// the layout all models of an ensemble share: block table and normalised signals once, activation buffers sized for the
// widest model
static WsLayout ensemble_layout(rs_model* const* models, int n_models, int B, int Lmax) {
    WsLayout w = ws_layout(models[0], B, Lmax);
    for (int k = 1; k < n_models; ++k) {
        const WsLayout wk = ws_layout(models[k], B, Lmax);
        if (wk.bufb_off - wk.bufa_off > w.bufb_off - w.bufa_off) w = wk;
    }
    return w;
}

static bool ensemble_compatible(rs_model* const* models, int n_models) {
    if (!models || n_models < 1 || !models[0]) return false;
    const rs_model* m0 = models[0];
    for (int k = 0; k < n_models; ++k)
        if (!models[k] || models[k]->n_layers != m0->n_layers || models[k]->device != m0->device ||
            esize(models[k]) != esize(m0) || models[k]->pad_shift != m0->pad_shift || models[k]->fine_shift != m0->fine_shift ||
            models[k]->split != m0->split || models[k]->fc.H != m0->fc.H)
            return false;
    return true;
}

size_t rs_ensemble_workspace_bytes(rs_model* const* models, int n_models, int B, int Lmax) {
    if (!ensemble_compatible(models, n_models) || B < 1 || Lmax < 1 || models[0]->fc.H) return 0;
    const WsLayout w = ensemble_layout(models, n_models, B, Lmax);
    return w.bufa_off + (size_t)n_models * 2 * (w.bufb_off - w.bufa_off);
}

int rs_classify_ensemble(rs_model* const* models, int n_models, const int16_t* d_sig, const int64_t* d_off,
                         const int32_t* d_len, const int32_t* h_len, int B, int Lmin, int Lmax, void* d_ws, size_t ws_bytes,
                         float* d_probs, uint8_t* d_decision, int max_len, float threshold, int mode, void* stream) {
    if (!models || n_models < 1 || !d_sig || !d_off || !d_len || !d_ws || !d_probs || B < 1) {
        set_error("rs_classify_ensemble: null argument or empty batch");
        return RS_ERR_ARG;
    }
    if (!ensemble_compatible(models, n_models)) {
        set_error("rs_classify_ensemble: a model is null or differs in depth / device / element size");
        return RS_ERR_ARG;
    }
    rs_model* m0 = models[0];
    if (d_decision && mode != RS_ENRICH && mode != RS_DEPLETE) {
        set_error("rs_classify_ensemble: bad mode");
        return RS_ERR_ARG;
    }
    if (Lmax < (1 << m0->n_layers) || Lmax > kMaxNormLen) {
        set_error("rs_classify_ensemble: Lmax %d outside [%d, %d]", Lmax, 1 << m0->n_layers, kMaxNormLen);
        return RS_ERR_LENGTH;
    }
    // the models share one plan and one copy of the normalised signals: same block size, same element size (checked
    // above), so one layout serves them all except for the width of the activation buffers
    const WsLayout w = ensemble_layout(models, n_models, B, Lmax);
    int rc = check_call("rs_classify_ensemble", m0, B, Lmax, w, ws_bytes);
    if (rc != RS_OK) return rc;
    Batch bt;
    rc = make_batch(m0, w, d_ws, h_len, B, Lmin, Lmax, &bt);
    if (rc != RS_OK) return rc;
    DeviceGuard guard(m0->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // With a workspace of rs_ensemble_workspace_bytes() every model has its own pair of activation buffers and the
    // forwards run CONCURRENTLY: model 0 on the caller's stream, model k on its own side stream, forked behind the
    // normalise launch and joined in front of the decision.  The forwards are independent (they read the shared block table
    // and normalised rows, write their own buffers and their own slice of d_probs), so the results are those of the serial
    // order, bit for bit; what overlaps is one model's tile-round tails, prologues and launch gaps with another's tiles.
    // A smaller workspace (rs_workspace_bytes of the widest model), a profiled or a tuning model, or RS_ENSEMBLE_SERIAL
    // run the forwards back to back on the caller's stream.
    const size_t buf_bytes = w.bufb_off - w.bufa_off;
    // ... and so does a batch that fills the chip by itself: measured (tools/ensemble_probe.py, three models, same box,
    // interleaved) concurrent / serial = 2.4x at 32 reads, 1.5x at 128, 1.14x (fp32) / 1.13x (bf16x3) at the live 357 x 8615
    // batch (1071 blocks), 1.01x / 0.99x at 512 x 16000 (2048 blocks): beyond ~1800 blocks of 4096 samples one model's
    // launches leave nothing for another's to use, and the fork / join is pure overhead
    constexpr int64_t kConcurrentBelowSamples = 1800LL * 4096;
    bool concurrent = n_models > 1 && ws_bytes >= w.bufa_off + (size_t)n_models * 2 * buf_bytes &&
                      !m0->hooks.ensemble_serial && !m0->fc.H && (int64_t)bt.NB * w.U < kConcurrentBelowSamples;
    for (int k = 0; k < n_models; ++k)
        if (models[k]->prof_on || models[k]->tuning || models[k]->dbg_dst) concurrent = false;
    for (int k = 1; k < n_models && concurrent; ++k)
        for (int j = 0; j < k; ++j)
            if (models[j] == models[k]) concurrent = false;                  // one handle twice: its side stream is one
    if (concurrent)
        for (int k = 1; k < n_models; ++k) {
            rs_model* mk = models[k];
            if (!mk->side_stream) RS_HIP(hipStreamCreateWithFlags(&mk->side_stream, hipStreamNonBlocking));
            if (!mk->ev_fork) RS_HIP(hipEventCreateWithFlags(&mk->ev_fork, hipEventDisableTiming));
            if (!mk->ev_join) RS_HIP(hipEventCreateWithFlags(&mk->ev_join, hipEventDisableTiming));
        }
    prof_mark(m0, -1, st);
    rc = normalise_packed(m0, d_sig, d_off, d_len, B, Lmax, w, bt, d_ws, st);
    if (rc != RS_OK) return rc;
    prof_mark(m0, 0, st);
    const float* xn = reinterpret_cast<const float*>(static_cast<char*>(d_ws) + w.xnorm_off);
    if (concurrent) {
        // Whatever fails after the first fork, every side stream that has received work is JOINED to the caller's stream
        // before this call returns: the caller owns the workspace and d_probs and may reuse or free them behind `st` the
        // moment it sees the error code.  A join that itself fails falls back to a host-side wait.
        int forked = 0;
        auto join_all = [&]() {
            for (int k = 1; k <= forked; ++k) {
                rs_model* mk = models[k];
                if (hipEventRecord(mk->ev_join, mk->side_stream) != hipSuccess ||
                    hipStreamWaitEvent(st, mk->ev_join, 0) != hipSuccess)
                    (void)hipStreamSynchronize(mk->side_stream);
            }
        };
        for (int k = 1; k < n_models && rc == RS_OK; ++k) {
            rs_model* mk = models[k];
            hipError_t he = hipEventRecord(mk->ev_fork, st);
            if (he == hipSuccess) he = hipStreamWaitEvent(mk->side_stream, mk->ev_fork, 0);
            if (he != hipSuccess) {
                set_error("rs_classify_ensemble: fork of model %d: %s", k, hipGetErrorString(he));
                rc = RS_ERR_HIP;
                break;
            }
            forked = k;
            WsLayout wk = w;
            wk.bufa_off += (size_t)k * 2 * buf_bytes;
            wk.bufb_off += (size_t)k * 2 * buf_bytes;
            rc = forward_impl(mk, xn, w.Uf, d_len, B, bt, wk, d_ws, d_probs + (size_t)k * B * 2, nullptr, mk->side_stream, true);
        }
        if (rc == RS_OK) rc = forward_impl(m0, xn, w.Uf, d_len, B, bt, w, d_ws, d_probs, nullptr, stream, true);
        join_all();
        if (rc != RS_OK) return rc;
    } else {
        for (int k = 0; k < n_models; ++k) {
            // every model keeps the block table and the normalised rows at the head of the workspace and ping-pongs behind them
            rc = forward_impl(models[k], xn, w.Uf, d_len, B, bt, w, d_ws, d_probs + (size_t)k * B * 2, nullptr, stream, true);
            if (rc != RS_OK) return rc;
        }
    }
    if (d_decision) rc = launch_decide(d_probs, n_models, B, d_len, max_len, threshold, mode, d_decision, st);
    return rc;
}

int rs_decide(const float* d_probs, int n_models, int B, const int32_t* d_len, int max_len, float threshold,
              int mode, uint8_t* d_out, void* stream) {
    if (B < 0 || n_models < 1 || (B > 0 && (!d_probs || !d_len || !d_out)) ||
        (mode != RS_ENRICH && mode != RS_DEPLETE)) {
        set_error("rs_decide: bad argument");
        return RS_ERR_ARG;
    }
    return launch_decide(d_probs, n_models, B, d_len, max_len, threshold, mode, d_out,
                         static_cast<hipStream_t>(stream));
}

int rs_polya_end(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B, int32_t* d_end,
                 void* stream) {
    if (B < 0 || (B > 0 && (!d_sig || !d_off || !d_len || !d_end))) {
        set_error("rs_polya_end: null argument");
        return RS_ERR_ARG;
    }
    return launch_polya(d_sig, d_off, d_len, B, d_end, static_cast<hipStream_t>(stream));
}

int rs_polya_end_resume(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B, const int32_t* d_state_in,
                        int32_t* d_end, int32_t* d_state_out, void* stream) {
    if (B < 0 || (B > 0 && (!d_sig || !d_off || !d_len || !d_end || !d_state_out))) {
        set_error("rs_polya_end_resume: null argument");
        return RS_ERR_ARG;
    }
    if (B > 0 && d_state_in == d_state_out) {
        set_error("rs_polya_end_resume: d_state_in and d_state_out must not be the same buffer");
        return RS_ERR_ARG;
    }
    return launch_polya(d_sig, d_off, d_len, B, d_end, static_cast<hipStream_t>(stream), d_state_in, d_state_out);
}

int rs_copy_segments(const int16_t* d_src, int16_t* d_dst, const int64_t* d_src_off, const int64_t* d_dst_off,
                     const int32_t* d_len, int n, void* stream) {
    if (n < 0 || (n > 0 && (!d_src || !d_dst || !d_src_off || !d_dst_off || !d_len))) {
        set_error("rs_copy_segments: null argument");
        return RS_ERR_ARG;
    }
    return launch_copy_segments(d_src, d_dst, d_src_off, d_dst_off, d_len, n, static_cast<hipStream_t>(stream));
}

int rs_model_saturated(rs_model* m, int reset, void* stream) {
    if (!m) {
        set_error("rs_model_saturated: null model");
        return RS_ERR_ARG;
    }
    if (!m->d_sat) return 0;                                  // fp32 / bf16 modes carry fp32's exponent range
    DeviceGuard guard(m->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // ONE atomic operation reads the flag and (with `reset`) clears it: an epilogue of a kernel on another stream that raises
    // the flag lands before the exchange (this call returns 1) or behind it (the flag stays set for the next call)
    hipLaunchKernelGGL(read_flag_kernel, dim3(1), dim3(1), 0, st, m->d_sat.p, m->h_sat.p, reset ? 1 : 0);
    RS_HIP(hipGetLastError());
    RS_HIP(hipStreamSynchronize(st));
    return *static_cast<volatile unsigned*>(m->h_sat.p) ? 1 : 0;
}

int rs_debug_capture_layer(rs_model* m, int layer, void* d_dst, size_t bytes) {
    if (!m) {
        set_error("rs_debug_capture_layer: null model");
        return RS_ERR_ARG;
    }
    m->dbg_layer = layer;
    m->dbg_dst = d_dst;
    m->dbg_bytes = bytes;
    return RS_OK;
}

int rs_profile_enable(rs_model* m, int on) {
    if (!m) {
        set_error("rs_profile_enable: null model");
        return RS_ERR_ARG;
    }
    m->prof_on = on != 0;
    m->prof_level = on == 2 ? 2 : 1;
    m->prof_open = false;
    if (!on) {
        m->ev_used = 0;
        m->prof_calls = 0;
    }
    return RS_OK;
}

int rs_profile_read(rs_model* m, float* stage_ms, int32_t* calls) {
    if (!m || !stage_ms) {
        set_error("rs_profile_read: null argument");
        return RS_ERR_ARG;
    }
    if (m->ev_used) RS_HIP(hipEventSynchronize(m->ev_pool[m->ev_used - 1]));
    for (size_t k = 1; k < m->ev_used; ++k) {
        const int stage = m->ev_stage[k];
        if (stage < 0) continue;
        float ms = 0.f;
        RS_HIP(hipEventElapsedTime(&ms, m->ev_pool[k - 1], m->ev_pool[k]));
        stage_ms[stage] += ms;
    }
    if (calls) *calls = m->prof_calls;
    m->ev_used = 0;
    m->prof_calls = 0;
    return RS_OK;
}

int rs_model_layer_info(const rs_model* m, int layer, rs_layer_info* out) {
    if (!m || !out || layer < 0 || layer >= m->n_layers) {
        set_error("rs_model_layer_info: bad argument");
        return RS_ERR_ARG;
    }
    memset(out, 0, sizeof(*out));
    out->c_out = m->channels[layer];
    out->cp_out = m->cp[layer];
    out->rows_format = (layer + 1 < m->n_layers && m->layers[layer + 1].f8_in) ? 2 : is_x3(m->dtype) ? 1 : 0;
    if (layer == 0) {
        out->c_in = 1;
        out->cp_in = 1;
        out->k_pad = 3;
        out->n_pad = m->cp[0];
        out->gemm_row_div = 1;
        out->block_samples = 1 << layer_shift(m, 0);
        return RS_OK;
    }
    const ConvLayerDev& L = m->layers[layer];
    out->c_in = L.c_in;
    out->cp_in = L.cp_in;
    out->k_pad = (m->dtype == RS_F32W ? (L.wino_m == 4 ? 6 : 4) : 3) * L.plan.kc * L.plan.nch;
    if (L.ring_tail) out->k_pad = (3 * (L.ring_panels - 1) + 1) * 32;                       // the last panel's taps share one K step
    if (m->last_ring[layer] && !is_x3(m->dtype)) out->k_pad = 3 * 64 * L.ring_panels;      // 64-channel panels
    out->n_pad = m->last_bn[layer] ? round_up(round_up(L.c_out, 16), m->last_bn[layer]) : round_up(L.c_out, 16);
    out->bm = m->last_bm[layer];
    out->bn = m->last_bn[layer];
    out->kc = L.plan.kc;
    out->gemm_row_div = m->dtype == RS_F32W ? L.wino_m : 1;
    out->block_samples = 1 << layer_shift(m, layer);
    return RS_OK;
}

}  // extern "C"
