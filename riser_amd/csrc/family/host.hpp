// The host pieces the ragged families share (tcn.hip, crnn.hip, gconv.hip): channel and LDS pitches, the 2 GiB buffer window,
// the carving of a caller's workspace, and the argument checks every rs_*_forward_ragged makes before it touches the device.
// Device memory is held in devbuf.hpp's DevBuf, filled by its upload().
#pragma once
#include "../common.hpp"
#include "../devbuf.hpp"

#include <algorithm>

namespace rs {

inline int cp4(int c) { return (c + 3) & ~3; }
inline int p16(int c) { return (c + 15) & ~15; }
// LDS row pitch: an odd number of float4 per row keeps the 16 rows x 4 k of an A fragment on distinct banks
inline int lds_pitch(int cp) { return ((cp / 4) % 2 == 0) ? cp + 4 : cp; }
inline size_t round256(size_t v) { return (v + 255) / 256 * 256; }

constexpr int64_t kWindow = (int64_t(1) << 31) - 4096;     // every activation buffer stays inside 2 GiB

// reads per call whose largest activation buffer (per_read_bytes each) stays inside the window
inline int max_batch_of(size_t per_read_bytes) {
    return (int)std::max<int64_t>(1, std::min<int64_t>(1 << 30, kWindow / (int64_t)per_read_bytes));
}

// the caller's workspace, handed out front to back in 256-byte steps
struct Carver {
    char* p;
    explicit Carver(void* ws) : p(static_cast<char*>(ws)) {}
    template <class T = float>
    T* take(size_t bytes) {
        T* r = reinterpret_cast<T*>(p);
        p += round256(bytes);
        return r;
    }
};

// what a family answers for one (B, ld), asked only once the handle is known to be there
struct RaggedLimits {
    int min_len;                // shortest row pitch the net runs (1: any)
    size_t ws_need;             // rs_*_workspace_bytes
    bool in_window;             // every buffer of B reads inside kWindow
};

// The checks of rs_*_forward_ragged in their order: arguments, row pitch, workspace, buffer window.  RS_OK, or the code with
// the message set.  fn / max_batch_fn: the entry point's name and that of its rs_*_max_batch.
template <class Limits>
int check_ragged_call(const char* fn, const char* max_batch_fn, const void* m, const void* d_x, const void* d_len,
                      const void* d_ws, const void* d_probs, int B, int ld, size_t ws_bytes, Limits limits) {
    if (!m || !d_x || !d_len || !d_ws || !d_probs || B < 1 || ld < 1) {
        set_error("%s: bad argument", fn);
        return RS_ERR_ARG;
    }
    const RaggedLimits l = limits();
    if (ld < l.min_len) {
        set_error("%s: reads of %d samples are shorter than the network minimum %d", fn, ld, l.min_len);
        return RS_ERR_LENGTH;
    }
    if (ws_bytes < l.ws_need) {
        set_error("%s: workspace too small", fn);
        return RS_ERR_WORKSPACE;
    }
    if (!l.in_window) {
        set_error("%s: %d reads of %d samples outgrow the 2 GiB buffer window: split the batch (%s)", fn, B, ld, max_batch_fn);
        return RS_ERR_ARG;
    }
    return RS_OK;
}

}  // namespace rs
