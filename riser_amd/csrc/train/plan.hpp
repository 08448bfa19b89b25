// Host arithmetic of the training family (train.hip): the buffers one forward + backward of B reads of L samples takes from the
// caller's workspace, and the slice plan of the weight-gradient contractions.  Everything here is a function of (B, L, layer
// shapes) alone - never of the device, a switch or a clock - so the same state and batch give the same bits on every box.
#pragma once
#include "../family/host.hpp"

#include <vector>

namespace rs {
namespace train {

struct LayerShape {
    int c_in = 0, c_out = 0;
    size_t w_off = 0, b_off = 0;        // floats into the flat parameter vector: W [c_out][c_in][3], then b [c_out]
    size_t wf_off = 0, wt_off = 0;      // floats into the packed vector: forward form [3][p16(c_in)][p16(c_out)], data-gradient
                                        // form [3][p16(c_out)][p16(c_in)]
};

constexpr int kSlicePositions = 256;                    // a weight-gradient slice contracts about this many positions
constexpr size_t kPartialBytes = size_t(32) << 20;      // and all slices' partial tiles of one layer stay below this

struct SlicePlan {
    int n_slices = 1;
    int slice_len = 4;          // positions per slice, a multiple of the MFMA's K = 4; the last slice may be short
};

// Layer `s` contracts B * (L >> level) positions (level = its index: the pools in front of it).  Slices of kSlicePositions,
// fewer where a layer's dW is so large that the partials would outgrow kPartialBytes: long contractions have tiny dW, and
// the reverse.
inline SlicePlan plan_slices(const LayerShape& s, int level, int B, int L) {
    const int64_t positions = (int64_t)B * (L >> level);
    const size_t tile_bytes = ((size_t)s.c_out * s.c_in * 3 + s.c_out) * sizeof(float);
    const int64_t cap = std::max<int64_t>(1, (int64_t)(kPartialBytes / tile_bytes));
    const int64_t want = (positions + kSlicePositions - 1) / kSlicePositions;
    SlicePlan p;
    p.n_slices = (int)std::max<int64_t>(1, std::min(want, cap));
    const int64_t len = (positions + p.n_slices - 1) / p.n_slices;
    p.slice_len = (int)((len + 3) / 4 * 4);
    p.n_slices = (int)std::max<int64_t>(1, (positions + p.slice_len - 1) / p.slice_len);
    return p;
}

// the buffers of one call, front to back as Carver hands them out
struct Workspace {
    std::vector<size_t> act, sel;       // per layer: pooled rows [B][L >> (l + 1)][cp4(c_out)] fp32 (and as many for dY_l), selectors uint8
    size_t gap = 0, dlogits = 0, flag = 256, partials = 0;
    size_t largest = 0;                 // the largest single buffer: the 2 GiB window applies to it
    size_t total = 0;
};

inline Workspace plan_workspace(const std::vector<LayerShape>& layers, int B, int L) {
    Workspace w;
    for (size_t l = 0; l < layers.size(); ++l) {
        const size_t elems = (size_t)B * (size_t)(L >> (l + 1)) * cp4(layers[l].c_out);
        w.act.push_back(elems * sizeof(float));
        w.sel.push_back(elems);
        w.total += 2 * round256(elems * sizeof(float)) + round256(elems);
        w.largest = std::max(w.largest, elems * sizeof(float));
        const SlicePlan sp = plan_slices(layers[l], (int)l, B, L);
        w.partials = std::max(w.partials, (size_t)sp.n_slices * ((size_t)layers[l].c_out * layers[l].c_in * 3 + layers[l].c_out) * sizeof(float));
    }
    w.gap = (size_t)B * layers.back().c_out * sizeof(float);
    w.dlogits = (size_t)B * 2 * sizeof(float);
    w.largest = std::max(w.largest, w.partials);
    w.total += round256(w.gap) + round256(w.dlogits) + round256(w.flag) + round256(w.partials);
    return w;
}

// bytes per read of the largest activation buffer: layer 0's pooled rows or a later, wider one
inline size_t per_read_bytes(const std::vector<LayerShape>& layers, int L) {
    size_t per = (size_t)L * sizeof(float);
    for (size_t l = 0; l < layers.size(); ++l)
        per = std::max(per, (size_t)(L >> (l + 1)) * cp4(layers[l].c_out) * sizeof(float));
    return per;
}

}  // namespace train
}  // namespace rs
