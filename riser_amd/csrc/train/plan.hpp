// Host arithmetic of the training family (train.hip): the buffers one forward + backward of B reads of L samples takes from the
// caller's workspace, and the slice plan of the weight-gradient contractions.  Everything here is a function of (B, L, conv
// shapes) alone - never of the device, a switch or a clock - so the same state and batch give the same bits on every box.
//
// A net is n_layers x [depth x (conv k_i + ReLU), pool]; its convs are numbered j = layer * depth + d.  Conv j sits behind
// level = j / depth pools and sees L >> level rows; the last conv of a layer pools (its buffers hold half the rows and a
// selector plane), every other - an inner conv - keeps all its rows.
#pragma once
#include "../family/host.hpp"

#include <vector>

namespace rs {
namespace train {

struct LayerShape {
    int c_in = 0, c_out = 0;
    int k = 3;                          // taps, odd
    int level = 0;                      // pools in front of this conv
    bool pool = true;                   // the last conv of its layer
    size_t w_off = 0, b_off = 0;        // floats into the flat parameter vector: W [c_out][c_in][k], then b [c_out]
    size_t wf_off = 0, wt_off = 0;      // floats into the packed vector: forward form [k][p16(c_in)][p16(c_out)], data-gradient
                                        // form [k][p16(c_out)][p16(c_in)]
    size_t n_w() const { return (size_t)c_out * c_in * k; }
    size_t tile_floats() const { return n_w() + c_out; }                   // one slice's partial: dW, then db
    size_t packed_floats() const { return (size_t)k * p16(c_in) * p16(c_out); }
    int rows_out(int L) const { return pool ? (L >> level) >> 1 : L >> level; }
    size_t out_elems(int B, int L) const { return (size_t)B * (size_t)rows_out(L) * cp4(c_out); }
};

constexpr int kSlicePositions = 256;                    // a weight-gradient slice contracts about this many positions
constexpr size_t kPartialBytes = size_t(32) << 20;      // and all slices' partial tiles of one conv stay below this
constexpr int kMaxGridY = 65535;                        // a grid's y extent: the slices of a weight gradient, the reads of a batch
constexpr int kTapGroup = 3;                            // taps one weight-gradient wave holds: k = 5 runs 3 + 2, k = 7 3 + 3 + 1

inline int tap_groups(int k) { return (k + kTapGroup - 1) / kTapGroup; }

struct SlicePlan {
    int n_slices = 1;
    int slice_len = 4;          // positions per slice, a multiple of the MFMA's K = 4; the last slice may be short
};

// Conv `s` contracts B * (L >> level) positions.  Slices of kSlicePositions, fewer where a conv's dW is so large that the
// partials would outgrow kPartialBytes: long contractions have tiny dW, and the reverse.  Never more than kMaxGridY: the
// slices are the y extent of train_wgrad_kernel's grid, and the largest batch of long reads would ask for more.
inline SlicePlan plan_slices(const LayerShape& s, int level, int B, int L) {
    const int64_t positions = (int64_t)B * (L >> level);
    const size_t tile_bytes = s.tile_floats() * sizeof(float);
    const int64_t cap = std::max<int64_t>(1, (int64_t)(kPartialBytes / tile_bytes));
    const int64_t want = (positions + kSlicePositions - 1) / kSlicePositions;
    SlicePlan p;
    p.n_slices = (int)std::max<int64_t>(1, std::min({want, cap, (int64_t)kMaxGridY}));
    const int64_t len = (positions + p.n_slices - 1) / p.n_slices;
    p.slice_len = (int)((len + 3) / 4 * 4);
    p.n_slices = (int)std::max<int64_t>(1, (positions + p.slice_len - 1) / p.slice_len);
    return p;
}

// the buffers of one call, front to back as Carver hands them out
struct Workspace {
    std::vector<size_t> act, sel;       // per conv: its rows [B][rows_out][cp4(c_out)] fp32 (and as many for their gradient);
                                        // selectors uint8 in the same shape, 0 bytes for an inner conv
    size_t gap = 0, dlogits = 0, flag = 256, partials = 0;
    size_t largest = 0;                 // the largest single buffer: the 2 GiB window applies to it
    size_t total = 0;
};

inline Workspace plan_workspace(const std::vector<LayerShape>& convs, int B, int L) {
    Workspace w;
    for (const LayerShape& s : convs) {
        const size_t elems = s.out_elems(B, L);
        w.act.push_back(elems * sizeof(float));
        w.sel.push_back(s.pool ? elems : 0);
        w.total += 2 * round256(elems * sizeof(float)) + (s.pool ? round256(elems) : 0);
        w.largest = std::max(w.largest, elems * sizeof(float));
        const SlicePlan sp = plan_slices(s, s.level, B, L);
        w.partials = std::max(w.partials, (size_t)sp.n_slices * s.tile_floats() * sizeof(float));
    }
    w.gap = (size_t)B * convs.back().c_out * sizeof(float);
    w.dlogits = (size_t)B * 2 * sizeof(float);
    w.largest = std::max(w.largest, w.partials);
    w.total += round256(w.gap) + round256(w.dlogits) + round256(w.flag) + round256(w.partials);
    return w;
}

// bytes per read of the largest activation buffer: the signals, a pooled plane or an inner conv's full-resolution rows
inline size_t per_read_bytes(const std::vector<LayerShape>& convs, int L) {
    size_t per = (size_t)L * sizeof(float);
    for (const LayerShape& s : convs) per = std::max(per, (size_t)s.rows_out(L) * cp4(s.c_out) * sizeof(float));
    return per;
}

}  // namespace train
}  // namespace rs
