// Host-side tile planner of the tiled ConvNet kernels (conv_f32 / conv_wino / conv_wino4 / conv_ring_h16 / conv_ring_f8).
//
// Every one of those kernels has a table of tile shapes <wm, wn, mt, nt> (waves along rows x waves along columns, 16-row and
// 16-column MFMA tiles per wave) and a cost model per tile; a launch over `rows` row units and n16 16-column groups costs
// (rounds over the CUs) x (one tile).  What the kernels share is everything around those two: the search over the table, the
// pins that override it (RS_FORCE_SHAPE_* string, the fused layer-0 form of F(2,3), rs_autotune's picks), and the head + tail
// split of a launch that ends in a mostly empty round.  That is here, once, as plain host C++ (no HIP header: a CPU test
// drives it with synthetic families, tests/tile_plan_check.cpp); a kernel file keeps its table, its LDS and cost formulas, its
// argument struct and one launch_part, and describes itself with a TileFamily.  DESIGN.md 3 has the per-family table.
//
// Nothing here allocates or calls through a pointer: the family's members are lambdas, plan_tiles is a template, and the
// result is a small record by value - this runs on the launch path of every layer.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

namespace rs {

// LDS of a CU: what one workgroup's tiles may fill (workgroups that share a CU: their sum)
constexpr size_t kConvLdsBudget = 160 * 1024;

// what every shape-table entry starts with; the kernels' Shape records derive from it and add their KernelFn members
struct TileGeom {
    int wm, wn, mt, nt;
    constexpr int bm() const { return wm * 16 * mt; }       // row units per tile (the family's own: conv rows, pooled rows, F(4,3) groups)
    constexpr int bnt() const { return wn * nt; }           // 16-column groups per tile
    constexpr int bn() const { return 16 * wn * nt; }       // columns per tile
    constexpr int waves() const { return wm * wn; }
    // tiles of a launch over `rows` row units and n16 column groups
    int64_t tiles(int64_t rows, int n16) const { return ((rows + bm() - 1) / bm()) * ((n16 + bnt() - 1) / bnt()); }
};

// index of table entry <wm, wn, mt, nt>, or -1 (a table names a shape once; of two equal entries the later one, as before)
template <class GeomOf>
inline int find_shape(int n_shapes, GeomOf geom, int wm, int wn, int mt, int nt) {
    int found = -1;
    for (int k = 0; k < n_shapes; ++k)
        if (geom(k).wm == wm && geom(k).wn == wn && geom(k).mt == mt && geom(k).nt == nt) found = k;
    return found;
}

// The RS_FORCE_SHAPE_* switches are lists "layer:wm,wn,mt,nt;...".  The next entry of `layer` in the list from q on: its numbers,
// and the text behind it to go on from (null: there is no further entry).  Where a layer is named more than once the LAST
// entry that suits wins, so plan_tiles asks until the answer is null.  (common.hpp: next_layer_value is its one-number sibling.)
inline const char* next_layer_shape(const char* q, int layer, int* wm, int* wn, int* mt, int* nt) {
    for (; q && *q; q = strchr(q, ';') ? strchr(q, ';') + 1 : nullptr) {
        int l, x[4];
        if (sscanf(q, "%d:%d,%d,%d,%d", &l, &x[0], &x[1], &x[2], &x[3]) == 5 && l == layer) {
            *wm = x[0], *wn = x[1], *mt = x[2], *nt = x[3];
            return strchr(q, ';') ? strchr(q, ';') + 1 : q + strlen(q);
        }
    }
    return nullptr;
}

// A kernel family as the planner sees it:
//   geom(k)                          geometry of table entry k < n_shapes
//   tile_cost(k)                     cycles per tile of a FULL launch (every CU has a tile); < 0: the planner never picks entry k
//   thin_tile_cost(k, per_cu, fill)  the two Winograd kernels only: cycles per tile of a launch that leaves CUs idle, per_cu
//                                    workgroups resident on a CU, fill = share of the CUs that stream; < 0: does not fit
//   can_run(k)                       entry k can run this layer at all: what a FORCED or TUNED shape must satisfy, which is less
//                                    than tile_cost(k) >= 0 (four-wave and experimental entries can be forced)
struct NoThinFit {};
template <class GeomOf, class TileCost, class ThinTileCost, class CanRun>
struct TileFamily {
    static constexpr bool has_thin = !std::is_same<ThinTileCost, NoThinFit>::value;
    int n_shapes;
    GeomOf geom;
    TileCost tile_cost;
    ThinTileCost thin_tile_cost;
    CanRun can_run;
};
template <class GeomOf, class TileCost, class ThinTileCost, class CanRun>
inline TileFamily<GeomOf, TileCost, ThinTileCost, CanRun> tile_family(int n_shapes, GeomOf geom, TileCost tile_cost,
                                                                      ThinTileCost thin_tile_cost, CanRun can_run) {
    return {n_shapes, geom, tile_cost, thin_tile_cost, can_run};
}

// The search.  Ties: a new best needs a strictly lower cost and the table is walked in order, so the FIRST of equal entries
// wins - the order of a table is part of its behaviour.
//   pass 1: (rounds over num_cu CUs) x tile_cost(k) over the entries with tile_cost(k) >= 0;
//   pass 2, families with a thin fit, when allowed and the best of pass 1 has fewer tiles than CUs: the thin fit over EVERY
//           entry, four-wave ones at one and two workgroups per CU.  Its scale differs from pass 1's by up to 25 %: `thin`
//           says which model `cost` is in, compare like with like.
struct TileChoice {
    int shape = -1;          // -1: no entry is usable
    double cost = 1e300;
    int per_cu = 1;
    bool thin = false;
};
template <class Family>
inline TileChoice choose_tile(const Family& f, int64_t rows, int n16, int num_cu, bool allow_thin = true) {
    TileChoice c;
    int64_t best_tiles = 0;
    for (int k = 0; k < f.n_shapes; ++k) {
        const double tile = f.tile_cost(k);
        if (tile < 0) continue;
        const int64_t tiles = f.geom(k).tiles(rows, n16);
        const double cost = (double)((tiles + num_cu - 1) / num_cu) * tile;
        if (cost < c.cost) {
            c.cost = cost;
            c.shape = k;
            best_tiles = tiles;
        }
    }
    if constexpr (Family::has_thin) {
        c.thin = allow_thin && c.shape >= 0 && best_tiles < num_cu;
        if (c.thin) {
            c.cost = 1e300;
            for (int k = 0; k < f.n_shapes; ++k) {
                const int64_t tiles = f.geom(k).tiles(rows, n16);
                const double fill = std::min(1.0, (double)tiles / num_cu);
                for (int per_cu = 1; per_cu <= (f.geom(k).waves() == 4 ? 2 : 1); ++per_cu) {
                    const double tile = f.thin_tile_cost(k, per_cu, fill);
                    if (tile < 0) continue;
                    const int64_t slots = (int64_t)num_cu * per_cu;
                    const double cost = (double)((tiles + slots - 1) / slots) * tile;
                    if (cost < c.cost) {
                        c.cost = cost;
                        c.shape = k;
                        c.per_cu = per_cu;
                    }
                }
            }
        }
    }
    return c;
}

// A launch costs (rounds over the CUs) x (one tile): 300 tiles of the best shape on 256 CUs cost two full rounds for 1.17
// rounds of work.  Run `head_mtiles` row tiles of shape h - as many whole rounds as the grid holds - and leave the rows
// behind them to a second launch with the shape that suits THAT row count best.  Every output keeps its accumulation order
// (it does not depend on the tile shape: the batch-invariance tests), so the bits are those of the single launch.  cost
// units: the planners' SIMD cycles.
struct TailSplit {
    int head_shape = -1;     // -1: single launch
    int head_mtiles = 0;
    int tail_shape = -1;
    double cost = 0.0;
};

// f / rows / n16 / num_cu as for choose_tile; single_cost: what ONE launch is priced at.  The tail is priced with the full-launch
// calibration like the head (one scale), whatever shape runs it in the end.
template <class Family>
inline TailSplit plan_tail_split(const Family& f, int64_t rows, int n16, int num_cu, double single_cost, double margin = 0.97) {
    constexpr double kLaunch = 6000.0;        // a second launch: boundary + its own prologue
    TailSplit out;
    out.cost = single_cost;
    for (int h = 0; h < f.n_shapes; ++h) {
        const double tc = f.tile_cost(h);
        if (tc < 0) continue;
        const int bm = f.geom(h).bm(), bnt = f.geom(h).bnt();
        const int64_t n_m = (rows + bm - 1) / bm, n_n = (n16 + bnt - 1) / bnt;
        const int64_t tiles = n_m * n_n;
        const int64_t full = tiles / num_cu;                     // whole rounds the launch holds
        if (full < 1 || tiles % num_cu == 0) continue;
        const int64_t m1 = full * num_cu / n_n;                  // row tiles of those rounds
        if (m1 < 1 || m1 >= n_m) continue;
        const int64_t head_rounds = (m1 * n_n + num_cu - 1) / num_cu;
        const TileChoice t = choose_tile(f, rows - m1 * bm, n16, num_cu, false);
        if (t.shape < 0) continue;
        const double cost = head_rounds * tc + t.cost + kLaunch;
        if (cost < margin * single_cost && cost < out.cost) {          // the margin is against ONE launch; the best split wins
            out.cost = cost;
            out.head_shape = h;
            out.head_mtiles = (int)m1;
            out.tail_shape = t.shape;
        }
    }
    return out;
}

// What overrides the search, in this order (a later pin replaces an earlier one):
//   force   the family's RS_FORCE_SHAPE_* string: the last entry of `layer` that names a table shape with can_run;
//   fused   a kernel form that exists for ONE shape pins that shape (F(2,3) with layer 0 folded into its staging: conv_wino.hip);
//           null: none;
//   tuned   tuned_pick() below; -1: none.  Must satisfy can_run.
// A pinned shape runs as ONE launch at one workgroup per CU.
//
// rs_autotune's pick for a launch: force_shape (>= 0 while it times a shape) before the recorded list of (conv input rows of the
// launch = B * P_in in EVERY family, whatever its row unit; table index) pairs; -1: neither
template <class TunedList>
inline int tuned_pick(int force_shape, const TunedList& tuned, int64_t conv_rows) {
    if (force_shape >= 0) return force_shape;
    for (const auto& t : tuned)
        if (t.first == conv_rows) return t.second;
    return -1;
}

struct TilePins {
    const char* force = nullptr;
    int layer = 0;
    int tuned = -1;
    const TileGeom* fused = nullptr;
};

// allowed: the family's switches permit head + tail launches (a pin forbids them whatever this says); margin: a split is taken
// when priced below this share of ONE launch; rechoose_tail: the tail launch runs the shape choose_tile picks for ITS rows
// with the thin fit allowed (and that fit's workgroups per CU) instead of the one the split was priced with.
struct SplitPolicy {
    bool allowed = false;
    double margin = 0.97;
    bool rechoose_tail = false;
};

struct TilePart {
    int shape;               // table index
    int m_base;              // first row unit (WalkArgs::m_base)
    int n_mtiles;            // row tiles
    int per_cu;              // workgroups per CU
};
struct TilePlan {
    int n_parts = 0;         // 0: no shape fits; 2: head + tail
    TilePart part[2] = {};
    double cost = 1e300;     // as planned (the split's where one is taken) ...
    double single_cost = 1e300;   // ... and of the search's single launch (not re-priced for a pinned shape)
    bool thin = false;       // single_cost is the thin fit's
    bool pinned = false;
};

template <class Family>
inline TilePlan plan_tiles(const Family& f, int64_t rows, int n16, int num_cu, const TilePins& pins, const SplitPolicy& split) {
    TilePlan p;
    const TileChoice c = choose_tile(f, rows, n16, num_cu);
    p.cost = p.single_cost = c.cost;
    p.thin = c.thin;
    int shape = c.shape, per_cu = c.per_cu;
    {
        int wm, wn, mt, nt;
        for (const char* q = pins.force; (q = next_layer_shape(q, pins.layer, &wm, &wn, &mt, &nt));)
            if (const int k = find_shape(f.n_shapes, f.geom, wm, wn, mt, nt); k >= 0 && f.can_run(k)) shape = k, p.pinned = true;
    }
    if (pins.fused) {
        p.pinned = true;
        if (const int k = find_shape(f.n_shapes, f.geom, pins.fused->wm, pins.fused->wn, pins.fused->mt, pins.fused->nt); k >= 0) shape = k;
    }
    if (pins.tuned >= 0 && pins.tuned < f.n_shapes && f.can_run(pins.tuned)) shape = pins.tuned, p.pinned = true;
    if (p.pinned) per_cu = 1;
    if (shape < 0) return p;
    auto mtiles = [&](int k, int64_t r) { return (int)((r + f.geom(k).bm() - 1) / f.geom(k).bm()); };
    TailSplit s;
    if (split.allowed && !p.pinned) s = plan_tail_split(f, rows, n16, num_cu, c.cost, split.margin);
    if (s.head_shape < 0) {
        p.n_parts = 1;
        p.part[0] = {shape, 0, mtiles(shape, rows), per_cu};
        return p;
    }
    const int m_base = s.head_mtiles * f.geom(s.head_shape).bm();
    int tail = s.tail_shape, tail_per_cu = 1;
    if (split.rechoose_tail)
        if (const TileChoice t = choose_tile(f, rows - m_base, n16, num_cu); t.shape >= 0) tail = t.shape, tail_per_cu = t.per_cu;
    p.n_parts = 2;
    p.part[0] = {s.head_shape, 0, s.head_mtiles, 1};              // the head: whole rounds, one workgroup per CU
    p.part[1] = {tail, m_base, mtiles(tail, rows - m_base), tail_per_cu};
    p.cost = s.cost;
    return p;
}

}  // namespace rs
