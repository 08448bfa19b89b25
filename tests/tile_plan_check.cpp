// Stand-alone check of the host-side tile planner (csrc/tile_plan.hpp, with the host half of csrc/tile_walk.hpp) on SYNTHETIC
// families: small tables and cost functions written here, so every expectation below can be worked out by hand or by brute
// force.  No HIP header, no GPU.  One line per case; the first failure prints FAIL and exits 1.  tests/test_tile_plan_cpu.py
// builds and runs it.
#include "tile_plan.hpp"
#include "tile_walk.hpp"

#include <stdio.h>
#include <stdlib.h>

using namespace rs;

static int n_cases = 0;
#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
            exit(1);                                                               \
        }                                                                          \
    } while (0)
static void ok(const char* what) { printf("ok %2d %s\n", ++n_cases, what); }

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- family A: one pass (like the direct and the ring kernels).  Entries 1 and 2 tile alike and cost alike (a tie), entry 4
// is unusable for the search but can run (forced), entry 5 can neither be picked nor run.
static const TileGeom kA[] = {{8, 1, 2, 2}, {8, 1, 1, 2}, {4, 2, 2, 1}, {4, 2, 1, 1}, {4, 1, 1, 1}, {2, 2, 8, 8}};
static const double kCostA[] = {100000.0, 56000.0, 56000.0, 31000.0, -1.0, -1.0};
constexpr int kNA = 6;
static auto family_a(const double* cost = kCostA) {
    return tile_family(
        kNA, [](int k) -> const TileGeom& { return kA[k]; }, [=](int k) { return cost[k]; }, NoThinFit{},
        [](int k) { return k != 5; });
}

// ---- family B: two passes (like the Winograd kernels): eight-wave entries for full launches, every entry in the thin fit,
// four-wave ones at one or two per CU (two does not fit for entry 4: its "LDS" is too large)
static const TileGeom kB[] = {{8, 1, 2, 2}, {8, 1, 1, 1}, {4, 2, 1, 1}, {4, 1, 1, 1}, {2, 2, 1, 2}};
constexpr int kNB = 5;
static int thin_calls = 0;
static auto family_b() {
    return tile_family(
        kNB, [](int k) -> const TileGeom& { return kB[k]; },
        [](int k) { return kB[k].waves() != 8 ? -1.0 : 20000.0 + 90.0 * kB[k].bm() * kB[k].bnt(); },
        [](int k, int per_cu, double fill) {
            ++thin_calls;
            if (k == 4 && per_cu == 2) return -1.0;
            return (9000.0 + 70.0 * kB[k].bm() * kB[k].bnt()) * (per_cu == 2 ? 1.3 : 1.0) * (1.0 + 0.1 * fill);
        },
        [](int) { return true; });
}

// the full-launch search by brute force: all costs first, then the minimum, the lowest index among equals
template <class F>
static int brute_single(const F& f, int64_t rows, int n16, int num_cu, double* cost_out, int64_t* tiles_out = nullptr) {
    double cost[16];
    int best = -1;
    for (int k = 0; k < f.n_shapes; ++k) {
        const double tc = f.tile_cost(k);
        const TileGeom& g = f.geom(k);
        cost[k] = tc < 0 ? -1.0 : (double)ceil_div(ceil_div(rows, g.wm * 16 * g.mt) * ceil_div(n16, g.wn * g.nt), num_cu) * tc;
    }
    for (int k = f.n_shapes - 1; k >= 0; --k)
        if (cost[k] >= 0 && (best < 0 || cost[k] <= cost[best])) best = k;
    if (cost_out) *cost_out = best < 0 ? 1e300 : cost[best];
    if (tiles_out && best >= 0) *tiles_out = f.geom(best).tiles(rows, n16);
    return best;
}

static void check_geometry() {
    const TileGeom g{4, 2, 3, 5};
    CHECK(g.bm() == 192 && g.bnt() == 10 && g.bn() == 160 && g.waves() == 8);
    CHECK(g.tiles(193, 11) == 4 && g.tiles(192, 10) == 1 && g.tiles(1, 1) == 1);
    CHECK(kConvLdsBudget == 163840);
    auto geom = [](int k) -> const TileGeom& { return kA[k]; };
    CHECK(find_shape(kNA, geom, 4, 2, 1, 1) == 3 && find_shape(kNA, geom, 8, 1, 2, 2) == 0 && find_shape(kNA, geom, 1, 1, 1, 1) == -1);
    CHECK(find_shape(0, geom, 8, 1, 2, 2) == -1);
    ok("geometry accessors, the LDS budget, shape lookup");
}

static void check_search() {
    const auto f = family_a();
    int n = 0, ties = 0;
    for (int num_cu : {1, 4, 7, 256})
        for (int n16 = 1; n16 <= 9; n16 += 2)
            for (int64_t rows = 1; rows <= 40000; rows = rows * 3 / 2 + 1, ++n) {
                double want_cost;
                const int want = brute_single(f, rows, n16, num_cu, &want_cost);
                const TileChoice c = choose_tile(f, rows, n16, num_cu);
                CHECK(c.shape == want && c.cost == want_cost && c.per_cu == 1 && !c.thin);
                CHECK(c.shape != 4 && c.shape != 5);                           // negative cost: never returned
                ties += c.shape == 1;
                const TilePlan p = plan_tiles(f, rows, n16, num_cu, {}, {});
                CHECK(p.n_parts == 1 && p.part[0].shape == want && p.part[0].m_base == 0 && p.part[0].per_cu == 1);
                CHECK(p.part[0].n_mtiles == ceil_div(rows, kA[want].bm()) && p.cost == want_cost && p.single_cost == want_cost);
                CHECK(!p.pinned && !p.thin);
            }
    CHECK(n > 100 && ties > 0);                                                // entry 1 won somewhere: never its equal, entry 2
    ok("single pass equals the brute-force minimum; of two equal entries the earlier; negative cost never returned");
    // entries 1 and 2 alone: always the earlier
    const double tie_only[] = {-1.0, 56000.0, 56000.0, -1.0, -1.0, -1.0};
    for (int64_t rows = 1; rows < 5000; rows += 97) CHECK(choose_tile(family_a(tie_only), rows, 2, 4).shape == 1);
    ok("a tie alone: the first entry");
    const double none[] = {-1.0, -1.0, -1.0, -1.0, -1.0, -1.0};
    const TileChoice c = choose_tile(family_a(none), 1000, 2, 4);
    CHECK(c.shape == -1 && c.cost == 1e300);
    const TilePlan p = plan_tiles(family_a(none), 1000, 2, 4, {}, {true, 0.97, false});
    CHECK(p.n_parts == 0 && !p.pinned && p.single_cost == 1e300);
    CHECK(choose_tile(tile_family(0, [](int k) -> const TileGeom& { return kA[k]; }, [](int) { return 1.0; }, NoThinFit{},
                                  [](int) { return true; }), 1000, 2, 4).shape == -1);
    ok("an empty feasible set (and an empty table): no shape");
    // ... unless a pin names an entry that can run
    const TilePlan q = plan_tiles(family_a(none), 1000, 2, 4, {"0:4,1,1,1", 0, -1}, {});
    CHECK(q.n_parts == 1 && q.part[0].shape == 4 && q.pinned && q.part[0].n_mtiles == ceil_div(1000, 64));
    ok("a forced entry runs where the search finds none");
}

static void check_two_pass() {
    const auto f = family_b();
    const int num_cu = 8;
    int n_thin = 0, n_full = 0, n_two = 0;
    for (int n16 = 1; n16 <= 4; ++n16)
        for (int64_t rows = 1; rows <= 6000; rows += 37) {
            double full_cost;
            int64_t full_tiles = 0;
            const int full = brute_single(f, rows, n16, num_cu, &full_cost, &full_tiles);
            thin_calls = 0;
            const TileChoice c = choose_tile(f, rows, n16, num_cu);
            CHECK(c.thin == (full_tiles < num_cu));                            // the thin pass runs exactly then ...
            CHECK((thin_calls > 0) == c.thin);                                 // ... and is not even evaluated otherwise
            if (c.thin) {
                ++n_thin;
                CHECK(thin_calls == 3 * 1 + 2 * 2);                            // every entry; four-wave ones at 1 and 2 per CU
                // brute force over (entry, per_cu) in table order
                int want = -1, want_pc = 1;
                double want_cost = 1e300;
                for (int k = 0; k < kNB; ++k)
                    for (int pc = 1; pc <= (kB[k].wm * kB[k].wn == 4 ? 2 : 1); ++pc) {
                        const int64_t tiles = kB[k].tiles(rows, n16);
                        const double fill = (double)tiles / num_cu < 1.0 ? (double)tiles / num_cu : 1.0;
                        const double tc = f.thin_tile_cost(k, pc, fill);
                        if (tc < 0) continue;
                        const double cost = (double)ceil_div(tiles, (int64_t)num_cu * pc) * tc;
                        if (cost < want_cost) want_cost = cost, want = k, want_pc = pc;
                    }
                CHECK(c.shape == want && c.per_cu == want_pc && c.cost == want_cost);
            } else {
                ++n_full;
                CHECK(c.shape == full && c.cost == full_cost && c.per_cu == 1);
            }
            CHECK(c.per_cu == 1 || (c.per_cu == 2 && kB[c.shape].waves() == 4));
            CHECK(!(c.shape == 4 && c.per_cu == 2));                           // the per_cu form that does not fit
            n_two += c.per_cu == 2;
            thin_calls = 0;
            const TileChoice d = choose_tile(f, rows, n16, num_cu, false);    // thin disallowed: the full-launch result
            CHECK(d.shape == full && d.cost == full_cost && d.per_cu == 1 && !d.thin && thin_calls == 0);
        }
    CHECK(n_thin > 10 && n_full > 10 && n_two > 0);
    ok("two passes: thin exactly when the full-launch best has fewer tiles than CUs; per_cu 2 only on four-wave entries; thin disallowed = full-launch result");
}

static const TileGeom kFused = {8, 1, 2, 2};          // the one shape a fused kernel form exists for
static void check_pins() {
    const auto f = family_a();
    const int64_t rows = 512;            // 2 tiles of entry 0, 4 of entries 1 and 2 (one round, the cheapest), 8 of entry 3
    const int planner = choose_tile(f, rows, 2, 4).shape;
    CHECK(planner == 1);
    // the last matching entry of the layer wins; other layers' entries and malformed text are skipped
    TilePlan p = plan_tiles(f, rows, 2, 4, {"3:8,1,2,2;5:4,2,2,1;3:4,2,1,1;junk;7:8,1,1,2", 3, -1}, {});
    CHECK(p.n_parts == 1 && p.part[0].shape == 3 && p.pinned && p.part[0].per_cu == 1);
    p = plan_tiles(f, rows, 2, 4, {"3:4,2,1,1;3:8,1,2,2", 3, -1}, {});
    CHECK(p.part[0].shape == 0 && p.pinned);
    ok("force string: the last matching entry of the layer wins");
    // an entry the search never picks (negative cost) can be forced as long as it can run
    p = plan_tiles(f, rows, 2, 4, {"3:4,1,1,1", 3, -1}, {});
    CHECK(p.part[0].shape == 4 && p.pinned && p.part[0].n_mtiles == ceil_div(rows, 64));
    // no table shape / one that cannot run / another layer: the planner's choice, not pinned; behind a good entry they change nothing
    for (const char* s : {"3:9,9,9,9", "3:2,2,8,8", "4:8,1,2,2", "", "3:8,1,2"}) {
        p = plan_tiles(f, rows, 2, 4, {s, 3, -1}, {});
        CHECK(p.n_parts == 1 && p.part[0].shape == planner && !p.pinned);
    }
    p = plan_tiles(f, rows, 2, 4, {nullptr, 3, -1}, {});
    CHECK(p.part[0].shape == planner && !p.pinned);
    p = plan_tiles(f, rows, 2, 4, {"3:8,1,2,2;3:9,9,9,9;3:2,2,8,8", 3, -1}, {});
    CHECK(p.part[0].shape == 0 && p.pinned);
    ok("force string: an entry naming no table shape or one that cannot run leaves the choice as it was");
    // rs_autotune: force_shape before the tuned list, the list before the force string; keyed by the conv rows handed in
    struct { int64_t first; int second; } tuned[] = {{1234, 2}, {6000, 3}, {6000, 0}};
    CHECK(tuned_pick(-1, tuned, 6000) == 3 && tuned_pick(-1, tuned, 1234) == 2 && tuned_pick(-1, tuned, 3000) == -1);
    CHECK(tuned_pick(1, tuned, 6000) == 1 && tuned_pick(0, tuned, 3000) == 0);
    p = plan_tiles(f, rows, 2, 4, {"3:8,1,2,2", 3, tuned_pick(-1, tuned, 6000)}, {});
    CHECK(p.part[0].shape == 3 && p.pinned);
    p = plan_tiles(f, rows, 2, 4, {"3:8,1,2,2", 3, tuned_pick(1, tuned, 6000)}, {});
    CHECK(p.part[0].shape == 1 && p.pinned);
    // a tuned index outside the table or one that cannot run is ignored
    for (int k : {5, 6, 99}) {
        p = plan_tiles(f, rows, 2, 4, {"3:8,1,2,2", 3, k}, {});
        CHECK(p.part[0].shape == 0 && p.pinned);
        p = plan_tiles(f, rows, 2, 4, {nullptr, 3, k}, {});
        CHECK(p.part[0].shape == planner && !p.pinned);
    }
    ok("force_shape beats the tuned list, the list beats the force string; an index that cannot run is ignored");
    // fused: <8,1,2,2>, behind the force string, before the tuned pick; pinned either way
    p = plan_tiles(f, rows, 2, 4, {"3:4,2,1,1", 3, -1, &kFused}, {});
    CHECK(p.part[0].shape == 0 && p.pinned);
    p = plan_tiles(f, rows, 2, 4, {"3:4,2,1,1", 3, 2, &kFused}, {});
    CHECK(p.part[0].shape == 2 && p.pinned);
    ok("fused pins <8,1,2,2> behind the force string and before the tuned pick");
    // any pin: one part at one workgroup per CU, where the search alone gives two per CU or two parts
    const auto b = family_b();
    int n_two = 0;
    for (int64_t r = 1; r <= 6000; r += 37) {
        const TilePlan free_ = plan_tiles(b, r, 2, 8, {}, {true, 5.0, true});
        n_two += free_.n_parts == 2 || free_.part[0].per_cu == 2;
        for (const TilePins& pins : {TilePins{"0:4,1,1,1", 0, -1}, TilePins{nullptr, 0, 3}, TilePins{nullptr, 0, -1, &kFused}}) {
            p = plan_tiles(b, r, 2, 8, pins, {true, 5.0, true});
            CHECK(p.pinned && p.n_parts == 1 && p.part[0].per_cu == 1 && p.part[0].m_base == 0);
            CHECK(p.part[0].shape == (pins.fused ? 0 : 3) && p.part[0].n_mtiles == ceil_div(r, kB[p.part[0].shape].bm()));
            CHECK(p.single_cost == free_.single_cost && p.thin == free_.thin);   // the search's own figures are kept
        }
    }
    CHECK(n_two > 10);
    ok("any pin: exactly one part at one workgroup per CU, no split");
}

// family C: ONE feasible shape, 128-row tiles, one column tile
static const TileGeom kC[] = {{8, 1, 1, 1}, {8, 1, 2, 1}};
static auto family_c(double big_cost) {
    return tile_family(
        2, [](int k) -> const TileGeom& { return kC[k]; }, [=](int k) { return k == 0 ? 60000.0 : big_cost; }, NoThinFit{},
        [](int) { return true; });
}

template <class F>
static void check_split_invariants(const F& f, const TilePlan& p, int64_t rows, int n16, int num_cu, double margin) {
    CHECK(p.n_parts == 2 && !p.pinned);
    const TileGeom &h = f.geom(p.part[0].shape), &t = f.geom(p.part[1].shape);
    const int64_t n_n = ceil_div(n16, h.bnt());
    CHECK(p.part[0].m_base == 0 && p.part[0].per_cu == 1 && p.part[0].n_mtiles >= 1);
    // the head is whole rounds: exactly where the row tiles divide them, else one more row of tiles would start a new round
    const int64_t head_tiles = p.part[0].n_mtiles * n_n, head_rounds = ceil_div(head_tiles, num_cu);
    CHECK(n_n != 1 || head_tiles % num_cu == 0);
    CHECK(head_tiles + n_n > head_rounds * num_cu);
    const int64_t rest = rows - (int64_t)p.part[0].n_mtiles * h.bm();
    CHECK(rest > 0);
    CHECK(p.part[1].m_base == p.part[0].n_mtiles * h.bm());                    // every row unit exactly once
    CHECK(p.part[1].n_mtiles == ceil_div(rest, t.bm()));
    CHECK(p.cost < margin * p.single_cost && p.cost < p.single_cost);
}

static void check_split() {
    const int num_cu = 4;
    // ONE feasible shape: no second shape makes a tail cheaper, and the three row counts around whole rounds
    for (int64_t tiles : {1, 3, num_cu, num_cu + 1, 2 * num_cu - 1, 2 * num_cu, 2 * num_cu + 1})
        for (int64_t rows : {tiles * 128, tiles * 128 - 127}) {
            const TilePlan p = plan_tiles(family_c(-1.0), rows, 1, num_cu, {}, {true, 100.0, false});
            CHECK(p.n_parts == 1 && p.part[0].shape == 0 && p.part[0].n_mtiles == tiles);
        }
    ok("split: one shape alone never splits (a split must be priced below ONE launch, whatever the margin)");
    // two shapes: 256-row tiles at 100000, 128-row tiles at 60000
    const auto f = family_c(100000.0);
    int n_split = 0, n_single = 0;
    for (int64_t rows = 1; rows <= 256 * 40; rows += 61) {
        const TilePlan p = plan_tiles(f, rows, 1, num_cu, {}, {true, 0.97, false});
        bool whole = true, below_round = true;                     // over the shapes the search may use
        for (int k = 0; k < 2; ++k) {
            const int64_t tiles = kC[k].tiles(rows, 1);
            whole = whole && tiles % num_cu == 0;
            below_round = below_round && tiles < num_cu;
        }
        if (whole || below_round) CHECK(p.n_parts == 1);
        if (p.n_parts == 2) {
            ++n_split;
            check_split_invariants(f, p, rows, 1, num_cu, 0.97);
            double c;
            CHECK(p.part[1].shape == brute_single(f, rows - p.part[1].m_base, 1, num_cu, &c) && p.part[1].per_cu == 1);
        } else {
            ++n_single;
            CHECK(p.cost == p.single_cost);
        }
        // the policy that forbids splitting: one part, the search's shape
        const TilePlan q = plan_tiles(f, rows, 1, num_cu, {}, {false, 100.0, true});
        CHECK(q.n_parts == 1 && q.part[0].shape == choose_tile(f, rows, 1, num_cu).shape && q.cost == q.single_cost);
        CHECK(plan_tiles(f, rows, 1, num_cu, {}, {}).n_parts == 1);            // the default policy forbids it too
    }
    CHECK(n_split > 10 && n_single > 10);
    ok("split: parts cover every row once, the head is whole rounds, priced below margin x single; none at whole rounds or below one; never where forbidden");
    // by hand: 1280 rows = 5 tiles of 256 (two rounds, 200000) or 10 of 128 (three rounds, 180000: the single launch).  Head: one
    // round of four 256-row tiles, tail 256 rows as two 128-row tiles: 100000 + 60000 + 6000 = 166000 < 0.97 x 180000 = 174600
    TilePlan p = plan_tiles(f, 1280, 1, num_cu, {}, {true, 0.97, false});
    CHECK(p.n_parts == 2 && p.single_cost == 180000.0 && p.cost == 166000.0);
    CHECK(p.part[0].shape == 1 && p.part[0].n_mtiles == 4 && p.part[1].shape == 0 && p.part[1].m_base == 1024 && p.part[1].n_mtiles == 2);
    // ... and not below 0.92 x 180000 = 165600: a margin override is honoured, both ways
    p = plan_tiles(f, 1280, 1, num_cu, {}, {true, 0.92, false});
    CHECK(p.n_parts == 1 && p.part[0].shape == 0 && p.part[0].n_mtiles == 10 && p.cost == 180000.0);
    p = plan_tiles(f, 1280, 1, num_cu, {}, {true, 0.93, false});
    CHECK(p.n_parts == 2 && p.cost == 166000.0);
    ok("split: the worked example; a margin override is honoured on both sides of the price");
    // the tail chosen again with the thin fit: its own shape and workgroups per CU, the head at one per CU
    const auto b = family_b();
    int n_re = 0, n_differs = 0;
    for (int n16 = 1; n16 <= 3; ++n16)
        for (int64_t rows = 1; rows <= 9000; rows += 29) {
            const TilePlan as_priced = plan_tiles(b, rows, n16, 8, {}, {true, 5.0, false});
            const TilePlan again = plan_tiles(b, rows, n16, 8, {}, {true, 5.0, true});
            CHECK(as_priced.n_parts == again.n_parts && as_priced.cost == again.cost);
            if (again.n_parts != 2) continue;
            ++n_re;
            check_split_invariants(b, again, rows, n16, 8, 5.0);
            check_split_invariants(b, as_priced, rows, n16, 8, 5.0);
            CHECK(again.part[0].shape == as_priced.part[0].shape && again.part[0].n_mtiles == as_priced.part[0].n_mtiles);
            const int64_t rest = rows - again.part[1].m_base;
            const TileChoice t = choose_tile(b, rest, n16, 8);
            CHECK(again.part[1].shape == t.shape && again.part[1].per_cu == t.per_cu);
            double c;
            CHECK(as_priced.part[1].shape == brute_single(b, rest, n16, 8, &c) && as_priced.part[1].per_cu == 1);
            n_differs += again.part[1].shape != as_priced.part[1].shape || again.part[1].per_cu == 2;
        }
    CHECK(n_re > 10 && n_differs > 0);
    ok("split: a tail chosen again takes the thin fit's shape and workgroups per CU; as priced it keeps the split's");
}

static void check_with_walk() {
    // a part's numbers are what plan_walk takes: the tile grid of the launch and its first row unit
    const auto f = family_c(100000.0);
    const TilePlan p = plan_tiles(f, 1280, 1, 8, {}, {});
    const TileGeom& g = f.geom(p.part[0].shape);
    WalkArgs w = plan_walk(p.part[0].n_mtiles, 1, 8, 8, g.bm(), 3.0 * g.bn(), 0);
    w.m_base = p.part[0].m_base;
    CHECK(w.n_mtiles == p.part[0].n_mtiles && w.q_total == p.part[0].n_mtiles && w.m_base == 0);
    ok("a part feeds tile_walk.hpp: plan_walk");
}

int main() {
    check_geometry();
    check_search();
    check_two_pass();
    check_pins();
    check_split();
    check_with_walk();
    printf("all %d cases passed\n", n_cases);
    return 0;
}
