// Stand-alone check of the LDS rows of the tiled F(4,3) kernel (csrc/conv_wino4.hip) through the host half of
// csrc/conv_wino_device.hpp: wino_pitch, wino_swizzle, wino_word, wino_buf_floats.  The kernel's address arithmetic - the
// staging map of store_unit, the lane constants a_rd / a_rd1 / b_rd and the slot offsets - is written out again below with
// the kernel's names, and every read and write pattern is walked through it for chunks of 16 (pitch 18) and of 20 (pitch
// 22, or, for the one tile that does not fit the LDS that way, pitch 20 with the k index swizzled by bit 3 of the row; the
// swizzled form is walked for every table shape, whether the kernel uses it there or not).  No HIP header, no GPU.  One line per case; the first failure prints FAIL and
// exits 1.  tests/test_wino_lds_cpu.py builds and runs it.
#include "conv_wino_device.hpp"
#include "tile_plan.hpp"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace rs;

static int n_cases = 0;
#define CHECK(cond)                                                                \
    do {                                                                           \
        if (!(cond)) {                                                             \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);                 \
            exit(1);                                                               \
        }                                                                          \
    } while (0)
static void ok(const char* what, int kc) { printf("ok %2d kc %d: %s\n", ++n_cases, kc, what); }

constexpr int M = 4, NC = 6;

// a ds_read_b32 serves lanes 0-31 and 32-63 as two groups, bank = word mod 32: the 32 words of a group on 32 banks
static bool conflict_free(const int (&word)[64]) {
    for (int g = 0; g < 2; ++g) {
        unsigned seen = 0;
        for (int l = 32 * g; l < 32 * g + 32; ++l) {
            if (word[l] < 0) return false;
            seen |= 1u << (word[l] & 31);
        }
        if (seen != 0xffffffffu) return false;
    }
    return true;
}

// ---- the kernel's tile constants (WinoTile<4, BG, BN, KC, kThreads>) and addresses, names as in conv_wino4.hip -------------
struct Tile {
    int KC, BG, BN, kThreads;
    bool UP;            // unpadded, swizzled rows (the kernel: wino_unpadded)
    int S() const { return wino_pitch(UP, KC); }
    int KQ() const { return KC / 4; }
    int PL() const { return (BG + 1) * S(); }
    int A_ELEMS() const { return M * PL(); }
    int BUF() const { return (M * (BG + 1) + NC * BN) * S(); }
    int RPT() const { return wino_stage_rows(UP, M, KC, kThreads, BG); }
    int A_ROWS() const { return M * BG + 2; }
    int A_PER() const { return (A_ROWS() + RPT() - 1) / RPT(); }
    int NPP() const { return wino_stage_cols(UP, M, KC, kThreads); }
    int B_PER() const { return (BN + NPP() - 1) / NPP(); }

    // store_unit, input slab: word of float e (0 .. 3) of thread tid's unit u, or -1 where the thread stores nothing
    int a_store(int tid, int u, int e, int* slab_row, int* chan) const {
        const int a_row = tid / KQ(), a_c4 = tid - a_row * KQ();
        if (a_row >= RPT() || a_row + u * RPT() >= A_ROWS()) return -1;
        const int a_st = (a_row & 3) * PL() + (a_row >> 2) * S() + 4 * a_c4;
        const int d = a_st + u * (RPT() / 4) * S();                      // uint2* d: d[0] at +0, d[1] at +2
        int h = UP ? (((a_row >> 2) + u * (RPT() / 4)) >> 3) & 1 : 0;
        const int a_h0 = (a_row >> 5) & 1;
        if (UP && RPT() % 32 == 0) {                              // the kernel's form without arithmetic per unit
            if (h != (a_h0 ^ ((u * (RPT() / 32)) & 1))) return -2;
            h = a_h0 ^ ((u * (RPT() / 32)) & 1);
        }
        *slab_row = a_row + u * RPT();
        *chan = 4 * a_c4 + e;
        return d + 2 * ((e >> 1) ^ h) + (e & 1);                         // floats 0, 1 -> d[h], floats 2, 3 -> d[h ^ 1]
    }
    // store_unit, weight slab
    int b_store(int tid, int v, int e, int* comp, int* n, int* chan) const {
        const int b_n = tid / (NC * KQ()), b_rem = tid - b_n * (NC * KQ());
        if (b_n >= NPP() || b_n + v * NPP() >= BN) return -1;
        const int b_st = A_ELEMS() + ((b_rem / KQ()) * BN + b_n) * S() + 4 * (b_rem % KQ());
        const int d = b_st + v * NPP() * S();
        int h = UP ? ((b_n + v * NPP()) >> 3) & 1 : 0;
        const int b_h0 = (b_n >> 3) & 1;
        if (UP && NPP() % 16 == 0) {
            if (h != b_h0) return -2;
            h = b_h0;
        }
        *comp = b_rem / KQ();
        *n = b_n + v * NPP();
        *chan = 4 * (b_rem % KQ()) + e;
        return d + 2 * ((e >> 1) ^ h) + (e & 1);
    }
    // fragment reads of lane (r, kq) of wave (wm, wn): raw input d_k of sub-tile i at k-step st, weight fragment of component
    // comp and sub-tile j.  MT / NT only place the wave in the tile
    int a_read(int wm, int MT, int r, int kq, int i, int k, int st) const {
        const int a_rd = (wm * 16 * MT + r) * S() + (kq ^ wino_swizzle(UP, r));
        const int a_rd1 = (wm * 16 * MT + r) * S() + (kq ^ wino_swizzle(UP, r + 1));
        return (k < 4 ? a_rd : a_rd1) + (k & 3) * PL() + (i * 16 + (k >> 2)) * S() + 4 * st;
    }
    int b_read(int wn, int NT, int r, int kq, int comp, int j, int st) const {
        const int b_rd = A_ELEMS() + (wn * 16 * NT + r) * S() + (kq ^ wino_swizzle(UP, r));
        return b_rd + (comp * BN + j * 16) * S() + 4 * st;
    }
};

// ---- 1. the helper itself: every 32-lane group of a fragment read on 32 banks, whatever the first row ---------------------
static void check_fragment_banks(int kc, bool up) {
    const int S = wino_pitch(up, kc);
    CHECK(S == (up ? kc : kc + 2));
    for (int bu : {16, 32, 64, 128}) {
        const int PL = (bu + 1) * S;
        for (int k = 0; k < 6; ++k)
            for (int row0 = 0; row0 < 32; ++row0)
                for (int st = 0; st < kc / 4; ++st) {
                    int word[64];
                    for (int l = 0; l < 64; ++l) word[l] = (k & 3) * PL + wino_word(up, kc, row0 + (l & 15) + (k >> 2), 4 * st + (l >> 4));
                    CHECK(conflict_free(word));
                }
    }
    ok(up ? "unpadded, A fragment: each k, first row 0 .. 31, each k-step: 32 banks per 32-lane group"
          : "padded, A fragment: each k, first row 0 .. 31, each k-step: 32 banks per 32-lane group", kc);
    for (int bn = 32; bn <= 96; bn += 16)
        for (int comp = 0; comp < NC; ++comp)
            for (int j = 0; j < bn / 16; ++j)
                for (int st = 0; st < kc / 4; ++st)
                    for (int a_elems : {M * 17 * S, M * 129 * S}) {
                        int word[64];
                        for (int l = 0; l < 64; ++l) word[l] = a_elems + wino_word(up, kc, comp * bn + j * 16 + (l & 15), 4 * st + (l >> 4));
                        CHECK(conflict_free(word));
                    }
    ok(up ? "unpadded, B fragment: each component, j, BN 32 .. 96, each k-step: 32 banks per 32-lane group"
          : "padded, B fragment: each component, j, BN 32 .. 96, each k-step: 32 banks per 32-lane group", kc);
}

// ---- 2. one tile of the kernel: what store_unit writes is what the slot loop reads -----------------------------------------
struct Cell {
    int row, chan;      // input: slab row, channel; weights: comp * BN + n, channel
};

static void check_tile(const Tile& t, int WM, int WN, int MT, int NT) {
    CHECK(t.BG == WM * 16 * MT && t.BN == WN * 16 * NT && t.kThreads == 64 * WM * WN);
    CHECK(t.UP != wino_unpadded(M, t.BG, t.BN, t.KC) || t.BUF() == wino_buf_floats(M, t.BG, t.BN, t.KC));
    std::vector<Cell> at(t.BUF(), Cell{-1, -1});
    int stored = 0;
    // both halves of every unit of an item, every thread
    for (int tid = 0; tid < t.kThreads; ++tid) {
        for (int u = 0; u < t.A_PER(); ++u)
            for (int e = 0; e < 4; ++e) {
                int s, c;
                const int w = t.a_store(tid, u, e, &s, &c);
                CHECK(w != -2);
                if (w < 0) continue;
                CHECK(w < t.A_ELEMS() && at[w].row < 0);                       // no two (row, channel) pairs share a word
                CHECK(w == (s & 3) * t.PL() + wino_word(t.UP, t.KC, s >> 2, c));  // the helper's word of plane s & 3, index s >> 2
                at[w] = Cell{s, c};
                ++stored;
            }
        for (int v = 0; v < t.B_PER(); ++v)
            for (int e = 0; e < 4; ++e) {
                int comp, n, c;
                const int w = t.b_store(tid, v, e, &comp, &n, &c);
                CHECK(w != -2);
                if (w < 0) continue;
                CHECK(w >= t.A_ELEMS() && w < t.BUF() && at[w].row < 0);
                CHECK(w == t.A_ELEMS() + wino_word(t.UP, t.KC, comp * t.BN + n, c));
                at[w] = Cell{comp * t.BN + n, c};
                ++stored;
            }
    }
    CHECK(stored == (t.A_ROWS() + NC * t.BN) * t.KC);                          // every slab row and weight row, every channel
    // every fragment read of every wave: the channel and row the MFMA expects, on 32 banks per group
    for (int wave = 0; wave < WM * WN; ++wave) {
        const int wm = wave % WM, wn = wave / WM;
        for (int st = 0; st < t.KQ(); ++st) {
            for (int i = 0; i < MT; ++i)
                for (int k = 0; k < 6; ++k) {
                    int word[64];
                    for (int l = 0; l < 64; ++l) {
                        const int r = l & 15, kq = l >> 4;
                        const int w = word[l] = t.a_read(wm, MT, r, kq, i, k, st);
                        CHECK(w >= 0 && w < t.A_ELEMS());
                        // raw input d_k of group g is slab row 4 g + k, channel 4 st + kq
                        CHECK(at[w].row == 4 * ((wm * MT + i) * 16 + r) + k && at[w].chan == 4 * st + kq);
                    }
                    CHECK(conflict_free(word));
                }
            for (int comp = 0; comp < NC; ++comp)
                for (int j = 0; j < NT; ++j) {
                    int word[64];
                    for (int l = 0; l < 64; ++l) {
                        const int r = l & 15, kq = l >> 4;
                        const int w = word[l] = t.b_read(wn, NT, r, kq, comp, j, st);
                        CHECK(w >= t.A_ELEMS() && w < t.BUF());
                        CHECK(at[w].row == comp * t.BN + (wn * NT + j) * 16 + r && at[w].chan == 4 * st + kq);
                    }
                    CHECK(conflict_free(word));
                }
        }
    }
}

static int n_kernel = 0;       // tiles walked in the form the kernel runs them in

static void check_tiles(int kc, bool up) {
    // the shape table of conv_wino4.hip: eight waves, then four
    static const int shapes[][4] = {{8, 1, 1, 2}, {8, 1, 1, 3}, {8, 1, 1, 4}, {8, 1, 1, 5}, {8, 1, 1, 6}, {4, 2, 1, 2}, {4, 2, 1, 3},
                                    {4, 2, 1, 4}, {4, 2, 2, 2}, {2, 4, 1, 2}, {2, 4, 1, 3}, {2, 4, 1, 4}, {2, 4, 2, 2}, {4, 2, 1, 1},
                                    {2, 4, 1, 1}, {4, 1, 1, 1}, {2, 2, 1, 1}, {1, 4, 1, 1}, {4, 1, 1, 2}, {2, 2, 1, 2}, {1, 4, 1, 2},
                                    {4, 1, 1, 3}, {2, 2, 1, 3}};
    int n = 0;
    for (const auto& s : shapes) {
        const Tile t{kc, s[0] * 16 * s[2], s[1] * 16 * s[3], 64 * s[0] * s[1], up};
        if (2 * (size_t)t.BUF() * sizeof(float) > kConvLdsBudget) continue;
        check_tile(t, s[0], s[1], s[2], s[3]);
        n_kernel += up == wino_unpadded(M, t.BG, t.BN, kc);
        ++n;
    }
    CHECK(n >= 16);
    ok(up ? "unpadded, every table shape that fits: stores and reads meet word for word, no word shared, reads on 32 banks"
          : "padded, every table shape that fits: stores and reads meet word for word, no word shared, reads on 32 banks", kc);
}

static void check_budget() {
    CHECK(kConvLdsBudget == 160 * 1024);
    // 512 x 80 at chunks of 20: 175 296 B padded, so it is the unpadded tile and fits; 512 x 96 at 20 fits neither way
    // (174 720 B unpadded) and stays padded
    CHECK(wino_unpadded(4, 128, 80, 20) && 2 * (size_t)wino_buf_floats(4, 128, 80, 20) * 4 == 159360 && 159360 <= kConvLdsBudget);
    CHECK(2 * 4 * (4 * 129 + 6 * 96) * 20 == 174720 && 174720 > kConvLdsBudget && !wino_unpadded(4, 128, 96, 20));
    CHECK(2 * (size_t)wino_buf_floats(4, 128, 96, 20) * 4 == 2 * (4 * 129 + 6 * 96) * 22 * 4);
    CHECK(!wino_unpadded(4, 64, 128, 20) && !wino_unpadded(4, 32, 256, 20));           // too large either way as well
    // every tile that fits padded stays padded: chunks of 16 always, 512 x 64 at 20
    CHECK(!wino_unpadded(4, 128, 96, 16) && 2 * (size_t)wino_buf_floats(4, 128, 96, 16) * 4 == 2 * (4 * 129 + 6 * 96) * 18 * 4);
    CHECK(2 * (size_t)wino_buf_floats(4, 128, 96, 16) * 4 <= kConvLdsBudget);
    CHECK(!wino_unpadded(4, 128, 64, 20) && 2 * (size_t)wino_buf_floats(4, 128, 64, 20) * 4 == 2 * (4 * 129 + 6 * 64) * 22 * 4);
    CHECK(!wino_unpadded(4, 128, 80, 16) && !wino_unpadded(4, 64, 128, 16));
    // F(2,3) keeps kc + 2 at every chunk, and no swizzle
    for (int kc : {16, 20, 24})
        for (int bn = 16; bn <= 256; bn += 16)
            CHECK(!wino_unpadded(2, 256, bn, kc) && wino_buf_floats(2, 256, bn, kc) == (2 * 257 + 4 * bn) * (kc + 2));
    for (int row = 0; row < 64; ++row) {
        CHECK(wino_swizzle(false, row) == 0 && wino_word(false, 20, row, 3) == 22 * row + 3);
        CHECK(wino_swizzle(true, row) == 2 * ((row >> 3) & 1) && wino_word(true, 20, row, 1) == 20 * row + (1 ^ wino_swizzle(true, row)));
    }
    CHECK(n_kernel >= 2 * 16);                                                 // both chunks, in the kernel's own form
    printf("ok %2d the LDS budget: 512 x 80 at chunks of 20 is the unpadded tile and fits, 512 x 96 fits at 16 only; F(2,3) keeps kc + 2\n", ++n_cases);
}

int main() {
    for (int kc : {16, 20}) {
        check_fragment_banks(kc, false);
        check_tiles(kc, false);
    }
    check_fragment_banks(20, true);
    check_tiles(20, true);
    check_budget();
    printf("all %d cases passed\n", n_cases);
    return 0;
}
