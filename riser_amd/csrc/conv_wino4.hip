// K3w4 (fp32, Winograd F(4,3)): ConvNet block i >= 1 for the wide late layers.
//
//   Conv1d(C_in -> C_out, k=3, stride 1, zero 'same' padding, bias) -> ReLU -> MaxPool1d(2,2)
//   (riser/nets/cnn.py:52-65, depth 1)
//
// F(4,3) produces FOUR consecutive conv outputs y[4G .. 4G+3] (two pooling pairs) from the six inputs
// d0..d5 = x[4G-1 .. 4G+4] with 6 multiplications per input channel instead of 12 (F(2,3): 8), i.e. half
// the matrix-pipe work of the direct lowering:
//     V = B^T d    B^T = [ 4  0 -5  0  1  0 ]      U = G g    G = [ 1/4    0     0  ]      y = A^T (U . V)
//                        [ 0 -4 -4  1  1  0 ]                     [-1/6  -1/6  -1/6 ]      A^T = [ 1 1  1 1  1 0 ]
//                        [ 0  4 -4 -1  1  0 ]                     [-1/6   1/6  -1/6 ]            [ 0 1 -1 2 -2 0 ]
//                        [ 0 -2 -1  2  1  0 ]                     [ 1/24  1/12  1/6 ]            [ 0 1  1 4  4 0 ]
//                        [ 0  2 -1 -2  1  0 ]                     [ 1/24 -1/12  1/6 ]            [ 0 1 -1 8 -8 1 ]
//                        [ 0  4  0 -5  0  1 ]                     [  0     0     1  ]
// (Lavin & Gray's transform set).  The layer is SIX GEMMs M_j[G][n] = sum_c V_j[G][c] * U_j[n][c] over
// groups G of four input rows; the epilogue forms y0..y3, the two pooled values max(y0,y1), max(y2,y3),
// + bias, ReLU, length mask, and stores two 16-byte pieces per lane and sub-tile.
// fp32 throughout; measured on the CPU in numpy the probabilities stay within 9e-6 of an fp64 evaluation
// (direct fp32: 6e-6), see tests/test_oracle_golden.py and tests/test_gpu_wino.py.
//
// Structure, data layout, staging (buffer loads, pass-major unit map), tile walk and MFMA orientation are
// those of conv_wino.hip; what differs: the input slab is split into FOUR planes by (row mod 4) so that the
// six inputs of group G are rows G, G+1 of the planes (unit lane stride, pitch KC + 2: conflict-free
// ds_read_b32), the weight slab has six components, a slot = (k-step, component) carries MT * NT MFMAs
// with MT * NT <= 6 (6 x 4 accumulator registers per 16 x 16 sub-tile), and LDS capacity limits the channel
// chunk: 16 or 20, and at 20 the tile.  512 x 64 holds chunks of 20 at the pitch of 22 floats; 512 x 80 would need
// 175 296 B and runs them on UNPADDED rows (159 360 B) with the k index swizzled by bit 3 of the row, which keeps
// every fragment read on 32 banks (conv_wino_device.hpp: wino_unpadded, wino_swizzle; tests/wino_lds_check.cpp);
// 512 x 96 (174 720 B even so) runs chunks of 16 only.  A layer of 100 padded channels is 5 chunks of 20 instead of
// 7 of 16 (112 K steps, 12 of them zeros); the MFMA order per accumulator is channels ascending whatever the chunk, so
// the bits do not depend on it.  Used for the layers where the matrix pipe is the bound (chosen in rs_model_create).
#include "conv_wino_host.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <utility>

// schedule knobs of the build (DESIGN_HISTORY.md): the defaults are the measured optima
#ifndef RS_UF_AHEAD
#define RS_UF_AHEAD 1
#endif
#ifndef RS_W4_DIST
#define RS_W4_DIST 6
#endif
#ifndef RS_W4_PRIO
#define RS_W4_PRIO 0
#endif

namespace rs {
namespace {

// the thin shapes' slots (one or two MFMAs): look-ahead of the weight fragments in slots x MFMAs per slot, the component
// slot that reads the raw rows of the next k-step and the first one that transforms them
constexpr int kAheadThin = 4, kReadThin = 0, kXformThin = 5;

// WinoArgs (conv_wino_host.hpp) without the fused layer-0 members, and with one member no kernel reads: one record for both
// kernels moved the SGPR spill counts of 49 of these 56 kernels (24 up, by 1 to 5: profiles/f32_device_checks.txt), so the
// layout stays; launch_wino fills both
struct Wino4Args {
    const float* x;
    const float* w;        // packed [n_alloc][nch][6][kc] (U0..U5), zero rows beyond c_out
    const float* bias;     // [n_alloc]
    float* y;
    const int32_t* len;
    unsigned x_bytes, w_bytes, y_bytes, y_row_bytes, len_bytes, bias_bytes;
    int rows_in;           // B * P_in
    int rows_out;          // B * P_out (pooled rows)
    int n_groups;          // ceil(rows_in / 4)
    int P_out;
    float inv_P_out;
    int cp_in, cp_out;
    int nch;
    int shift_out;
    WalkArgs walk;         // tile grid, order and dead-tile flag (tile_walk.hpp)
};

// DEEP: the staging loads of an item are issued ONE ITEM earlier (they stay in registers across the barrier and go to LDS
// during the next item): a thin launch (a few dozen tiles of the smallest shapes) has ~1.5 k cycles of MFMAs per item, far
// less than the trip to L2 / HBM that the six-slot distance of the default schedule covers.  Same MFMA sequence per
// accumulator, so the bits do not change.
template <int WM, int WN, int MT, int NT, int KCT, bool DEEP = false>
__global__ __launch_bounds__(512) void conv_wino4_kernel(const Wino4Args a) {   // 512 for the four-wave shapes too: a bound of 256 makes
                                                                                  // the compiler keep the accumulators in AGPRs, with
                                                                                  // a copy in and out per item
    // 8 waves (2 per SIMD), or 4 (1 per SIMD) for launches with fewer tiles than CUs: the VALU work of a wave (input
    // transform, staging, walk) and the f32-input MFMAs of its SIMD neighbour do not overlap, so a thin launch is faster
    // with its waves spread over twice the CUs
    static_assert(WM * WN == 8 || WM * WN == 4, "8 or 4 waves per workgroup");
    static_assert(KCT == 16 || KCT == 20, "channel chunk");
    constexpr int kThreads = 64 * WM * WN;
    constexpr int BG = WM * 16 * MT;                    // groups (of 4 conv rows = 2 pooled rows) per tile
    constexpr int BN = WN * 16 * NT;
    using T = WinoTile<4, BG, BN, KCT, kThreads>;       // planes by input row mod 4, staging passes (conv_wino_device.hpp)
    constexpr int NC = T::NC, S = T::S, KQ = T::KQ, PL = T::PL, A_ELEMS = T::A_ELEMS, BUF = T::BUF, RPT = T::RPT,
                  A_ROWS = T::A_ROWS, A_PER = T::A_PER, NPP = T::NPP, B_PER = T::B_PER;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 15, kq = lane >> 4;

    // ---- staging map (see conv_wino.hip) -----------------------------------------------------------------
    // slab row s (global input row 4*m0g - 1 + s) lives in plane s & 3 at index s >> 2; a thread's rows
    // a_row + u * RPT keep their plane because RPT is a multiple of 4
    const int a_row = tid / KQ, a_c4 = tid - a_row * KQ;
    const bool a_act = a_row < RPT;
    const int b_n = tid / (NC * KQ), b_rem = tid - b_n * (NC * KQ);
    const bool b_act = b_n < NPP;
    const int a_st = (a_row & 3) * PL + (a_row >> 2) * S + 4 * a_c4;                     // + u * (RPT/4) * S
    const int b_st = A_ELEMS + ((b_rem / KQ) * BN + b_n) * S + 4 * (b_rem % KQ);         // + u * NPP * S
    const int a_h0 = (a_row >> 5) & 1, b_h0 = (b_n >> 3) & 1;      // swizzled rows: bit 3 of the thread's first plane index / of its n
    const unsigned a_tb = (unsigned)(a_row * a.cp_in + 4 * a_c4) * 4u;
    const unsigned b_tb = (unsigned)(b_n * a.nch * NC * KCT + 4 * b_rem) * 4u;
    const unsigned a_step = (unsigned)(RPT * a.cp_in) * 4u;
    const unsigned b_step = (unsigned)(NPP * a.nch * NC * KCT) * 4u;
    const __amdgpu_buffer_rsrc_t rs_x = buffer_rsrc(a.x, a.x_bytes), rs_w = buffer_rsrc(a.w, a.w_bytes),
                                 rs_y = buffer_rsrc(a.y, a.y_bytes), rs_len = buffer_rsrc(a.len, a.len_bytes),
                                 rs_bias = buffer_rsrc(a.bias, a.bias_bytes);
    const const_len_ptr clen = as_const_len(a.len);

    u32x4 ra[A_PER], rb[B_PER];
    unsigned a_ib = kOob, b_ib = kOob;
    auto item_offsets = [&](int m0g, int n0, int c, bool live) {
        const bool a_ok = live && a_act && c * KCT + 4 * a_c4 < a.cp_in;
        a_ib = a_ok ? a_tb + (unsigned)((4 * m0g - 1) * a.cp_in + c * KCT) * 4u : kOob;   // row -1 wraps out of range
        b_ib = (live && b_act) ? b_tb + (unsigned)((n0 * a.nch + c) * NC * KCT) * 4u : kOob;
#ifdef RS_ABL_NOLOAD                                    // timing experiment only: every staging load out of range
        a_ib = kOob;
        b_ib = kOob;
#endif
    };
    auto load_unit = [&](auto U) {
        constexpr int u = decltype(U)::value;
        if constexpr (u < A_PER) {
            unsigned off = a_ib + (unsigned)u * a_step;
            if constexpr ((u + 1) * RPT > A_ROWS) off = (a_row + u * RPT < A_ROWS) ? off : kOob;
            ra[u] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0);
        } else {
            constexpr int v = u - A_PER;
            unsigned off = b_ib + (unsigned)v * b_step;
            if constexpr ((v + 1) * NPP > BN) off = (b_n + v * NPP < BN) ? off : kOob;
            rb[v] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, off, 0, 0);
        }
    };
    auto store_unit = [&](auto U, float* buf) {
        constexpr int u = decltype(U)::value;
        if constexpr (u < A_PER) {
            bool act = a_act;
            if constexpr ((u + 1) * RPT > A_ROWS) act = act && (a_row + u * RPT < A_ROWS);
#ifdef RS_ABL_NOLDSW
            asm volatile("" ::"v"(ra[u].x), "v"(ra[u].y), "v"(ra[u].z), "v"(ra[u].w));
            act = false;
#endif
            if (act) {
                uint2* d = reinterpret_cast<uint2*>(buf + a_st + u * (RPT / 4) * S);
                if constexpr (T::SWZ) {                // the halves change places in the rows with bit 3 set
                    int h = (((a_row >> 2) + u * (RPT / 4)) >> 3) & 1;
                    if constexpr (RPT % 32 == 0) h = a_h0 ^ ((u * (RPT / 32)) & 1);   // the same, without arithmetic per unit
                    d[h] = make_uint2(ra[u].x, ra[u].y);
                    d[h ^ 1] = make_uint2(ra[u].z, ra[u].w);
                } else {
                    d[0] = make_uint2(ra[u].x, ra[u].y);
                    d[1] = make_uint2(ra[u].z, ra[u].w);
                }
            }
        } else {
            constexpr int v = u - A_PER;
            bool act = b_act;
            if constexpr ((v + 1) * NPP > BN) act = act && (b_n + v * NPP < BN);
#ifdef RS_ABL_NOLDSW
            asm volatile("" ::"v"(rb[v].x), "v"(rb[v].y), "v"(rb[v].z), "v"(rb[v].w));
            act = false;
#endif
            if (act) {
                uint2* d = reinterpret_cast<uint2*>(buf + b_st + v * NPP * S);
                if constexpr (T::SWZ) {                // row = component * BN + n: bit 3 is n's
                    int h = ((b_n + v * NPP) >> 3) & 1;
                    if constexpr (NPP % 16 == 0) h = b_h0;
                    d[h] = make_uint2(rb[v].x, rb[v].y);
                    d[h ^ 1] = make_uint2(rb[v].z, rb[v].w);
                } else {
                    d[0] = make_uint2(rb[v].x, rb[v].y);
                    d[1] = make_uint2(rb[v].z, rb[v].w);
                }
            }
        }
    };

    // ---- tile walk (tile_walk.hpp), tiles counted in groups -----------------------------------------------
    const int tiles = a.walk.q_total;
    auto tile_origin = [&](int q, int& tm0, int& tn0) -> bool {
        int mi, nt_;
        const bool ok = walk_tile(a.walk, q, mi, nt_);
        tm0 = a.walk.m_base + mi * BG;
        tn0 = nt_ * BN;
        return ok;
    };
    TileWalk walk;
    auto order_index = [&]() { return walk.next_index(a.walk); };
    auto next_live = [&]() {
        int q = order_index();
        while (q < tiles) {
            int tm0, tn0;
            const bool valid = tile_origin(q, tm0, tn0);
            if (valid) {
                if (!a.walk.check_dead) break;
                const int pr0 = 2 * tm0;                                  // first pooled row of the tile
                const int b = pr0 / a.P_out;
                const int t0 = pr0 - b * a.P_out;
                if (!(b < a.rows_out / a.P_out && t0 + 2 * BG <= a.P_out && t0 >= (clen[b] >> a.shift_out))) break;
                zero_fill_tile<BN>(a.y, pr0, 2 * BG, tn0, a.rows_out, a.cp_out);
            }
            q = order_index();
        }
        return q;
    };
    int o = next_live();
    if (o >= tiles) return;

    f32x4 acc[MT][NT][NC];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int q = 0; q < NC; ++q) acc[i][j][q] = (f32x4){0.f, 0.f, 0.f, 0.f};

    int c = 0;
    int m0, n0;
    tile_origin(o, m0, n0);
    item_offsets(m0, n0, 0, true);
    static_for<A_PER + B_PER>([&](auto U) { load_unit(U); });
    static_for<A_PER + B_PER>([&](auto U) { store_unit(U, lds); });
    // the item after (oo, cc) of this workgroup's walk; oo >= tiles: none
    auto advance = [&](int& oo, int& cc, int& mm, int& nn) {
        if (oo >= tiles) return;
        if (++cc == a.nch) {
            cc = 0;
            oo = next_live();
            if (oo < tiles) tile_origin(oo, mm, nn);
        }
    };
    int o1 = o, c1 = 0, m1 = m0, n1 = n0;              // DEEP: the next item, already on its way in ra / rb
    if constexpr (DEEP) {
        advance(o1, c1, m1, n1);
        item_offsets(m1, n1, c1, o1 < tiles);
        static_for<A_PER + B_PER>([&](auto U) { load_unit(U); });
    }
    __syncthreads();
    int buf = 0;

    // unpadded rows (512 x 80 at chunks of 20): the k lane is swizzled by bit 3 of the row it reads (wino_swizzle).  Raw input
    // d_k of a lane's group is row r + (k >> 2) (+ multiples of 16), so d4 and d5 go by bit 3 of r + 1: two lane constants for
    // the input fragments, one for the weights'; the k offsets of the slots are multiples of 4 and pass through the XOR
    const int a_rd = (wm * 16 * MT + r) * S + (kq ^ T::swz(r));          // + (k & 3) * PL + (i * 16 + (k >> 2)) * S + c0
    const int a_rd1 = (wm * 16 * MT + r) * S + (kq ^ T::swz(r + 1));     // the same for k = 4, 5
    const int b_rd = A_ELEMS + (wn * 16 * NT + r) * S + (kq ^ T::swz(r));   // + (comp * BN + j * 16) * S + c0

    while (true) {
        int nc = c + 1, no = o;
        int nm0 = m0, nn0 = n0;
        int o2 = o1, c2 = c1, m2 = m1, n2 = n1;
        if constexpr (DEEP) {
            nc = c1, no = o1, nm0 = m1, nn0 = n1;
            advance(o2, c2, m2, n2);
        } else if (nc == a.nch) {
            nc = 0;
            no = next_live();
        }
        const bool has_next = no < tiles;
        if constexpr (!DEEP)
            if (has_next && nc == 0) tile_origin(no, nm0, nn0);
        const float* Ab = lds + buf * BUF + a_rd;
        const float* Ab1 = T::SWZ ? lds + buf * BUF + a_rd1 : Ab;
        const float* Bb = lds + buf * BUF + b_rd;
        float* nbuf = lds + (buf ^ 1) * BUF;
        if constexpr (DEEP)
            item_offsets(m2, n2, c2, o2 < tiles);
        else
            item_offsets(nm0, nn0, nc, has_next);

        constexpr int NSLOTS = NC * KQ;                // slot = (k-step, component): MT * NT MFMAs
        constexpr int UNITS = A_PER + B_PER;
        constexpr int DIST = RS_W4_DIST;               // slots between a unit's load and its LDS write
        constexpr int SPAN = NSLOTS - DIST;
        float dr[MT][6];                               // raw inputs d0..d5 of the lane's groups (next k-step)
        // a slot of the thin shapes is one or two MFMAs (32 / 64 cycles): an LDS read issued one slot ahead is not back
        // in time, so their weight fragments are read four (two) slots ahead, the raw rows at the first slot of a
        // k-step and transformed behind its last
        constexpr bool THIN = MT * NT <= 2;
        constexpr int AH = THIN ? (kAheadThin + MT * NT - 1) / (MT * NT) : RS_UF_AHEAD;   // slots of look-ahead of the weight-fragment reads
        constexpr int RD = THIN ? kReadThin : 1, XF0 = THIN ? kXformThin : 3;
        float uf[AH + 1][NT];                          // weight fragments, ring over the slots in flight
        float v[2][MT][NC];                            // transformed inputs: this k-step / the next one
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int k = 0; k < 6; ++k) dr[i][k] = (k < 4 ? Ab : Ab1)[(k & 3) * PL + (i * 16 + (k >> 2)) * S];
        static_for<AH>([&](auto SL) {
            constexpr int sl = decltype(SL)::value;
#pragma unroll
            for (int j = 0; j < NT; ++j) uf[sl][j] = Bb[((sl % NC) * BN + j * 16) * S + 4 * (sl / NC)];
        });
#pragma unroll
        for (int i = 0; i < MT; ++i) wino_input_transform<4>(v[0][i], dr[i]);      // first k-step of the item: exposed once
#ifdef RS_ABL_NOFRAG                                    // timing experiment only: no fragment reads after the item's first
#pragma unroll
        for (int j = 0; j < NT; ++j) uf[AH][j] = uf[0][j];
#define RS_FRAG_A(dst, expr) asm volatile("" : "+v"(dst))
#define RS_FRAG_B(dst, expr) asm volatile("" : "+v"(dst))
#else
#define RS_FRAG_A(dst, expr) dst = (expr)
#define RS_FRAG_B(dst, expr) dst = (expr)
#endif
        static_for<NSLOTS>([&](auto SL) {
            constexpr int sl = decltype(SL)::value;
            constexpr int st = sl / NC, comp = sl % NC;
            // the raw rows of the next k-step are read in slot 1 and transformed in slots 3 (+ 4 for MT = 2),
            // one VALU group behind each MFMA, so that the transform hides in the MFMA shadow
            constexpr bool rd_next = comp == RD && st + 1 < KQ;
            constexpr bool xf_next = comp >= XF0 && comp - XF0 < MT && st + 1 < KQ;
            if constexpr (rd_next) {
                constexpr int c0 = 4 * (st + 1);
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int k = 0; k < 6; ++k) RS_FRAG_A(dr[i][k], (k < 4 ? Ab : Ab1)[(k & 3) * PL + (i * 16 + (k >> 2)) * S + c0]);
            }
            if constexpr (xf_next) wino_input_transform<4>(v[(st + 1) & 1][comp - XF0], dr[comp - XF0]);
            if constexpr (sl + AH < NSLOTS) {
                constexpr int nst = (sl + AH) / NC, ncomp = (sl + AH) % NC;
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    RS_FRAG_B(uf[(sl + AH) % (AH + 1)][j], Bb[(ncomp * BN + j * 16) * S + 4 * nst]);
            }
#if RS_W4_PRIO
            __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j][comp] = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[sl % (AH + 1)][j], v[st & 1][i][comp],
                                                                           acc[i][j][comp], 0, 0, 0);
#if RS_W4_PRIO
            __builtin_amdgcn_s_setprio(0);
#endif
            {
                constexpr int n_mf = MT * NT;
                constexpr int n_rd = (sl + AH < NSLOTS ? NT : 0) + (rd_next ? 3 * MT : 0);
                constexpr int n_va = xf_next ? 12 : 0;
                static_for<n_mf>([&](auto M) {
                    constexpr int m = decltype(M)::value;
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    if constexpr (m < n_rd) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                    constexpr int va0 = n_va * m / n_mf, va1 = n_va * (m + 1) / n_mf;
                    if constexpr (va1 > va0) __builtin_amdgcn_sched_group_barrier(0x002, va1 - va0, 0);
                });
            }
            if constexpr (xf_next) {                   // pin the transformed values to this slot (they are pure
                float(&o)[NC] = v[(st + 1) & 1][comp - XF0];   // functions of dr: the compiler would sink them to their use)
                asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]));
            }
            __builtin_amdgcn_sched_barrier(0);
            static_for<UNITS>([&](auto U) {
                constexpr int u = decltype(U)::value;
                if constexpr (DEEP) {
                    // the unit loaded during the previous item goes to the next item's buffer, and its registers
                    // leave again for the item after that
                    if constexpr ((u * NSLOTS) / UNITS == sl) {
                        store_unit(U, nbuf);
                        load_unit(U);
                    }
                } else if constexpr ((u * SPAN) / UNITS == sl)
                    load_unit(U);
                if constexpr (!DEEP && (u * SPAN) / UNITS + DIST == sl) {
                    // unconditional (conv_wino_kernel.hpp stores if (has_next)): after the last item the writes land in the idle
                    // buffer, which nobody reads any more; saves a branch per unit: -1.2 % (clock-normalised A/B)
                    store_unit(U, nbuf);
                }
            });
            __builtin_amdgcn_sched_barrier(0);
        });

        if (c == a.nch - 1) {
            // ---- epilogue: y = A^T m, two pooled rows per group, bias + ReLU + length mask, 16-byte stores -----
            const int pr0 = 2 * m0;
            const int b0 = pr0 / a.P_out;
            const int p0 = pr0 - b0 * a.P_out;
            unsigned rowoff_[MT][2];
            bool valid_[MT][2];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int loc = 2 * ((wm * MT + i) * 16 + r) + h;
                    const int t = p0 + loc;
                    const int e = (int)(((float)t + 0.5f) * a.inv_P_out);      // t < P_out + 2 * BG < 2^16: exact
                    const int pin = t - e * a.P_out;
                    const unsigned lv = __builtin_amdgcn_raw_buffer_load_b32(rs_len, (unsigned)(b0 + e) * 4u, 0, 0);
                    rowoff_[i][h] = (unsigned)(pr0 + loc) * a.y_row_bytes;    // rows past the end: out of range
                    valid_[i][h] = pin < (int)(lv >> a.shift_out);
                }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = n0 + (wn * NT + j) * 16 + 4 * kq;
                const unsigned coloff = col < a.cp_out ? (unsigned)col * 4u : kOob;
                const f32x4 bi = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_bias, (unsigned)col * 4u, 0, 0));
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    f32x4 o[2];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {                      // wino_output_pool<4> + bias, ReLU, length mask
                        const float m0_ = acc[i][j][0][q], m1 = acc[i][j][1][q], m2 = acc[i][j][2][q],
                                    m3 = acc[i][j][3][q], m4 = acc[i][j][4][q], m5 = acc[i][j][5][q];
                        const float s12 = m1 + m2, d12 = m1 - m2, s34 = m3 + m4, d34 = m3 - m4;
                        const float y0 = (m0_ + s12) + s34;
                        const float y1 = fmaf(2.0f, d34, d12);
                        const float y2 = fmaf(4.0f, s34, s12);
                        const float y3 = fmaf(8.0f, d34, d12) + m5;
                        o[0][q] = valid_[i][0] ? fmaxf(fmaxf(y0, y1) + bi[q], 0.0f) : 0.0f;
                        o[1][q] = valid_[i][1] ? fmaxf(fmaxf(y2, y3) + bi[q], 0.0f) : 0.0f;
                    }
#ifdef RS_ABL_NOSTORE
                    asm volatile("" ::"v"(o[0][0]), "v"(o[0][1]), "v"(o[0][2]), "v"(o[0][3]), "v"(o[1][0]), "v"(o[1][1]), "v"(o[1][2]), "v"(o[1][3]));
#else
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[0]), rs_y, rowoff_[i][0] + coloff, 0, 0);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[1]), rs_y, rowoff_[i][1] + coloff, 0, 0);
#endif
#pragma unroll
                    for (int q = 0; q < NC; ++q) acc[i][j][q] = (f32x4){0.f, 0.f, 0.f, 0.f};
                }
            }
        }
        if (!has_next) break;
#ifndef RS_ABL_NOBARRIER                                // timing experiment only
        __syncthreads();
#endif
        buf ^= 1;
        o = no;
        c = nc;
        m0 = nm0;
        n0 = nn0;
        if constexpr (DEEP) o1 = o2, c1 = c2, m1 = m2, n1 = n2;
    }
}

using Shape = WinoShape<Wino4Args, 2>;     // chunk = 16, 20

#define RS_SHAPE(WM, WN, MT, NT) \
    {{WM, WN, MT, NT}, {conv_wino4_kernel<WM, WN, MT, NT, 16>, conv_wino4_kernel<WM, WN, MT, NT, 20>}, {nullptr, nullptr}}
#define RS_SHAPE_D(WM, WN, MT, NT)                                                                       \
    {{WM, WN, MT, NT}, {conv_wino4_kernel<WM, WN, MT, NT, 16>, conv_wino4_kernel<WM, WN, MT, NT, 20>}, \
     {conv_wino4_kernel<WM, WN, MT, NT, 16, true>, conv_wino4_kernel<WM, WN, MT, NT, 20, true>}}
// four-wave shapes exist in the one-item-ahead form only
#define RS_SHAPE_4(WM, WN, MT, NT) \
    {{WM, WN, MT, NT}, {conv_wino4_kernel<WM, WN, MT, NT, 16, true>, conv_wino4_kernel<WM, WN, MT, NT, 20, true>}, {nullptr, nullptr}}
const Shape kShapes[] = {
    // 512 x 80 at chunks of 20: 223 registers, no scratch, unpadded LDS rows (above); layers 5, 6 and 10 of the shipped net take it.
    // 512 x 96 (round 6): 36 accumulator tiles = 249 / 253 registers, no scratch; its LDS fits with chunks of 16 only (157 KB), so
    // rs_model_create's chunk choice moves layers 7 and 9 of the shipped net (22 and 48 column groups: 4 and 8 tiles of six) from
    // chunks of 20 to 16 for it: layer 9 becomes ONE round of 256 tiles at 512 reads (-9 %), the fp32 step -1.3 %
    RS_SHAPE_D(8, 1, 1, 2), RS_SHAPE(8, 1, 1, 3), RS_SHAPE(8, 1, 1, 4), RS_SHAPE(8, 1, 1, 5), RS_SHAPE(8, 1, 1, 6),
    RS_SHAPE_D(4, 2, 1, 2), RS_SHAPE(4, 2, 1, 3), RS_SHAPE(4, 2, 1, 4), RS_SHAPE(4, 2, 2, 2),
    RS_SHAPE_D(2, 4, 1, 2), RS_SHAPE(2, 4, 1, 3), RS_SHAPE(2, 4, 1, 4), RS_SHAPE(2, 4, 2, 2),
    // small tiles (round 4): a batch of 32 ... 200 reads leaves the late layers a few dozen tiles of the shapes above
    RS_SHAPE_D(4, 2, 1, 1), RS_SHAPE_D(2, 4, 1, 1),
    // four-wave workgroups (round 5): one wave per SIMD, for launches of fewer tiles than CUs
    RS_SHAPE_4(4, 1, 1, 1), RS_SHAPE_4(2, 2, 1, 1), RS_SHAPE_4(1, 4, 1, 1),
    RS_SHAPE_4(4, 1, 1, 2), RS_SHAPE_4(2, 2, 1, 2), RS_SHAPE_4(1, 4, 1, 2),
    RS_SHAPE_4(4, 1, 1, 3), RS_SHAPE_4(2, 2, 1, 3),
};
#undef RS_SHAPE
#undef RS_SHAPE_D
#undef RS_SHAPE_4
constexpr int kNumShapes = sizeof(kShapes) / sizeof(kShapes[0]);

// full launches: calibrated on tools/shape_sweep.py (B = 512); the input transform's 12 VALU per MT do not hide behind the
// MFMAs.  Thin launches: 16 ... 512 reads, every shape, layers 5 - 10 (4 % rms, 15 % worst)
constexpr WinoCost kCost = {6.0, 12.0, 0.02, 90.0, 23500.0, 71.6, 4.25, -920.0, 0.0062, 0.0124, -467.0, 554.0};

// row unit: GROUPS of four conv rows
auto family(int kc, int nch, bool unpadded) { return wino_family<4>(kShapes, kNumShapes, kCost, kc, nch, unpadded); }

}  // namespace

int conv_wino4_max_bn() { return 256; }
int conv_wino4_num_shapes() { return kNumShapes; }
bool conv_wino4_shape_ok(const ConvLayerDev& L, int k) {
    return k >= 0 && k < kNumShapes && wino_chunk_index<Shape>(L.plan.kc) >= 0 &&
           family(L.plan.kc, L.plan.nch, L.plan.unpadded).can_run(k);
}

// planner's estimate (SIMD cycles) of one launch with the best tile shape for this chunk size: lets
// rs_model_create pick the channel chunk (which fixes the weight packing) with the tile shapes it enables in mind
double conv_wino4_plan_cost(int64_t groups, int n16, int kc, int nch, bool unpadded, int num_cu) {
    return choose_tile(family(kc, nch, unpadded), groups, n16, num_cu, false).cost;
}
double conv_wino4_launch_cost(int64_t groups, int n16, int kc, int nch, bool unpadded, int num_cu, bool* thin_out) {
    return wino_launch_cost(family(kc, nch, unpadded), groups, n16, num_cu, kCost, thin_out);
}

int launch_conv_wino4(const ConvLayerDev& L, const float* d_x, float* d_y, const int32_t* d_len, int B, int P_in,
                      int layer_index, int num_cu, int check_dead, hipStream_t st, int* bm_out, int* bn_out) {
    return launch_wino<4>("conv_wino4", kShapes, kNumShapes, kCost, L.hooks->force_wino4, L, d_x, d_y, d_len, B, P_in, layer_index,
                          num_cu, check_dead, st, bm_out, bn_out);
}

}  // namespace rs
