// K3r (fp32, Winograd F(2,3) and F(4,3)): the narrow early tiled layers (2 and 3 of the shipped net) with the layer's
// WHOLE transformed weight tensor resident in LDS and no workgroup barrier behind the prologue.
//
//   Conv1d(C_in -> C_out, k=3, stride 1, zero 'same' padding, bias) -> ReLU -> MaxPool1d(2,2)
//
// The tiled kernels (conv_wino_kernel.hpp, conv_wino4.hip) re-stage the weight slab of every item: layer 3 of the shipped
// net (one column tile, three chunks) writes its 104 KB of weights into LDS once per row tile, eight times per CU and
// launch, and all eight waves of a workgroup meet at a barrier once per item.  Here
//   * the prologue copies the packed weights [n][chunk][component][kc] into LDS as [chunk][component][n][kc + 2] - the
//     tiled kernels' B-slab layout with a chunk index in front, so their conflict-free ds_read_b32 fragment address is
//     reused plus a chunk offset - and the bias behind a single __syncthreads();
//   * every WAVE then owns a run of consecutive steps (chosen on the host as conv_stream_f32.hip chooses sub_per_wave).  A
//     step is 16 Winograd units by all padded output columns: 16 pooled rows from 34 input rows (F(2,3)), or 16 groups =
//     32 pooled rows from 66 input rows (F(4,3));
//   * per chunk of a step the wave's input rows arrive by 16-byte buffer loads ONE CHUNK AHEAD in registers (at most five
//     per lane; the tiled kernels' descriptors: row -1, the K padding and rows past the buffer read as zeros) and go to a
//     wave-PRIVATE LDS image in the tiled kernels' plane layout (parity planes / row-mod-4 planes, pitch kc + 2).  LDS
//     operations of one wave execute in order, so the wave only waits on its own lgkmcnt: the waves of a SIMD drift apart
//     and cover each other's waits;
//   * the chunk's slots run as in the tiled kernels: raw-row reads, input transform, weight fragments one slot ahead, MFMAs.
// Per accumulator the MFMA sequence is the tiled kernels' (chunks ascending, k-steps ascending, the same operands in the
// same positions; the first k-step of a step accumulates onto a literal zero), the plane layout, the transforms and the
// epilogue's arithmetic are theirs (conv_wino_device.hpp): results are byte-identical (tests/test_gpu_f32_wres.py).
#include "conv_wino_device.hpp"
#include "tile_plan.hpp"

#include <stdlib.h>

#include <algorithm>
#include <utility>

namespace rs {
namespace {

constexpr int kWaves = 8;
constexpr int kKc = 16;                     // the channel chunk this kernel is instantiated for

struct WresF32Args {
    const float* x;
    const float* w;        // packed [n_alloc][nch][NC][kc], zero rows beyond c_out
    const float* bias;     // [n_alloc]
    float* y;
    const int32_t* len;
    unsigned x_bytes, w_bytes, y_bytes, y_row_bytes, len_bytes, bias_bytes;      // each < 2^31 (host-checked)
    int rows_out;          // B * P_out (pooled rows)
    int n_reads;
    int P_out;
    float inv_P_out;
    int cp_in, cp_out;
    int nch;
    int shift_out;         // valid output rows of read b: len[b] >> shift_out
    int n_sub;             // steps of the launch
    int sub_per_wave;
};

// geometry of one instantiation, shared by the kernel and the host's LDS arithmetic
template <int M, int NT, int KCT>
struct Geom : WinoGeom<M, KCT> {                       // NC, NP, S, KQ and the 17-row plane: conv_wino_device.hpp
    using W = WinoGeom<M, KCT>;
    static constexpr int ROWS = 8 * M;                 // pooled rows of a step (16 units of M / 2)
    static constexpr int A_ROWS = 16 * M + 2;          // input rows of a step
    static constexpr int PL = W::PL16;                 // one plane
    static constexpr int IMG = W::IMG16;               // one wave's image of one chunk
    static constexpr int BN = 16 * NT;
    static constexpr int WCH = W::NC * BN * W::S;      // one chunk of the resident weights
    static constexpr int NL = (A_ROWS * W::KQ + 63) / 64; // 16-byte loads per lane and chunk
    static size_t lds_bytes(int nch) { return ((size_t)BN + (size_t)nch * WCH + (size_t)kWaves * IMG) * sizeof(float); }
};

template <int M, int NT, int KCT, int BLOCKS>
__global__ __launch_bounds__(kWaves * 64, BLOCKS) void conv_wres_f32_kernel(const WresF32Args a) {
    static_assert(M == 2 || M == 4, "F(2,3) or F(4,3)");
    static_assert(KCT % 4 == 0 && KCT >= 8, "channel chunk");
    using G = Geom<M, NT, KCT>;
    constexpr int NC = G::NC, NP = G::NP, ROWS = G::ROWS, A_ROWS = G::A_ROWS, S = G::S, KQ = G::KQ, PL = G::PL, IMG = G::IMG,
                  BN = G::BN, WCH = G::WCH, NL = G::NL;
    constexpr int H = M / 2;                           // pooled rows per unit
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const bl = lds;                             // bias [BN]
    float* const wl = lds + BN;                        // weights [nch][NC][BN][S]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, kq = lane >> 4;

    const __amdgpu_buffer_rsrc_t rs_x = buffer_rsrc(a.x, a.x_bytes), rs_w = buffer_rsrc(a.w, a.w_bytes),
                                 rs_y = buffer_rsrc(a.y, a.y_bytes), rs_len = buffer_rsrc(a.len, a.len_bytes),
                                 rs_bias = buffer_rsrc(a.bias, a.bias_bytes);
    const const_len_ptr clen = as_const_len(a.len);

    const int gw = blockIdx.x * kWaves + wave;
    const int u0 = gw * a.sub_per_wave;
    const int u1 = min(u0 + a.sub_per_wave, a.n_sub);
    float* const img = wl + a.nch * WCH + wave * IMG;

    // ---- staging map: unit lane + 64 k of a chunk is input row s = (lane >> 2) + 16 k of the step (global row
    // 2 * ROWS * u - 1 + s), channels 4 * (lane & 3) of the chunk; 16 is a multiple of NP, so a lane's plane is fixed ----
    const int s0 = lane >> 2, c4 = lane & 3;
    const int a_st = (s0 % NP) * PL + (s0 / NP) * S + 4 * c4;                   // + k * (16 / NP) * S
    const unsigned a_step = (unsigned)(16 * a.cp_in) * 4u;
    u32x4 pre[NL];
    auto issue_load = [&](int u, int c, bool live) {
        const bool ok = live && c * KCT + 4 * c4 < a.cp_in;
        // row -1 (u = 0) wraps to an offset beyond the buffer: zeros, like the K padding and the rows past the end
        const unsigned base = (unsigned)((2 * ROWS * u - 1 + s0) * a.cp_in + c * KCT + 4 * c4) * 4u;
        static_for<NL>([&](auto K) {
            constexpr int k = decltype(K)::value;
            unsigned off = ok ? base + (unsigned)k * a_step : kOob;
            if constexpr ((k + 1) * 16 > A_ROWS) off = (s0 + 16 * k < A_ROWS) ? off : kOob;
            pre[k] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0);
        });
    };
    auto store_image = [&]() {
        static_for<NL>([&](auto K) {
            constexpr int k = decltype(K)::value;
            bool act = true;
            if constexpr ((k + 1) * 16 > A_ROWS) act = s0 + 16 * k < A_ROWS;
            if (act) {
                uint2* d = reinterpret_cast<uint2*>(img + a_st + k * (16 / NP) * S);
                d[0] = make_uint2(pre[k].x, pre[k].y);
                d[1] = make_uint2(pre[k].z, pre[k].w);
            }
        });
    };

    if (u0 < u1) issue_load(u0, 0, true);              // the first chunk travels while the weights do

    // ---- prologue: the first BN rows of the packed weights are contiguous in memory; 16-byte unit g is
    // (n, chunk, component, c4) = digits of g in the bases (nch, NC, KQ) ------------------------------------------------
    {
        const int per_n = a.nch * NC * KQ;
        const int total = BN * per_n;
        constexpr int PB = 6;                          // loads in flight per thread: one trip to L2 per PB units, not per unit
        for (int g0 = tid; g0 < total; g0 += PB * kWaves * 64) {
            u32x4 v[PB];
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                const int g = g0 + q * kWaves * 64;
                v[q] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, g < total ? (unsigned)g * 16u : kOob, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                const int g = g0 + q * kWaves * 64;
                if (g < total) {
                    const int n = g / per_n, rem = g - n * per_n;
                    const int cc = rem / (NC * KQ), rem2 = rem - cc * (NC * KQ);
                    const int comp = rem2 / KQ, c4 = rem2 - comp * KQ;
                    uint2* d = reinterpret_cast<uint2*>(wl + ((cc * NC + comp) * BN + n) * S + 4 * c4);
                    d[0] = make_uint2(v[q].x, v[q].y);
                    d[1] = make_uint2(v[q].z, v[q].w);
                }
            }
        }
        if (tid < BN) bl[tid] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_bias, (unsigned)tid * 4u, 0, 0));
    }
    __syncthreads();                                   // the only barrier of the kernel
    if (u0 >= u1) return;

    const float* const Ab = img + r * S + kq;          // + (k % NP) * PL + (k / NP) * S + c0: raw input d_k of the lane's unit
    const float* const Bb0 = wl + r * S + kq;          // + chunk * WCH + (comp * BN + j * 16) * S + c0

    f32x4 acc[NT][NC];
    constexpr int NSLOTS = NC * KQ;                    // slot = (k-step, component): NT MFMAs
    // a slot of one or two MFMAs is shorter than an LDS round trip: its weight fragments are read further ahead
    constexpr int AH = NT >= 4 ? 1 : NT == 3 ? 2 : (4 + NT - 1) / NT;
    constexpr int RD = 1, XF = NC - 1;                 // component slots that read / transform the raw rows of the next k-step
    auto run_chunk = [&](auto FIRST, const float* Bb) {
        constexpr bool first = decltype(FIRST)::value;   // first chunk of a step: accumulate onto zero
        float dr[NC];
        float uf[AH + 1][NT];
        float v[2][NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) dr[k] = Ab[(k % NP) * PL + (k / NP) * S];
        static_for<AH>([&](auto SL) {
            constexpr int sl = decltype(SL)::value;
#pragma unroll
            for (int j = 0; j < NT; ++j) uf[sl][j] = Bb[((sl % NC) * BN + j * 16) * S + 4 * (sl / NC)];
        });
        wino_input_transform<M>(v[0], dr);
        static_for<NSLOTS>([&](auto SL) {
            constexpr int sl = decltype(SL)::value;
            constexpr int st = sl / NC, comp = sl % NC;
            constexpr bool rd_next = comp == RD && st + 1 < KQ;
            constexpr bool xf_next = comp == XF && st + 1 < KQ;
            if constexpr (rd_next) {
                constexpr int c0 = 4 * (st + 1);
#pragma unroll
                for (int k = 0; k < NC; ++k) dr[k] = Ab[(k % NP) * PL + (k / NP) * S + c0];
            }
            if constexpr (xf_next) wino_input_transform<M>(v[(st + 1) & 1], dr);
            if constexpr (sl + AH < NSLOTS) {
                constexpr int nst = (sl + AH) / NC, ncomp = (sl + AH) % NC;
#pragma unroll
                for (int j = 0; j < NT; ++j) uf[(sl + AH) % (AH + 1)][j] = Bb[(ncomp * BN + j * 16) * S + 4 * nst];
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                if constexpr (first && st == 0)
                    acc[j][comp] = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[sl % (AH + 1)][j], v[st & 1][comp],
                                                                        (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                else
                    acc[j][comp] = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[sl % (AH + 1)][j], v[st & 1][comp], acc[j][comp], 0, 0, 0);
            }
            {   // one LDS read (and a share of the transform) in the shadow of each MFMA
                constexpr int n_rd = (sl + AH < NSLOTS ? NT : 0) + (rd_next ? NC : 0);
                constexpr int n_va = xf_next ? (M == 2 ? 4 : 12) : 0;
                static_for<NT>([&](auto MI) {
                    constexpr int m = decltype(MI)::value;
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    constexpr int r0 = n_rd * m / NT, r1 = n_rd * (m + 1) / NT;
                    if constexpr (r1 > r0) __builtin_amdgcn_sched_group_barrier(0x100, r1 - r0, 0);
                    constexpr int va0 = n_va * m / NT, va1 = n_va * (m + 1) / NT;
                    if constexpr (va1 > va0) __builtin_amdgcn_sched_group_barrier(0x002, va1 - va0, 0);
                });
            }
            if constexpr (xf_next) {                   // pin the transformed values to this slot (pure functions of dr: the
                float(&o)[NC] = v[(st + 1) & 1];       // compiler would sink them to their use)
                if constexpr (M == 2)
                    asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]));
                else
                    asm volatile("" : "+v"(o[0]), "+v"(o[1]), "+v"(o[2]), "+v"(o[3]), "+v"(o[4]), "+v"(o[5]));
            }
            __builtin_amdgcn_sched_barrier(0);
        });
    };

    // (block, position) of the step's first pooled row, carried in scalars
    int b = (u0 * ROWS) / a.P_out;
    int t0 = u0 * ROWS - b * a.P_out;
    for (int u = u0; u < u1; ++u) {
        const int first_row = u * ROWS;
        const bool more = u + 1 < u1;
        // wave-uniformly dead: the step lies in one block, beyond its read's length - zeros, no arithmetic
        bool dead = false;
        if (t0 + ROWS <= a.P_out) dead = t0 >= ((b < a.n_reads ? clen[b] : 0) >> a.shift_out);
        if (dead) {
            issue_load(u + 1, 0, more);
#pragma unroll
            for (int h = 0; h < H; ++h) {
                const unsigned rowoff = (unsigned)(first_row + H * r + h) * a.y_row_bytes;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    const int col = 16 * j + 4 * kq;
                    __builtin_amdgcn_raw_buffer_store_b128((u32x4){0u, 0u, 0u, 0u}, rs_y, col < a.cp_out ? rowoff + (unsigned)col * 4u : kOob,
                                                           0, 0);
                }
            }
        } else {
            // the epilogue's length look-ups (tiled kernels' arithmetic: rows past the end of the batch look up a read index
            // >= B: out of range -> 0 -> masked) leave ahead of the last chunk's prefetch, so waiting for them leaves it in flight
            int pin_[H];
            unsigned lenv_[H];
            for (int c = 0; c < a.nch; ++c) {
                store_image();
                const bool last = c + 1 == a.nch;
                if (last) {
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        const int t = t0 + H * r + h;
                        const int e = (int)(((float)t + 0.5f) * a.inv_P_out);     // t < P_out + ROWS < 2^16: exact
                        pin_[h] = t - e * a.P_out;
                        lenv_[h] = __builtin_amdgcn_raw_buffer_load_b32(rs_len, (unsigned)(b + e) * 4u, 0, 0);
                    }
                }
                issue_load(last ? u + 1 : u, last ? 0 : c + 1, !last || more);
                __builtin_amdgcn_wave_barrier();
                if (c == 0)
                    run_chunk(std::true_type{}, Bb0);
                else
                    run_chunk(std::false_type{}, Bb0 + c * WCH);
                __builtin_amdgcn_wave_barrier();
            }
            // ---- epilogue: the tiled kernels' output transform + max-pool + bias + ReLU + length mask, 16-byte stores (rows
            // past the end of the batch and columns past cp_out resolve to out-of-range offsets and are dropped) ------------
            unsigned rowoff_[H];
            bool valid_[H];
#pragma unroll
            for (int h = 0; h < H; ++h) {
                rowoff_[h] = (unsigned)(first_row + H * r + h) * a.y_row_bytes;
                valid_[h] = pin_[h] < (int)(lenv_[h] >> a.shift_out);
            }
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int col = 16 * j + 4 * kq;
                const unsigned coloff = col < a.cp_out ? (unsigned)col * 4u : kOob;
                f32x4 bi = *reinterpret_cast<const f32x4*>(bl + col);
                asm volatile("" : "+v"(bi));           // read here, for every lane: not inside the length mask's branches
                f32x4 o[H];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float m[NC], p[H];
#pragma unroll
                    for (int k = 0; k < NC; ++k) m[k] = acc[j][k][q];
                    wino_output_pool<M>(p, m);
#pragma unroll
                    for (int h = 0; h < H; ++h) o[h][q] = valid_[h] ? fmaxf(p[h] + bi[q], 0.0f) : 0.0f;
                }
#pragma unroll
                for (int h = 0; h < H; ++h)
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o[h]), rs_y, rowoff_[h] + coloff, 0, 0);
            }
        }
        t0 += ROWS;
        while (t0 >= a.P_out) {
            t0 -= a.P_out;
            ++b;
        }
    }
}

using KernelFn = void (*)(const WresF32Args);

// One entry per instantiation.  Workgroups per CU follow the registers the compiler reports (-Rpass-analysis=kernel-resource-usage,
// no scratch anywhere): the F(2,3) forms stay below 128 VGPRs (4 waves per SIMD: two workgroups per CU), the F(4,3) forms
// hold 6 x NT accumulator tiles (two waves per SIMD: one workgroup)
struct Inst {
    int m, nt, per_cu;
    KernelFn fn;
    size_t (*lds)(int nch);
};
#define RS_INST(M, NT, PER_CU) {M, NT, PER_CU, conv_wres_f32_kernel<M, NT, kKc, PER_CU>, Geom<M, NT, kKc>::lds_bytes}
const Inst kInst[] = {
    RS_INST(2, 1, 2), RS_INST(2, 2, 2), RS_INST(2, 3, 2),
    RS_INST(4, 1, 1), RS_INST(4, 2, 1), RS_INST(4, 3, 1), RS_INST(4, 4, 1), RS_INST(4, 5, 1),
};
#undef RS_INST

// the instantiation of layer L and the workgroups per CU its LDS allows; null: none
const Inst* pick(const ConvLayerDev& L, int* per_cu_out = nullptr) {
    if (L.plan.kc != kKc || L.plan.nch < 1) return nullptr;
    const int n16 = round_up(L.c_out, 16) / 16;
    for (const Inst& k : kInst) {
        if (k.m != L.wino_m || k.nt != n16) continue;
        const size_t bytes = k.lds(L.plan.nch);
        if (bytes > kConvLdsBudget) return nullptr;
        if (per_cu_out) *per_cu_out = bytes * k.per_cu <= kConvLdsBudget ? k.per_cu : 1;
        return &k;
    }
    return nullptr;
}

// steps of a launch of rows_in input rows, and the pooled rows of one
int64_t steps_of(const ConvLayerDev& L, int64_t rows_in) {
    const int rows = 8 * L.wino_m;
    return (rows_in / 2 + rows - 1) / rows;
}

}  // namespace

bool conv_wres_f32_ok(const ConvLayerDev& L) { return L.hooks->wres_f32 != 0 && pick(L) != nullptr; }

// a launch large enough that every wave slot of the chip gets a run of several steps (thin launches keep the small / tiled kernels)
bool conv_wres_f32_fills(const ConvLayerDev& L, int64_t rows_in, int num_cu) {
    int per_cu = 1;
    if (!pick(L, &per_cu)) return false;
    return steps_of(L, rows_in) >= (int64_t)4 * num_cu * per_cu * kWaves;
}

int launch_conv_wres_f32(const ConvLayerDev& L, const float* d_x, float* d_y, const int32_t* d_len, int B, int P_in,
                         int layer_index, int num_cu, hipStream_t st, int* bm_out, int* bn_out) {
    int per_cu = 1;
    const Inst* k = pick(L, &per_cu);
    if (!k) {
        set_error("conv_wres_f32: layer %d is not one of the kernel's packings", layer_index);
        return RS_ERR_ARG;
    }
    const ConvPlan& p = L.plan;
    const int nc = L.wino_m + 2;
    const int64_t rows64 = (int64_t)B * P_in;
    const int64_t xb = rows64 * L.cp_in * 4, wb = (int64_t)p.n_alloc * p.nch * nc * p.kc * 4, yb = rows64 / 2 * L.cp_out * 4;
    if (rows64 > 0x7fffffff || xb >= 0x80000000LL || wb >= 0x80000000LL || yb >= 0x80000000LL) {
        set_error("conv_wres_f32: batch too large for the 2 GiB buffer window, split it");
        return RS_ERR_ARG;
    }
    if (p.n_alloc < 16 * k->nt) {
        set_error("conv_wres_f32: packed weights of layer %d hold %d rows, the kernel reads %d", layer_index, p.n_alloc, 16 * k->nt);
        return RS_ERR_ARG;
    }
    WresF32Args a;
    a.x = d_x;
    a.w = static_cast<const float*>(L.d_w);
    a.bias = L.d_bias;
    a.y = d_y;
    a.len = d_len;
    a.x_bytes = (unsigned)xb;
    a.w_bytes = (unsigned)wb;
    a.y_bytes = (unsigned)yb;
    a.y_row_bytes = (unsigned)L.cp_out * 4u;
    a.len_bytes = (unsigned)B * 4u;
    a.bias_bytes = (unsigned)p.n_alloc * 4u;
    a.rows_out = (int)(rows64 / 2);
    a.n_reads = B;
    a.P_out = P_in / 2;
    a.inv_P_out = 1.0f / (float)a.P_out;
    a.cp_in = L.cp_in;
    a.cp_out = L.cp_out;
    a.nch = p.nch;
    a.shift_out = layer_index + 1;
    a.n_sub = (int)steps_of(L, rows64);
    // a wave's run, as conv_stream_f32.hip chooses it: eight steps or more once every SIMD has a wave, runs of two on a thin
    // launch; RS_SF32_MIN_RUN forces the floor
    const int waves = num_cu * per_cu * kWaves;
    const int simds = num_cu * 4;
    const int floor_run = L.hooks->sf32_min_run > 0 ? L.hooks->sf32_min_run : std::min(8, std::max(2, (a.n_sub + simds - 1) / simds));
    a.sub_per_wave = std::max(floor_run, (a.n_sub + waves - 1) / waves);
    const int n_waves = (a.n_sub + a.sub_per_wave - 1) / a.sub_per_wave;
    const int grid = (n_waves + kWaves - 1) / kWaves;
    RS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k->fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kConvLdsBudget));
    hipLaunchKernelGGL(k->fn, dim3(grid), dim3(kWaves * 64), k->lds(p.nch), st, a);
    RS_HIP(hipGetLastError());
    if (bm_out) *bm_out = 16 * L.wino_m;                  // conv rows of one step: 16 units of wino_m
    if (bn_out) *bn_out = 16 * k->nt;
    return RS_OK;
}

}  // namespace rs
