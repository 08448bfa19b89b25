// Sequential conv programs (seqnet.hip), host side: the program as a list of ops, the record of a fused launch, the pattern
// matcher that fills it at create (fuse_program) and the planner of a forward's launches (plan_launches).
#pragma once
#include <algorithm>
#include <vector>

#include "pack.hpp"

namespace rs {
namespace {
// sizes the packers, the planner and the launcher must agree on
constexpr size_t kLdsBudget = 160 * 1024;          // LDS of a CU: what a fused block's weights and tiles may fill
constexpr size_t kSmallKernelLds = 96 * 1024;      // dynamic LDS the unfused LDS conv and the stem opt in to: their weights' limit
constexpr size_t kCompactPitchAbove = 60 * 1024;   // a basic block's full-pitch weights beyond this take the compact column pitch
constexpr int kGemmTileRows = 128;                 // GEMM rows per tile of the unfused LDS conv and the stem
constexpr int kBneckRows = 128;                    // input positions per bottleneck tile (RA of its kernels) ...
constexpr int kBneckTileRows = kBneckRows + 4;     // ... and the rows of each of its two LDS tiles

// One precision's form of a fused launch: T = float for the f32-input MFMA (PackF32), unsigned short for split precision
// (PackSplit).  w1 .. w3 are the convs of the main path in order; the 1x1 shortcut conv, where the block has one, is the last
// K range of the last matrix.  The stem has w1 only, a basic block w1 and w2.
template <class T>
struct FusedWeights {
    DevBuf<T> w1, w2, w3;
    int np_mid = 0;           // column pitch of the matrices c_mid wide (bottleneck: w1, w2)
    int np_out = 0;           // column pitch of the matrices c_out wide (basic: w1, w2; bottleneck: w3)
    int cp = 0;               // row pitch of the LDS tile(s) between the convs, in elements
    int s1 = 0, s2 = 0, s3 = 0, ssc = 0;   // split precision: k-steps of 32 of conv 1 .. 3 and of the shortcut conv
    size_t w_bytes = 0;       // all matrices in LDS
};

enum FuseKind { FUSE_NONE = 0, FUSE_STEM, FUSE_BASIC, FUSE_BOTTLENECK };

// A fused launch (rs_seqnet_create, fuse_program), owned by the op it starts at.
struct FusedBlock {
    FuseKind kind = FUSE_NONE;
    int n_ops = 1;            // ops the launch spans, from its owner on
    int first = 0;            // op index of the main path's first conv (behind the shortcut conv, if any)
    int src = -1, dst = -1;   // buffers
    int c_in = 0, c_mid = 0, c_out = 0, stride = 1;
    int ksc = 0;              // c_in if the shortcut is a conv, else 0 (identity)
    int nt_mid = 0, nt_out = 0;          // 16-column tiles of c_mid / c_out
    DevBuf<float> b1, b2, b3;            // biases per conv, padded to 16 nt (the shortcut conv's added to the last)
    FusedWeights<float> f32;             // (the stem's fp32 form is its op's own d_wq / d_b)
    FusedWeights<unsigned short> x3;     // empty where the split form does not fit the LDS
    bool has_x3() const { return x3.w1 != nullptr; }
    // the launch starts at op k, its main path of n_main ops at op `first`
    void span(FuseKind kind_, size_t k, size_t first_, int n_main, int src_, int dst_) {
        kind = kind_;
        n_ops = (int)(first_ - k) + n_main;
        first = (int)first_;
        src = src_;
        dst = dst_;
    }
    void widths(int c_in_, int c_mid_, int c_out_, int stride_, int ksc_) {
        c_in = c_in_;
        c_mid = c_mid_;
        c_out = c_out_;
        stride = stride_;
        ksc = ksc_;
        nt_mid = (c_mid + 15) / 16;
        nt_out = (c_out + 15) / 16;
    }
};

struct OpDev {
    int kind, src, dst, add;
    int c_in, c_out, k, stride, pad, relu;
    DevBuf<float> d_w;        // [k][c_in][cq*4]
    DevBuf<float> d_b;        // [cq*4]
    DevBuf<float> d_wq;       // MFMA packing [K16 / 4][Npad][4] (K = k * c_in in im2col order), or null if too large for LDS
    int nt = 0;               // Npad / 16
    FusedBlock fb;            // kind != FUSE_NONE: this op starts a fused launch
};

// What the matcher and the planner read of a program (rs_seqnet adds the device it lives on).
struct Program {
    int64_t window = 0x7fffffffLL; // bytes a kernel addresses through one 32-bit-offset buffer window (RS_SEQ_WINDOW_BYTES at create:
                                   // tests force the size guards of the fused launches with a small one)
    int mode = 0;                  // rs_seqnet_set_mode: 0 fp32 (f32-input MFMA), 1 split precision on the bf16 MFMA
    bool bneck_x3 = false;         // RS_SEQ_BNECK_X3=1 (read at create): bottleneck blocks in split precision too.  Off: measured
                                   // SLOWER than their fp32 form (0.734 against 0.718 ms on the 32-48-68 net, stem included) - with
                                   // mid widths of 8-17 channels a block's GEMMs are a few k-steps and the split costs more VALU
                                   // time than the matrix pipe saves
    bool scalar_conv = false;      // RS_SEQ_SCALAR=1 (read at create): the scalar FMA conv kernel instead of the MFMA one
    int n_buffers = 0;
    int c_last = 0;
    std::vector<OpDev> ops;
};

// lengths and channel widths of every buffer for an input of L samples (buffer 0 = the input)
// (buffer ids are reused by later ops with other shapes: *max_elems is the largest T*C any buffer
// ever holds, which sizes the workspace regions)
struct OpShape {
    int t_in, t_out, c;
};

bool propagate(const Program* m, int L, std::vector<int>& T, std::vector<int>& C, size_t* max_elems = nullptr,
               std::vector<OpShape>* shapes = nullptr) {
    if (max_elems) *max_elems = 0;
    if (shapes) shapes->clear();
    T.assign(m->n_buffers, -1);
    C.assign(m->n_buffers, 0);
    T[0] = L;
    C[0] = 1;
    for (const OpDev& o : m->ops) {
        if (T[o.src] < 0) return false;
        int t_out;
        if (o.kind == 0) {
            if (T[o.src] + 2 * o.pad < o.k) return false;          // torch: kernel larger than padded input
            t_out = (T[o.src] + 2 * o.pad - o.k) / o.stride + 1;
            C[o.dst] = o.c_out;
        } else {
            t_out = o.pad ? T[o.src] / 2 + 1 : T[o.src] / 2;      // MaxPool1d(2, 2, padding 1 | 0)
            C[o.dst] = C[o.src];
        }
        if (t_out < 1) return false;
        if (o.add >= 0 && (T[o.add] != t_out || C[o.add] != C[o.dst])) return false;
        if (shapes) shapes->push_back({T[o.src], t_out, C[o.dst]});
        T[o.dst] = t_out;
        if (max_elems) *max_elems = std::max(*max_elems, (size_t)t_out * C[o.dst]);
    }
    return true;
}

// is buffer `buf` dead after op index `after` (never read again before it is rewritten)?
bool dead_after(const std::vector<OpDev>& ops, size_t after, int buf) {
    for (size_t k = after + 1; k < ops.size(); ++k) {
        if (ops[k].src == buf || ops[k].add == buf) return false;
        if (ops[k].dst == buf) return true;
    }
    return true;
}

// ---- the pattern matcher ---------------------------------------------------------------------------------------------------------
// Recognise what riser_amd/resnet.py:build_program emits for the reference's stem (resnet.py:79-84), BasicBlock (resnet.py:50-57
// + shortcut :21-24,45-47) and Bottleneck (resnet.py:60-70).  Each match_* looks at the ops from k on; on a match it packs and
// uploads the weights, fills ops[k].fb and returns true (err: a failed upload).  hw[k] = host copy of op k's [c_out][c_in][k]
// weights (conv ops), hb[k] its bias.
typedef std::vector<const float*> HostPtrs;

// row pitch of an LDS tile of c channels: fp32 = 4 (mod 8) floats, split = 8 (mod 16) halfwords - conflict-free ds_read_b128 over
// the 16 rows of a lane group
int tile_pitch_f32(int c) { return round_up(c, 4) % 8 == 0 ? round_up(c, 4) + 4 : round_up(c, 4); }
int tile_pitch_x3(int c) { return round_up(c, 8) % 16 == 0 ? round_up(c, 8) + 8 : round_up(c, 8); }
int steps32(int K) { return (K + 31) / 32; }

// bias of n channels padded with zeros to `len`; a block's last bias takes the shortcut conv's on top (sc, or null: + 0)
hipError_t upload_bias(DevBuf<float>& d, const float* b, int n, int len, bool last = false, const float* sc = nullptr) {
    std::vector<float> v(len, 0.0f);
    for (int i = 0; i < n; ++i) v[i] = last ? b[i] + (sc ? sc[i] : 0.0f) : b[i];
    return upload(d, v);
}

// stem: conv(1 -> C) + ReLU, then MaxPool1d(2, 2, padding 1) of it
bool match_stem(std::vector<OpDev>& ops, size_t k, const HostPtrs& hw, hipError_t& err) {
    OpDev& o = ops[k];
    if (!(o.c_in == 1 && o.relu && o.add < 0 && o.d_wq && k + 1 < ops.size() && ops[k + 1].kind == 1 && ops[k + 1].pad == 1 &&
          ops[k + 1].src == o.dst && dead_after(ops, k + 1, o.dst)))
        return false;
    FusedBlock& f = o.fb;
    f.span(FUSE_STEM, k, k, 2, o.src, ops[k + 1].dst);
    // the split-precision packing (seq_stem_pool_x3_kernel): planes [hi | lo] of [k-step][kq][16 nt][8]
    f.x3.s1 = steps32(o.k);
    err = pack_upload<PackSplit>(f.x3.w1, (size_t)2 * f.x3.s1 * 4 * 16 * o.nt * 8, 16 * o.nt, o.c_out, {{hw[k], 1, o.k, 1, 0}});
    return true;
}

// A residual block at k starts with an optional 1x1 shortcut conv (no ReLU, no add; null: none); its main path follows and adds,
// at its end, `res`: the shortcut conv's output, or the block's input X.
const OpDev* shortcut_at(const std::vector<OpDev>& ops, size_t k) {
    const OpDev& o = ops[k];
    return o.k == 1 && o.pad == 0 && !o.relu && o.add < 0 && k + 2 < ops.size() ? &o : nullptr;
}

// basic block: [1x1 shortcut conv]  conv3(stride) + ReLU  conv3 + residual + ReLU
bool match_basic(std::vector<OpDev>& ops, size_t k, const HostPtrs& hw, const HostPtrs& hb, hipError_t& err) {
    const OpDev* sc = shortcut_at(ops, k);
    const size_t k1 = sc ? k + 1 : k;
    if (k1 + 1 >= ops.size()) return false;
    const OpDev& c1 = ops[k1];
    const OpDev& c2 = ops[k1 + 1];
    const int X = sc ? sc->src : c1.src, res = sc ? sc->dst : X;
    const bool shape_ok = c1.kind == 0 && c2.kind == 0 && c1.k == 3 && c1.pad == 1 && c1.relu && c1.add < 0 && c1.src == X &&
                          c2.k == 3 && c2.pad == 1 && c2.stride == 1 && c2.relu && c2.src == c1.dst && c2.add == res &&
                          c2.c_in == c1.c_out && c2.c_out == c1.c_out && c2.dst != X && c1.dst != X &&
                          (sc ? (sc->stride == c1.stride && sc->c_in == c1.c_in && sc->c_out == c1.c_out)
                                : (c1.stride == 1 && c1.c_in == c1.c_out));
    if (!shape_ok) return false;
    if (!dead_after(ops, k1 + 1, c1.dst) || (sc && !dead_after(ops, k1 + 1, res))) return false;
    const int c_in = c1.c_in, c_out = c1.c_out, nt = (c_out + 15) / 16;
    if (nt > 5) return false;
    const float* wsc = sc ? hw[k] : nullptr;
    const int Ksc = sc ? c_in : 0;
    FusedWeights<float> w;
    // column pitch of the weight matrices in LDS: the compact one (c_out rounded to 4) only where the full 16 * nt would
    // cost the block its second workgroup per CU - it costs a select per weight fragment
    w.np_out = 16 * nt;
    if ((size_t)(round_up(3 * c_in, 16) + round_up(3 * (c_out + 7), 16) + round_up(c_in, 16)) * w.np_out * 4 > kCompactPitchAbove)
        w.np_out = round_up(c_out, 4);
    w.cp = tile_pitch_f32(c_out);
    const int K1_16 = round_up(3 * c_in, 16), K2a16 = round_up(3 * w.cp, 16), Ksc16 = round_up(Ksc, 16);
    w.w_bytes = (size_t)(K1_16 + K2a16 + Ksc16) * w.np_out * 4;
    if (w.w_bytes + (size_t)(64 + 4) * w.cp * 4 > kLdsBudget) return false;       // not even the smallest tile fits
    FusedBlock& f = ops[k].fb;
    // pack: conv 1 as the unfused kernel does; conv 2 over the LDS tile's K index tap * Cp + c, the shortcut behind it
    err = pack_upload<PackF32>(w.w1, (size_t)K1_16 * w.np_out, w.np_out, c_out, {{hw[k1], c_in, 3, c_in, 0}});
    if (err == hipSuccess)
        err = pack_upload<PackF32>(w.w2, (size_t)(K2a16 + Ksc16) * w.np_out, w.np_out, c_out,
                                   {{hw[k1 + 1], c_out, 3, w.cp, 0}, {wsc, c_in, 1, 0, K2a16}});
    if (err == hipSuccess) err = upload_bias(f.b1, hb[k1], c_out, 16 * nt);
    if (err == hipSuccess) err = upload_bias(f.b2, hb[k1 + 1], c_out, 16 * nt, true, sc ? hb[k] : nullptr);
    // the split-precision packing of the same block (seq_basic_block_x3_kernel): k-steps of 32, bf16 planes [hi | lo] of
    // [k-step][kq][n][8] - 128 bytes per k-step and column -, own tile row pitch and column pitch
    FusedWeights<unsigned short> x;
    x.cp = tile_pitch_x3(c_out);
    x.s1 = steps32(3 * c_in);
    x.s2 = steps32(3 * x.cp);
    x.ssc = steps32(Ksc);
    x.np_out = 16 * nt;
    if ((size_t)(x.s1 + x.s2 + x.ssc) * 128 * x.np_out > kCompactPitchAbove) x.np_out = round_up(c_out, 4);
    x.w_bytes = (size_t)(x.s1 + x.s2 + x.ssc) * 128 * x.np_out;
    if (err == hipSuccess && x.w_bytes + (size_t)(64 + 4) * x.cp * 4 <= kLdsBudget) {
        err = pack_upload<PackSplit>(x.w1, (size_t)2 * x.s1 * 4 * x.np_out * 8, x.np_out, c_out, {{hw[k1], c_in, 3, c_in, 0}});
        if (err == hipSuccess)
            err = pack_upload<PackSplit>(x.w2, (size_t)2 * (x.s2 + x.ssc) * 4 * x.np_out * 8, x.np_out, c_out,
                                         {{hw[k1 + 1], c_out, 3, x.cp, 0}, {wsc, c_in, 1, 0, 32 * x.s2}});
        f.x3 = std::move(x);
    }
    f.f32 = std::move(w);
    f.span(FUSE_BASIC, k, k1, 2, X, c2.dst);
    f.widths(c_in, 0, c_out, c1.stride, Ksc);
    return true;
}

// bottleneck block: [1x1 shortcut conv]  conv1 + ReLU  conv3(stride) + ReLU  conv1 + residual + ReLU
bool match_bottleneck(std::vector<OpDev>& ops, size_t k, const HostPtrs& hw, const HostPtrs& hb, hipError_t& err) {
    const OpDev* sc = shortcut_at(ops, k);
    const size_t k1 = sc ? k + 1 : k;
    if (k1 + 2 >= ops.size()) return false;
    const OpDev& d1 = ops[k1];
    const OpDev& d2 = ops[k1 + 1];
    const OpDev& d3 = ops[k1 + 2];
    const int X = sc ? sc->src : d1.src, res = sc ? sc->dst : X;
    const bool bn_ok = d1.kind == 0 && d2.kind == 0 && d3.kind == 0 && d1.k == 1 && d1.pad == 0 && d1.stride == 1 && d1.relu &&
                       d1.add < 0 && d1.src == X && d2.k == 3 && d2.pad == 1 && d2.relu && d2.add < 0 && d2.src == d1.dst &&
                       d2.c_in == d1.c_out && d2.c_out == d1.c_out && d3.k == 1 && d3.pad == 0 && d3.stride == 1 && d3.relu &&
                       d3.src == d2.dst && d3.add == res && d3.c_in == d2.c_out && d3.dst != X && d1.dst != X && d2.dst != X &&
                       (sc ? (sc->stride == d2.stride && sc->c_in == d1.c_in && sc->c_out == d3.c_out)
                             : (d2.stride == 1 && d1.c_in == d3.c_out));
    if (!bn_ok || (d2.stride != 1 && d2.stride != 2)) return false;
    if (!dead_after(ops, k1 + 2, d1.dst) || !dead_after(ops, k1 + 2, d2.dst) || (sc && !dead_after(ops, k1 + 2, res)))
        return false;
    const int c_in = d1.c_in, c_mid = d1.c_out, c_out = d3.c_out;
    const int ntm = (c_mid + 15) / 16, nto = (c_out + 15) / 16;
    if (ntm > 2 || nto > 5) return false;
    const float* wsc = sc ? hw[k] : nullptr;
    const int Ksc = sc ? c_in : 0;
    const int NPm = round_up(c_mid, 4), NPo = round_up(c_out, 4);
    FusedWeights<float> w;
    w.np_mid = NPm;
    w.np_out = NPo;
    w.cp = tile_pitch_f32(c_mid);
    const int K1_16 = round_up(c_in, 16), K2_16 = round_up(3 * w.cp, 16), K3_16 = round_up(w.cp, 16), Ksc16 = round_up(Ksc, 16);
    w.w_bytes = ((size_t)(K1_16 + K2_16) * NPm + (size_t)(K3_16 + Ksc16) * NPo) * 4;
    if (w.w_bytes + (size_t)2 * kBneckTileRows * w.cp * 4 > kLdsBudget) return false;
    FusedBlock& f = ops[k].fb;
    err = pack_upload<PackF32>(w.w1, (size_t)K1_16 * NPm, NPm, c_mid, {{hw[k1], c_in, 1, 0, 0}});
    if (err == hipSuccess) err = pack_upload<PackF32>(w.w2, (size_t)K2_16 * NPm, NPm, c_mid, {{hw[k1 + 1], c_mid, 3, w.cp, 0}});
    if (err == hipSuccess)
        err = pack_upload<PackF32>(w.w3, (size_t)(K3_16 + Ksc16) * NPo, NPo, c_out, {{hw[k1 + 2], c_mid, 1, 0, 0}, {wsc, c_in, 1, 0, K3_16}});
    if (err == hipSuccess) err = upload_bias(f.b1, hb[k1], c_mid, 16 * ntm);
    if (err == hipSuccess) err = upload_bias(f.b2, hb[k1 + 1], c_mid, 16 * ntm);
    if (err == hipSuccess) err = upload_bias(f.b3, hb[k1 + 2], c_out, 16 * nto, true, sc ? hb[k] : nullptr);
    // the split-precision packing (seq_bottleneck_block_x3_kernel)
    FusedWeights<unsigned short> x;
    x.np_mid = NPm;
    x.np_out = NPo;
    x.cp = tile_pitch_x3(c_mid);
    x.s1 = steps32(c_in);
    x.s2 = steps32(3 * x.cp);
    x.s3 = steps32(x.cp);
    x.ssc = steps32(Ksc);
    const size_t q1 = (size_t)x.s1 * 4 * NPm * 8, q2 = (size_t)x.s2 * 4 * NPm * 8, q3 = (size_t)(x.s3 + x.ssc) * 4 * NPo * 8;   // a plane
    x.w_bytes = (q1 + q2 + q3) * 2 * 2;
    if (err == hipSuccess && x.w_bytes + (size_t)2 * kBneckTileRows * x.cp * 4 <= kLdsBudget) {
        err = pack_upload<PackSplit>(x.w1, 2 * q1, NPm, c_mid, {{hw[k1], c_in, 1, 0, 0}});
        if (err == hipSuccess) err = pack_upload<PackSplit>(x.w2, 2 * q2, NPm, c_mid, {{hw[k1 + 1], c_mid, 3, x.cp, 0}});
        if (err == hipSuccess)
            err = pack_upload<PackSplit>(x.w3, 2 * q3, NPo, c_out, {{hw[k1 + 2], c_mid, 1, 0, 0}, {wsc, c_in, 1, 0, 32 * x.s3}});
        f.x3 = std::move(x);
    }
    f.f32 = std::move(w);
    f.span(FUSE_BOTTLENECK, k, k1, 3, X, d3.dst);
    f.widths(c_in, c_mid, c_out, d2.stride, Ksc);
    return true;
}

// mark the first op of each pattern as a fused launch; the ops it spans are not matched again
hipError_t fuse_program(std::vector<OpDev>& ops, const HostPtrs& hw, const HostPtrs& hb) {
    for (size_t k = 0; k < ops.size(); ++k) {
        if (ops[k].kind != 0) continue;
        hipError_t err = hipSuccess;
        const bool hit = match_stem(ops, k, hw, err) || match_basic(ops, k, hw, hb, err) || match_bottleneck(ops, k, hw, hb, err);
        if (err != hipSuccess) return err;
        if (hit) k += ops[k].fb.n_ops - 1;
    }
    return hipSuccess;
}

// 1 when every op of the program runs inside a fused launch (stem, residual blocks): what a ragged forward needs
bool all_fused(const Program* m) {
    for (size_t k = 0; k < m->ops.size(); k += m->ops[k].fb.n_ops)
        if (m->ops[k].fb.kind == FUSE_NONE) return false;
    return m->ops.size() <= 63;
}

size_t buffer_bytes(const Program* m, int B, int L) {
    std::vector<int> T, C;
    size_t elems = 0;
    if (!propagate(m, L, T, C, &elems)) return 0;
    return ((size_t)B * elems * sizeof(float) + 255) / 256 * 256;
}

// ---- the planner -----------------------------------------------------------------------------------------------------------------
// One launch of a forward: what seqnet_forward_impl runs and rs_seqnet_launch_plan reports (rs_seq_launch), plus the dynamic LDS
struct Launch : rs_seq_launch {
    size_t lds = 0;
    Launch() : rs_seq_launch{} {}
};

// tile of a basic block = (row tiles per wave, waves): rows R = 16 * mtw * waves of the intermediate, R - 2 outputs.  More rows
// per wave = fewer halo rows, weight-fragment reads and set-up instructions per MFMA; candidates must fit the LDS next to the
// weights, should leave room for a second workgroup on the CU, and must not waste more than ~6 % of their rows behind the end of
// the read; a block so wide that one workgroup owns the CU's LDS runs eight waves (two per SIMD: with one, every LDS / global
// round trip idles the matrix pipe).  w_bytes: the weights in LDS, row_bytes: one tile row (both planes in split precision).
// (256-row tiles - four row tiles per wave - were measured on the 20-channel stage: 168 against 165 us)
void block_tile(size_t w_bytes, size_t row_bytes, int t_out, Launch& l) {
    auto lds_of = [&](int rows) { return w_bytes + (size_t)(rows + 4) * row_bytes; };
    auto waste = [&](int rows) {
        const int to = rows - 2, n = (t_out + to - 1) / to;
        return (double)(n * to - t_out) / (double)(n * to);
    };
    l.mtw = 1;
    l.waves = 4;
    if (kLdsBudget / lds_of(64) < 2) {
        if (lds_of(128) <= kLdsBudget) l.waves = 8;
    } else {
        if (kLdsBudget / lds_of(128) >= 2 && waste(128) < 0.06) l.mtw = 2;
    }
    l.lds = lds_of(16 * l.mtw * l.waves);
}

// Every launch decision of a forward of B reads at length (or, ragged, row pitch) L in the program's current mode: which ops fuse
// into one launch (the fused forms need their buffers inside the 32-bit-offset windows), split precision or fp32, the tile of a
// basic block, the unfused kernel of every other op.  seqnet_forward_impl launches exactly this list and rs_seqnet_launch_plan
// reports it.  On a refusal: the forward's error text and code.  shp: per-op shapes, last / last_op: the head's input.
int plan_launches(const Program* m, int B, int L, bool ragged, std::vector<Launch>& out, std::vector<OpShape>& shp, int& last,
                  int& last_op) {
    out.clear();
    if (ragged && !all_fused(m)) {
        set_error("rs_seqnet_forward_ragged: this program has ops outside its fused launches (stem, residual blocks): group the "
                  "reads by length and call rs_seqnet_forward");
        return RS_ERR_ARG;
    }
    std::vector<int> T, C;                                         // buffer ids are reused: shapes are per op
    if (!propagate(m, L, T, C, nullptr, &shp)) {
        set_error("rs_seqnet_forward: input of %d samples is too short for this network", L);
        return RS_ERR_LENGTH;
    }
    last = 0;
    last_op = -1;
    auto in_window = [&](int64_t rows, int c) { return (int64_t)B * rows * c * 4 < m->window; };
    for (size_t k = 0; k < m->ops.size(); ++k) {
        const OpDev& o = m->ops[k];
        const FusedBlock& f = o.fb;
        const OpShape& sh = shp[k];
        Launch l;
        l.op = (int)k;
        if (f.kind == FUSE_STEM && (int64_t)B * 2 * shp[k + 1].t_out < m->window && in_window(sh.t_in, 1)) {
            // stem conv + ReLU + MaxPool(2, 2, pad 1) in one launch: GEMM rows = 2 * pooled rows
            l.family = RS_SEQ_STEM_POOL;
            l.nt = o.nt;
            l.np = 16 * o.nt;
            if (m->mode == 1 && f.has_x3()) {                      // the stem in split precision on the bf16 MFMA
                l.x3 = 1;
                l.lds = (size_t)f.x3.s1 * 4 * o.nt * 16 * 8 * 2 * 2 + (size_t)4 * 16 * o.c_out * 4;
            } else {
                l.lds = (size_t)round_up(o.k * o.c_in, 16) * o.nt * 16 * 4;
            }
        } else if (f.kind == FUSE_BASIC && in_window(shp[f.first].t_out, f.c_out) && in_window(shp[f.first].t_in, f.c_in)) {
            // residual basic block in one launch (shapes of its first 3x3 conv); in split precision the same tiling rules over
            // its own LDS footprint
            const bool x3 = m->mode == 1 && f.has_x3();
            l.family = RS_SEQ_BASIC_BLOCK;
            l.nt = f.nt_out;
            l.x3 = x3;
            l.np = x3 ? f.x3.np_out : f.f32.np_out;
            l.cp = x3 ? f.x3.cp : f.f32.cp;
            block_tile(x3 ? f.x3.w_bytes : f.f32.w_bytes, (size_t)l.cp * 4, shp[f.first].t_out, l);
        } else if (f.kind == FUSE_BOTTLENECK && in_window(shp[f.first].t_in, f.c_in) && in_window(shp[f.first + 1].t_out, f.c_out)) {
            // residual bottleneck block in one launch; shapes: conv 1 = ops[first], conv 2 (the strided one) = ops[first + 1]
            const bool x3 = m->mode == 1 && m->bneck_x3 && f.has_x3();
            l.family = RS_SEQ_BOTTLENECK;
            l.ntm = f.nt_mid;
            l.nt = f.nt_out;
            l.np = f.f32.np_out;
            l.x3 = x3;
            l.cp = x3 ? f.x3.cp : f.f32.cp;
            l.lds = (x3 ? f.x3.w_bytes : f.f32.w_bytes) + (size_t)2 * kBneckTileRows * l.cp * 4;
        } else if (ragged) {
            // a ragged batch runs in fused launches only (they mask by every read's own rows; the unfused kernels below treat
            // every read as `ld` samples long): a fused launch that does not fit its 2 GiB buffer windows is an error, not a
            // silent fall-through to wrong probabilities
            set_error("rs_seqnet_forward_ragged: op %zu of the program cannot run as a fused launch on %d reads of pitch %d (a buffer "
                      "beyond the 2 GiB window): split the batch", k, B, L);
            return RS_ERR_ARG;
        } else if (o.kind == 0 && m->scalar_conv) {
            l.family = RS_SEQ_CONV_SCALAR;
        } else if (o.kind == 0 && o.d_wq && in_window(sh.t_in, o.c_in)) {
            l.family = RS_SEQ_CONV_MFMA_LDS;
            l.nt = o.nt;
            l.np = 16 * o.nt;
            l.lds = (size_t)round_up(o.k * o.c_in, 16) * o.nt * 16 * 4;
        } else if (o.kind == 0) {
            l.family = RS_SEQ_CONV_MFMA;
            l.nt = o.c_out <= 16 ? 1 : o.c_out <= 32 ? 2 : 4;
            l.np = (o.c_out + 3) / 4 * 4;
        } else {
            l.family = RS_SEQ_MAXPOOL;
        }
        l.n_ops = l.family <= RS_SEQ_BOTTLENECK ? f.n_ops : 1;
        last = l.family <= RS_SEQ_BOTTLENECK ? f.dst : o.dst;
        last_op = (int)k + l.n_ops - 1;
        k += l.n_ops - 1;
        out.push_back(l);
    }
    if (C[last] != m->c_last) {
        set_error("rs_seqnet_forward: last buffer has %d channels, classifier expects %d", C[last], m->c_last);
        return RS_ERR_ARG;
    }
    return RS_OK;
}
}  // namespace
}  // namespace rs
