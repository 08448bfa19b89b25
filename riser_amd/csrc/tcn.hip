// TCN and bottleneck TCN (riser/nets/tcn.py, riser/nets/tcn_bot.py): the strided receptive cone of the last position.
//
// The nets classify x[:, :, -1] (tcn.py:87) through causal convs only, so block i (dilation d_i) is needed at positions
// L-1 - d_i * m alone (m = 0, 1, ... counting back from the last sample).  On that subsequence the block's k-tap convs of
// dilation d_i are dense k-tap convs, and block i + 1 reads every base-th of block i's outputs (base = d_{i+1} / d_i).
// Buffers are position-major [read][m][channels padded to 4]: row m of read b is position L_b - 1 - d_i * m.
//
// One launch per temporal block (tcn_block_kernel).  A workgroup (4 waves) takes `nb` reads x `T` output positions:
//   - stages the block input rows it needs into LDS (block 0: straight from the signal, right-aligned to each read's own
//     length), zero at every position below 0 - the reference's per-conv left padding;
//   - runs the block's convs on the f32-input MFMA (v_mfma_f32_16x16x4_f32) with LDS-resident intermediates: the convs
//     up to the last k-tap conv over every m the tile needs, that conv and the 1x1 convs after it only at m = base * m'
//     (a stride-base conv, not a full conv followed by a subsample); ReLU after every conv; every value at a position
//     below 0 is set to exactly 0 (not relu(bias));
//   - adds the 1x1 shortcut or the identity at the same strided rows, applies the ReLU, and writes only the rows the
//     next block reads.
// The GEMM M dimension is reads x positions: late blocks have a handful of positions per read and tile across reads.
// last_row_head_kernel (family/head.hpp) runs Linear(n_filters -> 2) + softmax on the one remaining position.  Every output element is a fixed
// k-ordered fmaf chain whatever the tile, the batch or the row pitch: a read's result is that of the read alone, bit for bit.
// rs_tcn_set_mode(m, RS_BF16X3) runs the blocks on csrc/tcn_x3.hip instead (split precision on the bf16 MFMA); the head and
// the activation buffers are shared.
#include "common.hpp"
#include "family/head.hpp"
#include "family/host.hpp"
#include "tcn_x3.hpp"

#include <algorithm>
#include <cstring>
#include <new>

namespace rs {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMaxConvs = 4;
constexpr int kLdsBudget = 64 * 1024;             // bytes of LDS per workgroup: two workgroups per CU
constexpr int64_t kMaxDil = int64_t(1) << 40;      // dilations beyond any read length behave alike

struct BlockArgs {
    const float* x;             // block input: [B][in_rows][cp_in] (block 0: the signal, [B][ld])
    const int32_t* len;         // read lengths
    float* y;                   // block output: [B][out_rows][cp_out]
    int B, ld, first;
    int64_t dil;                // d_i
    int r;                      // base: output m' is input m = r * m'
    int in_rows, out_rows;      // per read, in global memory
    int cp_in, cp_out;
    int T, nb, tiles_pos;       // tile: nb reads x T output positions
    int rows_in;                // X rows per read in LDS
    int nconv, jk;
    const float* w[kMaxConvs];  // packed [k][cpi][np]
    const float* b[kMaxConvs];  // [np]
    int k[kMaxConvs], cpi[kMaxConvs], cpo[kMaxConvs], np[kMaxConvs];
    int rows[kMaxConvs];        // output rows per read in the tile
    int step[kMaxConvs];        // input rows per output row (r for the conv jk, else 1)
    int ostride[kMaxConvs];     // m per output row (r from the conv jk on, else 1)
    int src[kMaxConvs], dst[kMaxConvs];   // LDS buffers: 0 = X, 1 = P, 2 = Q; dst -1 = global
    const float* sw;            // shortcut [cp_in][np_out] or null (identity)
    const float* sb;
    int off[3], pitch[3];       // LDS buffer offsets (floats) and row pitches
};

__device__ __forceinline__ int read_len(const BlockArgs& a, int b) {
    int L = as_const_len(a.len)[b];
    return L < 0 ? 0 : (L > a.ld ? a.ld : L);
}

__global__ __launch_bounds__(256) void tcn_block_kernel(const BlockArgs a) {
    extern __shared__ float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int tile_b = blockIdx.x / a.tiles_pos, tile_p = blockIdx.x - tile_b * a.tiles_pos;
    const int b0 = tile_b * a.nb, mo0 = tile_p * a.T;      // first read, first output position m'
    const int64_t mbase = (int64_t)a.r * mo0;               // first input / intermediate m of the tile

    // ---- block input rows -> LDS X, zero below position 0 and beyond the window
    {
        float* X = lds + a.off[0];
        const int c4n = a.cp_in / 4;
        const int n = a.nb * a.rows_in * c4n;
        for (int e = threadIdx.x; e < n; e += 256) {
            const int c4 = e % c4n, rq = e / c4n;
            const int bl = rq / a.rows_in, q = rq - bl * a.rows_in;
            const int b = b0 + bl;
            const int64_t m = mbase + q;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (b < a.B && m < a.in_rows) {
                const int L = read_len(a, b);
                const int64_t pos = (int64_t)L - 1 - a.dil * m;
                if (pos >= 0) {
                    if (a.first) {
                        if (c4 == 0) v.x = a.x[(int64_t)b * a.ld + pos];
                    } else {
                        v = *reinterpret_cast<const f32x4*>(a.x + ((int64_t)b * a.in_rows + m) * a.cp_in + 4 * c4);
                    }
                }
            }
            *reinterpret_cast<f32x4*>(X + (int64_t)(bl * a.rows_in + q) * a.pitch[0] + 4 * c4) = v;
        }
    }
    __syncthreads();

    for (int j = 0; j < a.nconv; ++j) {
        const bool last = j == a.nconv - 1;
        const float* S = lds + a.off[a.src[j]];
        const int sp = a.pitch[a.src[j]];
        const int srows = a.src[j] == 0 ? a.rows_in : a.rows[j - 1];
        const int R = a.rows[j], M = a.nb * R, np = a.np[j], cpi = a.cpi[j];
        const int steps = a.k[j] * cpi / 4;
        const int mt = (M + 15) / 16, ng = (np + 63) / 64;
        const float* __restrict__ W = a.w[j];
        for (int u = wave; u < mt * ng; u += 4) {
            const int rt = u / ng, cg = u - rt * ng;
            // the output row this lane feeds into the A operand
            const int arow = rt * 16 + rl;
            const bool a_ok = arow < M;
            const int abl = a_ok ? arow / R : 0, aq = a_ok ? arow - abl * R : 0;
            const float* Arow = S + (abl * srows + aq * a.step[j]) * sp + kq;
            const int n0 = cg * 64;
            f32x4 acc[4], accs[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = accs[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < steps; ++s) {
                const int kidx0 = 4 * s;
                const int tap = kidx0 / cpi, ci = kidx0 - tap * cpi;
                const float av = a_ok ? Arow[tap * sp + ci] : 0.0f;
                const float* wr = W + (int64_t)(kidx0 + kq) * np + n0 + rl;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (n0 + 16 * t < np) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[16 * t], acc[t], 0, 0, 0);
            }
            if (last && a.sw) {                            // 1x1 shortcut on the block input at the strided rows
                const float* Xr = lds + a.off[0] + (abl * a.rows_in + aq * a.r) * a.pitch[0] + kq;
                for (int s = 0; s < a.cp_in / 4; ++s) {
                    const float av = a_ok ? Xr[4 * s] : 0.0f;
                    const float* wr = a.sw + (int64_t)(4 * s + kq) * np + n0 + rl;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (n0 + 16 * t < np) accs[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[16 * t], accs[t], 0, 0, 0);
                }
            }
            // accumulator element e of this lane: row 4 * kq + e of the tile, column rl of each 16-column tile
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int col = n0 + 16 * t + rl;
                if (n0 + 16 * t >= np || col >= a.cpo[j]) continue;
                const float bias = a.b[j][col];
                const float sbias = (last && a.sw) ? a.sb[col] : 0.0f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = rt * 16 + 4 * kq + e;
                    if (row >= M) continue;
                    const int bl = row / R, q = row - bl * R;
                    const int b = b0 + bl;
                    const int64_t m = mbase + (int64_t)q * a.ostride[j];
                    bool valid = false;
                    if (b < a.B && m <= a.ld) valid = (int64_t)read_len(a, b) - 1 - a.dil * m >= 0;
                    float v = fmaxf(acc[t][e] + bias, 0.0f);
                    if (!last) {
                        lds[a.off[a.dst[j]] + (bl * R + q) * a.pitch[a.dst[j]] + col] = valid ? v : 0.0f;
                    } else {
                        const int mo = mo0 + q;
                        if (b >= a.B || mo >= a.out_rows) continue;
                        const float res = a.sw ? accs[t][e] + sbias
                                               : lds[a.off[0] + (bl * a.rows_in + q * a.r) * a.pitch[0] + col];
                        a.y[((int64_t)b * a.out_rows + mo) * a.cp_out + col] = valid ? fmaxf(v + res, 0.0f) : 0.0f;
                    }
                }
            }
        }
        __syncthreads();
    }
}

struct ConvDev {
    int c_in = 0, c_out = 0, cpi = 0, cpo = 0, np = 0, k = 0;
    DevBuf<float> w;            // [k][cpi][np]: element (tap t reads m + t, ci, co) = w_ref[co][ci][k - 1 - t]
    DevBuf<float> b;            // [np]
    DevBuf<unsigned short> xw;  // RS_BF16X3: tcn_x3_pack planes
    int xsteps = 0;
};

struct BlockDev {
    int nconv = 0, base = 1, jk = 0, c_in = 0, c_out = 0;
    int64_t dil = 1;
    ConvDev conv[kMaxConvs];
    DevBuf<float> sw;           // [cp_in][np_out]; null: identity
    DevBuf<float> sb;
    DevBuf<unsigned short> xsw; // RS_BF16X3: the shortcut's tcn_x3_pack planes
    int xsw_steps = 0;
    int span = 0;               // sum of (k - 1) over the block's causal convs
};

}  // namespace
}  // namespace rs

struct rs_tcn {
    int device = 0;
    std::vector<rs::BlockDev> blocks;
    rs::DevBuf<float> d_fcw, d_fcb;
    int c_last = 0;
    int64_t rf = 1;
    int mode = 0;               // rs_tcn_set_mode: 0 fp32 (f32-input MFMA), 1 split precision on the bf16 MFMA
};

namespace rs {
namespace {

// positions every block reads (need[i], i < n) and the last block's one output (need[n] = 1) for reads of up to ld samples
void tcn_windows(const rs_tcn* m, int ld, std::vector<int64_t>& need) {
    const int n = (int)m->blocks.size();
    need.assign(n + 1, 1);
    for (int i = n - 1; i >= 0; --i) {
        const BlockDev& b = m->blocks[i];
        const int64_t cap = (ld + b.dil - 1) / b.dil;
        // (need - 1) * base can only exceed cap when it exceeds ld: compare before multiplying
        const int64_t prev = need[i + 1] - 1;
        int64_t want = prev > (int64_t)ld / b.base + 1 ? cap + 1 : prev * b.base + 1 + b.span;
        need[i] = std::min(want, cap);
    }
}

// rows of every conv's output per read for a tile of T outputs, and the X rows; LDS floats of a tile of nb reads
struct TilePlan {
    int rows[kMaxConvs], rows_in;
    int off[3], pitch[3];
    size_t lds_bytes;
};

TilePlan plan_tile(const BlockDev& b, int T, int nb) {
    TilePlan p;
    int64_t need = T;                                       // capped: a tile that large is refused by its LDS size anyway
    for (int j = b.nconv - 1; j >= 0; --j) {
        p.rows[j] = (int)need;
        need = std::min<int64_t>(1 << 24, (need - 1) * (j == b.jk ? b.base : 1) + b.conv[j].k);
    }
    p.rows_in = (int)need;
    p.pitch[0] = lds_pitch(b.conv[0].cpi);
    int rows_buf[3] = {p.rows_in, 0, 0}, pitch_buf[3] = {p.pitch[0], 4, 4};
    for (int j = 0; j + 1 < b.nconv; ++j) {
        const int d = 1 + (j & 1);
        rows_buf[d] = std::max(rows_buf[d], p.rows[j]);
        pitch_buf[d] = std::max(pitch_buf[d], lds_pitch(b.conv[j].cpo));
    }
    size_t off = 0;
    for (int d = 0; d < 3; ++d) {
        p.off[d] = (int)off;
        p.pitch[d] = pitch_buf[d];
        off += (size_t)nb * rows_buf[d] * pitch_buf[d];
    }
    p.lds_bytes = off * 4;
    return p;
}

// the tile of a block in `mode` (rs_tcn::mode) for out_rows outputs per read: up to 64 output positions of one read, or -
// where a read has fewer - several reads, inside the LDS budget.  The forward and rs_tcn_tile_plan both take it from here.
// Returns the tile's LDS bytes: above kLdsBudget, the block is too wide for one tile even at T = 1.
size_t choose_tile(const BlockDev& bd, int mode, int B, int out_rows, int* T_out, int* nb_out) {
    int k[kMaxConvs], cpi[kMaxConvs], cpo[kMaxConvs];
    for (int j = 0; j < bd.nconv; ++j) {
        k[j] = bd.conv[j].k;
        cpi[j] = tcn_cp8(bd.conv[j].c_in);
        cpo[j] = tcn_cp8(bd.conv[j].c_out);
    }
    auto lds = [&](int T, int nb) {
        return mode == 1 ? tcn_x3_plan(bd.nconv, k, cpi, cpo, bd.jk, bd.base, T, nb).lds_bytes : plan_tile(bd, T, nb).lds_bytes;
    };
    int T = std::min(out_rows, 64);
    while (T > 1 && lds(T, 1) > (size_t)kLdsBudget) --T;
    int nb = 1;
    if (T == out_rows) {
        nb = std::max(1, std::min(B, 64 / T));
        while (nb > 1 && lds(T, nb) > (size_t)kLdsBudget) --nb;
    }
    *T_out = T;
    *nb_out = nb;
    return lds(T, nb);
}

size_t buffer_bytes(const rs_tcn* m, int64_t B, int ld) {
    std::vector<int64_t> need;
    tcn_windows(m, ld, need);
    size_t mx = 0;
    for (size_t i = 0; i < m->blocks.size(); ++i)
        mx = std::max(mx, (size_t)need[i + 1] * (size_t)rs::cp4(m->blocks[i].c_out) * 4);
    return ((size_t)B * mx + 255) / 256 * 256;
}

// a * b for a, b >= 0, saturated at INT64_MAX
int64_t sat_mul(int64_t a, int64_t b) { return (a != 0 && b > INT64_MAX / a) ? INT64_MAX : a * b; }

// block i of an RS_BF16X3 forward (csrc/tcn_x3.hip): the tile choice of the fp32 path on the split LDS layout
int launch_block_x3(const BlockDev& bd, int i, const float* in, const int32_t* d_len, float* out, int B, int ld, int in_rows,
                    int out_rows, hipStream_t st) {
    int k[kMaxConvs], cpi[kMaxConvs], cpo[kMaxConvs];
    for (int j = 0; j < bd.nconv; ++j) {
        k[j] = bd.conv[j].k;
        cpi[j] = tcn_cp8(bd.conv[j].c_in);
        cpo[j] = tcn_cp8(bd.conv[j].c_out);
    }
    int T = 1, nb = 1;
    choose_tile(bd, 1, B, out_rows, &T, &nb);
    const TcnX3Plan p = tcn_x3_plan(bd.nconv, k, cpi, cpo, bd.jk, bd.base, T, nb);
    if (p.lds_bytes > (size_t)kLdsBudget) {
        set_error("rs_tcn_forward_ragged: block %d is too wide for one tile of LDS", i);
        return RS_ERR_ARG;
    }
    TcnX3Args a;
    memset(&a, 0, sizeof(a));
    a.x = in;
    a.len = d_len;
    a.y = out;
    a.B = B;
    a.ld = ld;
    a.first = i == 0;
    a.dil = std::min<int64_t>(bd.dil, (int64_t)ld + 1);
    a.r = bd.base;
    a.in_rows = in_rows;
    a.out_rows = out_rows;
    a.cp_in = cp4(bd.c_in);
    a.cp_out = cp4(bd.c_out);
    a.T = T;
    a.nb = nb;
    a.tiles_pos = (out_rows + T - 1) / T;
    a.rows_in = p.rows_in;
    a.nconv = bd.nconv;
    for (int j = 0; j < bd.nconv; ++j) {
        const ConvDev& c = bd.conv[j];
        a.w[j] = c.xw;
        a.b[j] = c.b;
        a.k[j] = c.k;
        a.cpi[j] = cpi[j];
        a.cpo[j] = cpo[j];
        a.np[j] = c.np;
        a.steps[j] = c.xsteps;
        a.rows[j] = p.rows[j];
        a.step[j] = j == bd.jk ? bd.base : 1;
        a.ostride[j] = j >= bd.jk ? bd.base : 1;
        a.src[j] = j == 0 ? 0 : 1 + ((j - 1) & 1);
        a.dst[j] = j + 1 == bd.nconv ? -1 : 1 + (j & 1);
    }
    a.sw = bd.xsw;
    a.sb = bd.sb;
    a.sw_steps = bd.xsw_steps;
    for (int d = 0; d < 3; ++d) {
        a.off[d] = p.off[d];
        a.pitch[d] = p.pitch[d];
        a.plane[d] = p.plane[d];
    }
    for (int j = 0; j < bd.nconv; ++j) {
        const int s = a.src[j], d = std::max(a.dst[j], 0);
        a.s_off[j] = p.off[s];
        a.s_pitch[j] = p.pitch[s];
        a.s_plane[j] = p.plane[s];
        a.s_rows[j] = s == 0 ? p.rows_in : p.rows[j - 1];
        a.d_off[j] = p.off[d];
        a.d_pitch[j] = p.pitch[d];
        a.d_plane[j] = p.plane[d];
    }
    const int64_t grid = (int64_t)((B + nb - 1) / nb) * a.tiles_pos;
    if (grid > INT32_MAX) {
        set_error("rs_tcn_forward_ragged: grid too large: split the batch");
        return RS_ERR_ARG;
    }
    RS_HIP(tcn_x3_launch(a, (unsigned)grid, p.lds_bytes, st));
    return RS_OK;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" {

int rs_tcn_create(const rs_tcn_block* blocks, int n_blocks, const float* fc_w, const float* fc_b, int c_last, int device,
                  rs_tcn** out) {
    if (!blocks || n_blocks < 1 || !fc_w || !fc_b || !out || c_last < 1) {
        set_error("rs_tcn_create: bad argument");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    DeviceGuard guard(device);
    RS_HIP(guard.err);
    rs_tcn* m = new (std::nothrow) rs_tcn();
    if (!m) return RS_ERR_OOM;
    m->device = device;
    m->c_last = c_last;
    int64_t dil = 1, rf = 1;
    int64_t rf_dil = 1;                 // the receptive field's dilation: not clamped to kMaxDil, saturated at INT64_MAX
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_blocks && e == hipSuccess; ++i) {
        const rs_tcn_block& s = blocks[i];
        BlockDev bd;
        bd.nconv = s.n_convs;
        bd.base = s.base;
        bd.dil = dil;
        bool ok = s.n_convs >= 1 && s.n_convs <= kMaxConvs && s.base >= 1;
        bd.jk = -1;
        for (int j = 0; ok && j < s.n_convs; ++j) {
            const rs_tcn_conv& c = s.convs[j];
            ok = c.w && c.b && c.c_in >= 1 && c.c_out >= 1 && c.k >= 1 && (c.causal || c.k == 1) &&
                 (j == 0 || c.c_in == s.convs[j - 1].c_out);
            if (ok && c.k > 1) bd.jk = j;
        }
        if (ok) {
            bd.c_in = s.convs[0].c_in;
            bd.c_out = s.convs[s.n_convs - 1].c_out;
            ok = bd.jk >= 0 && (i == 0 || bd.c_in == m->blocks[i - 1].c_out) &&
                 (s.has_shortcut ? (s.sc_w && s.sc_b) : bd.c_in == bd.c_out);
        }
        if (!ok) {
            rs_tcn_destroy(m);
            set_error("rs_tcn_create: bad block %d (1-4 chained convs with one of k > 1, causal where k > 1, base >= 1, a "
                      "shortcut when in != out channels)", i);
            return RS_ERR_ARG;
        }
        for (int j = 0; j < s.n_convs && e == hipSuccess; ++j) {
            const rs_tcn_conv& c = s.convs[j];
            ConvDev& cd = bd.conv[j];
            cd.c_in = c.c_in; cd.c_out = c.c_out; cd.k = c.k;
            cd.cpi = cp4(c.c_in); cd.cpo = cp4(c.c_out); cd.np = p16(c.c_out);
            std::vector<float> w((size_t)c.k * cd.cpi * cd.np, 0.0f), b(cd.np, 0.0f);
            for (int co = 0; co < c.c_out; ++co) {
                b[co] = c.b[co];
                for (int ci = 0; ci < c.c_in; ++ci)
                    for (int t = 0; t < c.k; ++t)
                        w[((size_t)t * cd.cpi + ci) * cd.np + co] = c.w[((size_t)co * c.c_in + ci) * c.k + (c.k - 1 - t)];
            }
            e = upload(cd.w, w);
            if (e == hipSuccess) e = upload(cd.b, b);
            int xnp = 0;
            if (e == hipSuccess) e = upload(cd.xw, tcn_x3_pack(c.w, c.c_out, c.c_in, c.k, &cd.xsteps, &xnp));
            if (c.k > 1) {
                bd.span += c.k - 1;
                const int64_t add = sat_mul(c.k - 1, rf_dil);
                rf = (rf > INT64_MAX - add) ? INT64_MAX : rf + add;
            }
        }
        if (e == hipSuccess && s.has_shortcut) {
            const int cpi = cp4(bd.c_in), np = p16(bd.c_out);
            std::vector<float> w((size_t)cpi * np, 0.0f), b(np, 0.0f);
            for (int co = 0; co < bd.c_out; ++co) {
                b[co] = s.sc_b[co];
                for (int ci = 0; ci < bd.c_in; ++ci) w[(size_t)ci * np + co] = s.sc_w[(size_t)co * bd.c_in + ci];
            }
            e = upload(bd.sw, w);
            if (e == hipSuccess) e = upload(bd.sb, b);
            int xnp = 0;
            if (e == hipSuccess) e = upload(bd.xsw, tcn_x3_pack(s.sc_w, bd.c_out, bd.c_in, 1, &bd.xsw_steps, &xnp));
        }
        m->blocks.push_back(std::move(bd));
        dil = std::min<int64_t>(kMaxDil, dil * s.base);
        rf_dil = sat_mul(rf_dil, s.base);
    }
    if (e == hipSuccess && m->blocks.back().c_out != c_last) {
        rs_tcn_destroy(m);
        set_error("rs_tcn_create: c_last %d is not the last block's %d channels", c_last, m->blocks.back().c_out);
        return RS_ERR_ARG;
    }
    m->rf = rf;
    if (e == hipSuccess) e = upload(m->d_fcw, std::vector<float>(fc_w, fc_w + 2 * (size_t)c_last));
    if (e == hipSuccess) e = upload(m->d_fcb, std::vector<float>(fc_b, fc_b + 2));
    if (e != hipSuccess) {
        rs_tcn_destroy(m);
        return hip_fail(e, "rs_tcn_create upload");
    }
    *out = m;
    return RS_OK;
}

int rs_tcn_destroy(rs_tcn* m) {
    if (!m) return RS_OK;
    DeviceGuard guard(m->device);
    delete m;                           // every device buffer is a DevBuf: freed with its holder
    return RS_OK;
}

int rs_tcn_set_mode(rs_tcn* m, int dtype) {
    if (!m) {
        set_error("rs_tcn_set_mode: null program");
        return RS_ERR_ARG;
    }
    if (dtype == RS_F32 || dtype == RS_F32W) {
        m->mode = 0;
        return RS_OK;
    }
    if (dtype != RS_BF16X3) {
        set_error("rs_tcn_set_mode: a TCN runs in RS_F32 / RS_F32W (f32-input MFMA) or RS_BF16X3 (split precision on the "
                  "bf16 MFMA)");
        return RS_ERR_ARG;
    }
    m->mode = 1;
    return RS_OK;
}

int64_t rs_tcn_receptive_field(const rs_tcn* m) { return m ? m->rf : 0; }

int rs_tcn_tile_plan(const rs_tcn* m, int block, int B, int ld, int* T, int* nb, int* tiles_pos) {
    if (!m || block < 0 || block >= (int)m->blocks.size() || B < 1 || ld < 1 || !T || !nb || !tiles_pos) {
        set_error("rs_tcn_tile_plan: bad argument");
        return RS_ERR_ARG;
    }
    std::vector<int64_t> need;
    tcn_windows(m, ld, need);
    const int out_rows = (int)need[block + 1];
    int t = 1, n = 1;
    if (choose_tile(m->blocks[block], m->mode, B, out_rows, &t, &n) > (size_t)kLdsBudget) {
        set_error("rs_tcn_tile_plan: block %d is too wide for one tile of LDS", block);
        return RS_ERR_ARG;
    }
    *T = t;
    *nb = n;
    *tiles_pos = (out_rows + t - 1) / t;
    return RS_OK;
}

size_t rs_tcn_workspace_bytes(const rs_tcn* m, int B, int ld) {
    if (!m || B < 1 || ld < 1) return 0;
    return 2 * buffer_bytes(m, B, ld);
}

int rs_tcn_max_batch(const rs_tcn* m, int ld) {
    if (!m || ld < 1) return 0;
    return max_batch_of(buffer_bytes(m, 1, ld));
}

int rs_tcn_forward_ragged(rs_tcn* m, const float* d_x, const int32_t* d_len, int B, int ld, void* d_ws, size_t ws_bytes,
                          float* d_probs, float* d_logits, void* stream) {
    size_t per = 0;                     // one of the two buffers, B reads
    const int rc = check_ragged_call("rs_tcn_forward_ragged", "rs_tcn_max_batch", m, d_x, d_len, d_ws, d_probs, B, ld, ws_bytes, [&] {
        per = buffer_bytes(m, B, ld);
        return RaggedLimits{1, 2 * per, (int64_t)per <= kWindow};
    });
    if (rc != RS_OK) return rc;
    DeviceGuard guard(m->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::vector<int64_t> need;
    tcn_windows(m, ld, need);
    Carver ws(d_ws);
    float* buf[2] = {ws.take(per), ws.take(per)};
    const float* in = d_x;
    const int n = (int)m->blocks.size();
    for (int i = 0; i < n; ++i) {
        const BlockDev& bd = m->blocks[i];
        const int out_rows = (int)need[i + 1];
        if (m->mode == 1) {
            const int rcx = launch_block_x3(bd, i, in, d_len, buf[i & 1], B, ld, (int)need[i], out_rows, st);
            if (rcx != RS_OK) return rcx;
            in = buf[i & 1];
            continue;
        }
        int T = 1, nb = 1;
        choose_tile(bd, 0, B, out_rows, &T, &nb);
        const TilePlan p = plan_tile(bd, T, nb);
        if (p.lds_bytes > (size_t)kLdsBudget) {
            set_error("rs_tcn_forward_ragged: block %d is too wide for one tile of LDS", i);
            return RS_ERR_ARG;
        }
        BlockArgs a;
        memset(&a, 0, sizeof(a));
        a.x = in;
        a.len = d_len;
        a.y = buf[i & 1];
        a.B = B;
        a.ld = ld;
        a.first = i == 0;
        a.dil = std::min<int64_t>(bd.dil, (int64_t)ld + 1);    // beyond ld only m = 0 is a position >= 0 either way
        a.r = bd.base;
        a.in_rows = (int)need[i];
        a.out_rows = out_rows;
        a.cp_in = cp4(bd.c_in);
        a.cp_out = cp4(bd.c_out);
        a.T = T;
        a.nb = nb;
        a.tiles_pos = (out_rows + T - 1) / T;
        a.rows_in = p.rows_in;
        a.nconv = bd.nconv;
        a.jk = bd.jk;
        for (int j = 0; j < bd.nconv; ++j) {
            const ConvDev& c = bd.conv[j];
            a.w[j] = c.w;
            a.b[j] = c.b;
            a.k[j] = c.k;
            a.cpi[j] = c.cpi;
            a.cpo[j] = c.cpo;
            a.np[j] = c.np;
            a.rows[j] = p.rows[j];
            a.step[j] = j == bd.jk ? bd.base : 1;
            a.ostride[j] = j >= bd.jk ? bd.base : 1;
            a.src[j] = j == 0 ? 0 : 1 + ((j - 1) & 1);
            a.dst[j] = j + 1 == bd.nconv ? -1 : 1 + (j & 1);
        }
        a.sw = bd.sw;
        a.sb = bd.sb;
        for (int d = 0; d < 3; ++d) {
            a.off[d] = p.off[d];
            a.pitch[d] = p.pitch[d];
        }
        const int64_t grid = (int64_t)((B + nb - 1) / nb) * a.tiles_pos;
        if (grid > INT32_MAX) {
            set_error("rs_tcn_forward_ragged: grid too large: split the batch");
            return RS_ERR_ARG;
        }
        hipLaunchKernelGGL(tcn_block_kernel, dim3((unsigned)grid), dim3(256), p.lds_bytes, st, a);
        RS_HIP(hipGetLastError());
        in = a.y;
    }
    hipLaunchKernelGGL(last_row_head_kernel<AlwaysValid>, dim3((B + 255) / 256), dim3(256), 0, st, in, B, cp4(m->c_last), m->c_last,
                       m->d_fcw, m->d_fcb, AlwaysValid{}, d_probs, d_logits);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

}  // extern "C"
