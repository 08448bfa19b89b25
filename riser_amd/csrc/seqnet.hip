// Sequential conv programs: the ResNet variant of the reference (riser/nets/resnet.py:7-131) - a secondary
// architecture that riser/model.py cannot even load (it hard-imports ConvNet) and for which no config or weights are
// shipped - and ConvNet configurations outside the shipped class (depth > 1, kernels other than 3:
// riser/nets/cnn.py:17,52-65).  BatchNorm (eval mode) is folded into the preceding conv on the host, so the device
// executes a list of
//   CONV    y = [relu]( conv1d(x; k, stride, pad) + bias [+ residual] )
//   MAXPOOL y = MaxPool1d(2, stride 2, padding 0 | 1)          (cnn.py:64 / the ResNet stem, resnet.py:83)
// over position-major activations [B][T][C] (exactly C channels per row) with one uniform length per batch, then
// GAP -> FC -> softmax.
// CONV runs on the f32-input MFMA (seq_conv_mfma_kernel): in the position-major layout the im2col row of output
// position t IS a contiguous run of memory - x[b][t*s - pad .. t*s - pad + k) x [0, c_in) - so the GEMM
// (M = B * T_out, N = c_out, K = k * c_in) needs no gather: lane (row r, k-group kq) of a 16x16x4 MFMA reads
// xflat[row_base(r) + 4 * step + kq], zero outside the batch element's own [0, T_in * c_in).  The scalar kernel the
// first round shipped (one thread per position x 4 channels) is kept behind RS_SEQ_SCALAR=1 for the comparison.
// Generic over k / stride / pad / widths, not tuned per shape: the hot path of this repository is the ConvNet in
// conv_wino*.hip / conv_ring_h16.hip.
//
// seqnet/conv.hpp, stem_pool.hpp, basic_block.hpp, stem_pool_x3.hpp, bottleneck.hpp, tail.hpp: the kernels, one family each
// seqnet/mfma_split.hpp: the bf16 split helpers (shared with tcn_x3.hip); seqnet/pack.hpp: weight layouts, packer, device buffers
// seqnet/program.hpp: ops, the fused-launch record, the pattern matcher, the planner.  Here: rs_seqnet, the C ABI, the launcher.
#include "common.hpp"

#include <stdlib.h>
#include <string.h>

#include <new>
#include <type_traits>

#include "seqnet/conv.hpp"
#include "seqnet/stem_pool.hpp"
#include "seqnet/basic_block.hpp"
#include "seqnet/stem_pool_x3.hpp"
#include "seqnet/bottleneck.hpp"
#include "seqnet/tail.hpp"
#include "seqnet/program.hpp"

using namespace rs;

struct rs_seqnet : Program {
    int device = 0;
    int num_cu = 256;
    DevBuf<float> d_fcw, d_fcb;
};

namespace {

// ---- run-time tile parameters -> the kernel instantiation: a block kernel's template as a variable template of its tag, one
// select per block family, used for both precisions ----------------------------------------------------------------------------
struct BasicF32 {
    typedef BlockArgs Args;
    template <int NT, int MTW, int WAVES> static constexpr auto kernel = seq_basic_block_kernel<NT, MTW, WAVES>;
};
struct BasicX3 {
    typedef BlockX3Args Args;
    template <int NT, int MTW, int WAVES> static constexpr auto kernel = seq_basic_block_x3_kernel<NT, MTW, WAVES>;
};
struct BneckF32 {
    typedef BneckArgs Args;
    template <int NTM, int NTO> static constexpr auto kernel = seq_bottleneck_block_kernel<NTM, NTO>;
};
struct BneckX3 {
    typedef BneckX3Args Args;
    template <int NTM, int NTO> static constexpr auto kernel = seq_bottleneck_block_x3_kernel<NTM, NTO>;
};

// f(std::integral_constant<int, n>) for the run-time n in [1, N]
template <int N, class F>
auto with_int(int n, F&& f) {
    if constexpr (N == 1)
        return f(std::integral_constant<int, 1>{});
    else
        return n >= N ? f(std::integral_constant<int, N>{}) : with_int<N - 1>(n, f);
}
// a basic block's tile: 4 waves x 1 | 4 waves x 2 | 8 waves x 1 row tiles per wave
template <class K>
auto select_basic(int nt, int mtw, int waves) {
    return with_int<5>(nt, [&](auto NT) {
        constexpr int n = decltype(NT)::value;
        return waves == 8 ? K::template kernel<n, 1, 8> : mtw == 2 ? K::template kernel<n, 2, 4> : K::template kernel<n, 1, 4>;
    });
}
template <class K>
auto select_bneck(int ntm, int nto) {
    return with_int<5>(nto, [&](auto NTO) {
        constexpr int n = decltype(NTO)::value;
        return ntm == 2 ? K::template kernel<2, n> : K::template kernel<1, n>;
    });
}

// a block kernel with its struct of arguments, the whole LDS budget opted in
template <class Args>
hipError_t launch_block(void (*fn)(const Args), int grid, int threads, size_t lds, hipStream_t st, const Args& a) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget);
    if (e == hipSuccess) hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, st, a);
    return e;
}

// one forward: the planner's launches, then the head
int seqnet_forward_impl(rs_seqnet* m, const float* d_x, const int32_t* d_len, int B, int L, void* d_ws, size_t ws_bytes, float* d_probs,
                        float* d_logits, void* stream) {
    if (!m || !d_x || !d_ws || !d_probs || B < 1 || L < 1) {
        set_error("rs_seqnet_forward: bad argument");
        return RS_ERR_ARG;
    }
    std::vector<Launch> plan;
    std::vector<OpShape> shp;
    int last = 0, last_op = -1;
    if (const int rc = plan_launches(m, B, L, d_len != nullptr, plan, shp, last, last_op); rc != RS_OK) return rc;
    const size_t per = buffer_bytes(m, B, L);
    if (ws_bytes < rs_seqnet_workspace_bytes(m, B, L)) {
        set_error("rs_seqnet_forward: workspace too small");
        return RS_ERR_WORKSPACE;
    }
    DeviceGuard guard(m->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto buf = [&](int i) -> float* {
        return i == 0 ? const_cast<float*>(d_x) : reinterpret_cast<float*>(static_cast<char*>(d_ws) + per * (size_t)(i - 1));
    };
    // ragged batch: the rows of every read after every op, computed on the device from its length (no host copy needed);
    // L is then the row pitch of d_x and every buffer keeps the pitches of an L-sample read
    int32_t* table = nullptr;
    std::vector<int> prod(m->ops.size(), -1);
    if (d_len) {
        table = reinterpret_cast<int32_t*>(static_cast<char*>(d_ws) + per * (size_t)(m->n_buffers - 1));
        LenRecipe rc;
        memset(&rc, 0, sizeof(rc));
        rc.n_ops = (int)m->ops.size();
        for (size_t k = 0; k < m->ops.size(); ++k) {
            const OpDev& o = m->ops[k];
            for (size_t j = 0; j < k; ++j)
                if (m->ops[j].dst == o.src) prod[k] = (int)j;
            rc.kind[k] = (signed char)o.kind;
            rc.pad[k] = (signed char)o.pad;
            rc.k[k] = (short)o.k;
            rc.stride[k] = (short)(o.stride > 0 ? o.stride : 1);
            rc.prod[k] = (short)prod[k];
        }
        hipLaunchKernelGGL(seq_lengths_kernel, dim3((B + 255) / 256), dim3(256), 0, st, d_len, B, L, rc, table);
        RS_HIP(hipGetLastError());
    }
    auto rows_after = [&](int op) -> const int32_t* { return table ? table + (size_t)(op + 1) * B : nullptr; };   // op = -1: the input
    // workgroups per CU that `lds` bytes each leave room for, at most `cap`
    auto per_cu = [](size_t lds, size_t cap) { return (int)std::max<size_t>(1, std::min<size_t>(cap, kLdsBudget / std::max<size_t>(lds, 1))); };
    for (const Launch& l : plan) {
        const size_t k = (size_t)l.op;
        const OpDev& o = m->ops[k];
        const FusedBlock& f = o.fb;
        const OpShape& sh = shp[k];
        // what the four block kernels' argument structs share; sin / sout: the shapes of the block's first and last strided op
        auto fill_block = [&](auto& a, const OpShape& sin, const OpShape& sout, int out_op, int rows_per_tile) {
            a.x = buf(f.src);
            a.x_bytes = (unsigned)((int64_t)B * sin.t_in * f.c_in * 4);
            a.y = buf(f.dst);
            a.b1 = f.b1;
            a.b2 = f.b2;
            a.B = B;
            a.T_in = sin.t_in;
            a.T_out = sout.t_out;
            a.c_in = f.c_in;
            a.c_out = f.c_out;
            a.stride = f.stride;
            a.Ksc = f.ksc;
            a.tin = rows_after(prod[f.first]);
            a.tout = rows_after(out_op);
            a.tiles_per_read = (sout.t_out + rows_per_tile - 1) / rows_per_tile;
            a.n_tiles = B * a.tiles_per_read;
            return std::min(a.n_tiles, m->num_cu * per_cu(l.lds, 4));      // the grid
        };
        if (l.family == RS_SEQ_STEM_POOL) {
            const OpShape& ps = shp[k + 1];
            const int rows = B * 2 * ps.t_out;
            const int n_tiles = (rows + kGemmTileRows - 1) / kGemmTileRows;
            const int grid = std::min(n_tiles, m->num_cu * per_cu(l.lds, 8));
            const unsigned x_bytes = (unsigned)((int64_t)B * sh.t_in * 4);
            if (l.x3) {
                auto fx = with_int<5>(o.nt, [](auto NT) { return seq_stem_pool_x3_kernel<decltype(NT)::value>; });
                RS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fx), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmallKernelLds));
                hipLaunchKernelGGL(fx, dim3(grid), dim3(256), l.lds, st, buf(f.src), x_bytes, f.x3.w1, o.d_b, buf(f.dst), B, sh.t_in,
                                   sh.t_out, ps.t_out, o.c_out, o.k * o.c_in, f.x3.s1, o.stride, o.pad, n_tiles, rows_after(prod[k]),
                                   rows_after((int)k));
            } else {
                auto fn = with_int<5>(o.nt, [](auto NT) { return seq_stem_pool_kernel<decltype(NT)::value>; });
                RS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmallKernelLds));
                hipLaunchKernelGGL(fn, dim3(grid), dim3(256), l.lds, st, buf(f.src), x_bytes, o.d_wq, o.d_b, buf(f.dst), B, sh.t_in,
                                   sh.t_out, ps.t_out, o.c_out, o.k * o.c_in, o.stride, o.pad, n_tiles, rows_after(prod[k]),
                                   rows_after((int)k));
            }
        } else if (l.family == RS_SEQ_BASIC_BLOCK) {
            const OpShape& s1 = shp[f.first];
            auto run = [&](auto fam, const auto& w) {
                typename decltype(fam)::Args a;
                const int grid = fill_block(a, s1, s1, f.first, 16 * l.mtw * l.waves - 2);
                a.NPs = w.np_out;
                a.Cp = w.cp;
                a.K1 = 3 * f.c_in;
                if constexpr (std::is_same_v<decltype(fam), BasicX3>) {
                    a.w1 = w.w1;
                    a.w2 = w.w2;
                    a.S1 = w.s1;
                    a.S2a = w.s2;
                    a.Ssc = w.ssc;
                } else {
                    a.w1q = w.w1;
                    a.w2q = w.w2;
                    a.K2a = 3 * w.cp;
                }
                return launch_block(select_basic<decltype(fam)>(l.nt, l.mtw, l.waves), grid, 64 * l.waves, l.lds, st, a);
            };
            RS_HIP(l.x3 ? run(BasicX3{}, f.x3) : run(BasicF32{}, f.f32));
        } else if (l.family == RS_SEQ_BOTTLENECK) {
            auto run = [&](auto fam, const auto& w) {
                typename decltype(fam)::Args a;
                const int R2 = (kBneckRows - 3) / f.stride + 1;
                const int grid = fill_block(a, shp[f.first], shp[f.first + 1], f.first + 1, R2);
                a.b3 = f.b3;
                a.NPm = w.np_mid;
                a.NPo = w.np_out;
                a.c_mid = f.c_mid;
                a.Cmp = w.cp;
                a.R2 = R2;
                if constexpr (std::is_same_v<decltype(fam), BneckX3>) {
                    a.w1 = w.w1; a.w2 = w.w2; a.w3 = w.w3;
                    a.S1 = w.s1; a.S2 = w.s2; a.S3 = w.s3; a.Ssc = w.ssc;
                } else {
                    a.w1q = w.w1; a.w2q = w.w2; a.w3q = w.w3;
                }
                return launch_block(select_bneck<decltype(fam)>(l.ntm, l.nt), grid, 256, l.lds, st, a);
            };
            RS_HIP(l.x3 ? run(BneckX3{}, f.x3) : run(BneckF32{}, f.f32));
        } else if (l.family == RS_SEQ_CONV_SCALAR) {
            const int cq = (o.c_out + 3) / 4;
            const int64_t total = (int64_t)B * sh.t_out * cq;
            hipLaunchKernelGGL(seq_conv_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, buf(o.src),
                               o.d_w, o.d_b, o.add >= 0 ? buf(o.add) : nullptr, buf(o.dst), B, sh.t_in, sh.t_out,
                               o.c_in, o.c_out, cq, o.k, o.stride, o.pad, o.relu);
        } else if (l.family == RS_SEQ_CONV_MFMA_LDS) {
            const int64_t rows = (int64_t)B * sh.t_out;
            const int n_tiles = (int)((rows + kGemmTileRows - 1) / kGemmTileRows);
            auto fn = with_int<5>(o.nt, [](auto NT) { return seq_conv_mfma_lds_kernel<decltype(NT)::value>; });
            RS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmallKernelLds));
            // small workgroups (256 threads, <= 96 KB LDS, few registers): as many per CU as the weights in LDS allow
            const int grid = std::min(n_tiles, m->num_cu * per_cu(l.lds, 8));
            hipLaunchKernelGGL(fn, dim3(grid), dim3(256), l.lds, st, buf(o.src), (unsigned)((int64_t)B * sh.t_in * o.c_in * 4),
                               o.d_wq, o.d_b, o.add >= 0 ? buf(o.add) : nullptr, buf(o.dst), B, sh.t_in, sh.t_out, o.c_in,
                               o.c_out, o.k * o.c_in, o.stride, o.pad, o.relu, n_tiles);
        } else if (l.family == RS_SEQ_CONV_MFMA) {
            const int64_t rows = (int64_t)B * sh.t_out;
            const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((o.c_out + 16 * l.nt - 1) / (16 * l.nt)));
            auto fn = l.nt == 1 ? seq_conv_mfma_kernel<1> : l.nt == 2 ? seq_conv_mfma_kernel<2> : seq_conv_mfma_kernel<4>;
            hipLaunchKernelGGL(fn, grid, dim3(256), 0, st, buf(o.src), o.d_w, o.d_b, o.add >= 0 ? buf(o.add) : nullptr,
                               buf(o.dst), B, sh.t_in, sh.t_out, o.c_in, o.c_out, l.np, o.k * o.c_in, o.stride, o.pad,
                               o.relu);
        } else {
            const int64_t total = (int64_t)B * sh.t_out * sh.c;
            hipLaunchKernelGGL(seq_maxpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                               buf(o.src), buf(o.dst), B, sh.t_in, sh.t_out, sh.c, o.pad);
        }
        RS_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(gap_head_kernel<false>, dim3(B), dim3(256), 0, st, buf(last), shp[last_op].t_out, m->c_last, m->c_last,
                       m->d_fcw, m->d_fcb, rows_after(last_op), d_probs, d_logits);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

}  // namespace

extern "C" {

int rs_seqnet_create(const rs_seq_op* ops, int n_ops, int n_buffers, const float* fc_w, const float* fc_b, int c_last,
                     int device, rs_seqnet** out) {
    if (!ops || n_ops < 1 || n_buffers < 2 || n_buffers > 16 || !fc_w || !fc_b || !out || c_last < 1) {
        set_error("rs_seqnet_create: bad argument");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    DeviceGuard guard(device);            // the caller's current device is restored on return
    RS_HIP(guard.err);
    rs_seqnet* m = new (std::nothrow) rs_seqnet();
    if (!m) return RS_ERR_OOM;
    m->device = device;
    m->n_buffers = n_buffers;
    m->c_last = c_last;
    m->scalar_conv = getenv("RS_SEQ_SCALAR") != nullptr;
    if (const char* e = getenv("RS_SEQ_WINDOW_BYTES"); e && atoll(e) > 0) m->window = std::min<int64_t>(atoll(e), 0x7fffffffLL);
    m->bneck_x3 = getenv("RS_SEQ_BNECK_X3") != nullptr;
    HostPtrs hw, hb;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) m->num_cu = cus;
    }
    for (int i = 0; i < n_ops; ++i) {
        const rs_seq_op& s = ops[i];
        OpDev o;
        o.kind = s.kind; o.src = s.src; o.dst = s.dst; o.add = s.add;
        o.c_in = s.c_in; o.c_out = s.c_out; o.k = s.k; o.stride = s.stride; o.pad = s.pad; o.relu = s.relu;
        const bool bad_buf = s.src < 0 || s.src >= n_buffers || s.dst < 1 || s.dst >= n_buffers || s.dst == s.src ||
                             s.add >= n_buffers || s.add == s.dst;
        if (bad_buf || (s.kind != 0 && s.kind != 1) || (s.kind == 1 && s.pad != 0 && s.pad != 1) ||
            (s.kind == 0 && (!s.w || !s.b || s.c_in < 1 || s.c_out < 1 || s.k < 1 || s.stride < 1 || s.pad < 0))) {
            rs_seqnet_destroy(m);
            set_error("rs_seqnet_create: bad op %d", i);
            return RS_ERR_ARG;
        }
        hipError_t e = hipSuccess;
        if (s.kind == 0) {
            const int cq = (s.c_out + 3) / 4;
            std::vector<float> wp((size_t)s.k * s.c_in * cq * 4, 0.0f), bp((size_t)cq * 4, 0.0f);
            for (int co = 0; co < s.c_out; ++co) {
                bp[co] = s.b[co];
                for (int ci = 0; ci < s.c_in; ++ci)
                    for (int kk = 0; kk < s.k; ++kk)
                        wp[((size_t)kk * s.c_in + ci) * cq * 4 + co] = s.w[((size_t)co * s.c_in + ci) * s.k + kk];
            }
            e = upload(o.d_w, wp);
            if (e == hipSuccess) e = upload(o.d_b, bp);
            // MFMA packing: element (kidx, n) of the im2col GEMM at [kidx / 4][n][kidx % 4], K padded to 16, N to 16
            const int K16 = round_up(s.k * s.c_in, 16), nt = (s.c_out + 15) / 16;
            if (e == hipSuccess && nt <= 5 && (size_t)K16 * nt * 16 * 4 <= kSmallKernelLds) {
                e = pack_upload<PackF32>(o.d_wq, (size_t)K16 * nt * 16, 16 * nt, s.c_out, {{s.w, s.c_in, s.k, s.c_in, 0}});
                o.nt = nt;
            }
        }
        m->ops.push_back(std::move(o));
        hw.push_back(s.kind == 0 ? s.w : nullptr);
        hb.push_back(s.kind == 0 ? s.b : nullptr);
        if (e != hipSuccess) {
            rs_seqnet_destroy(m);
            return hip_fail(e, "rs_seqnet_create upload");
        }
    }
    if (getenv("RS_SEQ_NOFUSE") == nullptr && !m->scalar_conv) {   // (RS_SEQ_NOFUSE=1: one launch per op, as the program is written)
        const hipError_t fe = fuse_program(m->ops, hw, hb);
        if (fe != hipSuccess) {
            rs_seqnet_destroy(m);
            return hip_fail(fe, "rs_seqnet_create fused packing");
        }
    }
    hipError_t e = upload(m->d_fcw, std::vector<float>(fc_w, fc_w + (size_t)2 * c_last));
    if (e == hipSuccess) e = upload(m->d_fcb, std::vector<float>(fc_b, fc_b + 2));
    if (e != hipSuccess) {
        rs_seqnet_destroy(m);
        return hip_fail(e, "rs_seqnet_create upload");
    }
    *out = m;
    return RS_OK;
}

int rs_seqnet_destroy(rs_seqnet* m) {
    if (!m) return RS_OK;
    DeviceGuard guard(m->device);
    delete m;                             // every device buffer is freed by its holder
    return RS_OK;
}

int rs_seqnet_set_mode(rs_seqnet* m, int dtype) {
    if (!m) {
        set_error("rs_seqnet_set_mode: null program");
        return RS_ERR_ARG;
    }
    if (dtype == RS_F32 || dtype == RS_F32W) {
        m->mode = 0;
        return RS_OK;
    }
    if (dtype != RS_BF16X3) {
        set_error("rs_seqnet_set_mode: generic conv programs run in RS_F32 or RS_BF16X3 (split precision on the bf16 MFMA)");
        return RS_ERR_ARG;
    }
    // split precision covers the stem and the residual BASIC blocks of a program (where a ResNet's time is), and its bottleneck
    // blocks when RS_SEQ_BNECK_X3 was set at create (measured slower than their fp32 form: off); the head and unfused ops keep
    // fp32.  A program without a single fused residual block has nothing to switch.
    bool any = false;
    for (const OpDev& o : m->ops) any = any || ((o.fb.kind == FUSE_BASIC || o.fb.kind == FUSE_BOTTLENECK) && o.fb.has_x3());
    if (!any) {
        set_error("rs_seqnet_set_mode: this program has no residual block that runs in split precision");
        return RS_ERR_ARG;
    }
    m->mode = 1;
    return RS_OK;
}

size_t rs_seqnet_workspace_bytes(const rs_seqnet* m, int B, int L) {
    if (!m || B < 1 || L < 1) return 0;
    const size_t per = buffer_bytes(m, B, L);
    if (!per) return 0;
    // the activation buffers, then the per-read length table of a ragged forward ((ops + 1) x B)
    return per * (size_t)(m->n_buffers - 1) + ((m->ops.size() + 1) * (size_t)B * 4 + 255) / 256 * 256;
}

int rs_seqnet_max_batch(const rs_seqnet* m, int L) {
    // every activation buffer of B reads stays inside one buffer window: B x (the largest buffer of one read) bytes
    if (!m || L < 1) return 0;
    const size_t per = buffer_bytes(m, 1, L);
    if (!per) return 0;
    return (int)std::max<int64_t>(1, std::min<int64_t>(1 << 30, (m->window - 4096) / (int64_t)per));
}

int rs_seqnet_forward(rs_seqnet* m, const float* d_x, int B, int L, void* d_ws, size_t ws_bytes, float* d_probs,
                      float* d_logits, void* stream) {
    return seqnet_forward_impl(m, d_x, nullptr, B, L, d_ws, ws_bytes, d_probs, d_logits, stream);
}

int rs_seqnet_forward_ragged(rs_seqnet* m, const float* d_x, const int32_t* d_len, int B, int ld, void* d_ws, size_t ws_bytes,
                             float* d_probs, float* d_logits, void* stream) {
    if (!d_len) {
        set_error("rs_seqnet_forward_ragged: null lengths");
        return RS_ERR_ARG;
    }
    return seqnet_forward_impl(m, d_x, d_len, B, ld, d_ws, ws_bytes, d_probs, d_logits, stream);
}

int rs_seqnet_ragged_ok(const rs_seqnet* m) { return m && all_fused(m) ? 1 : 0; }

int rs_seqnet_launch_plan(const rs_seqnet* m, int B, int L, int ragged, rs_seq_launch* out, int cap, int* n) {
    if (!m || !n || B < 1 || L < 1 || cap < 0 || (cap > 0 && !out)) {
        set_error("rs_seqnet_launch_plan: bad argument");
        return RS_ERR_ARG;
    }
    std::vector<Launch> plan;
    std::vector<OpShape> shp;
    int last = 0, last_op = -1;
    const int rc = plan_launches(m, B, L, ragged != 0, plan, shp, last, last_op);
    if (rc != RS_OK) return rc;
    for (size_t i = 0; i < plan.size() && (int)i < cap; ++i) out[i] = plan[i];
    *n = (int)plan.size();
    return RS_OK;
}

}  // extern "C"
