// Generic ConvNets (riser/nets/cnn.py:12-18,43-65 at any depth and odd kernel): n_layers x [depth x (Conv1d(k, stride 1,
// 'same') + bias + ReLU), MaxPool1d(2, 2)], then GAP + FC + softmax.
//
// Activations are position-major fp32 [read][t][cp4(C)], every buffer at the pitches of an ld-sample read: after l pools a
// read owns ld >> l rows of its buffer and uses the first len >> l of them.  Three kernels:
//
//   gconv_lengths_kernel   table[l][b] = clamp(len[b], 0, ld) >> l, l = 0 .. n_layers: the rows of read b behind l pools.
//   gconv_tile_kernel      one launch per conv, on v_mfma_f32_16x16x4_f32.  A workgroup (4 waves) owns a tile of conv positions
//                          of ONE read times a block of output channels.  K runs over input-channel chunks, then taps, then
//                          groups of 4 vec channels, ascending.  Per chunk the workgroup stages the activation slab (tile rows
//                          + k - 1 halo rows x chunk channels) into LDS once and reads it for all k taps, and next to it the
//                          chunk's weight panel, packed at create in the order the lanes read it (gconv/plan.hpp).  A slab
//                          position before the read's row 0, at or behind its own row count, or in a pad channel is an exact
//                          zero by select: what lies behind a read in its buffer is never multiplied.  Epilogue: bias + ReLU;
//                          in the POOL form (a layer's last conv) the max of conv rows 2j and 2j + 1 - elements (0, 1) and
//                          (2, 3) of one lane's accumulator - so that only pooled rows are written and no pool launch exists.
//   gap_head_kernel        (family/head.hpp) GAP over a read's own rows + FC + softmax; a read with no row left gets NaN.
//
// The tile shape and the chunk size depend on the conv's (c_in, c_out, k) only, never on the batch: every output element is
// one fixed k-ordered MFMA chain and a read gets its solo bits in any batch, at any ld.
//
// rs_gconv_set_mode(m, RS_BF16X3) runs every conv with c_in > 4 on gconv_tile_x3_kernel instead (csrc/gconv_x3.hip: split
// precision on the bf16 MFMA, the same plan, grid, buffers and epilogue); the other two kernels serve both modes.
#include "device_prelude.hpp"
#include "family/head.hpp"
#include "family/host.hpp"
#include "gconv/plan.hpp"
#include "gconv_x3.hpp"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

namespace rs {
namespace {

using namespace gconv;


__global__ __launch_bounds__(256) void gconv_lengths_kernel(const int32_t* __restrict__ len, int B, int ld, int n_pools,
                                                            int32_t* __restrict__ table) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int L = min(max(len[b], 0), ld);                  // a length beyond the row pitch would read the next read's row
    for (int l = 0; l <= n_pools; ++l) table[(size_t)l * B + b] = L >> l;
}

struct TileArgs {
    const float* x;             // [B][in_rows][in_pitch]
    float* y;                   // [B][out_rows][out_pitch]
    const int32_t* rows;        // [B] rows of each read at this conv's input
    const float* w;             // packed, gconv/plan.hpp
    const float* b;             // [cols of every block], zero padded
    int in_rows, in_pitch, out_rows, out_pitch;
    int c_in, c_out, k, kc, nchunk, lpitch, slab_floats, panel_floats, tiles;
};

template <int VEC>
__device__ __forceinline__ void load_frag(float (&d)[VEC], const float* p) {
    if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = v[i];
    } else {
        d[0] = p[0];
    }
}

template <int RT, int WGC, int WC, int VEC, bool POOL>
__global__ __launch_bounds__(256) void gconv_tile_kernel(const TileArgs a) {
    constexpr int WGR = 4 / WGC, RW = RT / WGR;             // wave rows of the workgroup, row tiles per wave
    constexpr int ROWS = 16 * RT, NCOL = 16 * WC * WGC, KG = 4 * VEC;
    static_assert(RW >= 1 && RW * WGR == RT, "row tiles split evenly over the wave rows");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rl = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / a.tiles, tile = blockIdx.x - b * a.tiles;
    const int q0 = tile * ROWS;
    const int T = as_const_len(a.rows)[b];
    if (q0 >= T) return;                                    // the whole workgroup: no barrier is skipped by a part of it
    const int nb = blockIdx.y;
    const int wr = wave / WGC, wc = wave - wr * WGC;
    float* slab = lds;
    float* panel = lds + a.slab_floats;
    const int G = a.kc / KG, c4n = a.kc / 4;
    const int pad = a.k >> 1, rows_in = ROWS + a.k - 1;
    const float* xb = a.x + (int64_t)b * a.in_rows * a.in_pitch;
    const float* wp = a.w + (int64_t)nb * a.nchunk * a.panel_floats;
    const bool in_vec = (a.in_pitch & 3) == 0;
    const int col0 = nb * NCOL + 16 * WC * wc;              // this wave's first column

    f32x4 acc[RW][WC];
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
        for (int j = 0; j < WC; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int chunk = 0; chunk < a.nchunk; ++chunk) {
        if (chunk) __syncthreads();
        for (int e = threadIdx.x; e < rows_in * c4n; e += 256) {
            const int r = e / c4n, c4 = e - r * c4n;
            const int q = q0 - pad + r, ch = chunk * a.kc + 4 * c4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q >= 0 && q < T && ch < a.c_in) {
                const float* p = xb + (int64_t)q * a.in_pitch + ch;
                if (in_vec) {
                    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = ch + i < a.c_in ? t[i] : 0.0f;     // pad channels are never written
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (ch + i < a.c_in) v[i] = p[i];
                }
            }
            *reinterpret_cast<f32x4*>(slab + r * a.lpitch + 4 * c4) = v;
        }
        {
            const f32x4* src = reinterpret_cast<const f32x4*>(wp + (int64_t)chunk * a.panel_floats);
            f32x4* dst = reinterpret_cast<f32x4*>(panel);
            for (int e = threadIdx.x; e < a.panel_floats / 4; e += 256) dst[e] = src[e];
        }
        __syncthreads();
        if (col0 >= a.c_out) continue;                      // a wave without columns only stages
        for (int tap = 0; tap < a.k; ++tap) {
            const float* Ar = slab + (16 * RW * wr + rl + tap) * a.lpitch + VEC * kq;
            const float* Bp = panel + ((int64_t)(WC * wc * a.k + tap) * G) * (64 * VEC) + lane * VEC;
            for (int g = 0; g < G; ++g) {
                float av[RW][VEC], bv[WC][VEC];
#pragma unroll
                for (int i = 0; i < RW; ++i) load_frag<VEC>(av[i], Ar + 16 * i * a.lpitch + KG * g);
#pragma unroll
                for (int j = 0; j < WC; ++j) load_frag<VEC>(bv[j], Bp + (int64_t)(j * a.k * G + g) * (64 * VEC));
#pragma unroll
                for (int sub = 0; sub < VEC; ++sub)
#pragma unroll
                    for (int i = 0; i < RW; ++i)
#pragma unroll
                        for (int j = 0; j < WC; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][sub], bv[j][sub], acc[i][j], 0, 0, 0);
            }
        }
    }
    // lane element e of row tile i: conv row q0 + 16 (RW wr + i) + 4 kq + e, column col0 + 16 j + rl
    float* yb = a.y + (int64_t)b * a.out_rows * a.out_pitch;
#pragma unroll
    for (int j = 0; j < WC; ++j) {
        const int col = col0 + 16 * j + rl;
        if (col >= a.c_out) continue;
        const float bias = a.b[col];
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            const int row = q0 + 16 * (RW * wr + i) + 4 * kq;
            if constexpr (POOL) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int p = (row >> 1) + h;
                    // max(relu(u + bias), relu(v + bias)) == relu(max(u, v) + bias): rounding is monotonic
                    if (p < (T >> 1))
                        yb[(int64_t)p * a.out_pitch + col] = fmaxf(fmaxf(acc[i][j][2 * h], acc[i][j][2 * h + 1]) + bias, 0.0f);
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (row + e < T) yb[(int64_t)(row + e) * a.out_pitch + col] = fmaxf(acc[i][j][e] + bias, 0.0f);
            }
        }
    }
}

typedef void (*TileFn)(const TileArgs);

template <int RT, int WGC, int WC>
TileFn tile_fn_of(int vec, bool pool) {
    if (vec == 1) return pool ? gconv_tile_kernel<RT, WGC, WC, 1, true> : gconv_tile_kernel<RT, WGC, WC, 1, false>;
    return pool ? gconv_tile_kernel<RT, WGC, WC, 4, true> : gconv_tile_kernel<RT, WGC, WC, 4, false>;
}

TileFn tile_fn(int shape, int vec, bool pool) {
    switch (shape) {
        case 0: return tile_fn_of<4, 1, 2>(vec, pool);
        case 1: return tile_fn_of<4, 2, 2>(vec, pool);
        case 2: return tile_fn_of<4, 4, 2>(vec, pool);
        case 3: return tile_fn_of<1, 4, 1>(vec, pool);
        default: return tile_fn_of<1, 4, 2>(vec, pool);
    }
}

struct ConvDev {
    int c_in = 0, c_out = 0, k = 0, pool = 0, level = 0;    // level: pools in front of this conv
    TilePlan plan{};
    DevBuf<float> w, b;
    X3Plan x3{};                                            // rs_gconv_set_mode: plan.vec == 4 only
    DevBuf<uint16_t> wx;                                    // pack_weights_x3, from the first switch to RS_BF16X3 on
};

}  // namespace
}  // namespace rs

struct rs_gconv {
    int device = 0;
    int n_layers = 0, depth = 0, c_last = 0;
    int mode = 0;               // rs_gconv_set_mode: 0 fp32 (f32-input MFMA), 1 split precision on the bf16 MFMA
    std::vector<rs::ConvDev> convs;
    rs::DevBuf<float> d_fcw, d_fcb;
};

namespace rs {
namespace {

// bytes of one ping-pong buffer per read of pitch ld: the largest conv output
size_t per_read_bytes(const rs_gconv* m, int ld) {
    size_t per = 0;
    for (const ConvDev& c : m->convs)
        per = std::max(per, (size_t)(ld >> (c.level + c.pool)) * cp4(c.c_out) * 4);
    return per;
}

}  // namespace
}  // namespace rs

using namespace rs;

extern "C" {

int rs_gconv_layer_plan(int c_in, int c_out, int k, rs_gconv_plan* out) {
    TilePlan p;
    if (!out || c_in < 1 || c_out < 1 || k < 1 || (k & 1) == 0 || !plan_conv(c_in, c_out, k, &p)) {
        set_error("rs_gconv_layer_plan: bad argument, an even kernel, or a conv no tile shape holds in LDS");
        return RS_ERR_ARG;
    }
    out->rows = kShapes[p.shape].rows();
    out->cols = kShapes[p.shape].cols();
    out->kc = p.kc;
    out->n_chunks = p.nchunk;
    out->vec = p.vec;
    out->lds_bytes = p.lds_bytes;
    out->shape = p.shape;
    out->reserved = 0;
    return RS_OK;
}

int rs_gconv_destroy(rs_gconv* m) {
    if (!m) return RS_OK;
    DeviceGuard guard(m->device);
    delete m;                           // every device buffer is a DevBuf: freed with its holder
    return RS_OK;
}

int rs_gconv_create(const rs_gconv_conv* convs, int n_layers, int depth, const float* fc_w, const float* fc_b, int device,
                    rs_gconv** out) {
    if (!out) {
        set_error("rs_gconv_create: null output handle");
        return RS_ERR_ARG;
    }
    *out = nullptr;
    if (!convs || n_layers < 1 || depth < 1 || depth > 64 || !fc_w || !fc_b) {
        set_error("rs_gconv_create: bad argument (convs, n_layers >= 1, depth 1-64, fc weights)");
        return RS_ERR_ARG;
    }
    if (n_layers > kMaxPools) {
        set_error("rs_gconv_create: %d layers: the length table holds %d pools", n_layers, kMaxPools);
        return RS_ERR_ARG;
    }
    std::vector<TilePlan> plans((size_t)n_layers * depth);
    for (int i = 0; i < n_layers * depth; ++i) {
        const rs_gconv_conv& c = convs[i];
        const int ci = i == 0 ? 1 : convs[i - 1].c_out;
        if (!c.w || !c.b || c.c_in != ci || c.c_out < 1 || c.k < 1) {
            set_error("rs_gconv_create: bad conv %d (chained channels from 1, k >= 1, weights and bias)", i);
            return RS_ERR_ARG;
        }
        if ((c.k & 1) == 0) {
            set_error("rs_gconv_create: conv %d has the even kernel %d: 'same' pads it asymmetrically", i, c.k);
            return RS_ERR_ARG;
        }
        if (!plan_conv(c.c_in, c.c_out, c.k, &plans[i])) {
            set_error("rs_gconv_create: conv %d (%d -> %d channels, kernel %d): the slab and the weight panel of one chunk "
                      "fit no tile shape's %d KB of LDS", i, c.c_in, c.c_out, c.k, kLdsMax / 1024);
            return RS_ERR_ARG;
        }
    }
    DeviceGuard guard(device);
    RS_HIP(guard.err);
    rs_gconv* m = new (std::nothrow) rs_gconv();
    if (!m) return RS_ERR_OOM;
    m->device = device;
    m->n_layers = n_layers;
    m->depth = depth;
    m->c_last = convs[n_layers * depth - 1].c_out;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n_layers * depth && e == hipSuccess; ++i) {
        const rs_gconv_conv& c = convs[i];
        ConvDev cd;
        cd.c_in = c.c_in; cd.c_out = c.c_out; cd.k = c.k;
        cd.level = i / depth;
        cd.pool = (i % depth) == depth - 1;
        cd.plan = plans[i];
        std::vector<float> b((size_t)cd.plan.ncb * kShapes[cd.plan.shape].cols(), 0.0f);
        std::copy(c.b, c.b + c.c_out, b.begin());
        // beyond 64 KB of dynamic LDS a kernel needs leave: once per handle, here, so that the forward path only launches.
        // The limit is the family's cap, not this plan's bytes: handles share an instantiation, and a later one may need more
        if (cd.plan.lds_bytes > 64 * 1024)
            e = hipFuncSetAttribute(reinterpret_cast<const void*>(tile_fn(cd.plan.shape, cd.plan.vec, cd.pool != 0)),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
        if (e == hipSuccess) e = upload(cd.w, pack_weights(c.w, c.c_in, c.c_out, c.k, cd.plan));
        if (e == hipSuccess) e = upload(cd.b, b);
        m->convs.push_back(std::move(cd));
    }
    if (e == hipSuccess) e = upload(m->d_fcw, std::vector<float>(fc_w, fc_w + 2 * (size_t)m->c_last));
    if (e == hipSuccess) e = upload(m->d_fcb, std::vector<float>(fc_b, fc_b + 2));
    if (e != hipSuccess) {
        rs_gconv_destroy(m);
        return hip_fail(e, "rs_gconv_create upload");
    }
    *out = m;
    return RS_OK;
}

int rs_gconv_set_mode(rs_gconv* m, int dtype) {
    if (!m) {
        set_error("rs_gconv_set_mode: null handle");
        return RS_ERR_ARG;
    }
    if (dtype == RS_F32 || dtype == RS_F32W) {
        m->mode = 0;
        return RS_OK;
    }
    if (dtype != RS_BF16X3) {
        set_error("rs_gconv_set_mode: a generic ConvNet runs in RS_F32 / RS_F32W (f32-input MFMA) or RS_BF16X3 (split "
                  "precision on the bf16 MFMA)");
        return RS_ERR_ARG;
    }
    for (size_t i = 0; i < m->convs.size(); ++i) {
        ConvDev& c = m->convs[i];
        if (c.plan.vec != 4) continue;
        c.x3 = plan_x3(c.plan, c.k);
        if (c.x3.lds_bytes > kLdsMax) {
            set_error("rs_gconv_set_mode: conv %d (%d -> %d channels, kernel %d): the split slab and weight panel of one chunk "
                      "take %d bytes of LDS, more than %d KB", (int)i, c.c_in, c.c_out, c.k, c.x3.lds_bytes, kLdsMax / 1024);
            return RS_ERR_ARG;
        }
    }
    DeviceGuard guard(m->device);
    RS_HIP(guard.err);
    for (ConvDev& c : m->convs) {
        if (c.plan.vec != 4 || c.wx) continue;              // packed on the first switch, kept until rs_gconv_destroy
        std::vector<float> packed((size_t)c.plan.ncb * c.plan.nchunk * c.plan.panel_floats);
        RS_HIP(hipMemcpy(packed.data(), c.w, packed.size() * sizeof(float), hipMemcpyDeviceToHost));
        const std::vector<float> w = unpack_weights(packed.data(), c.c_in, c.c_out, c.k, c.plan);
        if (c.x3.lds_bytes > 64 * 1024) RS_HIP(gconv_x3_allow_lds(c.plan.shape, c.pool != 0, kLdsMax));
        DevBuf<uint16_t> wx;
        const hipError_t e = upload(wx, pack_weights_x3(w.data(), c.c_in, c.c_out, c.k, c.plan));
        if (e != hipSuccess) return hip_fail(e, "rs_gconv_set_mode upload");
        c.wx = std::move(wx);
    }
    m->mode = 1;
    return RS_OK;
}

int rs_gconv_x3_layout(int c_in, int c_out, int k, rs_gconv_x3_plan* out, const float* w, uint16_t* packed) {
    TilePlan p;
    if (!out || c_in < 5 || c_out < 1 || k < 1 || (k & 1) == 0 || !plan_conv(c_in, c_out, k, &p)) {
        set_error("rs_gconv_x3_layout: bad argument, c_in <= 4 (such a conv stays fp32), an even kernel, or a conv no tile shape "
                  "holds in LDS");
        return RS_ERR_ARG;
    }
    const X3Plan x = plan_x3(p, k);
    if (x.lds_bytes > kLdsMax) {
        set_error("rs_gconv_x3_layout: the split slab and weight panel of one chunk take %d bytes of LDS, more than %d KB",
                  x.lds_bytes, kLdsMax / 1024);
        return RS_ERR_ARG;
    }
    out->steps = x.steps;
    out->slab_rows = x.slab_rows;
    out->slab_pitch = x.xpitch;
    out->lds_bytes = x.lds_bytes;
    out->plane = (int64_t)p.ncb * p.nchunk * x.panel_half;
    if (w && packed) {
        const std::vector<uint16_t> v = pack_weights_x3(w, c_in, c_out, k, p);
        memcpy(packed, v.data(), v.size() * sizeof(uint16_t));
    }
    return RS_OK;
}

int rs_gconv_min_length(const rs_gconv* m) {
    if (!m) {
        set_error("rs_gconv_min_length: null handle");
        return RS_ERR_ARG;
    }
    return 1 << m->n_layers;
}

size_t rs_gconv_workspace_bytes(const rs_gconv* m, int B, int ld) {
    if (!m || B < 1 || ld < (1 << m->n_layers)) return 0;
    return 2 * round256((size_t)B * per_read_bytes(m, ld)) + round256((size_t)(m->n_layers + 1) * B * sizeof(int32_t));
}

int rs_gconv_max_batch(const rs_gconv* m, int ld) {
    if (!m || ld < (1 << m->n_layers)) return 0;
    return max_batch_of(per_read_bytes(m, ld));
}

int rs_gconv_forward_ragged(rs_gconv* m, const float* d_x, const int32_t* d_len, int B, int ld, void* d_ws, size_t ws_bytes,
                            float* d_probs, float* d_logits, void* stream) {
    const int rc = check_ragged_call("rs_gconv_forward_ragged", "rs_gconv_max_batch", m, d_x, d_len, d_ws, d_probs, B, ld, ws_bytes, [&] {
        return RaggedLimits{1 << m->n_layers, rs_gconv_workspace_bytes(m, B, ld), B <= rs_gconv_max_batch(m, ld)};
    });
    if (rc != RS_OK) return rc;
    DeviceGuard guard(m->device);
    RS_HIP(guard.err);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t buf_bytes = (size_t)B * per_read_bytes(m, ld);
    Carver ws(d_ws);
    float* bufs[2] = {ws.take(buf_bytes), ws.take(buf_bytes)};
    int32_t* table = ws.take<int32_t>((size_t)(m->n_layers + 1) * B * sizeof(int32_t));

    hipLaunchKernelGGL(gconv_lengths_kernel, dim3((B + 255) / 256), dim3(256), 0, st, d_len, B, ld, m->n_layers, table);
    RS_HIP(hipGetLastError());
    const float* in = d_x;
    int in_pitch = 1;
    for (size_t i = 0; i < m->convs.size(); ++i) {
        const ConvDev& c = m->convs[i];
        const Shape& s = kShapes[c.plan.shape];
        TileArgs a;
        memset(&a, 0, sizeof(a));
        a.x = in;
        a.y = bufs[i & 1];
        a.rows = table + (size_t)c.level * B;
        a.w = c.w;
        a.b = c.b;
        a.in_rows = ld >> c.level;
        a.in_pitch = in_pitch;
        a.out_rows = ld >> (c.level + c.pool);
        a.out_pitch = cp4(c.c_out);
        a.c_in = c.c_in;
        a.c_out = c.c_out;
        a.k = c.k;
        a.kc = c.plan.kc;
        a.nchunk = c.plan.nchunk;
        a.lpitch = c.plan.lpitch;
        a.slab_floats = c.plan.slab_floats;
        a.panel_floats = c.plan.panel_floats;
        a.tiles = (a.in_rows + s.rows() - 1) / s.rows();
        const int64_t grid = (int64_t)B * a.tiles;
        if (grid > INT32_MAX) {
            set_error("rs_gconv_forward_ragged: grid too large: split the batch");
            return RS_ERR_ARG;
        }
        if (m->mode == 1 && c.plan.vec == 4) {
            GconvX3Args xa;
            memset(&xa, 0, sizeof(xa));
            xa.x = a.x; xa.y = a.y; xa.rows = a.rows; xa.b = a.b;
            xa.w = c.wx;
            xa.w_plane = (int64_t)c.plan.ncb * c.plan.nchunk * c.x3.panel_half;
            xa.in_rows = a.in_rows; xa.in_pitch = a.in_pitch; xa.out_rows = a.out_rows; xa.out_pitch = a.out_pitch;
            xa.c_in = a.c_in; xa.c_out = a.c_out; xa.k = a.k; xa.kc = a.kc; xa.nchunk = a.nchunk; xa.tiles = a.tiles;
            xa.c8_shift = a.kc == 16 ? 1 : a.kc == 32 ? 2 : 3;
            xa.steps = c.x3.steps; xa.xpitch = c.x3.xpitch; xa.slab_rows = c.x3.slab_rows;
            xa.slab_half = c.x3.slab_half; xa.panel_half = c.x3.panel_half;
            RS_HIP(gconv_x3_launch(c.plan.shape, c.pool != 0, xa, dim3((unsigned)grid, (unsigned)c.plan.ncb),
                                   (size_t)c.x3.lds_bytes, st));
        } else {
            TileFn fn = tile_fn(c.plan.shape, c.plan.vec, c.pool != 0);
            hipLaunchKernelGGL(fn, dim3((unsigned)grid, (unsigned)c.plan.ncb), dim3(256), (size_t)c.plan.lds_bytes, st, a);
            RS_HIP(hipGetLastError());
        }
        in = a.y;
        in_pitch = a.out_pitch;
    }
    hipLaunchKernelGGL(gap_head_kernel<true>, dim3(B), dim3(256), 0, st, in, ld >> m->n_layers, in_pitch, m->c_last, m->d_fcw,
                       m->d_fcb, table + (size_t)m->n_layers * B, d_probs, d_logits);
    RS_HIP(hipGetLastError());
    return RS_OK;
}

}  // extern "C"
