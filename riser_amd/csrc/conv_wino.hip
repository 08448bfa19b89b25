// K3 (fp32, Winograd): one ConvNet block i >= 1 with the conv lowered to Winograd F(2,3) on the
// f32-input MFMA.
//
//   Conv1d(C_in -> C_out, k=3, stride 1, zero 'same' padding, bias) -> ReLU -> MaxPool1d(2,2)
//   (riser/nets/cnn.py:52-65, depth 1)
//
// MaxPool(2,2) consumes the conv outputs in pairs (y[2T], y[2T+1]) - exactly the output tile of
// the minimal-filtering algorithm F(2,3), which produces such a pair from the four inputs
// d0..d3 = x[2T-1 .. 2T+2] with 4 multiplications per input channel instead of 6:
//     m1 = (d0 - d2) * g0              m2 = (d1 + d2) * (g0 + g1 + g2) / 2
//     m4 = (d1 - d3) * g2              m3 = (d2 - d1) * (g0 - g1 + g2) / 2
//     y[2T] = m1 + m2 + m3             y[2T+1] = m2 - m3 - m4
// so the layer is FOUR GEMMs  M_j[T][n] = sum_c V_j[T][c] * U_j[n][c]  (j = 0..3) over POOLED
// rows T, i.e. 2/3 of the matrix-pipe work of the direct lowering (conv_f32.hip), and the
// output transform + bias + ReLU + MaxPool is a handful of VALU operations per pooled value in
// the epilogue: out[T][n] = relu(max(m1 + m2 + m3, m2 - m3 - m4) + bias[n]).
// The filter transform U_j is done once on the host in fp64 (rs_model_create); the input
// transform V_j is done on the fly at fragment-read time (4 LDS reads + 4 VALU per 4 fragments).
// fp32 throughout; the result differs from the direct fp32 chain by a few ulp (same error
// against an fp64 evaluation, see tests/test_gpu_parity.py).
//
// Data layout as in conv_f32.hip (position-major activations, P-row slots, zero rows beyond each
// read's length).  GEMM orientation: MFMA "A" operand = weights (rows = output channels), "B"
// operand = transformed activations (columns = pooled positions), so a lane of the 16x16
// accumulator holds 4 CONSECUTIVE CHANNELS of one pooled position: the epilogue stores 16 bytes
// per lane straight into the position-major output.
//
// LDS per item (one K chunk of KC input channels): the (2*BMP + 2) input rows of the tile are
// split by parity into two planes (x[2T+1] -> odd plane, x[2T] -> even plane) so that the four
// inputs of pooled row T are rows T, T+1 of the two planes - unit row stride across lanes, and
// with a row pitch of KC + 2 floats (= 2 mod 4) every ds_read_b32 of a 32-lane half hits 32
// distinct banks.  Weights: [component][n][KC + 2].
// Schedule: persistent 8-wave workgroups, double-buffered LDS, register prefetch of the next
// item distributed over the MFMA slots of the current one (conv_f32.hip has the rationale).
#include "conv_wino_kernel.hpp"

namespace rs {

// conv_wino_thin.hip: the thin-launch instantiation of a shape for chunk index ki (16 / 20 / 24), or null
KernelFn conv_wino_thin_fn(int wm, int wn, int mt, int nt, int ki);

namespace {

using Shape = WinoShape<WinoArgs, 3>;      // chunk = 16, 20, 24
// layer 1 of the shipped net (20 -> 30 channels) with layer 0 folded into its staging: this one instantiation, so the form pins its shape
const KernelFn kFusedL1 = conv_wino_kernel<8, 1, 2, 2, 20, true>;
constexpr TileGeom kFusedGeom = {8, 1, 2, 2};
constexpr int kFusedBMP = kFusedGeom.bm(), kFusedBN = kFusedGeom.bn();

#define RS_SHAPE(WM, WN, MT, NT)                                                                         \
    {{WM, WN, MT, NT}, {conv_wino_kernel<WM, WN, MT, NT, 16>, conv_wino_kernel<WM, WN, MT, NT, 20>,     \
                        conv_wino_kernel<WM, WN, MT, NT, 24>}, {nullptr, nullptr, nullptr}}
// the thin-launch forms are instantiated in conv_wino_thin.hip
#define RS_THIN3(WM, WN, MT, NT) \
    {conv_wino_thin_fn(WM, WN, MT, NT, 0), conv_wino_thin_fn(WM, WN, MT, NT, 1), conv_wino_thin_fn(WM, WN, MT, NT, 2)}
#define RS_SHAPE_D(WM, WN, MT, NT)                                                                       \
    {{WM, WN, MT, NT}, {conv_wino_kernel<WM, WN, MT, NT, 16>, conv_wino_kernel<WM, WN, MT, NT, 20>,     \
                        conv_wino_kernel<WM, WN, MT, NT, 24>}, RS_THIN3(WM, WN, MT, NT)}
// four-wave shapes exist in the one-item-ahead form only
#define RS_SHAPE_4(WM, WN, MT, NT) {{WM, WN, MT, NT}, RS_THIN3(WM, WN, MT, NT), {nullptr, nullptr, nullptr}}
const Shape kShapes[] = {
    // all 8 waves stacked along pooled rows
    RS_SHAPE(8, 1, 2, 2), RS_SHAPE(8, 1, 2, 3), RS_SHAPE(8, 1, 2, 4), RS_SHAPE(8, 1, 1, 5), RS_SHAPE(8, 1, 1, 6),
    RS_SHAPE(8, 1, 1, 7), RS_SHAPE(8, 1, 1, 8),
    // 4 x 2 waves
    RS_SHAPE(4, 2, 2, 3), RS_SHAPE(4, 2, 2, 4), RS_SHAPE(4, 2, 1, 5), RS_SHAPE(4, 2, 1, 7), RS_SHAPE(4, 2, 1, 8),
    // 2 x 4 waves (few rows)
    RS_SHAPE(2, 4, 2, 2), RS_SHAPE(2, 4, 2, 3), RS_SHAPE(2, 4, 1, 4),
    // small tiles (round 4): a batch of 32 ... 200 reads leaves the late layers a few dozen tiles of the shapes above
    RS_SHAPE_D(8, 1, 1, 2), RS_SHAPE(8, 1, 1, 3), RS_SHAPE(8, 1, 1, 4), RS_SHAPE_D(4, 2, 1, 2), RS_SHAPE(4, 2, 1, 3),
    RS_SHAPE(4, 2, 1, 4), RS_SHAPE_D(2, 4, 1, 2), RS_SHAPE_D(2, 4, 1, 1),
    // four-wave workgroups (round 5): one wave per SIMD, for launches of fewer tiles than CUs
    RS_SHAPE_4(4, 1, 1, 1), RS_SHAPE_4(2, 2, 1, 1), RS_SHAPE_4(4, 1, 1, 2), RS_SHAPE_4(2, 2, 1, 2), RS_SHAPE_4(1, 4, 1, 2),
    RS_SHAPE_4(4, 1, 1, 3), RS_SHAPE_4(2, 2, 1, 3),
};
#undef RS_SHAPE
#undef RS_SHAPE_D
#undef RS_SHAPE_4
#undef RS_THIN3
constexpr int kNumShapes = sizeof(kShapes) / sizeof(kShapes[0]);

// full launches: calibrated at B = 512.  Thin launches: layers 4 and 11 at 16 ... 512 reads, every shape (tools/shape_sweep.py;
// profiles/r05_wino_shape_sweep_16_to_512_reads.txt); launch, byte and per-tile terms are conv_wino4.hip's
constexpr WinoCost kCost = {4.0, 0.0, 0.0, 60.0, 23500.0, 60.0, 4.25, -250.0, 0.0062, 0.0124, -467.0, 554.0};

// row unit: POOLED rows
auto family(int kc, int nch) { return wino_family<2>(kShapes, kNumShapes, kCost, kc, nch); }

}  // namespace

int conv_wino_max_bn() { return 256; }
// planner's estimate (SIMD cycles) of one launch with the best tile shape (compared with the small-batch kernel's in convnet_forward.hpp: select_kernel)
double conv_wino_plan_cost(int64_t rows_out, int n16, int kc, int nch, int num_cu) {
    return choose_tile(family(kc, nch), rows_out, n16, num_cu, false).cost;
}
double conv_wino_launch_cost(int64_t rows_out, int n16, int kc, int nch, int num_cu, bool* thin_out) {
    return wino_launch_cost(family(kc, nch), rows_out, n16, num_cu, kCost, thin_out);
}
int conv_wino_num_shapes() { return kNumShapes; }
bool conv_wino_shape_ok(const ConvLayerDev& L, int k) {
    return k >= 0 && k < kNumShapes && wino_chunk_index<Shape>(L.plan.kc) >= 0 && family(L.plan.kc, L.plan.nch).can_run(k);
}

// layer 0 can be folded into this layer's staging when the layer is the shipped net's layer 1
// (20 input channels = one 20-channel chunk, <= 32 outputs) and a tile spans at most two reads; an F(4,3) layer 1 (RS_WINO4)
// runs conv_wino4.hip, which has no such staging: layer 0 must then be a launch of its own
bool conv_wino_can_fuse0(const ConvLayerDev& L, int P_in) {
    return L.wino_m == 2 && L.cp_in == 20 && L.plan.kc == 20 && L.plan.nch == 1 && L.c_out <= kFusedBN &&
           P_in >= 2 * kFusedBMP + 2 && !L.hooks->no_fuse0;
}

int launch_conv_wino(const ConvLayerDev& L, const float* d_x, float* d_y, const int32_t* d_len, int B, int P_in,
                     int layer_index, int num_cu, const float* d_zero, int check_dead, hipStream_t st, int* bm_out,
                     int* bn_out, const float* fuse_xs, const float* fuse_w0) {
    if (fuse_xs && (!conv_wino_can_fuse0(L, P_in) || !fuse_w0)) {
        set_error("conv_wino: layer cannot take the fused layer-0 path");
        return RS_ERR_ARG;
    }
    return launch_wino<2>("conv_wino", kShapes, kNumShapes, kCost, L.hooks->force_wino, L, d_x, d_y, d_len, B, P_in, layer_index,
                          num_cu, check_dead, st, bm_out, bn_out, WinoFuse0<Shape>{fuse_xs, fuse_w0, kFusedL1, &kFusedGeom});
}

}  // namespace rs
