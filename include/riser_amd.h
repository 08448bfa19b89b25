/*
 * riser_amd.h -- C ABI of the MI355X (gfx950) squiggle-classification hot path.
 *
 * This is the drop-in boundary for the path
 *     SignalProcessor.mad_normalise -> Model.classify -> ConvNet.forward -> softmax
 * of comprna/riser.  The reference has no native code and therefore no FFI of its own;
 * each entry point below names the reference Python interface it replaces
 * (file:line under /root/reference).  INTEGRATION.md shows the ctypes stub a RISER
 * maintainer would add to riser/model.py and riser/preprocess.py.
 *
 * Conventions
 *   - plain C, no exceptions cross the boundary; every function returns RS_OK (0) or a
 *     negative rs_status and records a message readable with rs_last_error()
 *     (thread-local).
 *   - all `d_` pointers are DEVICE pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); the library owns only the packed weight copies made by
 *     rs_model_create and frees them in rs_model_destroy.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all launches
 *     are asynchronous on it, nothing here synchronises the device.
 *   - raw signal samples are int16 ADC counts, as delivered by
 *     riser/client.py:47 (np.frombuffer(read.raw_data, signal_dtype)).
 *   - a batch is B reads; read b is the `d_len[b]` samples starting at element
 *     `d_off[b]` of `d_sig` (so a trim is just an offset: riser/preprocess.py:100,105).
 *   - `h_len` (rs_forward / rs_classify / rs_classify_ensemble / rs_autotune) is the HOST's copy of d_len, or NULL.
 *     With it the conv stack lays the batch out in packed blocks (each read occupies len / U + 1 blocks of
 *     U = rs_block_samples() samples, work proportional to every read's own length) - the host needs the block count to
 *     size the launches; without it every read takes the blocks of an Lmax-sample read.  Results are bit-identical
 *     either way.  It must mirror d_len: a device length that disagrees can only cost that read and the reads BEHIND it in
 *     the batch their results (a read whose blocks no longer fit the table the host sized is dropped: NaN probabilities),
 *     never a read in front of it, and never an access outside the workspace or the length array.
 *   - reads shorter than 2^n_layers samples (4096 for the shipped 12-layer net,
 *     riser/preprocess.py:8) cannot be classified: RS_ERR_LENGTH, matching the
 *     RuntimeError torch raises in max_pool1d for the reference.
 */
#ifndef RISER_AMD_H
#define RISER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#define RS_API __attribute__((visibility("default")))

typedef enum rs_status {
    RS_OK = 0,
    RS_ERR_ARG = -1,        /* null pointer, bad size, unsupported configuration */
    RS_ERR_HIP = -2,        /* a HIP runtime call failed; message has hipGetErrorString */
    RS_ERR_LENGTH = -3,     /* a read is empty / shorter than the network minimum / too long */
    RS_ERR_OOM = -4,        /* device or host allocation failed */
    RS_ERR_WORKSPACE = -5   /* caller's workspace is smaller than rs_workspace_bytes() */
} rs_status;

/* arithmetic type of the conv stack (accumulation is always fp32) */
typedef enum rs_dtype {
    RS_F32 = 0,             /* f32-input MFMA (v_mfma_f32_16x16x4_f32): exact fmaf chains */
    RS_BF16 = 1,            /* bf16 activations/weights, v_mfma_f32_16x16x32_bf16, fp32 accumulate */
    RS_F16 = 2,             /* f16 activations/weights, v_mfma_f32_16x16x32_f16, fp32 accumulate */
    RS_F32W = 3,            /* fp32 throughout, conv lowered to Winograd F(2,3) / F(4,3) on the f32-input MFMA:
                               2/3 resp. 1/2 of the multiplications of RS_F32, probabilities within ~1e-5 of it */
    RS_BF16X3 = 4,          /* split precision on the bf16 MFMA: every activation and weight is a pair hi + lo of bf16
                               values (~16 significand bits), a product is hi*hi + lo*hi + hi*lo on three
                               v_mfma_f32_16x16x32_bf16 with fp32 accumulate.  The 16-bit mode that meets the 1e-3
                               probability tolerance of BASELINE configs 3 / 5; RS_BF16 / RS_F16 are the fast,
                               approximate variants */
    RS_F16X3 = 5,           /* the same with f16 pairs (~22 significand bits above 2^-14, less below) */
    RS_F16XF8 = 6           /* RS_F16X3 whose wide layers keep hi*hi on v_mfma_f32_16x16x32_f16 and evaluate the two cross
                               terms hi*lo + lo*hi as ONE K-concatenated product of OCP e4m3 values on the block-scaled
                               v_mfma_scale_f32_16x16x128_f8f6f4 (an E8M0 scale per activation row and 32 channels): two
                               instruction times per 64 K where split precision spends three; probabilities within ~3e-4
                               of fp32 (inside the 1e-3 tolerance), same activation range as RS_F16X3 */
} rs_dtype;

/* decisions of riser/control.py:75-82, as written into rs_decide's output */
typedef enum rs_decision {
    RS_TRY_AGAIN = 0,
    RS_ACCEPT = 1,
    RS_REJECT = 2,
    RS_NO_DECISION = 3
} rs_decision;

typedef enum rs_mode { RS_ENRICH = 0, RS_DEPLETE = 1 } rs_mode;

typedef struct rs_model rs_model;

/* Message of the last failing call on this thread ("" if none). */
RS_API const char* rs_last_error(void);

/* ABI version of this header: (major << 16) | minor. */
RS_API int rs_version(void);

/* Number of HIP devices visible (0 if none / no driver).  Does not select a device. */
RS_API int rs_device_count(void);

/*
 * Build a model on `device` from a reference-format ConvNet state dict.
 * Replaces Model.__init__ (riser/model.py:7-20) + ConvNet.__init__ (riser/nets/cnn.py:8-41)
 * for the shipped configuration: depth 1, kernel 3, classifier `gap_fc`.
 *   n_layers            number of conv blocks (config.cnn.n_layers, 12 in every shipped yaml)
 *   channels[n_layers]  config.cnn.channels
 *   conv_w[i]           HOST fp32 [channels[i], channels[i-1] (1 for i==0), 3]  = layers.{i}.0.weight
 *   conv_b[i]           HOST fp32 [channels[i]]                                   = layers.{i}.0.bias
 *   fc_w                HOST fp32 [n_classes, channels[n_layers-1]]               = classifier.2.weight
 *   fc_b                HOST fp32 [n_classes]                                     = classifier.2.bias
 *   n_classes           must be 2 (riser/control.py:69 unpacks exactly two probabilities)
 * Host pointers need only live for the duration of the call.
 */
RS_API int rs_model_create(int n_layers, const int32_t* channels, int n_classes,
                    const float* const* conv_w, const float* const* conv_b,
                    const float* fc_w, const float* fc_b,
                    int dtype /* rs_dtype */, int device, rs_model** out);

RS_API int rs_model_destroy(rs_model* m);

/*
 * ABI 2.2.  Replace the model's gap_fc head by the reference's `fc` classifier (riser/nets/cnn.py:22-27):
 *     Flatten(1) -> Linear(C * positions, hidden) -> ReLU -> Linear(hidden, 2),
 * C = the last conv layer's channels.  w1 [hidden][C * positions] (row-major, features channel-major as Flatten orders
 * them: f = c * positions + p), b1 [hidden], w2 [2][hidden], b2 [2]: host pointers, copied.  The reference hard-codes
 * C * positions = 67 * 753 and hidden = 4096 (one input length, 12048 .. 12063 samples, of one 4-layer net); here any
 * positions >= 1 and any hidden that is a multiple of 64.  fp32 models only (RS_F32 / RS_F32W).  After this call a read
 * whose len >> n_layers differs from `positions` cannot be classified - the reference's matmul raises for it
 * (riser/nets/cnn.py:47) - and gets NaN probabilities (decision RS_NO_DECISION); rs_workspace_bytes() grows by the
 * partial sums of the first Linear.  The fc model runs in rs_forward / rs_classify / rs_classify_ensemble like any other
 * (ensemble members must agree on `hidden`).  Call once, before the first forward.
 */
RS_API int rs_model_set_fc_classifier(rs_model* m, int positions, int hidden, const float* w1, const float* b1,
                               const float* w2, const float* b2);

/* Bytes of device workspace rs_forward / rs_classify need for a batch of B reads of at
 * most Lmax samples (0 on bad arguments): the block table, the normalised signals and two activation buffers. */
RS_API size_t rs_workspace_bytes(const rs_model* m, int B, int Lmax);

/* Largest B one call accepts for reads of up to Lmax samples: every activation buffer is addressed through a 2 GiB
 * buffer-resource window (32-bit offsets, hardware bounds checking).  Reads are independent: split bigger batches. */
RS_API int rs_max_batch(const rs_model* m, int Lmax);

/* Block size U of the packed activation layout in samples: 2^max(n_layers, 12) (4096 for the shipped net; doubled when
 * RS_WINO4 puts the last layer on the F(4,3) lowering).  Read b of a batch occupies len_b / U + 1 blocks.  Since ABI 2.1 the
 * layout has TWO LEVELS: this is the block of the last three conv layers and of the head; the layers before them (and the
 * normalised signal) run on finer blocks - rs_layer_info.block_samples, 1024 samples for the shipped net - so that a read
 * costs its own length more closely (a live 8615-sample read: 9 x 1024 instead of 3 x 4096 samples of rows); the library
 * re-packs the (small) buffer in between.  In conv layer `layer`'s output buffer read b starts at row
 * (Uf * sum_{i<b}(len_i / Uf + 1)) >> (layer + 1), Uf = that layer's block_samples.  Results do not depend on the layout. */
RS_API int rs_block_samples(const rs_model* m);

/*
 * MAD normalisation + outlier smoothing of B reads.
 * Replaces SignalProcessor.mad_normalise (riser/preprocess.py:108-147), bit-exact in
 * float64: exact integer median / MAD, y = (x - med) / (1.4826 * mad), then the
 * sequential in-place smoothing of |y| > 3.5 (order-dependent recurrence, un-clipped
 * ends).  mad == 0 gives zeros (the reference returns an int64 zero array).
 *   d_out32  fp32 [B, ld32] or NULL: (float)y, i.e. the cast of riser/model.py:25;
 *            elements [len, pad_to) of each row are zero-filled (pad_to <= ld32)
 *   d_out64  fp64 [B, ld64] or NULL: y exactly as the reference returns it
 *   d_stats  fp64 [B, 2] or NULL: (median, mad)
 * Lmax is the host-known maximum of d_len (sizes the LDS staging buffer); every read
 * must have 1 <= len <= Lmax <= 65536.
 */
RS_API int rs_normalise(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B, int Lmax,
                 float* d_out32, int64_t ld32, int32_t pad_to,
                 double* d_out64, int64_t ld64, double* d_stats, void* stream);

/*
 * The same for FLOATING-POINT signals (elem_bytes = 2: float16 (since ABI 2.2), 4: float32, 8: float64), the other input
 * SignalProcessor.mad_normalise accepts (riser/preprocess.py:108-115; the retrain path normalises pA-scaled float
 * signals, riser/retrain/preprocess.py:79).  numpy keeps the input's precision end to end (float32 in -> float32
 * arithmetic -> float32 out, the Python constant 1.4826 adopting the array's dtype under NEP 50), and so does this
 * entry: d_out has the element type of d_sig, rows of `ld` elements, bit-identical to the reference's result (float16:
 * every operation as numpy evaluates it - in float32, rounded to half - and the median's mean of the two middle values
 * with its float32 accumulator).
 * Every read must have 1 <= len; read b is d_sig[d_off[b] .. d_off[b] + d_len[b]) in elements.  d_stats: fp64 [B, 2]
 * = (median, mad) or NULL.  Off the live path: an exact radix select per read, not tuned.
 */
RS_API int rs_normalise_float(const void* d_sig, int elem_bytes, const int64_t* d_off, const int32_t* d_len, int B,
                       void* d_out, int64_t ld, double* d_stats, void* stream);

/*
 * Forward pass + softmax on already normalised fp32 signals.
 * Replaces Model.classify (riser/model.py:22-28) -> ConvNet.forward
 * (riser/nets/cnn.py:43-65) for a batch: B independent reads of individual length.
 *   d_x       fp32 [B, ldx]; row b holds d_len[b] samples (what follows them is not read)
 *   h_len     host copy of d_len or NULL (see the conventions above)
 *   d_probs   fp32 [B, 2] = (p_off_target, p_on_target), the order of riser/control.py:69
 *   d_logits  fp32 [B, 2] or NULL
 *   Lmin      host-known lower bound of d_len (0 if unknown; ignored when h_len is given).  Only a speed hint:
 *             tiles that fall entirely into the padding behind a read are skipped; when Lmin says no such tile
 *             can exist the per-tile test is not even compiled into the walk.
 */
RS_API int rs_forward(rs_model* m, const float* d_x, int64_t ldx, const int32_t* d_len, const int32_t* h_len, int B, int Lmin,
               int Lmax, void* d_ws, size_t ws_bytes, float* d_probs, float* d_logits, void* stream);

/* Samples a read of Lmax samples occupies in the packed layout: (Lmax / U + 1) * U, U = rs_block_samples(). */
RS_API int rs_padded_length(const rs_model* m, int Lmax);

/*
 * Fused path: raw int16 reads -> normalise -> forward -> probabilities.
 * Equivalent to the pair of calls at riser/control.py:63 and :69 for every read of the
 * batch; the normalised signals live in the workspace.
 */
RS_API int rs_classify(rs_model* m, const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, const int32_t* h_len,
                int B, int Lmin, int Lmax, void* d_ws, size_t ws_bytes,
                float* d_probs, float* d_logits, void* stream);

/*
 * Optional tile-shape tuning for one batch geometry (not part of the reference; like a BLAS "find" mode).
 * Runs rs_classify on the given batch and, for every conv layer that runs a tiled kernel, times each feasible
 * entry of that kernel's tile-shape table in place (HIP events on `stream`, which is synchronised repeatedly);
 * a shape more than 3 % faster than the launch planner's choice is remembered for launches with the same number of
 * rows (blocks x block length) of that layer.  Results are bit-identical whatever shape runs (the accumulation order
 * over channels does not depend on the tile shape; 16-bit: on the panel width it does, within fp32 round-off).
 * d_probs receives the batch's probabilities as rs_classify would produce them; *n_changed (optional) the number
 * of layers whose choice changed.  Costs a few hundred launches: call once per deployment batch size, not per batch.
 */
RS_API int rs_autotune(rs_model* m, const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, const int32_t* h_len, int B,
                int Lmin, int Lmax, void* d_ws, size_t ws_bytes, float* d_probs, int32_t* n_changed, void* stream);

/*
 * Ensemble form of rs_classify: the model loop of riser/control.py:68-71 for a whole batch.
 * The reads are normalised ONCE (riser/control.py:63), every model of `models` (same architecture,
 * e.g. the mRNA / mtRNA / globin stand-ins of one kit) runs its forward pass on the same normalised
 * signals, and - if d_decision is not NULL - the decision of riser/control.py:75-82 is taken on the
 * device (see rs_decide for `max_len`, `threshold`, `mode`).
 *   d_probs     fp32 [n_models, B, 2]
 *   d_decision  uint8 [B] or NULL
 * The workspace is shared by the models (block table and normalised signals once).  With
 * rs_ensemble_workspace_bytes(models, n_models, B, Lmax) bytes every model has its own pair of activation buffers and the
 * forwards run CONCURRENTLY (model 0 on `stream`, the others on library-owned side streams forked behind the normalise
 * launch and joined in front of the decision; everything the call enqueues is ordered on `stream` as before) whenever the
 * batch under-fills the chip (fewer than ~1800 blocks of 4096 samples: a live ReadUntil batch; larger batches fill it by
 * themselves and run back to back).  With less,
 * but at least the MAXIMUM of rs_workspace_bytes(models[k], B, Lmax) over the models, they run back to back on `stream`;
 * below that the call is refused with RS_ERR_WORKSPACE.  The probabilities are the same bits either way.
 */
RS_API size_t rs_ensemble_workspace_bytes(rs_model* const* models, int n_models, int B, int Lmax);
RS_API int rs_classify_ensemble(rs_model* const* models, int n_models, const int16_t* d_sig, const int64_t* d_off,
                         const int32_t* d_len, const int32_t* h_len, int B, int Lmin, int Lmax, void* d_ws,
                         size_t ws_bytes, float* d_probs, uint8_t* d_decision, int max_len, float threshold, int mode,
                         void* stream);

/*
 * Ensemble decision of riser/control.py:75-82 for B reads and n_models models.
 *   d_probs   fp32 [n_models, B, 2]
 *   max_len   SignalProcessor.get_max_length() (riser/preprocess.py:36-40)
 *   d_out     uint8 [B], rs_decision values
 * Comparisons are strict `>` in fp32, as torch does for `tensor > python_float`.
 */
RS_API int rs_decide(const float* d_probs, int n_models, int B, const int32_t* d_len, int max_len,
              float threshold, int mode /* rs_mode */, uint8_t* d_out, void* stream);

/*
 * poly(A) end detector on raw reads.
 * Replaces SignalProcessor.get_polyA_end (riser/preprocess.py:42-79): 500-sample
 * windows, start when the window mean rose > 20 % over the previous 1000 samples with
 * window MAD <= 20, end at the first later window with MAD > 20.
 *   d_end     int32 [B]: the end index (a multiple of 500) or -1 where the reference
 *             returns None
 * Reads may have any length (the whole signal is scanned, as the reference does; the scan stops at the first end
 * found, which nothing later in the signal can change).
 */
RS_API int rs_polya_end(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B,
                 int32_t* d_end, void* stream);

/*
 * ABI 2.2.  The same detector, RESUMABLE: for a caller that sees a read again, longer, with an unchanged prefix (a read that
 * stays in its pore between two ReadUntil batches; riser/control.py:53 re-scans it from its first sample each time).
 * The detector's state after W whole 500-sample windows without an end - W, the `start` index, the sums of the last two
 * windows - depends on the read's first 500 W samples only:
 *   d_state_in   int32 [B][4] (windows done, start, sum of window W - 2, sum of window W - 1) as a previous call returned
 *                it for the SAME read, all zeros for a read seen for the first time, or NULL (= all zeros for every read);
 *                a state whose window count exceeds the read's is ignored (the read is scanned whole)
 *   d_state_out  int32 [B][4]: the state after this scan; for a read whose end is found, its input state unchanged
 *                (resumed from it the scan finds the same end).  Must not be d_state_in.
 * d_end as rs_polya_end: the results are identical to a scan from the first sample.  The caller answers for the prefix being
 * unchanged (riser_amd's control loop: the signal store's verified delta path).
 */
RS_API int rs_polya_end_resume(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B,
                        const int32_t* d_state_in, int32_t* d_end, int32_t* d_state_out, void* stream);

/*
 * Scatter n segments of raw samples between device buffers: segment k = d_src[d_src_off[k] .. + d_len[k]) is copied to
 * d_dst[d_dst_off[k] ..) (offsets in samples).  The batched control loop keeps the raw signal of every read in flight
 * resident on the device: an AccumulatingCache client (riser/client.py:29-31) re-sends a read's whole signal with every
 * batch, and only the samples that are new since the last batch are uploaded (compacted, one transfer) and scattered
 * behind the ones already there.
 */
RS_API int rs_copy_segments(const int16_t* d_src, int16_t* d_dst, const int64_t* d_src_off, const int64_t* d_dst_off,
                     const int32_t* d_len, int n, void* stream);

/* Introspection used by bench.py for roofline accounting: per conv layer i (0-based),
 * fills the padded GEMM shape the kernels execute.  Returns RS_ERR_ARG if out of range. */
typedef struct rs_layer_info {
    int32_t c_in, c_out;        /* logical channels */
    int32_t cp_in, cp_out;      /* padded row widths of the activation buffers */
    int32_t k_pad;              /* padded reduction length (3 * padded input channels) */
    int32_t n_pad;              /* padded output channels the MFMA tiles cover */
    int32_t bm, bn, kc;         /* workgroup tile (rows x couts) and channel chunk of the last launch (0 if never run) */
    int32_t gemm_row_div;       /* conv rows per GEMM row: 1 direct lowering, 2 Winograd F(2,3), 4 Winograd F(4,3) */
    int32_t block_samples;      /* ABI 2.1: block size (samples) of the packed layout this layer runs on - its input rows and
                                   its output rows; the output of the last fine layer is then re-packed to coarse blocks */
    int32_t rows_format;        /* ABI 2.5: layout of the layer's OUTPUT rows: 0 one value per channel (fp32 / 16-bit), 1 split
                                   precision (panels [hi x 32 | lo x 32]), 2 F8 rows (RS_F16XF8: per 64 channels hi16 x 64, then
                                   [hi8 | lo8 | hi8 | lo8] x 32 e4m3 bytes; E8M0 scale plane behind the rows) */
} rs_layer_info;
RS_API int rs_model_layer_info(const rs_model* m, int layer, rs_layer_info* out);

/*
 * Sequential conv programs: the secondary ResNet architecture (riser/nets/resnet.py:7-131; not
 * loadable by the reference's Model, no shipped config or weights).  The host folds eval-mode
 * BatchNorm into each conv and hands over an execution list; activations live in `n_buffers`
 * numbered buffers (0 = the normalised input [B, L], the rest carved from the workspace).
 * One uniform length per batch.  Convs run on the f32-input MFMA (generic over k / stride / pad, not tuned per shape);
 * also used for ConvNet configurations outside the shipped class (depth > 1, kernels other than 3).
 */
typedef struct rs_seq_op {
    int32_t kind;           /* 0 = conv1d (+bias, +residual, +relu), 1 = MaxPool1d(2, 2, padding `pad` = 0 or 1) */
    int32_t src, dst, add;  /* buffer ids; add = -1 for no residual input */
    int32_t c_in, c_out, k, stride, pad, relu;
    const float* w;         /* HOST fp32 [c_out, c_in, k], BN already folded in (conv only) */
    const float* b;         /* HOST fp32 [c_out] */
} rs_seq_op;
typedef struct rs_seqnet rs_seqnet;
RS_API int rs_seqnet_create(const rs_seq_op* ops, int n_ops, int n_buffers, const float* fc_w /* [2, c_last] */,
                     const float* fc_b, int c_last, int device, rs_seqnet** out);
RS_API int rs_seqnet_destroy(rs_seqnet* m);
RS_API size_t rs_seqnet_workspace_bytes(const rs_seqnet* m, int B, int L);
RS_API int rs_seqnet_forward(rs_seqnet* m, const float* d_x /* fp32 [B, L] */, int B, int L, void* d_ws, size_t ws_bytes,
                      float* d_probs, float* d_logits, void* stream);
/*
 * ABI 2.3: arithmetic of a program's stem and residual basic blocks (riser/nets/resnet.py:50-57, shortcuts :21-24,45-47; the
 * bottleneck blocks :60-70 too when RS_SEQ_BNECK_X3 was set at rs_seqnet_create - measured slower than their fp32 form, so off):
 * where a ResNet's time is.  RS_F32 (default: the f32-input MFMA) or RS_BF16X3: split precision
 * on the bf16 MFMA as RS_BF16X3 of rs_model_create computes it (hi + lo pairs, three v_mfma_f32_16x16x32_bf16 per product, fp32
 * accumulate; activations stay fp32 between launches) - BASELINE.json's "1D-ResNet forward pass ... MFMA bf16" inside the 1e-3
 * tolerance.  The head and unfused ops keep fp32.  RS_ERR_ARG for any other dtype, or for a program without a fused residual block.
 */
RS_API int rs_seqnet_set_mode(rs_seqnet* m, int dtype /* rs_dtype */);
/*
 * ABI 2.4: RAGGED batches - the reads of a ReadUntil batch have their own lengths (riser/control.py:36-60: anything from the
 * minimum to the kit's maximum), and rs_seqnet_forward takes one length per call.  Here read b is d_x[b * ld .. b * ld + d_len[b]):
 * the rows of every read after every op are computed on the device from d_len, every kernel masks by them, the buffers keep the
 * row pitches of an ld-sample read (rs_seqnet_workspace_bytes(m, B, ld)).  A read's probabilities are those of a uniform call on
 * it alone, bit for bit.  Only for programs whose ops all run inside fused launches (stem + residual blocks: what
 * riser/nets/resnet.py builds): rs_seqnet_ragged_ok(m) == 1; otherwise RS_ERR_ARG (group the reads by length instead).
 */
/* Preconditions of rs_seqnet_forward_ragged: d_len[b] in [0, ld] (a larger value is read as ld); a read shorter than the network
 * needs (no output row left behind some op) gets NaN probabilities - a defined result, no out-of-range access; a batch whose
 * buffers outgrow the kernels' 2 GiB windows returns RS_ERR_ARG ("split the batch") before anything wrong is written:
 * rs_seqnet_max_batch(m, ld) is the largest B that cannot. */
RS_API int rs_seqnet_max_batch(const rs_seqnet* m, int L);
RS_API int rs_seqnet_ragged_ok(const rs_seqnet* m);
RS_API int rs_seqnet_forward_ragged(rs_seqnet* m, const float* d_x /* fp32 [B, ld] */, const int32_t* d_len, int B, int ld, void* d_ws,
                             size_t ws_bytes, float* d_probs, float* d_logits, void* stream);
/*
 * ABI 2.9: the launches a forward of B reads at length (ragged = 0) or row pitch (ragged = 1) L makes, in order, in the program's
 * current mode.  Read-only: the forward takes every decision from the same planner.  The per-read length table of a ragged batch
 * and the classifier head are not listed.  Writes the first min(*n, cap) entries to out (out may be NULL when cap is 0) and the
 * number of launches to *n.  Refuses (RS_ERR_ARG / RS_ERR_LENGTH, with the forward's error text) what the forward refuses:
 * a null model or n, B < 1, an L too short for the program, a ragged call on a program that is not ragged_ok or whose fused
 * launches outgrow the buffer windows.
 */
enum {
    RS_SEQ_STEM_POOL = 1,     /* seq_stem_pool_kernel<nt> (x3: seq_stem_pool_x3_kernel): stem conv + ReLU + MaxPool(2, 2, 1) */
    RS_SEQ_BASIC_BLOCK = 2,   /* seq_basic_block_kernel<nt, mtw, waves> (x3: seq_basic_block_x3_kernel) */
    RS_SEQ_BOTTLENECK = 3,    /* seq_bottleneck_block_kernel<ntm, nt> (x3: seq_bottleneck_block_x3_kernel) */
    RS_SEQ_CONV_MFMA_LDS = 4, /* seq_conv_mfma_lds_kernel<nt>: one conv, packed weights in LDS */
    RS_SEQ_CONV_MFMA = 5,     /* seq_conv_mfma_kernel<nt>: one conv, weights from global memory, ceil(c_out / 16 nt) column groups */
    RS_SEQ_CONV_SCALAR = 6,   /* seq_conv_kernel (RS_SEQ_SCALAR) */
    RS_SEQ_MAXPOOL = 7,       /* seq_maxpool_kernel */
};
typedef struct rs_seq_launch {
    int32_t op, n_ops;        /* first op index of the program, ops the launch covers */
    int32_t family;           /* RS_SEQ_* above */
    int32_t nt, ntm, mtw, waves;   /* template arguments (0 where the kernel has none; ntm: bottleneck mid tiles) */
    int32_t np;               /* weight column pitch (the output columns' for a bottleneck); 0 for the scalar conv and the pool */
    int32_t cp;               /* row pitch of the intermediate tile in LDS (floats, or bf16 halfwords when x3); 0 without one */
    int32_t x3;               /* 1: split precision on the bf16 MFMA */
} rs_seq_launch;
RS_API int rs_seqnet_launch_plan(const rs_seqnet* m, int B, int L, int ragged, rs_seq_launch* out, int cap, int* n);

/*
 * ABI 2.6: TCN and bottleneck TCN (riser/nets/tcn.py:62-91, riser/nets/tcn_bot.py:63-92; chosen by riser/train.py:175-182
 * for `model: tcn` / `tcn-bot`; not loadable by the reference's Model).  The host folds weight_norm (g * v / ||v||) and hands
 * over per temporal block its convs - TCN: two causal k-convs (tcn.py:27-30), TCNBot: 1x1, k, k, 1x1 (tcn_bot.py:27-32) -
 * each followed by ReLU, the optional 1x1 shortcut (should_apply_shortcut, tcn.py:57-59; null = identity residual), and
 * base = d_{i+1} / d_i (block 0 has dilation 1).  The block output is relu(convs + residual) (tcn.py:47-51); the head is
 * linear(x[:, :, -1]) (tcn.py:87) + softmax (riser/model.py:27).
 * Only the last receptive field of a read matters, and inside it only positions L-1 - d_i * m of block i: the device runs
 * that cone (csrc/tcn.hip), one fused launch per block, fp32 on the f32-input MFMA.  Cost does not grow with read length.
 */
typedef struct rs_tcn_conv {
    int32_t c_in, c_out, k;
    int32_t causal;         /* 1: left-padded by (k - 1) * dilation and chomped (k > 1); 0 only for k == 1 */
    const float* w;         /* HOST fp32 [c_out, c_in, k], weight_norm folded */
    const float* b;         /* HOST fp32 [c_out] */
} rs_tcn_conv;
typedef struct rs_tcn_block {
    int32_t n_convs;        /* 1..4, chained; at least one with k > 1 */
    int32_t base;           /* dilation of the next block / this block's (>= 1) */
    rs_tcn_conv convs[4];
    int32_t has_shortcut;   /* 1: sc_w / sc_b ([c_out, c_in] / [c_out]); 0: identity (c_in == c_out) */
    int32_t reserved;
    const float* sc_w;
    const float* sc_b;
} rs_tcn_block;
typedef struct rs_tcn rs_tcn;
RS_API int rs_tcn_create(const rs_tcn_block* blocks, int n_blocks, const float* fc_w /* [2, c_last] */, const float* fc_b,
                         int c_last, int device, rs_tcn** out);
RS_API int rs_tcn_destroy(rs_tcn* m);
/* 1 + sum over the causal convs of (k - 1) * dilation (the reference's get_receptive_field), saturated at INT64_MAX; exact for
 * dilations past any read length too (before ABI 2.8 a dilation above 2^40 was counted as 2^40) */
RS_API int64_t rs_tcn_receptive_field(const rs_tcn* m);
RS_API size_t rs_tcn_workspace_bytes(const rs_tcn* m, int B, int ld);
/* largest B whose activation buffers stay inside the 2 GiB buffer window for reads of pitch ld; callers split bigger batches */
RS_API int rs_tcn_max_batch(const rs_tcn* m, int ld);
/* Read b is d_x[b * ld .. b * ld + d_len[b]) (d_len in [1, ld]; a larger value is read as ld), right-aligned: its last sample
 * is the position the head classifies, and every position before its start is zero padding.  A uniform batch is the same call
 * with equal lengths.  A read's result does not depend on ld or on the other reads, bit for bit.  d_logits may be null. */
RS_API int rs_tcn_forward_ragged(rs_tcn* m, const float* d_x /* fp32 [B, ld] */, const int32_t* d_len, int B, int ld, void* d_ws,
                                 size_t ws_bytes, float* d_probs /* [B, 2] */, float* d_logits, void* stream);
/* ABI 2.7: arithmetic of a TCN's temporal blocks.  RS_BF16X3 runs every conv of every block (the 1x1 shortcut included) in
 * split precision on the bf16 MFMA (csrc/tcn_x3.hip): each activation and weight is hi = bf16(v), lo = bf16(v - hi), a product
 * is hi*hi + lo*hi + hi*lo with fp32 accumulation; bias, ReLU, the residual add and the head stay fp32.  RS_F32 / RS_F32W go
 * back to fp32 (the default), whose bits are those of a freshly created handle.  Any other dtype, or a null handle, returns
 * RS_ERR_ARG.  The split weights are packed at rs_tcn_create and freed by rs_tcn_destroy.  Both modes keep the same fp32
 * activation buffers, so rs_tcn_workspace_bytes and rs_tcn_max_batch report the same figures in either.  A read in a ragged
 * batch gets the bits it gets alone in either mode.  Not safe to call while a forward of the handle is being enqueued. */
RS_API int rs_tcn_set_mode(rs_tcn* m, int dtype);
/* ABI 2.8: the tile the forward launches for block `block` (0-based) of a batch of B reads of pitch ld in the handle's current
 * mode: *T output positions of *nb reads per workgroup, *tiles_pos tiles along the positions of a read.  Read-only: it changes
 * no launch.  A bad argument, or a block too wide for one tile of LDS (what the forward refuses), returns RS_ERR_ARG. */
RS_API int rs_tcn_tile_plan(const rs_tcn* m, int block, int B, int ld, int* T, int* nb, int* tiles_pos);

/*
 * CNN-RNN (added after ABI 2.8; rs_version is unchanged): riser/nets/cnn_rnn.py's ConvRecNet, loaded by Model for
 * `model: cnn-rnn`.  The conv front is n_conv x [valid Conv1d(c_in, c_out, k) + bias -> MaxPool1d(2, 2) -> ReLU]: a read of
 * L samples has L_{i+1} = (L_i - k_i + 1) // 2 and T = L_n recurrent steps.  The recurrent stack is a flat list of LSTM / GRU
 * layers (the reference nests n_rec_layers modules of n_rec_layers layers each: n_rec_layers^2 layers, a ReLU on the output
 * sequence after each module, `relu_after`); the head is Linear(out_dim -> 2) on the last step + softmax.  Gate order as
 * torch stores it: LSTM i, f, g, o; GRU r, z, n with n = tanh(W_in x + b_in + r * (W_hn h + b_hn)).  Zero initial state.
 * fp32 throughout on the f32-input MFMA (csrc/crnn.hip): one fused launch per conv layer, per recurrent layer one input
 * projection GEMM per direction and one persistent launch that loops over t (both directions in it).  The last layer's
 * output sequence is never written, and its backward direction runs one step (the head reads its first step).
 */
typedef struct rs_crnn_conv {
    int32_t c_in, c_out, k;
    int32_t reserved;
    const float* w;         /* HOST fp32 [c_out, c_in, k] */
    const float* b;         /* HOST fp32 [c_out] */
} rs_crnn_conv;
typedef struct rs_crnn_layer {
    int32_t cell;           /* 0 LSTM, 1 GRU */
    int32_t in_dim;         /* the last conv's c_out, or the previous layer's hidden x (2 if bidirectional) */
    int32_t hidden;         /* 1..320 */
    int32_t bidirectional;  /* 0 / 1: index 1 of the arrays below is the backward direction (torch's `_reverse`) */
    int32_t relu_after;     /* 1: ReLU on this layer's output (the last layer of a module); the last layer always has it */
    int32_t reserved;
    const float* w_ih[2];   /* HOST fp32 [gates * hidden, in_dim] */
    const float* w_hh[2];   /* HOST fp32 [gates * hidden, hidden] */
    const float* b_ih[2];   /* HOST fp32 [gates * hidden] */
    const float* b_hh[2];
} rs_crnn_layer;
typedef struct rs_crnn rs_crnn;
RS_API int rs_crnn_create(const rs_crnn_conv* convs, int n_conv, const rs_crnn_layer* layers, int n_layers,
                          const float* fc_w /* [2, out_dim] */, const float* fc_b, int out_dim, int device, rs_crnn** out);
RS_API int rs_crnn_destroy(rs_crnn* m);
/* shortest read the reference can run (shorter: its conv or max_pool raises); a null handle returns RS_ERR_ARG */
RS_API int rs_crnn_min_length(const rs_crnn* m);
/* recurrent steps T of a read of `len` samples (0 below the minimum); a null handle or len < 0 returns RS_ERR_ARG */
RS_API int rs_crnn_steps(const rs_crnn* m, int len);
/* 0 for a null handle, B < 1 or ld below the minimum */
RS_API size_t rs_crnn_workspace_bytes(const rs_crnn* m, int B, int ld);
/* largest B whose activation buffers each stay inside the 2 GiB buffer window for reads of pitch ld; callers split bigger
 * batches.  0 for a null handle or ld below the minimum */
RS_API int rs_crnn_max_batch(const rs_crnn* m, int ld);
/* Read b is d_x[b * ld .. b * ld + d_len[b]) (a larger d_len is read as ld) with its own T_b steps; the reads' recurrences
 * are aligned to end on the same step and a read gets the bits it gets alone, whatever the batch or ld.  ld below the
 * minimum returns RS_ERR_LENGTH; a read whose d_len is below it gets NaN probabilities (check lengths on the host).
 * d_logits may be null. */
RS_API int rs_crnn_forward_ragged(rs_crnn* m, const float* d_x /* fp32 [B, ld] */, const int32_t* d_len, int B, int ld,
                                  void* d_ws, size_t ws_bytes, float* d_probs /* [B, 2] */, float* d_logits, void* stream);
/* Added after ABI 2.9 (rs_version stays 2.9): arithmetic of the gate GEMMs whose input is a hidden state - the recurrence
 * h_{t-1} W_hh^T of every layer and direction, and the input projection of every layer but the first.  RS_F16X3 runs them in
 * split precision on the f16 MFMA (csrc/crnn/x3.hpp): hi = f16(v), lo = f16(v - hi), a product is hi*hi + lo*hi + hi*lo on
 * three v_mfma_f32_16x16x32_f16 with fp32 accumulation.  The conv front, the first layer's projection (its input is the conv
 * output, unbounded), the gate non-linearities, c, the GRU update, the head stay fp32.  A hidden state lies in (-1, 1) and the
 * weights are packed with an exact power-of-two scale per matrix, so no f16 operand can overflow: the mode has no range check
 * and no saturation flag.  RS_F32 / RS_F32W go back to fp32 (the default), whose bits are those of a freshly created handle.
 * Any other dtype, or a null handle, returns RS_ERR_ARG and leaves the mode as it was; so does RS_F16X3 for a recurrent
 * weight that is not finite.  The f16 weights are packed on the first switch to RS_F16X3 and freed by rs_crnn_destroy.  Both
 * modes use the same fp32 activation buffers: rs_crnn_workspace_bytes and rs_crnn_max_batch report the same figures in
 * either.  A read in a ragged batch gets the bits it gets alone in either mode.  Not safe to call while a forward of the
 * handle is being enqueued. */
RS_API int rs_crnn_set_mode(rs_crnn* m, int dtype /* rs_dtype */);

/*
 * Generic ConvNets (added after ABI 2.9; rs_version is unchanged): riser/nets/cnn.py:12-18,43-65 at any `depth` and any odd
 * `kernels` - n_layers x [depth x (Conv1d(k, stride 1, 'same') + bias + ReLU), MaxPool1d(2, 2)], then the `gap_fc` head
 * (mean over a read's positions, Linear(c_last -> 2)) + softmax.  A read of L samples has L >> i rows behind i pools; the
 * shortest read is 2^n_layers samples.  fp32 on the f32-input MFMA (csrc/gconv.hip): one launch for the reads' row counts,
 * one tiled launch per conv (bias, ReLU and - in a layer's last conv - the max-pool in its epilogue), one for the head.
 */
typedef struct rs_gconv_conv {      /* riser/nets/cnn.py:12-18,43-65 */
    int32_t c_in, c_out, k;         /* chained from c_in = 1; k odd */
    int32_t reserved;
    const float* w;                 /* HOST fp32 [c_out, c_in, k] */
    const float* b;                 /* HOST fp32 [c_out] */
} rs_gconv_conv;
typedef struct rs_gconv rs_gconv;
/* convs: n_layers * depth entries, layer-major (riser/nets/cnn.py:12-18,43-65).  Refused with RS_ERR_ARG before a device is
 * touched: an even kernel, a conv whose activation slab and weight panel fit no tile shape's LDS, more than 16 layers,
 * channels that do not chain. */
RS_API int rs_gconv_create(const rs_gconv_conv* convs, int n_layers, int depth, const float* fc_w /* [2, c_last] */,
                           const float* fc_b, int device, rs_gconv** out);
/* riser/nets/cnn.py:12-18,43-65 */
RS_API int rs_gconv_destroy(rs_gconv* m);
/* 2^n_layers (riser/nets/cnn.py:12-18,43-65: below it a max_pool has no output); a null handle returns RS_ERR_ARG */
RS_API int rs_gconv_min_length(const rs_gconv* m);
/* largest B whose two activation buffers each stay inside the 2 GiB buffer window for reads of pitch ld (riser/nets/cnn.py:12-18,
 * 43-65 has no such limit); callers split bigger batches.  0 for a null handle or ld below the minimum */
RS_API int rs_gconv_max_batch(const rs_gconv* m, int ld);
/* two ping-pong activation buffers + the table of row counts (riser/nets/cnn.py:12-18,43-65); 0 for a null handle, B < 1 or
 * ld below the minimum */
RS_API size_t rs_gconv_workspace_bytes(const rs_gconv* m, int B, int ld);
/* riser/nets/cnn.py:12-18,43-65 on a ragged batch: read b is d_x[b * ld .. b * ld + d_len[b]); what lies behind it in its row
 * is never read as data.  A read gets the bits it gets alone, whatever the batch, its order or ld.  A d_len beyond ld gives
 * the bits of d_len = ld; a d_len below the minimum, or negative, gives NaN probabilities for that read and leaves every other
 * read's bits alone.  ld below the minimum returns RS_ERR_LENGTH.  d_logits may be null. */
RS_API int rs_gconv_forward_ragged(rs_gconv* m, const float* d_x /* fp32 [B, ld] */, const int32_t* d_len, int B, int ld,
                                   void* d_ws, size_t ws_bytes, float* d_probs /* [B, 2] */, float* d_logits, void* stream);
typedef struct rs_gconv_plan {
    int32_t rows, cols;             /* conv positions x output channels of one workgroup's tile */
    int32_t kc, n_chunks;           /* input channels per K chunk, chunks */
    int32_t vec;                    /* 4: K groups of 16 channels; 1: groups of 4 (c_in <= 4) */
    int32_t lds_bytes;              /* activation slab + weight panel of one chunk */
    int32_t shape, reserved;        /* index of the tile shape */
} rs_gconv_plan;
/* the tile a conv (riser/nets/cnn.py:12-18,43-65) of these sizes takes: a function of (c_in, c_out, k) alone, never of the
 * batch.  Needs no device.  RS_ERR_ARG for what rs_gconv_create refuses. */
RS_API int rs_gconv_layer_plan(int c_in, int c_out, int k, rs_gconv_plan* out);
/* Added after ABI 2.9 (rs_version stays 2.9): arithmetic of a generic ConvNet's convs (riser/nets/cnn.py:12-18,43-65).
 * RS_BF16X3 runs every conv with c_in > 4 in split precision on the bf16 MFMA (csrc/gconv_x3.hip): each activation and weight
 * is hi = bf16(v), lo = bf16(v - hi), a product is hi*hi + lo*hi + hi*lo on three v_mfma_f32_16x16x32_bf16 with fp32
 * accumulation; bias, ReLU, the max-pool, the head and the activation buffers stay fp32, and a conv with c_in <= 4 (the first)
 * keeps the fp32 kernel.  Every conv keeps the tile, the K chunk and the chunk count rs_gconv_layer_plan reports.  RS_F32 /
 * RS_F32W go back to fp32 (the default), whose bits are those of a freshly created handle.  Any other dtype, or a null handle,
 * returns RS_ERR_ARG and leaves the mode as it was; so does RS_BF16X3, before any device call, where the split slab and
 * weight panel of a conv exceed 160 KB of LDS.  The split weights are packed on the first switch to RS_BF16X3 and freed by
 * rs_gconv_destroy.  rs_gconv_workspace_bytes and rs_gconv_max_batch report the same figures in either mode, and a read in a
 * ragged batch gets the bits it gets alone in either.  Not safe to call while a forward of the handle is being enqueued. */
RS_API int rs_gconv_set_mode(rs_gconv* m, int dtype /* rs_dtype */);
typedef struct rs_gconv_x3_plan {
    int32_t steps;                  /* k-steps of 32 per K chunk: ceil(k kc / 32) */
    int32_t slab_rows, slab_pitch;  /* rows (tile + halo + a zeroed spare row where a pair addresses tap k) x bf16 per row */
    int32_t lds_bytes;              /* both planes of the slab and of one chunk's weight panel */
    int64_t plane;                  /* bf16 per plane of the packed weights */
} rs_gconv_x3_plan;
/* The RS_BF16X3 form of a conv (riser/nets/cnn.py:12-18,43-65) with c_in > 4, on the host: its LDS layout and, where `w` (HOST
 * fp32 [c_out, c_in, k]) and `packed` (2 * plane uint16) are both given, its split weights as the device reads them - planes
 * [hi | lo], each [column block][chunk][column tile][step][lane][8]; lane (rl, kq) of step s holds column block * cols + 16 tile
 * + rl, pair p = 4 s + kq, tap p / (kc / 8), channels chunk * kc + 8 (p % (kc / 8)) .. + 7; zero where the tap >= k, the channel
 * >= c_in or the column >= c_out.  Needs no device.  RS_ERR_ARG for what rs_gconv_set_mode refuses and for c_in <= 4. */
RS_API int rs_gconv_x3_layout(int c_in, int c_out, int k, rs_gconv_x3_plan* out, const float* w, uint16_t* packed);

/* Added after ABI 2.9 (rs_version stays 2.9): poly(A) START and END at any window size and MAD threshold - the window rule of
 * the reference's offline evaluation script (riser/test.py:80-117), which takes both from its command line; rs_polya_end is
 * the live rule (riser/preprocess.py:42-79) with 500 and 20 built in, and returns the end alone.  With R = resolution, for
 * window w = 0, 1, ... while (w + 1) R <= len, i = w R:
 *   - median and MAD of the window's R samples (an even R: the mean of the two middle values, for both); mean of the window;
 *     rolling = the mean of the 2 R samples before i when i > 2 R (strictly), else the window's own mean;
 *     change = (mean - rolling) / rolling * 100 in float64 - a zero or negative rolling mean takes no special path, inf and
 *     nan compare as IEEE does;
 *   - no start yet, change > 20 and MAD <= mad_threshold: start = i;
 *   - a start, no end yet and MAD > 20 (a literal, NOT the threshold): end = i - in the start's own window where
 *     mad_threshold > 20.
 * d_start / d_end: int32 [B], -1 where the script returns None; a start without an end is (start, -1).  Sums, twice the
 * median and four times the MAD are integers, so the results equal the reference's for every input.  A read's result never
 * depends on its batch.  Nothing outside [d_off[b], d_off[b] + min(d_len[b], max_len)) is read: a d_len beyond max_len is
 * scanned as max_len, a d_len <= 0 gives (-1, -1).  At (500, 20) d_end equals rs_polya_end's.
 * d_ws: rs_polya_coords_workspace_bytes(B, max_len, resolution) bytes (a table of B x (max_len / resolution) windows), never
 * assumed clean; the function returns 0 for B <= 0 or arguments rs_polya_coords refuses.  The table is int32 pairs
 * [B][max_len / resolution] = (window sum, 4 x MAD); entries of windows a read does not have are not written, nor is any byte
 * behind the table.
 * Refused before any device call: resolution outside [1, 16384] (one window and its histogram are staged in a wave's share
 * of LDS), negative B or max_len, null pointers with B > 0 -> RS_ERR_ARG; a workspace that is too small -> RS_ERR_WORKSPACE.
 * B == 0 is RS_OK.  Any int32 mad_threshold is accepted (a negative one never starts). */
RS_API size_t rs_polya_coords_workspace_bytes(int B, int max_len, int resolution);
RS_API int rs_polya_coords(const int16_t* d_sig, const int64_t* d_off, const int32_t* d_len, int B, int max_len,
                           int resolution, int mad_threshold, int32_t* d_start, int32_t* d_end,
                           void* d_ws, size_t ws_bytes, void* stream);

/* Added after ABI 2.9, rs_version unchanged: the reference's retraining preprocessing (riser/retrain/preprocess.py) for a
 * batch of reads, at up to four prefix lengths in one launch.  For read b and cutoff n = cutoffs[c], unless
 * d_rows[c * B + b] < 0 or d_len[b] < n (the pair is skipped and nothing is written for it):
 *   - x[i], i < n: elem_bytes 2 - float32(scale * (float64(raw[i]) + offset)), evaluated in float64 and rounded once, with
 *     (offset, scale) = d_calib[2 b], d_calib[2 b + 1] and scale = range / digitisation: the numpy expression
 *     np.array(scale * (raw + offset), dtype=np.float32), which is what the tests pin; it is believed, not verified here, to be
 *     what ont_fast5_api's get_raw_data(scale=True) evaluates.  elem_bytes 4 - the float32 pA values as given (finite).
 *   - med = np.median(x) and mad = np.median(|x - med|) in float32 (an even n: (a + b) / 2 of the two middle values; -0.0
 *     orders below +0.0);
 *   - y = (x - med) / (float32(1.4826) * mad), one rounding per operation, IEEE division, NO zero-MAD guard (:42-44): a zero
 *     MAD gives NaN where x == med and +-inf elsewhere - where rs_normalise_float, the live rule, writes zeros;
 *   - the script's smoothing (:18-33) with lim = outlier_lim as a float32: the outliers are {|y| > lim}, taken once (NaN is
 *     none, +-inf is one), and are replaced in ascending order in place: index 0 by y[1], index n - 1 by the updated
 *     y[n - 2], any other by (updated y[i - 1] + original y[i + 1]) / 2 clipped to [-lim, lim] (NaN passes the clip).
 * The n results go to d_out[c] + d_rows[c * B + b] * n; (median, MAD) as doubles to d_stats[2 (c * B + b)] where d_stats is
 * given.  Every value equals the reference function's bit for bit, NaN comparing as NaN whatever its sign and payload.  A
 * read's result depends neither on its batch nor on the other cutoffs, and nothing at or behind sample n influences it; no
 * sample at or behind the longest cutoff that applies to a read is loaded.
 * cutoffs and d_out are HOST arrays of n_cut entries; everything else named d_ is device memory.
 * Refused before any device call with RS_ERR_ARG: elem_bytes other than 2 or 4; n_cut outside [1, 4] or null cutoffs; a
 * cutoff below 2 (the script indexes arr[1]) or above 32768 (the read is staged in LDS); cutoffs not strictly ascending;
 * B < 0; outlier_lim not finite or negative; with B > 0 a null d_sig, d_off, d_len, d_rows, d_out or d_out[c], and a null
 * d_calib with elem_bytes 2.  B == 0 is RS_OK. */
RS_API int rs_retrain_prepare(const void* d_sig, int elem_bytes, const int64_t* d_off, const int32_t* d_len,
                              const double* d_calib, int B, const int32_t* cutoffs, int n_cut, float outlier_lim,
                              const int64_t* d_rows, float* const* d_out, double* d_stats, void* stream);

/* Added after ABI 2.9, rs_version unchanged: training of the ConvNet class every shipped config uses (riser/nets/cnn.py:12-18,
 * 43-65 at depth 1, every kernel 3, the `gap_fc` head, two classes; riser/train.py:31-80,197-198): forward, cross-entropy with
 * mean reduction, backward and torch.optim.Adam, fp32, on the device (csrc/train.hip).  A batch is B reads of ONE length L
 * (the reference's datasets are [N, cutoff] tensors); d_x is fp32 [B, ld], ld >= L, d_labels int32 [B] in {0, 1}.
 *
 * rs_train_create takes the layer table (rs_gconv_conv, k = 3, weights [c_out][c_in][3]) and the Linear [2, c_last]; the
 * parameters then live on the device as one flat fp32 vector with its gradient and the two Adam moments, and no weight
 * crosses the bus inside a step.  device < 0 makes a handle WITHOUT device memory: the plan functions and every argument
 * check below answer for it, and a call that would launch is refused with RS_ERR_ARG after its checks.
 * rs_train_workspace_bytes: the bytes one call of B reads of L samples needs - per layer the pooled rows, their gradient and
 * one selector byte per pooled element, the head's buffers, and the partial tiles of the sliced weight gradients; 0 for a
 * null handle or an L that leaves no row behind the last pool.  rs_train_max_batch: the largest B whose every buffer stays
 * inside the 2 GiB window, and at most 65535 - the y extent of a launch grid, which holds the reads of the head's backward
 * launch: every B it returns is a B every launch of a training call can express.  rs_train_slice_plan: into how many slices
 * of how many positions layer `layer`'s weight-gradient contraction over B * (L >> layer) positions is cut - a function of
 * (B, L, layer shape) alone, so the sums are the same bits on every device and run; at most 65535 slices, for the same
 * reason.
 * rs_train_forward_backward writes d_out[0] = loss, d_out[1] = reads whose argmax equals their label, d_out[2 + 2 b + j] =
 * logit j of read b, leaves the gradients in the handle, and waits for `stream`: a label outside {0, 1} is found on the
 * device and returned as RS_ERR_ARG.  Checks before any device call, in this order: null pointers, B < 1, L < 1 or ld < L
 * (RS_ERR_ARG); L >> n_layers < 1 (RS_ERR_LENGTH); ws_bytes (RS_ERR_WORKSPACE); B > rs_train_max_batch (RS_ERR_ARG).
 * rs_train_evaluate: the forward pass and the head alone, same outputs, gradients untouched.
 * rs_train_adam_step: one step on the gradients of the last rs_train_forward_backward (the step count lives in the handle;
 * no weight decay, no amsgrad), then the packed weight forms the kernels read are rebuilt on the device.
 * rs_train_get_params / set_params / get_grads: one tensor per call between the device and a host array in the reference's
 * shape; index 2 l = layers.l.0.weight, 2 l + 1 = layers.l.0.bias, 2 n_layers = classifier.2.weight, 2 n_layers + 1 = its bias;
 * count = the tensor's elements.
 * rs_train_debug_copy (test hook): layer `layer`'s buffer as the last rs_train_forward_backward left it in ITS workspace,
 * which the caller has kept alive and untouched since.  Every training call forgets that workspace when it begins and only
 * an rs_train_forward_backward that returns RS_OK records its own: after an rs_train_evaluate - which carves the same
 * workspace at the offsets of its own (B, L) - or after a refused call, rs_train_debug_copy is RS_ERR_ARG, never a mixture
 * of two calls.  Device to device - what 0: pooled rows fp32 [B][L >> (layer + 1)][cp4(c_out)], 1: selectors uint8 in the same shape (1:
 * conv row 2 j + 1 won), 2: the gradient dY arriving at those pooled rows, fp32, same shape (cp4(c) = c rounded up to 4; pad
 * channels are not written).
 *
 * rs_train_create_generic makes the same handle type for the net of the generic ConvNet family (rs_gconv_create): n_layers x
 * [depth x (Conv1d(k_i, stride 1, 'same') + ReLU), MaxPool1d(2, 2)], `gap_fc`, any depth, every k_i odd.  convs is the table
 * rs_gconv_create takes: n_layers * depth records, layer-major, conv j = layer * depth + d, weights [c_out][c_in][k].  It
 * refuses, before a device is touched and with RS_ERR_ARG, exactly what rs_gconv_create refuses: an even kernel, channels that
 * do not chain from 1, more than 16 layers, a depth outside 1-64, a conv that fits no tile shape of the inference family - a
 * net that trains is a net that runs.  rs_train_create itself still takes kernels of 3 at depth 1 only.
 * Every other rs_train_* call works on a handle from either constructor.  Where a call takes `layer` or a tensor index it
 * means the CONV index j: tensors 2 j = layers.{j / depth}.{2 (j % depth)}.weight, 2 j + 1 = its bias, 2 n_convs and
 * 2 n_convs + 1 the Linear - at depth 1 the numbering above.  rs_train_slice_plan(j) contracts B * (L >> (j / depth))
 * positions.  The last conv of a layer pools and has the three buffers above with L >> (j / depth + 1) rows.  A conv that is
 * not the last of its layer keeps every row: rs_train_debug_copy's what 0 is its ReLU rows and what 2 their gradient, both
 * fp32 [B][L >> (j / depth)][cp4(c_out)], and what 1 is RS_ERR_ARG - it has no selectors; the backward pass gates on row > 0.
 * The workspace holds those full-resolution rows and gradients too, and rs_train_max_batch applies the window to them. */
typedef struct rs_train rs_train;
RS_API int rs_train_create(const rs_gconv_conv* convs, int n_layers, const float* fc_w /* [2, c_last] */, const float* fc_b,
                           int device, rs_train** out);
RS_API int rs_train_create_generic(const rs_gconv_conv* convs /* [n_layers * depth] */, int n_layers, int depth,
                                   const float* fc_w /* [2, c_last] */, const float* fc_b, int device, rs_train** out);
RS_API int rs_train_destroy(rs_train* h);
RS_API size_t rs_train_workspace_bytes(const rs_train* h, int B, int L);
RS_API int rs_train_max_batch(const rs_train* h, int L);
RS_API int rs_train_slice_plan(const rs_train* h, int layer, int B, int L, int32_t* n_slices, int32_t* slice_len);
RS_API int rs_train_forward_backward(rs_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
                                     size_t ws_bytes, float* d_out /* [2 + 2 B] */, void* stream);
RS_API int rs_train_evaluate(rs_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
                             size_t ws_bytes, float* d_out /* [2 + 2 B] */, void* stream);
RS_API int rs_train_adam_step(rs_train* h, float lr, float beta1, float beta2, float eps, void* stream);
RS_API int rs_train_get_params(rs_train* h, int index, float* dst, size_t count);
RS_API int rs_train_set_params(rs_train* h, int index, const float* src, size_t count);
RS_API int rs_train_get_grads(rs_train* h, int index, float* dst, size_t count);
RS_API int rs_train_debug_copy(rs_train* h, int layer, int what, void* d_dst, size_t bytes);

/* Added after ABI 2.9, rs_version unchanged: TCN training (riser/nets/tcn.py as riser/train.py builds it) through the receptive
 * cone of the last sample alone - csrc/tcn_train.hip.  fp32, two classes, one input channel, B reads of ONE length L >= 1 per
 * call (pitch ld >= L; lengths below the receptive field are legal).  The calls mean what their rs_train_* namesakes mean and
 * return their statuses; only the differences are stated here.
 * rs_tcn_train_create: RS_ERR_ARG before a device is touched for `bottleneck` != 0 (tcn-bot), a dtype other than RS_F32,
 * n_classes != 2, in_channels != 1, kernel < 2, dropout outside [0, 1).  `tensors` are host arrays in the order of the flat
 * parameter vector and of the tensor index of get_params / set_params / get_grads: per block weight_g [F], weight_v
 * [F][c_in][k], bias [F] of conv1, the same of conv2, then - only where c_in != n_filters, i.e. where the reference applies
 * it - the shortcut's weight [F][c_in] and bias; after the blocks the Linear [2][F] and its bias.  A shortcut the reference
 * builds but never applies has no tensor here: it takes no gradient and no update.  device < 0: a handle without device memory.
 * rs_tcn_train_slice_plan: conv `which` (0 conv1, 1 conv2, 2 an applied shortcut) of `block` contracts B * rows positions (the
 * rows per read of its output gradient inside the cone) in n_slices of slice_len.
 * rs_tcn_train_max_batch promises what every launch and the 2 GiB window take.
 * Dropout: element (conv c, read b, q, channel ch) - c = 2 block for conv1, 2 block + 1 for conv2; q = L-1 - position, the
 * distance from the read's last sample, so that a longer read gives the bits of its own tail - is kept iff
 *     mix(mix(mix(key_c + b) + q) + ch) >= floor(p * 2^32),
 *     key_c = mix(mix(mix(mix(mix(lo32(seed) + 0x9e3779b9) + hi32(seed)) + lo32(counter)) + hi32(counter)) + c),
 *     mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16        (all in 32-bit unsigned)
 * and a kept element is scaled by the fp32 value of 1 / (1 - p).  `counter` counts the rs_tcn_train_forward_backward calls on
 * the handle that returned RS_OK; rs_tcn_train_set_dropout sets p, the seed and the counter.  rs_tcn_train_evaluate is eval
 * mode: no mask.  p = 0 applies none.
 * rs_tcn_train_debug_copy (test hook): block `block`'s a1 = drop(relu(conv1)) (what 0) on the rows conv2 reads, a2 =
 * drop(relu(conv2)) (1) and out = relu(a2 + residual) (2) on the rows the next block reads, and the raw gradients arriving at
 * a1 (3) and at out (4), position-major [B][rows][n_filters padded to 4], row m at position L-1 - dilation_block * m (a2, out:
 * * base).  RS_ERR_ARG after an rs_tcn_train_evaluate or a refused call, as rs_train_debug_copy. */
typedef struct rs_tcn_train rs_tcn_train;
typedef struct {
    int32_t n_layers, n_filters, kernel, dilation;
    int32_t in_channels, n_classes;
    int32_t dtype;              /* rs_dtype: RS_F32 */
    int32_t bottleneck;         /* 0: riser/nets/tcn.py */
    double dropout;
    uint64_t seed;
} rs_tcn_train_config;
RS_API int rs_tcn_train_create(const rs_tcn_train_config* cfg, const float* const* tensors, int n_tensors, int device,
                               rs_tcn_train** out);
RS_API int rs_tcn_train_destroy(rs_tcn_train* h);
RS_API size_t rs_tcn_train_workspace_bytes(const rs_tcn_train* h, int B, int L);
RS_API int rs_tcn_train_max_batch(const rs_tcn_train* h, int L);
RS_API int rs_tcn_train_slice_plan(const rs_tcn_train* h, int block, int which, int B, int L, int32_t* n_slices,
                                   int32_t* slice_len, int32_t* rows);
RS_API int rs_tcn_train_forward_backward(rs_tcn_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld,
                                         void* d_ws, size_t ws_bytes, float* d_out, void* stream);
RS_API int rs_tcn_train_evaluate(rs_tcn_train* h, const float* d_x, const int32_t* d_labels, int B, int L, int ld, void* d_ws,
                                 size_t ws_bytes, float* d_out, void* stream);
RS_API int rs_tcn_train_set_dropout(rs_tcn_train* h, double p, uint64_t seed, int64_t counter);
RS_API int rs_tcn_train_adam_step(rs_tcn_train* h, float lr, float beta1, float beta2, float eps, void* stream);
RS_API int rs_tcn_train_get_params(rs_tcn_train* h, int index, float* dst, size_t count);
RS_API int rs_tcn_train_set_params(rs_tcn_train* h, int index, const float* src, size_t count);
RS_API int rs_tcn_train_get_grads(rs_tcn_train* h, int index, float* dst, size_t count);
RS_API int rs_tcn_train_debug_copy(rs_tcn_train* h, int block, int what, void* d_dst, size_t bytes);

/* Half precision has a range: RS_F16 / RS_F16X3 / RS_F16XF8 store activations as IEEE half, and a value beyond 65504 leaves the
 * conversion as +inf - the forward pass goes on, the probabilities of that read are wrong, and the reference's fp32 path
 * (riser/model.py:22-28) has no such failure.  Every kernel epilogue of those modes checks its conversions and raises a sticky flag
 * on the model; the launch entry points still return RS_OK.  rs_model_saturated waits for `stream` and returns 1 if any call
 * since the last reset overflowed, 0 if none did (always 0 for the fp32 and bf16 modes, before any device call), a negative
 * rs_status on error; `reset` != 0 clears the flag.  The read and the clear are ONE atomic exchange in a single-thread kernel
 * on `stream` (its result reaches the host through a pinned word the model owns): an overflow raised by a kernel on ANY
 * stream is either seen by this call or left for the next one - it is never dropped between a read and a separate clear.
 * One call at a time per model (the pinned word is the model's), as for the launch entry points.  (ABI 2.5) */
RS_API int rs_model_saturated(rs_model* m, int reset, void* stream);

/*
 * Test hook: every following forward pass of `m` also copies the output buffer of conv layer `layer`
 * (1 <= layer < n_layers; position-major [NB * (U >> (layer + 1)), cp_out] in the packed block layout - see
 * rs_block_samples - fp32 or 16-bit) into d_dst
 * (at most `bytes`).  d_dst = NULL switches it off.  Used by the layer-wise parity tests.
 */
RS_API int rs_debug_capture_layer(rs_model* m, int layer, void* d_dst, size_t bytes);

/*
 * Stage timing with HIP events on the launch stream (used by bench.py's roofline leg).
 * While enabled, rs_forward / rs_classify record one event before their first launch and
 * one after every kernel launch, on the caller's stream; no synchronisation is added.
 * rs_profile_read synchronises on the last recorded event and ADDS the elapsed
 * milliseconds per stage into stage_ms[0 .. n_layers + 1]:
 *   stage 0 = normalise, stage 1 = layer-0 conv, stage 1 + i = conv layer i (i >= 1),
 *   stage n_layers + 1 = GAP/FC/softmax head;
 * *calls receives the number of profiled forward calls.  Recorded events are consumed.
 * on = 1: one event per launch (an event costs ~4.5 us of stream time: 14 per call).  on = 2: coarse - events only
 * at the call's start, after normalise + layer 0 (their time lands in stage 1), after the LAST conv layer (the
 * whole conv stack, layers 1 .. n-1, lands in stage n_layers) and after the head: what bench.py's timed region uses.
 */
RS_API int rs_profile_enable(rs_model* m, int on);
RS_API int rs_profile_read(rs_model* m, float* stage_ms, int32_t* calls);

#ifdef __cplusplus
}
#endif
#endif /* RISER_AMD_H */
