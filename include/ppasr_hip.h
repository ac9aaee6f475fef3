/*
 * ppasr_hip.h -- C-ABI of libppasr_hip.so, the MI355X (gfx950) implementation of
 * PPASR's encoder-forward + CTC-decode hot path.
 *
 * PPASR has no FFI of its own (it is pure Python on PaddlePaddle); the boundary a
 * maintainer would bind is the set of Python call sites listed per entry point
 * below (paths relative to the reference checkout, `ppasr/...`).  INTEGRATION.md
 * shows the ctypes stub for each.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *   - all work is enqueued on the caller's HIP stream (`stream`, a hipStream_t
 *     passed as void*); nothing synchronises, nothing allocates after create();
 *   - the caller owns every buffer including the scratch workspace
 *     (size from ppasr_workspace_bytes); the handle owns only packed weights;
 *   - what workspace, scratch and output buffers hold on entry is irrelevant:
 *     results are a function of the inputs, the handle and the carried state
 *     (stream / group caches, beam-search state buffers) only, and every output
 *     is written in full unless its entry point says which part is undefined;
 *   - a handle is not re-entrant; distinct handles are independent;
 *   - no exceptions cross the ABI: int status + ppasr_last_error() (thread-local).
 */
#ifndef PPASR_HIP_H
#define PPASR_HIP_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with -fvisibility=hidden: these entry points are its whole dynamic symbol table
 * (tests/test_capi_cpu.py compares `nm -D --defined-only` with this header). */
#define PPASR_API __attribute__((visibility("default")))

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ppasr_model_s* ppasr_handle;
typedef struct ppasr_stream_s* ppasr_stream;

typedef enum {
  PPASR_OK = 0,
  PPASR_EINVAL = 1,       /* bad argument / shape */
  PPASR_EHIP = 2,         /* a HIP runtime call failed */
  PPASR_EUNSUPPORTED = 3, /* configuration outside what the kernels are built for */
  PPASR_EMISSING = 4,     /* a required weight blob is absent */
  PPASR_ENOSPACE = 5      /* workspace too small */
} ppasr_status;

enum { PPASR_MODEL_CONFORMER = 0, PPASR_MODEL_EFFICIENT_CONFORMER = 1,
       PPASR_MODEL_SQUEEZEFORMER = 2, PPASR_MODEL_DEEPSPEECH2 = 3 };

/* One named parameter of a Paddle state dict (`model.pdparams`, trainer.py:302-328):
 * float32, C-contiguous, HOST memory, Paddle layout (Linear.weight is [in,out]). */
typedef struct {
  const char* name;
  const float* data_host;
  int ndim;
  int64_t shape[4];
} ppasr_weight_blob;

/* Mirrors `encoder_conf` of configs/conformer.yml:2-16 plus the constructor
 * arguments of ConformerModel (model_utils/conformer/model.py:17-29). */
typedef struct {
  int model_type;        /* PPASR_MODEL_* */
  int input_dim;         /* fbank bins F (80) */
  int vocab_size;        /* V */
  int output_size;       /* d (256) */
  int attention_heads;   /* h (4) */
  int linear_units;      /* FFN hidden (2048) */
  int num_blocks;        /* L (12) */
  int cnn_module_kernel; /* 15 */
  int causal;            /* streaming model => causal depthwise conv (model.py:35-39) */
  int max_len;           /* positional table length (embedding.py:30), 5000 */
  /* Squeezeformer (configs/squeezeformer.yml:7-8, squeezeformer/encoder.py:30-31); -1 = none */
  int reduce_idx;
  int recover_idx;
  /* Efficient-Conformer (configs/efficient_conformer.yml:16-21) */
  int stride_layer_idx;   /* layer with the stride-2 depthwise conv, -1 = none */
  int group_layer_mask;   /* bit i set: layer i uses grouped attention */
  int group_size;         /* 2, 3 (the shipped value) or 4 frames per attention token */
  /* DeepSpeech2 (configs/deepspeech2.yml:5, deepspeech2/encoder.py:36-42): nn.GRU layers instead of nn.LSTM */
  int use_gru;
  /* Conformer / Efficient-Conformer front end, `input_layer` (conformer/encoder.py:93-104, subsampling.py):
     0 = conv2d (Conv2dSubsampling4: 3x3/2, 3x3/2), 6 = conv2d6 (Conv2dSubsampling6: 3x3/2, 5x5/3, `embed.linear`),
     8 = conv2d8 (Conv2dSubsampling8: 3x3/2 three times, `embed.linear`).  6 / 8: batched encode and single stream
     handles (no session groups); key-padding / conv pad masks use 6t / 8t < len (the reference's mask slicing) */
  int input_layer;        /* 1 = linear (LinearNoSubsampling, subsampling.py:24-65: no time reduction; general route only) */
  /* Non-default ConformerEncoder constructor arguments (conformer/encoder.py:38-48), PPASR_OPT_* below; 0 = the shipped
     configuration (rel_pos, normalize_before, macaron_style, use_cnn_module, swish).  Any other value -- like
     output_size != 256, input_layer = linear or a cnn_module_kernel other than 7 / 15 / 31 -- selects the general layer
     route (capi_generic.hip: the same packed weights and matrix-core GEMMs, one launch per layer piece instead of the
     fused 256-wide row-block kernels).  options / input_layer = linear: model_type = conformer only; output_size 512 / 768 /
     1024 (heads of 64): conformer, efficient_conformer and squeezeformer, batched and streaming. */
  int options;
  /* Efficient-Conformer with SEVERAL stride layers (`stride_layer_idx: [1, 3]`, `stride: [2, 2]`, efficient_conformer/
     encoder.py:50-54,117-128): bit i set = layer i is a stride-2 layer (its depthwise conv strides, the residual goes
     through AvgPool1D(2, ceil_mode), every later layer's conv kernel is halved once more).  0 = use stride_layer_idx.  More
     than one bit: the general layer route, batched encode only (stream handles are refused). */
  int stride_layer_mask;
} ppasr_model_desc;

enum {
  PPASR_OPT_POS_REL = 0,       /* pos_enc_layer_type: rel_pos -> RelPositionMultiHeadedAttention */
  PPASR_OPT_POS_ABS = 1,       /*   abs_pos: x * sqrt(d) + pe, MultiHeadedAttention (embedding.py:25-84) */
  PPASR_OPT_POS_NONE = 2,      /*   no_pos: MultiHeadedAttention, x unchanged (embedding.py:10-22) */
  PPASR_OPT_POS_MASK = 3,
  PPASR_OPT_POST_NORM = 4,     /* normalize_before = False (encoder.py:380-428; no after_norm) */
  PPASR_OPT_CONCAT_AFTER = 8,  /* concat_after = True: x + concat_linear([x | att(x)]) (encoder.py:395-397) */
  PPASR_OPT_NO_MACARON = 16,   /* macaron_style = False: no feed_forward_macaron, ff_scale 1 (encoder.py:330-334) */
  PPASR_OPT_NO_CNN = 32,       /* use_cnn_module = False: no conv module, no norm_final */
  PPASR_OPT_SQ_NO_ADAPTIVE_SCALE = 4096, /* model_type squeezeformer only: adaptive_scale = False (squeezeformer/encoder.py:44;
                                  the checkpoint's ada_scale / ada_bias are then not applied).  The two other options of that
                                  encoder need no flag: dw_stride = True is recognised by the [d][1][3][3] shape of
                                  encoder.embed.dw_conv.weight, final_proj by the presence of encoder.final_proj.weight */
  PPASR_OPT_SQ_PRE_NORM = 8192, /* model_type squeezeformer only: normalize_before = True (squeezeformer/encoder.py:49,467-493:
                                  LayerNorm_k in front of module k instead of behind the residual sum); general layer route */
  PPASR_OPT_ACT_SHIFT = 8,     /* activation_type (utils/common.py:189-206) in bits 8..11: */
  PPASR_OPT_ACT_MASK = 15
};
enum { PPASR_ACT_SWISH = 0, PPASR_ACT_RELU = 1, PPASR_ACT_GELU = 2, PPASR_ACT_TANH = 3, PPASR_ACT_HARDTANH = 4,
       PPASR_ACT_RELU6 = 5, PPASR_ACT_LEAKYRELU = 6, PPASR_ACT_SELU = 7, PPASR_ACT_ELU = 8, PPASR_ACT_HARDSWISH = 9,
       PPASR_ACT_HARDSHRINK = 10 };

PPASR_API const char* ppasr_last_error(void);
PPASR_API const char* ppasr_version(void);

/* Replaces: model construction + paddle.inference.create_predictor
 * (infer_utils/inference_predictor.py:41-77) / PPASRTrainer.__setup_model
 * (trainer.py:172-210).  Uploads and re-packs the weights into MFMA fragment order. */
PPASR_API ppasr_status ppasr_create(const ppasr_model_desc* desc, const ppasr_weight_blob* weights_host, int n_weights,
                          ppasr_handle* out);
PPASR_API ppasr_status ppasr_destroy(ppasr_handle h);

/* frames after the conv front-end: ((T-1)/2-1)/2  (conformer/subsampling.py:84-94,115) */
PPASR_API int ppasr_out_frames(ppasr_handle h, int T);
PPASR_API size_t ppasr_workspace_bytes(ppasr_handle h, int B, int T);

/* Replaces ConformerModel.get_encoder_out (model_utils/conformer/model.py:148-162), as called by
 * PPASRTrainer.evaluate (trainer.py:626) and InferencePredictor.predict (inference_predictor.py:103-145).
 *   feats [B,T,F] f32 zero-padded, lens [B] i64  ->  any of
 *   probs  [B,T',V] f32  softmax(ctc_lo(enc))       (what the reference returns)
 *   logits [B,T',V] f32  pre-softmax                (parity tap)
 *   frame_argmax [B,T'] i32, frame_maxprob [B,T'] f32: per-frame argmax / probability at the
 *     argmax, produced inside the CTC-head kernel (fused ctc_greedy first stage,
 *     decoders/ctc_greedy_decoder.py:21-22); pass NULL for outputs not wanted. */
PPASR_API ppasr_status ppasr_encode(ppasr_handle h, const float* feats, const int64_t* lens, int B, int T,
                          float* probs, float* logits, int32_t* frame_argmax, float* frame_maxprob,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Debug taps: when set (host call, before ppasr_encode), intermediate activations are copied
 * to `taps` in the order documented in DESIGN.md; pass NULL to clear. */
PPASR_API ppasr_status ppasr_set_debug_taps(ppasr_handle h, float* taps, size_t n_floats);

/* Ragged batches.  The reference computes every padded row of a batch (its batched decoders even consume them,
 * trainer.py:347).  With enable != 0, ppasr_encode computes, per utterance, only the rows its VALID output frames
 * depend on (t < ceil(len/4), or ceil(len/8) after a rate change, plus a few rows of slack for the grouped-attention /
 * stride / time-reduction reads): whole 32-row blocks behind them are skipped in every kernel and attention stops at
 * the last valid key.  Valid rows are bit-identical to the default mode AS LONG AS both runs use the same block form of the
 * layer kernels (ppasr_set_row_block): with the default rule (-1) the form is chosen from the rows actually computed
 * (ppasr_set_lengths_hint), so a ragged call may take the 16-row kernels where the padded call takes the 32-row ones --
 * the same sums in another order, equal to ~1e-6 relative; pin the form (16 / 32) where bit-identity between the modes,
 * between ranks or between batch compositions is required.  Rows of `probs` / `logits` behind an
 * utterance's last valid frame are set to 0, `frame_argmax` to 0 (blank) and `frame_maxprob` to 0 -- pass frame_lens
 * to the decoders.  Default: off (= the reference's outputs for every row).  Built into the fused 256-column kernels and
 * the general layer route (widths 512 .., constructor options) behind the conv front ends (behind conv2d6 / conv2d8 and on
 * the general route the layers and the head skip, the front end itself computes every row): enabling it on an
 * input_layer = linear or DeepSpeech2 handle returns PPASR_EUNSUPPORTED (those compute every row). */
PPASR_API ppasr_status ppasr_set_skip_padding(ppasr_handle h, int enable);

/* Under-filled launches.  A kernel with fewer 32-row blocks than the chip has CUs takes as long as a full one.  When a
 * call has <= 128 row blocks (small batches, the half-rate layers of the Efficient-Conformer, a single streaming
 * session) the Conformer-family layer tail is cut at its two feed-forward modules and each module's hidden dimension is
 * split over 2 / 4 / 8 workgroups per row block (partial sums joined by the next launch).  Same arithmetic up to the
 * order of the final sum over hidden chunks.  mode: -1 = decide by grid size (default), 0 = never (always the fused
 * kernels, the fused attention kernel included), 2 / 4 / 8 = always that many slices.  The partial sums live in the
 * workspace: ppasr_workspace_bytes / ppasr_chunk_workspace_bytes / ppasr_group_chunk_workspace_bytes follow the mode, so
 * query them again after changing it (a call with a smaller workspace returns PPASR_ENOSPACE). */
PPASR_API ppasr_status ppasr_set_ffn_split(ppasr_handle h, int mode);

/* Conv2dSubsampling4 (conformer/subsampling.py:84-88) as ONE launch (csrc/front_fused.hip: conv1's output is computed
 * tile by tile inside conv2's implicit GEMM and never written to HBM) or as two (k_conv1, then conv2 reading its output).
 * Bit-identical results.  mode: -1 (default) / 1 = one launch, 0 = two.  The one-launch kernel is 0.5 - 0.8 % faster
 * end to end on its own stream; with a beam search of the previous batch running on a second stream the two-launch form
 * is the faster one (conv2's workgroups leave room on a CU for the search's, the fused kernel's do not), which is why
 * the pipelined plans of ppasr_amd/parallel.py select it.  Other front ends ignore the setting. */
PPASR_API ppasr_status ppasr_set_front_fused(ppasr_handle h, int mode);

/* Block form of the layer kernels (no reference counterpart; csrc/rbt.h): -1 (default) = by grid size -- up to 32 row
 * blocks of 32 rows the split route above; 16-row blocks (v_mfma_f32_16x16x4_f32 on 8 waves) where two short rounds of
 * them beat the 32-row rounds (33 .. 128 blocks: under-filled launches); else 32-row blocks (v_mfma_f32_32x32x2_f32 on
 * 8 waves).  16 / 32 = always that form; PPASR_ROW_BLOCK_32_W16 = 32 rows on SIXTEEN waves (v_mfma_f32_16x16x4_f32 on
 * four waves per SIMD; measured equal to the 8-wave kernels end to end, kept as an option).  Same arithmetic up to the
 * summation order inside a 16-wide k step (1e-6 relative).  Built for the Conformer / Efficient-Conformer /
 * Squeezeformer layer kernels behind the conv2d (4x) front end; other routes ignore it. */
#define PPASR_ROW_BLOCK_32_W16 1032
PPASR_API ppasr_status ppasr_set_row_block(ppasr_handle h, int rows);

/* Arithmetic of the large GEMMs of the fused Conformer-family routes (no reference counterpart; csrc/h3.h).
 * PPASR_GEMM_F32 (default): v_mfma_f32_32x32x2_f32, exact fp32 products.  PPASR_GEMM_F16X3 (opt-in): every operand is the
 * sum of two fp16 pieces (22 significant bits; products of pieces are exact in fp32, accumulation in fp32), three
 * v_mfma_f32_32x32x16_f16 per 16-wide k step instead of eight fp32 MFMAs -- one feed-forward module deviates from float64
 * by 2.7e-7 where fp32 arithmetic deviates by 5.5e-7 (tools/experiments/r05/ffn_h3.hip), but NOT bit-identical to the
 * default mode.  The first call re-packs the weights concerned on the device (second copy, ~ 10 MB per layer).
 * Range.  Weights are scaled by 2^8, activations by 2^4 before they are cut into fp16 pieces: a weight of magnitude >= 255.9
 * makes this call fail with PPASR_EUNSUPPORTED (the handle stays in its previous mode; a Squeezeformer handle re-packs
 * diag(ada_scale) w_1, so the product counts there); an activation beyond 4 094 at a GEMM input is handled by the range
 * guard below -- never Inf / NaN.  The guarded inputs: ReLU outputs in front of conv2 / the input projection, LayerNorm
 * outputs in front of W1, Q/K/V, pointwise_conv1 and the CTC head, swish values in front of W2 and pointwise_conv2, the
 * attention context in front of linear_out, and in the fused attention K (projection + bias), q + pos_bias_u and
 * q + pos_bias_v (tests/guard_sites.py lists every one with its source line; each is tripped alone by
 * tests/test_gemm_guard_sites_gpu.py).
 * Built for the fused 256-wide routes: Conformer / Efficient-Conformer -- feed-forward modules, Q/K/V, pointwise_conv2
 * (8-wave 32-row layer kernels incl. the Efficient-Conformer's stride layer; depthwise kernel sizes 15 and 7), linear_out +
 * pointwise_conv1 and the score contraction
 * [q+u | q+v] [k | p]^T of the fused attention kernel (K as fp16 hi / lo planes from the QKV stage, the layer's positional
 * table re-packed by this call: + 1 KiB per table row; an entry beyond 4 094 refuses the mode like a weight does);
 * Squeezeformer -- both feed-forward modules of the 32-row layer kernels (depthwise kernel sizes 31 and 15); all three -- the
 * second convolution of the 4x front end (then its own launch behind conv1), the input projection (full launches; an
 * under-filled launch splits its K over several workgroups in fp32), the CTC head;
 * Conformer / Efficient-Conformer also on the split route of under-filled launches and therefore on their stream handles and
 * session groups (ppasr_encode_chunk*: a saturated chunk is counted in the guard statistics, NOT re-run; a chunk's front
 * end and CTC head keep fp32 arithmetic, as do linear_out + pointwise_conv1 of a grouped-attention layer on full launches,
 * which has no fused attention kernel).  The other block
 * forms (16 rows, 16 waves), the non-feed-forward units of Squeezeformer's split route and streams, the attention's P V product and depthwise convolutions keep fp32 arithmetic.  ppasr_gemm_coverage
 * tells which of the three parts switched (a Conformer with cnn_module_kernel 31 gets the front end and the head only).
 * PPASR_EUNSUPPORTED on DeepSpeech2 handles and on the general layer route.  Measured (NOTES.md 9.8): logits within 1e-6 .. 3e-6
 * of the default mode's, the reference-source pin tests pass with unchanged criteria, 1.2 - 1.7 x faster end to end. */
#define PPASR_GEMM_F32 0
#define PPASR_GEMM_F16X3 1
#define PPASR_GEMM_COVERS_LAYERS 1 /* the encoder layers' GEMMs */
#define PPASR_GEMM_COVERS_FRONT 2  /* conv2 + input projection of the 4x front end */
#define PPASR_GEMM_COVERS_HEAD 4   /* the CTC head */
PPASR_API ppasr_status ppasr_set_gemm_mode(ppasr_handle h, int mode);
PPASR_API int ppasr_gemm_coverage(ppasr_handle h); /* PPASR_GEMM_COVERS_* bits of the current mode; 0 in PPASR_GEMM_F32 */
/* Range guard of PPASR_GEMM_F16X3.  The kernels saturate an out-of-range (or NaN) GEMM input to +-65 504 / 2^4 and count
 * the event in a device counter.  enable = 1 (default): ppasr_encode reads the counters back after its launches (it then
 * SYNCHRONISES `stream` before it returns) and, if the call saturated anything, runs the call again on the fp32 kernels:
 * the caller always gets finite-input-exact results, the fp32 mode's bit for bit in that case.  enable = 0: ppasr_encode
 * stays asynchronous, a saturated result stands, and the caller polls ppasr_gemm_guard_stats.  The counters are shared by
 * the handles of a process: concurrent fp16 x3 handles can cause each other a spurious fp32 re-run, never a missed one. */
PPASR_API ppasr_status ppasr_set_gemm_guard(ppasr_handle h, int enable);
/* -> calls that were re-run on the fp32 kernels / saturation events seen by this handle (guard off: waits for the device,
 * then counts the events since this handle last looked).  Either pointer may be NULL. */
PPASR_API ppasr_status ppasr_gemm_guard_stats(ppasr_handle h, long long* fallbacks_host, long long* events_host);
/* Host copy of the `lens` the following ppasr_encode calls of a batch of B utterances will pass (NULL / 0: forget it).
 * Only ever used to CHOOSE between kernel variants for ragged batches (ppasr_set_skip_padding), whose count of computed
 * rows the host cannot otherwise know; no kernel reads it.  A wrong hint costs speed; the variants differ in the order of
 * their sums (~1e-6 relative, see ppasr_set_row_block), so two calls with different hints need not agree bit for bit. */
PPASR_API ppasr_status ppasr_set_lengths_hint(ppasr_handle h, const int64_t* lens_host, int B);

/* Host helper (no device work): Levenshtein distance between two int32 sequences -- what ppasr/utils/metrics.py:4-29
 * (cer / wer) gets from the `Levenshtein` C extension.  Returns -1 on a null argument with a positive length. */
PPASR_API long long ppasr_edit_distance(const int32_t* a, int na, const int32_t* b, int nb);

/* Replaces the third-party `paddlespeech_ctcdecoders` entry points PPASR calls:
 *   ctc_beam_search_decoding / ctc_beam_search_decoding_batch  (decoders/swig_wrapper.py:61-62,98-100,
 *     from BeamSearchDecoder.decode_beam_search_offline / decode_batch_beam_search_offline,
 *     decoders/beam_search_decoder.py:45-73), with init_state = 1;
 *   CtcBeamSearchDecoderBatch.next() + decode() (swig_wrapper.py:106-121, beam_search_decoder.py:75-96):
 *     call again with init_state = 0 and the SAME state buffer for every further chunk.
 * CTC prefix beam search; the external scorer variant is ppasr_ctc_beam_search_lm below.
 *   probs [B,T,V] f32, frame_lens [B] i32 or NULL; per utterance the `nbest` best prefixes:
 *   tokens [B,nbest,max_tokens] i32 (-1 padded), lens [B,nbest] (-1 = no such hypothesis: its tokens are all -1 and
 *   its score is 0), scores [B,nbest] f64 = -log P(prefix) (the upstream return convention).
 *   state: device scratch of ppasr_ctc_beam_state_bytes(B, max total frames, beam_size) bytes that
 *   holds the beam, the prefix arena (both kept between chunk calls) and the per-frame records of the
 *   pruning pre-pass (get_pruned_log_probs of every frame of the call: T <= max total frames). */
PPASR_API size_t ppasr_ctc_beam_state_bytes(int B, int max_frames, int beam_size);
/* Extra device scratch a call with this pruning configuration needs (0 for every configuration the reference ships:
 * cutoff_prob < 1 with cutoff_top_n <= 128).  Non-zero when more than 128 characters of a frame can survive the pruning
 * -- cutoff_prob >= 1, the default of swig_wrapper.py:38,71, where upstream ignores cutoff_top_n and keeps the WHOLE
 * vocabulary; or cutoff_top_n > 128 -- or when beam_size x (1 + candidates) elements do not fit LDS: the per-frame pruning
 * records and the element list of a frame then live in this scratch (T x (2 + 2 V) words + beam x (1 + V) x 5 bytes per
 * utterance).  Pass it to ppasr_ctc_beam_search_ws; the plain entry points return PPASR_ENOSPACE for such a call.
 * There is no cap on the candidates of a frame. */
PPASR_API size_t ppasr_ctc_beam_scratch_bytes(int B, int T, int V, int beam_size, double cutoff_prob, int cutoff_top_n);
/* Streaming past the sized capacity: copies the beams and prefix arenas of a state buffer into a LARGER one (sized with
 * ppasr_ctc_beam_state_bytes for more frames), which then continues the same search.  The reference's decoder object has
 * no frame limit; callers double the buffer when the next chunk would not fit.  Asynchronous on `stream`. */
PPASR_API ppasr_status ppasr_ctc_beam_state_grow(const void* old_state, size_t old_bytes, void* new_state, size_t new_bytes, int B,
                                       int beam_size, void* stream);
/* Reads back the per-utterance status words of a (streaming) state buffer: non-zero = the prefix arena ran out because
 * more cumulative frames were decoded than the buffer was sized for; returns PPASR_ENOSPACE then.  Synchronises. */
PPASR_API ppasr_status ppasr_ctc_beam_status(const void* state, size_t state_bytes, int B, int beam_size, int32_t* status_host,
                                   void* stream);
/* Streaming without an ever-growing state: compacts the prefix arenas of the B blocks of a state buffer (layout of
 * ppasr_ctc_beam_search_ws) in place.  Every node that is neither in the beam nor an ancestor of a beam entry is dropped
 * -- what PathTrie::remove does upstream after every frame -- and the rest is renumbered in creation order; the search
 * continues from the compacted buffer with the same results bit for bit (node ids take part in no comparison).
 * rebuild_table: 1 for searches with a word-based scorer (their node table is rebuilt from the compacted arena).  For
 * those, compaction moves the search TO the upstream behaviour: without it a prefix keeps its node and the dictionary state
 * saved there even after it left the beam with no live descendant; upstream, the C oracle and a compacted search delete
 * such a node and create it fresh.  The two differ only for a prefix that died childless, had its dictionary state reset
 * while alive, and is created again.
 * live_nodes_host [B] or NULL: with it the blocks' node counts afterwards are copied back (-1: a block whose arena was
 * exhausted, left untouched) and `stream` is synchronised; without it the call is asynchronous.  A caller that kept
 * count of the frames decoded may continue with ceil((L - 1) / beam_size) for the largest L.  PPASR_EINVAL (null state,
 * B <= 0, a state too small for one frame) before any device work. */
PPASR_API ppasr_status ppasr_ctc_beam_state_compact(void* state, size_t state_bytes, int B, int beam_size, int rebuild_table,
                                          int32_t* live_nodes_host, void* stream);
PPASR_API ppasr_status ppasr_ctc_beam_search(const float* probs, const int32_t* frame_lens, int B, int T, int V, int beam_size,
                                   double cutoff_prob, int cutoff_top_n, int blank, int nbest, int max_tokens,
                                   int32_t* tokens, int32_t* lens, double* scores, void* state, size_t state_bytes,
                                   int init_state, void* stream);

/* External scorer = `Scorer(alpha, beta, model_path, vocabulary)` of paddlespeech_ctcdecoders (decoders/swig_wrapper.py:18-33,
 * built by BeamSearchDecoder.__init__, decoders/beam_search_decoder.py:19-29): back-off n-gram model, either
 * CHARACTER-based (every LM word is one UTF-8 character, as PPASR's Mandarin models are: scored on every extension) or
 * WORD-based (configs/english_example.yml: scored when a space completes a word, the prefixes constrained to spellings
 * of the model's vocabulary by a dictionary -- upstream's OpenFST acceptor, here a character trie; the acoustic vocabulary
 * must contain the space token " " or "<space>").  Model files: the ARPA text format (csrc/lm.hip) and KenLM binaries
 * (.klm, what PPASR ships: decoders/beam_search_decoder.py:19-29) of every model type: "probing" / "rest probing",
 * "trie", and the quantised (-q) / Bhiksha-array (-a) trie variants (csrc/klm.hip).  ppasr_lm_create sniffs the format
 * from the file's magic, like KenLM's loader.
 * vocab_utf8[V]: the acoustic vocabulary (token id -> string), used to map token ids to LM words (unknown -> OOV). */
typedef struct ppasr_lm_s* ppasr_lm_handle;
PPASR_API ppasr_status ppasr_lm_create(const char* model_path, const char* const* vocab_utf8, int V, ppasr_lm_handle* out);
PPASR_API ppasr_status ppasr_lm_create_arpa(const char* arpa_path, const char* const* vocab_utf8, int V, ppasr_lm_handle* out);
PPASR_API ppasr_status ppasr_lm_create_klm(const char* klm_path, const char* const* vocab_utf8, int V, ppasr_lm_handle* out);
PPASR_API const char*  ppasr_lm_format(ppasr_lm_handle lm);              /* "arpa", "klm-probing", "klm-rest-probing", "klm-trie",
                                                                  "klm-quant-trie", "klm-array-trie", "klm-quant-array-trie" */
PPASR_API int          ppasr_lm_word_index(ppasr_lm_handle lm, int token); /* LM word index of an acoustic token, 0 = OOV */
PPASR_API int          ppasr_lm_bos(ppasr_lm_handle lm);
PPASR_API int          ppasr_lm_eos(ppasr_lm_handle lm);
/* Verification hooks of the model-file readers (no device is touched; the decoder never calls them):
 * ppasr_lm_debug_load_host parses a model into the host-side table only, ppasr_lm_debug_host_score evaluates
 * Scorer::get_log_cond_prob for a window of `order` LM word indices (oldest first) on that table. */
PPASR_API ppasr_status ppasr_lm_debug_load_host(const char* model_path, const char* const* vocab_utf8, int V, ppasr_lm_handle* out);
PPASR_API double       ppasr_lm_debug_host_score(ppasr_lm_handle lm, const int32_t* window);
/* Verification hooks of the device scorer (csrc/lm.h).  ppasr_lm_debug_table copies out the host mirror of the n-gram
 * table as it is laid out for the device: 16-byte slots (uint64 key, 0 = empty; float log10 prob; float log10 back-off),
 * `mask + 2` of them -- the power-of-two table and, behind it, the copy of slot 0.  It returns that slot count; with
 * slots_out == NULL it only returns it, otherwise n_slots must equal it (else -1).  Works on a host-only handle.
 * ppasr_lm_debug_device_score evaluates Scorer::get_log_cond_prob of n_windows windows ([n_windows][order] int32 LM word
 * indices, oldest first, device memory) with the device functions, one thread per window, into out_dev[n_windows]
 * (doubles, device memory): form 0 = the plain back-off walk, 1 = the factorised form the search uses per (hypothesis,
 * candidate) pair, 2 = the same with the candidate's unigram handed in by the caller.  PPASR_EINVAL for a host-only
 * handle, a null pointer, n_windows < 0 or another form; n_windows == 0 launches nothing. */
PPASR_API long long    ppasr_lm_debug_table(ppasr_lm_handle lm, void* slots_out, long long n_slots);
PPASR_API ppasr_status ppasr_lm_debug_device_score(ppasr_lm_handle lm, const int32_t* windows_dev, int n_windows, int form,
                                                   double* out_dev, void* stream);
PPASR_API ppasr_status ppasr_lm_destroy(ppasr_lm_handle lm);
PPASR_API int          ppasr_lm_order(ppasr_lm_handle lm);
PPASR_API int          ppasr_lm_is_character_based(ppasr_lm_handle lm);
PPASR_API long long    ppasr_lm_dict_size(ppasr_lm_handle lm);   /* Scorer::get_dict_size(): words in the dictionary (word-based models) */
PPASR_API int          ppasr_lm_space_id(ppasr_lm_handle lm);    /* acoustic token id of the space (" " or "<space>"), -1 if none */
PPASR_API long long    ppasr_lm_ngram_count(ppasr_lm_handle lm);
/* ppasr_ctc_beam_search with the scorer: alpha * ln P_lm(c | prefix) + beta on every extension, the min_cutoff pruning
 * of ctc_beam_search_decoder.cpp, and result scores = -(score - len*beta - alpha*ln P_lm(sentence)) ("approx_ctc").
 * lm == NULL: identical to ppasr_ctc_beam_search. */
PPASR_API ppasr_status ppasr_ctc_beam_search_lm(const float* probs, const int32_t* frame_lens, int B, int T, int V, int beam_size,
                                      double cutoff_prob, int cutoff_top_n, int blank, int nbest, int max_tokens,
                                      int32_t* tokens, int32_t* lens, double* scores, void* state, size_t state_bytes,
                                      int init_state, ppasr_lm_handle lm, double alpha, double beta, void* stream);
/* ... with caller-owned scratch of at least ppasr_ctc_beam_scratch_bytes(B, T, V, beam_size, cutoff_prob, cutoff_top_n)
 * bytes (may be NULL / 0 when that is 0).  The scratch is only used during the call. */
PPASR_API ppasr_status ppasr_ctc_beam_search_ws(const float* probs, const int32_t* frame_lens, int B, int T, int V, int beam_size,
                                      double cutoff_prob, int cutoff_top_n, int blank, int nbest, int max_tokens,
                                      int32_t* tokens, int32_t* lens, double* scores, void* state, size_t state_bytes,
                                      int init_state, ppasr_lm_handle lm, double alpha, double beta, void* scratch,
                                      size_t scratch_bytes, void* stream);

/* ---- hypothesis records of the utterance-parallel path (north_star: "a single RCCL all-gather ... for decoded
 * hypotheses"; no reference counterpart -- the reference has no multi-GPU inference, trainer.py:529-544 is training DP).
 * A record row is int32 [cols + extra]: tokens (-1 padded to cols) | n_tokens | score (f64, low word first)
 * [| utterance index when extra = 4].  ppasr_hyp_pack writes the k hypotheses of one decoder call (tokens [k][L] with
 * row stride token_stride; n_tokens / score with element strides, so that the n-best = 1 column of the beam search's
 * [B][nbest] outputs can be passed in place; index [k] or NULL) into rows row0 .. row0 + k - 1 of `rec`;
 * ppasr_hyp_unpack reads N rows (row order[r], or r when order is NULL) back into tokens [N][cols], n_tokens [N],
 * score [N] and (optionally) the index column.  One launch each, on `stream`. */
PPASR_API ppasr_status ppasr_hyp_pack(const int32_t* tokens, long long token_stride, int L, const int32_t* n_tokens,
                                      long long n_stride, const double* score, long long score_stride, const int32_t* index,
                                      int k, int32_t* rec, int row0, int cols, int extra, void* stream);
PPASR_API ppasr_status ppasr_hyp_unpack(const int32_t* rec, const int64_t* order, int N, int cols, int extra, int32_t* tokens,
                                        int32_t* n_tokens, double* score, int32_t* index, void* stream);

/* ---- streaming: ConformerModel.get_encoder_out_chunk (model_utils/conformer/model.py:164-184) =
 * ConformerEncoder.forward_chunk (conformer/encoder.py:208-283) + ctc softmax, as driven by
 * InferencePredictor.predict_chunk_conformer / reset_stream (inference_predictor.py:184-220) and
 * PPASRPredictor.predict_stream (predict.py:232-337).  The attention key/value cache and the conv-module
 * cache stay resident on the device inside the stream object; `offset` (inference_predictor.py:39,211)
 * is tracked by the object.  B = 1 per stream (encoder.py:238); run several streams for several sessions.
 * Any causal Conformer-family handle behind a conv front end, general-route handles (output_size 512 .. 1024,
 * ppasr_model_desc.options) included; use_cnn_module = 0 handles carry no conv cache (export: cnn_cache untouched). */
PPASR_API ppasr_status ppasr_stream_create(ppasr_handle h, ppasr_stream* out);
PPASR_API ppasr_status ppasr_stream_destroy(ppasr_stream s);
PPASR_API ppasr_status ppasr_stream_reset(ppasr_stream s, void* stream);
PPASR_API int ppasr_stream_offset(ppasr_stream s);        /* encoder frames emitted so far */
PPASR_API int ppasr_stream_cache_frames(ppasr_stream s);  /* cache_t1: key/value frames currently cached */
PPASR_API size_t ppasr_chunk_workspace_bytes(ppasr_handle h, int T);  /* (the chunk's activations, the cache-trim scratch and
                                                                         the front end's K-split tiles; never decreases as T
                                                                         grows, so a workspace sized for the longest chunk
                                                                         serves every shorter one) */
/*   feats [1,T,F] f32; required_cache_size as in encoder.py:255-260 (<0 keep everything, the value
 *   predict_stream uses; 0 none; >0 last n frames); probs [1,c,V] or NULL; c = ((T-1)/2-1)/2 is also
 *   written to *c_out_host (host int, may be NULL). */
PPASR_API ppasr_status ppasr_encode_chunk(ppasr_stream s, const float* feats, int T, int required_cache_size, float* probs,
                                int32_t* frame_argmax, float* frame_maxprob, int* c_out_host, void* workspace,
                                size_t workspace_bytes, void* stream);
/* Reference tensor layouts of the caches: att_cache [L][h][t][2*dk] (h = attention_heads, dk = 64), cnn_cache [L][1][d][k-1]
 * (d = output_size). */
PPASR_API ppasr_status ppasr_stream_export_cache(ppasr_stream s, float* att_cache, float* cnn_cache, void* stream);
PPASR_API ppasr_status ppasr_stream_import_cache(ppasr_stream s, const float* att_cache, int cache_t, const float* cnn_cache,
                                       int offset, void* stream);

/* ---- DeepSpeech2: DeepSpeech2Model.get_encoder_out / get_encoder_out_chunk (model_utils/deepspeech2/model.py:62-72),
 * as called by trainer.py:626 and InferencePredictor.predict / predict_chunk_deepspeech
 * (inference_predictor.py:103-145,147-182).  Create the handle with model_type = PPASR_MODEL_DEEPSPEECH2,
 * output_size = rnn_size, num_blocks = num_rnn_layers, causal = 1 for the streaming ('forward') model and 0 for
 * the bidirectional one (deepspeech2/model.py:40).
 *   feats [B,T,F], lens [B] i64 -> probs [B,T',V] f32, out_lens [B] i64 (= ((len-1)/2-1)/2, may be NULL);
 *   init_h / init_c / final_h / final_c: [num_rnn_layers*dirs, B, rnn_size] state boxes (NULL = zeros / not wanted).
 * Synchronisation: asynchronous on `stream`, EXCEPT single-utterance LSTM calls (B = 1, rnn_size 1024) on the persistent
 * recurrence route: its launches need every workgroup of their grid resident at once, so the call ends with a stream
 * synchronisation and a 4-byte read-back of the kernels' give-up flag; when a launch gave up (the chip was shared with
 * another stream / process) the call re-runs on the per-step kernels before it returns, and the handle stays on those for
 * the next 64 .. 1 024 calls before it tries the persistent route again.  PPASR_DS2_PERSIST=0 switches the route off. */
PPASR_API size_t ppasr_ds2_workspace_bytes(ppasr_handle h, int B, int T);  /* (never decreases as B or T grows) */
/* Test hook, not part of any product path: `n_workgroups` workgroups that each take a whole CU (1 024 threads, 128
 * registers per lane) and spin for `milliseconds` on `stream`.  With part of the chip held like this the persistent
 * recurrence above cannot become fully resident and gives up: the tests check that the call then returns the per-step
 * kernels' result. */
PPASR_API ppasr_status ppasr_debug_occupy_cus(int n_workgroups, int milliseconds, void* stream);
PPASR_API ppasr_status ppasr_ds2_encode(ppasr_handle h, const float* feats, const int64_t* lens, int B, int T, const float* init_h,
                              const float* init_c, float* probs, int64_t* out_lens, float* final_h, float* final_c,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Measurement hook (bench.py roofline leg; no reference counterpart): when enabled, every kernel launch
 * of the next ppasr_encode is bracketed by a HIP event pair on the caller's stream; ppasr_profile_read
 * synchronises those events and returns, per kernel class, the summed duration (ms) and launch count
 * into HOST arrays of PPASR_N_KERNEL_CLASSES entries.  Conformer / Efficient-Conformer handles of width 256 only
 * (PPASR_EUNSUPPORTED otherwise); ppasr_kprof_* below covers every route by kernel name. */
#define PPASR_N_KERNEL_CLASSES 10
PPASR_API ppasr_status ppasr_profile_enable(ppasr_handle h, int enable);
PPASR_API ppasr_status ppasr_profile_read(ppasr_handle h, float* total_ms_host, int* launches_host);
PPASR_API const char* ppasr_kernel_class_name(int cls);

/* Kernel-name profiler (bench.py roofline leg for every model family and the decoders; no reference counterpart).
 * Between begin and end, every kernel the CALLING THREAD launches through this library carries a dispatch-attached HIP
 * event pair; end synchronises them and returns one entry per distinct kernel (the names rocprofv3's kernel trace
 * prints, without the parameter list): names_host [max_entries][PPASR_KPROF_NAME_LEN] chars, total_ms_host /
 * launches_host [max_entries], *n_out_host = entries written.  Not to be combined with ppasr_profile_enable. */
#define PPASR_KPROF_NAME_LEN 160
PPASR_API ppasr_status ppasr_kprof_begin(void);
PPASR_API ppasr_status ppasr_kprof_end(int max_entries, char* names_host, float* total_ms_host, int* launches_host, int* n_out_host);

/* Replaces greedy_decoder / greedy_decoder_batch (decoders/ctc_greedy_decoder.py:6-49), as called
 * from PPASRPredictor.decode (predict.py:128) and PPASRTrainer.__decoder_result (trainer.py:351).
 *   probs [B,Tp,V] f32 (any row-normalised or not: argmax + value at argmax)
 *   frame_lens [B] i32 or NULL (NULL = decode all Tp rows, the reference's batch behaviour)
 *   tokens [B,Tp] i32 (-1 padded), n_tokens [B] i32, score [B] f64 (mean non-blank max prob * 100) */
PPASR_API ppasr_status ppasr_ctc_greedy(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank,
                              int32_t* tokens, int32_t* n_tokens, double* score,
                              void* workspace /* >= 8*B*Tp bytes */, size_t workspace_bytes, void* stream);

/* Second stage only: collapse repeats / drop blank / score, from per-frame argmax+maxprob
 * (the outputs of ppasr_encode).  Same outputs as ppasr_ctc_greedy. */
PPASR_API ppasr_status ppasr_ctc_collapse(const int32_t* frame_argmax, const float* frame_maxprob, const int32_t* frame_lens,
                                int B, int Tp, int blank, int32_t* tokens, int32_t* n_tokens, double* score,
                                void* stream);

/* ---- multi-session streaming (no reference counterpart: PPASR streams one session per call) -----------------------
 * A group of Conformer (fused or general route, ppasr_gen_stream_group_create), Squeezeformer or Efficient-Conformer
 * sessions whose K/V and conv caches live in one allocation
 * (DeepSpeech2 groups: the sessions' recurrent states, ppasr_ds2_stream_group_create);
 * ppasr_encode_chunk_group advances any subset of them by one chunk with ONE set of launches (rows of all listed sessions
 * stacked).  Every session
 * follows the single-session arithmetic of ppasr_encode_chunk with required_cache_size < 0 (full history, what
 * PPASRPredictor.predict_stream passes, predict.py:306-307).  max_frames caps the per-session cache (<= max_len).
 *   sessions_host [n] distinct slot indices; feats [n][T][F]; outputs by list position: probs [n][c][V] or NULL,
 *   frame_argmax / frame_maxprob [n][c] or NULL. */
typedef struct ppasr_stream_group_s* ppasr_stream_group;
PPASR_API ppasr_status ppasr_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out);
/* The same kind of group for a streaming (causal) Squeezeformer handle on the conv2d front end and the fused 256-wide
 * route (conv kernel 31 or 15); PPASR_EUNSUPPORTED for any other handle.  ppasr_stream_group_create stays Conformer-only.
 * Each session keeps its full-rate and half-rate caches (the reference's trim of the reduced cache, as on a stream
 * handle) and ppasr_encode_chunk_group refuses, with PPASR_EINVAL and no session changed, a round in which any listed
 * session would leave an odd cache length or exceed max_len / max_frames.  The other group calls take it unchanged. */
PPASR_API ppasr_status ppasr_sq_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out);
/* The same kind of group for a streaming (causal) Efficient-Conformer handle on the conv2d front end and the fused
 * 256-wide route with at most one stride layer (grouped-attention layers of group size 2 / 3 / 4 included): what
 * ppasr_stream_create runs on that route.  PPASR_EUNSUPPORTED for any other handle (several stride layers, the general
 * route, the 6x / 8x front ends, non-causal models); ppasr_stream_group_create and ppasr_sq_stream_group_create refuse
 * Efficient-Conformer handles.  Each session keeps its full-rate and half-rate caches and its offset; a round emits
 * ppasr_out_frames(h, T) frames per session, and ppasr_encode_chunk_group refuses, with PPASR_EINVAL and no session
 * changed, a round in which any listed session would leave an odd cache length or exceed max_len / max_frames. */
PPASR_API ppasr_status ppasr_eff_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out);
/* The same kind of group for a streaming (causal = 1, unidirectional) DeepSpeech2 handle, LSTM or GRU, rnn_size 1024 or
 * 2048.  Each session keeps its recurrent state on the device -- h [L][H], and c [L][H] for the LSTM (a GRU has none: the
 * reference hands its c box through unchanged) -- and its output-frame offset; max_frames is accepted and ignored (the
 * state does not grow with the stream).  PPASR_EUNSUPPORTED for a bidirectional handle (the reference streams no such
 * model) and any other model type; the three create calls above refuse DeepSpeech2 handles.  A round is what
 * ppasr_ds2_encode computes for the n stacked windows with every length T and those sessions' states as the h / c boxes
 * (the (layer, time) wavefront route whatever n, bit for bit, with no stream synchronisation; the launches do not depend
 * on n except for the CTC head's K-split join, which ppasr_ds2_encode adds up to 512 stacked frames), c =
 * ((T-1)/2-1)/2 frames per session; the states move between the sessions' slots and the recurrence by one launch each way.
 * ppasr_stream_group_reset zeroes a session's state and offset.  ppasr_group_chunk_workspace_bytes(h, n, T) gives the
 * round's workspace for such a handle. */
PPASR_API ppasr_status ppasr_ds2_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out);
/* The same kind of group for a streaming (causal) Conformer handle on the general layer route with the conv2d front end:
 * output_size 512 / 768 / 1024, or any of the ConformerEncoder options that route streams (abs_pos / no_pos,
 * normalize_before = False, concat_after, macaron_style = False, use_cnn_module = False, any activation, any causal
 * cnn_module_kernel).  Each session keeps K / V caches [L][cap][D] (cap = max_frames, or max_len), its conv-module input
 * history [L][cnn_module_kernel - 1][D] (none without a conv module), its cache length and offset.  A round runs the
 * general route's pieces once over the n stacked chunks; per-session kernels append the keys / values, assemble each
 * session's [history | chunk] conv input, move the histories on and, with abs_pos, add each session's positional rows.
 * ppasr_encode_chunk_group refuses, with PPASR_EINVAL and no session changed, a round in which any listed session would
 * exceed max_len / max_frames.  PPASR_EUNSUPPORTED for every other handle (the fused 256-wide route, Squeezeformer /
 * Efficient-Conformer, the 6x / 8x and linear front ends, non-causal models, DeepSpeech2); the four create calls above
 * keep refusing general-route handles. */
PPASR_API ppasr_status ppasr_gen_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out);
PPASR_API ppasr_status ppasr_stream_group_destroy(ppasr_stream_group g);
PPASR_API ppasr_status ppasr_stream_group_reset(ppasr_stream_group g, int session /* < 0: all */, void* stream);
PPASR_API int          ppasr_stream_group_offset(ppasr_stream_group g, int session);
PPASR_API size_t       ppasr_group_chunk_workspace_bytes(ppasr_handle h, int n, int T);
PPASR_API ppasr_status ppasr_encode_chunk_group(ppasr_stream_group g, const int* sessions_host, int n, const float* feats, int T,
                                      float* probs, int32_t* frame_argmax, float* frame_maxprob, int* c_out_host,
                                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- beam-search session pools (no reference counterpart as a pool) ---------------------------------------------
 * Replaces N x CtcBeamSearchDecoderBatch.next() + decode() (swig_wrapper.py:106-121, beam_search_decoder.py:75-96: one
 * streaming decoder object per session) for a server that decodes many streams: n_sessions independent streaming CTC
 * prefix beam searches with one configuration (V, beam_size, cutoff_prob / cutoff_top_n, blank, optional scorer with
 * alpha / beta; lm must outlive the pool).  ppasr_beam_pool_decode advances any subset of the sessions by one chunk with
 * ONE pruning launch and ONE search launch; each listed session's result is the one its own
 * ppasr_ctc_beam_search_ws(init_state = 1, then 0, ...) sequence on the same chunks gives.  Refused configurations
 * (vocabulary, beam, LDS fit): the codes of ppasr_ctc_beam_search_ws, at create.
 * The pool owns its device memory: each session a state block sized for its own frame capacity, init_frames at first.
 * A call whose chunk would take a session past its capacity first moves that session's block into one twice the size
 * (doubling until it fits; the other sessions' blocks are not touched) and SYNCHRONISES `stream` once before freeing the
 * replaced blocks.  Calls on one pool are serialised on one stream. */
typedef struct ppasr_beam_pool_s* ppasr_beam_pool;
PPASR_API ppasr_status ppasr_beam_pool_create(int n_sessions, int V, int beam_size, double cutoff_prob, int cutoff_top_n,
                                              int blank, ppasr_lm_handle lm /* or NULL */, double alpha, double beta,
                                              int init_frames, ppasr_beam_pool* out);
PPASR_API ppasr_status ppasr_beam_pool_destroy(ppasr_beam_pool pool);
/* A new search for one session (session < 0: all): one small launch per session on `stream`. */
PPASR_API ppasr_status ppasr_beam_pool_reset(ppasr_beam_pool pool, int session, void* stream);
/* Cumulative frames a session decoded since its last reset; its current frame capacity (-1: bad argument). */
PPASR_API long long    ppasr_beam_pool_frames(ppasr_beam_pool pool, int session);
PPASR_API long long    ppasr_beam_pool_capacity(ppasr_beam_pool pool, int session);
/* Reads back the n_sessions status words (non-zero: a prefix arena ran out -- growth is planned so that it does not);
 * PPASR_ENOSPACE if any is set.  Synchronises `stream`. */
PPASR_API ppasr_status ppasr_beam_pool_status(ppasr_beam_pool pool, int32_t* status_host, void* stream);
/* Device workspace of a call listing n sessions with chunks of T frames: the pruning records and, for cutoff_prob >= 1
 * or element lists that do not fit LDS, the search's scratch (ppasr_ctc_beam_scratch_bytes).  May be 0. */
PPASR_API size_t       ppasr_beam_pool_workspace_bytes(ppasr_beam_pool pool, int n, int T);
/* sessions_host [n] distinct indices; probs device [n][T][V] f32; frame_lens_host [n] in [0, T] or NULL (all T).  Outputs
 * by list position, the n-best = 1 hypothesis: tokens [n][max_tokens] (-1 padded), lens [n], scores [n] f64 = -log P
 * (approx_ctc with a scorer).  Every argument is checked before any device work; a refused call (PPASR_EINVAL,
 * PPASR_ENOSPACE) changes no session. */
PPASR_API ppasr_status ppasr_beam_pool_decode(ppasr_beam_pool pool, const int* sessions_host, int n, const float* probs, int T,
                                              const int32_t* frame_lens_host, int max_tokens, int32_t* tokens, int32_t* lens,
                                              double* scores, void* workspace, size_t workspace_bytes, void* stream);
/* The nbest best prefixes of each listed session's CURRENT beam: tokens [n][nbest][max_tokens] (-1 padded), lens
 * [n][nbest] (-1: the beam holds fewer hypotheses), scores [n][nbest] f64 = -log P -- the conventions of
 * ppasr_ctc_beam_search.  It is ppasr_beam_pool_decode with T = 0: one search launch that finalizes and consumes no frame,
 * so no session is advanced, grown or compacted and every state block keeps its bits (workspace:
 * ppasr_beam_pool_workspace_bytes(pool, n, 0)).  PPASR_EINVAL: nbest outside [1, beam_size], and what decode refuses. */
PPASR_API ppasr_status ppasr_beam_sessions_nbest(ppasr_beam_pool pool, const int* sessions_host, int n, int nbest, int max_tokens,
                                             int32_t* tokens, int32_t* lens, double* scores, void* workspace,
                                             size_t workspace_bytes, void* stream);

/* ---- compaction of a pool's prefix arenas: long streams in bounded memory --------------------------------------
 * A session's arena otherwise keeps every prefix node it ever created (36 bytes per node, beam_size nodes per frame) and
 * its block doubles whenever its stream does.  ppasr_beam_arena_compact rewrites the listed sessions' blocks in place with
 * ONE launch (ppasr_ctc_beam_state_compact's rule; the node table of word-based scorers is rebuilt, with the semantic note
 * given there), reads the live node counts back (live_nodes_host [n] by list position, or NULL; -1: exhausted, left
 * untouched), synchronises `stream` once and lowers each session's arena use to ceil((L - 1) / beam_size) frame-equivalents;
 * ppasr_beam_pool_frames stays cumulative.  n < 0 or a NULL list: every session.  Results of later decodes do not change.
 * ppasr_beam_arena_set_auto(pool, 1): ppasr_beam_pool_decode compacts every listed session whose chunk does not fit its
 * block (one launch for all of them) before it plans growth; such a session keeps its block if at least half of it is
 * free behind the chunk and otherwise grows by doubling until that holds.  Default 0: the pool behaves as without these
 * calls.  Capacity never shrinks.  Every argument is checked before any device work; a refused call (PPASR_EINVAL: null
 * pool, index out of range or repeated) changes nothing. */
PPASR_API ppasr_status ppasr_beam_arena_compact(ppasr_beam_pool pool, const int* sessions_host, int n, long long* live_nodes_host,
                                                void* stream);
PPASR_API ppasr_status ppasr_beam_arena_set_auto(ppasr_beam_pool pool, int enable);
/* Node count read back at the session's last compaction (0: none since its reset; -1: bad argument). */
PPASR_API long long    ppasr_beam_arena_live_nodes(ppasr_beam_pool pool, int session);
/* Device bytes of all state blocks now. */
PPASR_API size_t       ppasr_beam_arena_bytes(ppasr_beam_pool pool);

/* ---- Kaldi-compatible fbank front-end --------------------------------------------
 * Replaces AudioFeaturizer.featurize (ppasr/data_utils/featurizer/audio_featurizer.py:37-67,120-138):
 * AudioSegment.normalize(target_dB) (data_utils/audio.py:287-304) -> .to('int16') (audio.py:244) ->
 * paddleaudio.compliance.kaldi.fbank(n_mels, frame_length=25, frame_shift=10, dither=0, sr) (third-party,
 * paddleaudio>=1.0.1).  samples: device f32 mono in [-1,1]; feats: device f32 [frames][n_mels]. */
typedef struct ppasr_fbank_s* ppasr_fbank_handle;
PPASR_API ppasr_status ppasr_fbank_create(int sample_rate, int n_mels, float frame_length_ms, float frame_shift_ms,
                                ppasr_fbank_handle* out);
PPASR_API ppasr_status ppasr_fbank_destroy(ppasr_fbank_handle f);
PPASR_API int          ppasr_fbank_frames(ppasr_fbank_handle f, int n_samples);          /* snip_edges frame count */
/* (workspace: one float per 8192-sample chunk of the mean square -- summed in numpy's order, see csrc/fbank.hip -- + the gain
 *  + the gain in dB (ws[chunks], ws[chunks + 1]: the host mirror raises ValueError beyond 300 dB like audio.py:301); never less
 *  than 8 KiB) */
PPASR_API size_t       ppasr_fbank_workspace_bytes(ppasr_fbank_handle f, int n_samples);
PPASR_API ppasr_status ppasr_fbank_compute(ppasr_fbank_handle f, const float* samples, int n_samples, int use_db_norm,
                                 float target_db, float* feats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- batch form: n independent waveforms ("segments") packed back to back in one device buffer, featurized by one set of
 * launches (three with dB normalisation, one without, whatever n is).  Every segment's features, chunk sums and gain
 * equal those of a call of its own, byte for byte.  One table entry per segment: */
typedef struct {
  long long first_sample; /* index of the segment's first sample in `samples` */
  long long out_row;      /* row of `feats` that takes the segment's first frame; frame j goes to out_row + j */
  int n_samples;          /* 0 and counts below one window are legal: no frame */
  int first_chunk;        /* the segment's first 8192-sample chunk in the workspace's chunk sums */
  int first_frame;        /* the segment's first frame in the compact numbering 0 .. total_frames - 1 */
  int reserved;
} ppasr_fbank_segment;
/* Host only, no device and no handle: fills table[0 .. n) for segments of n_samples[b] samples in the order given.
 * t_max == 0: compact rows (out_row = first_frame, feats is [total_frames][n_mels]); t_max > 0: out_row = b * t_max
 * (feats is [n][t_max][n_mels]; the rows past a segment's frames are not written).  PPASR_EINVAL: a negative count, a
 * t_max below the longest segment's frame count, more than 2^31 - 1 chunks or frames. */
PPASR_API ppasr_status ppasr_fbank_plan_batch(int sample_rate, float frame_length_ms, float frame_shift_ms, const int* n_samples,
                                    int n, int t_max, ppasr_fbank_segment* table, int* total_chunks, int* total_frames);
/* (workspace: total_chunks floats, the chunk sums, then {gain, gain in dB} per segment for the caller to read) */
PPASR_API size_t       ppasr_fbank_batch_workspace_bytes(int n, int total_chunks);
/* Asynchronous on `stream`.  samples, table_dev (a device copy of the planned table), feats, workspace: device memory.
 * PPASR_ENOSPACE: workspace too small; PPASR_EINVAL: a null argument. */
PPASR_API ppasr_status ppasr_fbank_compute_batch(ppasr_fbank_handle f, const float* samples, const ppasr_fbank_segment* table_dev,
                                       int n, int total_chunks, int total_frames, int use_db_norm, float target_db,
                                       float* feats, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MFCC form of the same front-end (`preprocess_conf.feature_method: mfcc`, audio_featurizer.py:55-61,140-154) ----
 * paddleaudio.compliance.kaldi.mfcc(n_mels, n_mfcc, frame_length=25, frame_shift=10, dither=0, sr) with its other
 * arguments at their defaults (use_energy False, subtract_mean False, cepstral_lifter 22): the log-mel stage above, then
 *   mfcc[t][k] = L[k] * sum_m logmel[t][m] * D[m][k],   D[m][0] = sqrt(1/M),  D[m][k] = sqrt(2/M) cos(pi/M (m + 1/2) k),
 *   L[k] = 1 + (Q/2) sin(pi k / Q)  (1 when Q == 0),    M = n_mels, Q = cepstral_lifter,
 * one extra contraction per frame inside the frame kernel: no further launch.  The handle is a ppasr_fbank_handle: every
 * ppasr_fbank_* call above takes it, and wherever those say "[n_mels]" for a row of `feats` its rows are n_mfcc floats.
 * Third-party and not installable offline like the fbank: parity unpinned.
 * PPASR_EINVAL: n_mfcc < 1, n_mfcc > n_mels, cepstral_lifter < 0 (or not finite), whatever ppasr_fbank_create refuses. */
PPASR_API ppasr_status ppasr_mfcc_create(int sample_rate, int n_mels, int n_mfcc, float frame_length_ms, float frame_shift_ms,
                               float cepstral_lifter, ppasr_fbank_handle* out);
/* Floats per row of `feats`: n_mels for a handle of ppasr_fbank_create, n_mfcc for one of ppasr_mfcc_create, 0 for NULL. */
PPASR_API int          ppasr_fbank_feature_dim(ppasr_fbank_handle f);
/* Host only, no device: the very tables ppasr_mfcc_create uploads -- dct [n_mels][n_mfcc] = D, lifter [n_mfcc] = L --
 * computed in double and rounded to float once.  Same refusals as ppasr_mfcc_create, and PPASR_EINVAL for a null pointer. */
PPASR_API ppasr_status ppasr_mfcc_tables(int n_mels, int n_mfcc, float cepstral_lifter, float* dct, float* lifter);

/* ---- Polyphase FIR resampler: audio at any other rate -> the model's rate, in front of the fbank front-end -------------
 * AudioSegment.resample (data_utils/audio.py:306-317; audio_featurizer.py:46-47 calls it first).  The reference uses
 * resampy's 'kaiser_best', which is not installable offline; this is the filter the host route of
 * data_utils/featurizer.py::resample has always used, scipy.signal.resample_poly(x, up, down, window=("kaiser",
 * 14.769656459379492)): parity with resampy unpinned, like the host route.
 *   g = gcd(in_rate, out_rate), up = out_rate / g, down = in_rate / g, half_len = 10 max(up, down), L = 2 half_len + 1,
 *   h = up * firwin(L, 1 / max(up, down), kaiser beta),  n_pre_pad = down - half_len % down,
 *   n_pre_remove = (half_len + n_pre_pad) / down,  hp = [0] * n_pre_pad + h,
 *   y[m] = sum_i hp[(m + n_pre_remove) down - i up] x[i],  0 <= m < out_len = ceil(n_in up / down),  x = 0 outside the stream.
 * Stored by phase: with k = (m + n_pre_remove) down, q(m) = k / up, p = k % up,  y[m] = sum_t table[p][t] x[q(m) - t] over
 * t = 0 .. T - 1, table[p][t] = hp[p + t up] (exactly 0 past hp's end), T = taps_per_phase = ceil((L + n_pre_pad) / up):
 * 21 / 21 / 29 / 32 / 43 / 58 / 64 taps for 8 k / 11.025 k / 22.05 k / 24 k / 32 k / 44.1 k / 48 k -> 16 k.  The table is
 * computed in double and rounded to float once.
 * Accumulation (the contract): every output is ONE fp32 accumulator that starts at 0 and takes its T taps in ascending t with
 * fmaf; a sample outside the stream or outside the window a call was given enters as 0.  The result depends on the output's
 * absolute index and the samples alone -- not on the call, the segment, in_first or where a packet boundary fell -- so whole
 * utterances, packed batches and packet-by-packet streams give the same bytes.  Inputs are assumed finite (0 * inf is NaN).
 * PPASR_EINVAL: a rate <= 0, equal rates (nothing to do), a null pointer, a position or count outside 0 .. 2^40;
 * PPASR_EUNSUPPORTED: max(up, down) > 1024 (every standard rate to or from 8 k / 16 k lies inside).  A refused call writes
 * nothing.  There is no host fallback. */
#define PPASR_RESAMPLE_TILE 256                     /* outputs per workgroup */
#define PPASR_RESAMPLE_MAX_SAMPLES (1LL << 40)      /* largest stream position / count a call takes */
typedef struct ppasr_resampler_s* ppasr_resampler_handle;
/* Host only, no device and no handle. */
PPASR_API ppasr_status ppasr_resampler_geometry(int in_rate, int out_rate, int* up, int* down, int* taps_per_phase, int* n_pre_pad,
                                                int* n_pre_remove);
/* table [up][taps_per_phase]: the very table ppasr_resampler_create uploads */
PPASR_API ppasr_status ppasr_resampler_table(int in_rate, int out_rate, float* table);
/* The three below return -1 (and set ppasr_last_error) for what they refuse.
 * out_len: ceil(n_in up / down).
 * ready: how many leading outputs have q(m) < n_in_total, i.e. read no sample past the first n_in_total of the stream
 *        (= max(0, out_len(n_in_total) - n_pre_remove)): what a stream can emit so far.
 * first_needed: max(0, q(m) - (T - 1)), the lowest sample index output m reads: the tail a stream keeps for output m on. */
PPASR_API long long    ppasr_resampler_out_len(int in_rate, int out_rate, long long n_in);
PPASR_API long long    ppasr_resampler_ready(int in_rate, int out_rate, long long n_in_total);
PPASR_API long long    ppasr_resampler_first_needed(int in_rate, int out_rate, long long m);
/* Uploads the table to the current device. */
PPASR_API ppasr_status ppasr_resampler_create(int in_rate, int out_rate, ppasr_resampler_handle* out);
PPASR_API ppasr_status ppasr_resampler_destroy(ppasr_resampler_handle r);
/* One call for every use; asynchronous on `stream`; in, out: device f32.  `in` holds the stream's samples with absolute
 * indices in_first .. in_first + n_in - 1 (everything outside is zero); the call writes out[0 .. n_out), the outputs with
 * absolute indices out_first .. out_first + n_out - 1, and nothing else.  A whole waveform: in_first = out_first = 0, n_out =
 * out_len.  A stream packet: the kept tail + the new samples, out_first = the outputs emitted so far.  n_in == 0 and
 * n_out == 0 are legal (then the buffer may be null). */
PPASR_API ppasr_status ppasr_resample_compute(ppasr_resampler_handle r, const float* in, long long in_first, long long n_in,
                                              float* out, long long out_first, long long n_out, void* stream);
/* Batch form: n independent windows ("segments") of any streams, ONE launch whatever n is (n <= 65535).  Segment s reads
 * in[in_offset ..] and writes out[out_offset .. out_offset + n_out) as a ppasr_resample_compute call of its own would, byte
 * for byte.  segments_dev: a device copy of the table; its entries are the caller's to keep inside the buffers.  max_n_out:
 * the largest n_out in the table (it sizes the grid; outputs past it are not computed). */
typedef struct {
  long long in_offset;  /* index in `in` of the segment's first held sample */
  long long in_first;   /* absolute stream index of that sample */
  long long n_in;
  long long out_offset; /* index in `out` of the segment's first output */
  long long out_first;  /* absolute index of that output */
  long long n_out;
} ppasr_resample_segment;
PPASR_API ppasr_status ppasr_resample_compute_batch(ppasr_resampler_handle r, const float* in,
                                                    const ppasr_resample_segment* segments_dev, int n, long long max_n_out,
                                                    float* out, void* stream);

/* ---- attention rescoring of CTC n-best lists with the checkpoint's attention decoder ----
 * The reference trains a BiTransformerDecoder with every Conformer-family model (conformer/model.py:48,
 * transformer/decoder.py) and never calls it at inference; the use defined here is WeNet's `attention_rescoring`:
 * score every hypothesis of the CTC prefix beam search with the left (and right) decoder over the encoder output and add
 * the CTC score.
 *
 * Encoder output.  While `memory_dev` is set (host call; NULL clears), every offline ppasr_encode on the handle also
 * writes memory [B,T',D] f32 = the first return value of the reference's encoder(xs, lens, -1, -1): behind after_norm
 * (Conformer, Efficient-Conformer), the last layer's output (Squeezeformer).  n_floats: capacity of the buffer; a call
 * that needs more returns PPASR_ENOSPACE.  The route and every other output are unchanged, bit for bit.  With
 * ppasr_set_skip_padding, rows behind an utterance's valid frames are 0.  Streaming calls do not write it.
 * PPASR_EUNSUPPORTED on DeepSpeech2 handles and on a Squeezeformer with final_proj (folded into the CTC head). */
PPASR_API ppasr_status ppasr_set_memory_out(ppasr_handle h, float* memory_dev, size_t n_floats);

typedef struct ppasr_rescorer_s* ppasr_rescorer;
/* decoder_conf of the reference's YAML + the model's vocabulary.  Built for d_model 256 with 4 heads, linear_units a
 * multiple of 256 up to 4096, num_blocks 1..6, r_num_blocks 0..6, vocab_size >= 2, normalize_before = True and
 * concat_after = False (the constructor defaults, the only ones the reference's configurations use); anything else is
 * PPASR_EUNSUPPORTED. */
typedef struct {
  int vocab_size;
  int d_model;
  int attention_heads;
  int linear_units;
  int num_blocks;
  int r_num_blocks;
  int max_len;          /* positional table length, 0 = 5000 */
} ppasr_rescorer_desc;
/* Weights by the reference's names: decoder.{left,right}_decoder.{embed.0.weight, after_norm.*, output_layer.*,
 * decoders.N.{self_attn,src_attn}.linear_{q,k,v,out}.*, decoders.N.feed_forward.w_{1,2}.*, decoders.N.norm{1,2,3}.*}; a
 * missing one is PPASR_EMISSING with its name in ppasr_last_error(). */
PPASR_API ppasr_status ppasr_rescorer_create(const ppasr_rescorer_desc* desc, const ppasr_weight_blob* weights_host,
                                             int n_weights, ppasr_rescorer* out);
PPASR_API ppasr_status ppasr_rescorer_destroy(ppasr_rescorer r);
PPASR_API size_t ppasr_rescorer_workspace_bytes(ppasr_rescorer r, int B, int Tp, int nbest, int max_tokens);
/* One call, asynchronous on `stream`, no read-back: the decoders run over one packed row per (utterance, hypothesis,
 * direction, position) that exists (a device-side row table made from `lens`).
 *   memory [B,Tp,D] f32; out_lens [B] i32 valid memory frames (NULL: all Tp; cross-attention sees t < out_lens[b] only)
 *   tokens [B,nbest,max_tokens] i32, lens [B,nbest] i32 (-1: no such hypothesis), ctc_scores [B,nbest] f64 (-log P):
 *     the three outputs of ppasr_ctc_beam_search as they are.  Out-of-range values are clamped, not refused: a lens
 *     entry above max_tokens counts as max_tokens, and a token id outside [0, V - 1] inside a hypothesis as 0 or V - 1.
 *   sos = eos = V - 1.  att = sum_j logp_left[j][y_j] + logp_left[n][eos] over the input [sos, y0 .. y(n-1)]; r_att the
 *   same over the reversed tokens with the right decoder; total = (1 - reverse_weight) att + reverse_weight r_att +
 *   ctc_weight (-ctc_scores).
 *   att_scores, r_att_scores, total_scores [B,nbest] f64 (absent hypothesis: total = -inf; r_att = 0 when
 *     reverse_weight == 0, and then the right decoder does not run); best [B] i32: the largest total, lowest index on a tie
 *   token_logp [B,nbest,2,max_tokens+1] f32 or NULL: the summed log-probabilities (0: left, 1: right; 0.0 where no row)
 *   logits_tap [B,nbest,2,max_tokens+1,V] f32 or NULL: the decoders' pre-softmax outputs (parity tests; 0.0 where no row)
 * Refused before any device work: reverse_weight > 0 on a rescorer without right blocks (PPASR_EINVAL); max_tokens + 1
 * above max_len or above 256 rows per hypothesis (PPASR_EUNSUPPORTED); a workspace below
 * ppasr_rescorer_workspace_bytes (PPASR_ENOSPACE). */
PPASR_API ppasr_status ppasr_rescore(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp,
                                     const int32_t* tokens, const int32_t* lens, const double* ctc_scores, int nbest,
                                     int max_tokens, double ctc_weight, double reverse_weight, double* att_scores,
                                     double* r_att_scores, double* total_scores, int32_t* best, float* token_logp,
                                     float* logits_tap, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CTC forced alignment: when each token of a transcript was spoken (no reference counterpart) ----
 * The Viterbi path of tokens[b, 0..n_tokens[b]) through the CTC trellis of probs[b], and per token its frames and its
 * confidence.  The transcript may be a decoder's own output (greedy, beam search, rescoring) or the caller's.  The
 * trellis, the clamp of the emissions, the tie rule and the feasibility rule are defined once, in the header comment of
 * csrc/ctc_align.hip.  One call, asynchronous on `stream`, no read-back; every pointer is a device pointer.
 *   probs [B,Tp,V] f32 (the head's softmax output); frame_lens [B] i32 or NULL (all Tp rows; clamped to [0, Tp])
 *   tokens [B,max_tokens] i32 (only the first n_tokens[b] of a row are read), n_tokens [B] i32; max_tokens <= 255
 *   frame_token [B,Tp] i32: the index l of the token the path emits at that frame, -1 on blank frames and for t >= frame_lens
 *   begin, end [B,max_tokens] i32 or NULL: first frame of token l, one past its last; peak [B,max_tokens] i32 and
 *   conf [B,max_tokens] f32 or NULL: the largest probs[b, t, tokens[b, l]] over begin <= t < end, copied from the table,
 *   and the first frame that attains it.  Entries l >= n_tokens[b] are -1 (conf: 0.0).
 *   score [B] f32: the path's log-probability (fp32, one add per frame); status [B] i32:
 *     0 aligned; 1 infeasible (frame_lens < n_tokens + adjacent repeats); 2 bad input (n_tokens outside [0, max_tokens], a
 *     token id outside [0, V) or equal to blank).  Status 1 and 2 are results, not errors: score -inf, every entry -1.
 * Refused before any launch: a NULL required pointer, B <= 0, Tp < 0, V < 2, blank outside [0, V), max_tokens < 0, a
 * workspace below ppasr_ctc_align_workspace_bytes or not 16-byte aligned (PPASR_EINVAL); max_tokens > 255
 * (PPASR_EUNSUPPORTED).  Tp = 0 is a valid call that writes status and score only.  tokens may be NULL when max_tokens
 * is 0, probs and frame_token when Tp is 0. */
PPASR_API size_t ppasr_ctc_align_workspace_bytes(int B, int Tp, int max_tokens);
PPASR_API ppasr_status ppasr_ctc_align(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank,
                                       const int32_t* tokens, const int32_t* n_tokens, int max_tokens, int32_t* frame_token,
                                       int32_t* begin, int32_t* end, int32_t* peak, float* conf, float* score,
                                       int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* ---- probability arena: the CTC tables of many streaming sessions, kept on the device so that a stream can be aligned ----
 * A stream's table arrives one chunk per round.  The arena keeps the rows of every session in pages of page_frames rows
 * inside one slab [n_pages][page_frames][V] f32 that is allocated once; the page list of every session and the free list
 * live on the host.  ALL CALLS ON ONE ARENA GO ON ONE STREAM: reset and append are ordered against the launches that still
 * read a page only by that stream's order.  The calls are not thread-safe.
 *   create: n_sessions >= 1, V >= 2, page_frames >= 1, n_pages >= 1, the slab below 2^40 bytes (PPASR_EINVAL otherwise,
 *     checked before any device call).
 *   append: rows 0 .. frames_host[k] - 1 (NULL: all c) of probs_dev[k] ([n][c][V], device) go behind the last frame of
 *     session sessions_host[k].  One kernel launch for all n sessions, plus one asynchronous upload of the call's table
 *     from pinned memory; nothing is read back and the host does not wait for the device (the upload slots are a ring of
 *     8: the ninth call waits for the first one's launch).  All or nothing: a call that needs more pages than are free
 *     returns PPASR_ENOSPACE and changes no session, frame count or free page.  PPASR_EINVAL: n < 1, a session outside
 *     [0, n_sessions) or listed twice, c < 0, a frames_host[k] outside [0, c], a NULL list or table.
 *   reset: the session's (session < 0: every session's) pages go back to the free list; host bookkeeping only.
 *   frames / free_pages: frames held for the session / pages not in use (-1 for a bad argument).
 *   read: dense_dev [frames][V] = the session's table, one launch.
 *   ppasr_ctc_align_arena: ppasr_ctc_align with B = n, Tp = the longest listed session and every session's own frame
 *     count as its frame_lens; the emissions are read through the page lists, the chain and the workspace layout are
 *     ppasr_ctc_align's, and every output equals, bit for bit, ppasr_ctc_align on the dense tables of the same sessions
 *     (frame_token [n][Tp]).  tokens, n_tokens and the outputs are device pointers; sessions_host is a host list.
 *     ppasr_ctc_align_arena_workspace_bytes(n, Tp, max_tokens) = ppasr_ctc_align_workspace_bytes.  Refusals: a session
 *     outside the arena or listed twice, n < 1, blank outside [0, V), a NULL required pointer, a workspace that is not
 *     16-byte aligned (PPASR_EINVAL); max_tokens > 255, n * Tp > 2^26 (PPASR_EUNSUPPORTED; an append: n * c > 2^30); a workspace below
 *     ppasr_ctc_align_arena_workspace_bytes (PPASR_ENOSPACE).  A refused call leaves the arena as it was. */
typedef struct ppasr_prob_arena_s* ppasr_prob_arena;
PPASR_API ppasr_status ppasr_prob_arena_create(int n_sessions, int V, int page_frames, int n_pages, ppasr_prob_arena* out);
PPASR_API ppasr_status ppasr_prob_arena_destroy(ppasr_prob_arena arena);
PPASR_API ppasr_status ppasr_prob_arena_append(ppasr_prob_arena arena, const int* sessions_host, int n, const float* probs_dev,
                                               int c, const int* frames_host, void* stream);
PPASR_API ppasr_status ppasr_prob_arena_reset(ppasr_prob_arena arena, int session);
PPASR_API long long    ppasr_prob_arena_frames(ppasr_prob_arena arena, int session);
PPASR_API long long    ppasr_prob_arena_free_pages(ppasr_prob_arena arena);
PPASR_API ppasr_status ppasr_prob_arena_read(ppasr_prob_arena arena, int session, float* dense_dev, void* stream);
/* read_many: dense_dev [n][Tp][V] = the listed sessions' rows, zeros at and behind each session's frame count, and
 *   lens_dev [n] i32 = the counts: ONE launch, nothing read back.  Each session's rows equal ppasr_prob_arena_read byte for
 *   byte.  PPASR_EINVAL: Tp below the longest listed session, a session outside the arena or listed twice, n < 1, a NULL
 *   pointer (dense_dev may be NULL when Tp = 0); PPASR_EUNSUPPORTED: n * Tp > 2^30. */
PPASR_API ppasr_status ppasr_prob_arena_read_many(ppasr_prob_arena arena, const int* sessions_host, int n, int Tp,
                                                  float* dense_dev, int32_t* lens_dev, void* stream);
/* ---- encoder memory of streaming rounds, for attention rescoring at end of stream ----
 * The arena is a row store of any width >= 2: created with V = 256 it keeps the ENCODER OUTPUT of streams (what
 * ppasr_set_memory_out gives for an offline encode: encoder.after_norm of the rows the CTC head reads).
 * ppasr_encode_chunk_group_mem is ppasr_encode_chunk_group plus (mem, mem_frames_host): rows 0 .. mem_frames_host[k] - 1
 * (NULL: all c; 0: nothing is kept for that session) of list position k's c frames go behind the last frame arena
 * session sessions_host[k] holds.  With mem = NULL it IS ppasr_encode_chunk_group, launch for launch; with an arena the
 * round ends with ONE more kernel launch, whatever n is, and every other output is the same bits.  Arena and group calls
 * go on one stream (the arena's rule).  All or nothing: the pages are planned and every argument is checked before any
 * device work of the round; a refused round changes no session of the group and nothing in the arena.
 *   PPASR_ENOSPACE: the round needs more pages than are free.
 *   PPASR_EINVAL: arena rows not 256 wide; an arena with fewer sessions than the group; a mem_frames_host entry outside
 *     [0, c]; whatever ppasr_encode_chunk_group refuses.
 *   PPASR_EUNSUPPORTED: every group but the Conformer's on the fused 256-wide route -- DeepSpeech2, the general route,
 *     Squeezeformer and Efficient-Conformer groups.
 * ppasr_encode_chunk_mem: the same for one stream handle (ppasr_encode_chunk plus the arena, the session that takes the
 * rows and mem_frames in [0, c], < 0: all c); Conformer handles on the fused route, PPASR_EUNSUPPORTED otherwise. */
PPASR_API ppasr_status ppasr_encode_chunk_group_mem(ppasr_stream_group g, const int* sessions_host, int n, const float* feats,
                                                    int T, float* probs, int32_t* frame_argmax, float* frame_maxprob,
                                                    int* c_out_host, void* workspace, size_t workspace_bytes,
                                                    ppasr_prob_arena mem, const int* mem_frames_host, void* stream);
PPASR_API ppasr_status ppasr_encode_chunk_mem(ppasr_stream s, const float* feats, int T, int required_cache_size, float* probs,
                                              int32_t* frame_argmax, float* frame_maxprob, int* c_out_host, void* workspace,
                                              size_t workspace_bytes, ppasr_prob_arena mem, int session, int mem_frames,
                                              void* stream);
PPASR_API size_t ppasr_ctc_align_arena_workspace_bytes(int n, int Tp, int max_tokens);
PPASR_API ppasr_status ppasr_ctc_align_arena(ppasr_prob_arena arena, const int* sessions_host, int n, int blank,
                                             const int32_t* tokens, const int32_t* n_tokens, int max_tokens,
                                             int32_t* frame_token, int32_t* begin, int32_t* end, int32_t* peak, float* conf,
                                             float* score, int32_t* status, void* workspace, size_t workspace_bytes,
                                             void* stream);

/* ---- the loss half of evaluation: CTC and attention losses, forward only (the reference's ConformerModel.forward) ----
 * CTC negative log-likelihood: nll[b] = -log P_ctc(tokens[b] | probs[b]), the sum over every alignment where
 * ppasr_ctc_align takes the best one.  Inputs, trellis, emission clamp, statuses and refusals are ppasr_ctc_align's; the
 * definition is the header comment of csrc/ctc_loss.hip.  One call, asynchronous on `stream`, no read-back.
 *   nll [B] f32; status [B] i32: 0 ok; 1 infeasible and 2 bad input, both with nll = +inf.  n_tokens = 0 with
 *   frame_lens = 0 gives nll = 0.  A result depends on its own utterance only (the same bits alone and in any batch). */
PPASR_API size_t ppasr_ctc_loss_workspace_bytes(int B, int Tp, int max_tokens);
PPASR_API ppasr_status ppasr_ctc_loss(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank,
                                      const int32_t* tokens, const int32_t* n_tokens, int max_tokens, float* nll,
                                      int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

/* Label-smoothing loss of the attention decoder (loss/label_smoothing_loss.py of the reference), teacher-forced over one
 * label per utterance: the decoder walk is ppasr_rescore's with nbest = 1.
 *   memory, out_lens: as ppasr_rescore; labels [B,max_tokens] i32, label_lens [B] i32 (clamped as ppasr_rescore clamps)
 *   att_kl, r_att_kl [B] f64: the sum over the label_lens[b] + 1 target rows (tokens, then eos) of
 *     kl_row = sum_v t_v (ln t_v - logp_v),  t = (1 - lsm_weight) at the target and lsm_weight / (V - 1) elsewhere, 0 ln 0 = 0
 *   of the left decoder and of the right decoder over the reversed label (0 when reverse_weight == 0: it does not run);
 *   row terms are summed in double in row order.  rows [B] i32: label_lens[b] + 1.
 *   At lsm_weight = 0, att_kl[b] is -att_scores[b] of ppasr_rescore on the same label, bit for bit.
 * Refusals as ppasr_rescore; lsm_weight outside [0, 1) is PPASR_EINVAL. */
PPASR_API size_t ppasr_rescorer_loss_workspace_bytes(ppasr_rescorer r, int B, int Tp, int max_tokens);
PPASR_API ppasr_status ppasr_rescorer_loss(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp,
                                           const int32_t* labels, const int32_t* label_lens, int max_tokens,
                                           double lsm_weight, double reverse_weight, double* att_kl, double* r_att_kl,
                                           int32_t* rows, void* workspace, size_t workspace_bytes, void* stream);

/* ---- attention beam-search decoding: WeNet's `attention` decode mode with the checkpoint's left decoder ----
 * An autoregressive beam search driven by the attention decoder itself (the reference's forward_one_step); the hypotheses
 * are not limited to what the CTC head proposed.  The semantics -- candidates, tie rules, the eos carry-over, stopping and
 * the outputs -- are defined once, in the header comment of csrc/attn_decode.hip.  One call, asynchronous on `stream`, no
 * read-back: every one of the max_steps steps is enqueued, and the steps behind the end of the search return at once.
 * `r`: any rescorer (r_num_blocks = 0 is fine: only the left decoder runs).  sos = eos = V - 1.
 *   memory [B,Tp,D] f32, out_lens [B] i32 or NULL: as ppasr_rescore
 *   tokens [B,beam_size,max_steps] i32 (-1 behind the hypothesis), lens [B,beam_size] i32, scores [B,beam_size] f64 (best
 *     first), ended [B,beam_size] i32 (0: cut at max_steps), steps_run [1] i32
 *   token_logp [B,beam_size,max_steps+1] f32 or NULL; trace_parent, trace_token [max_steps,B,beam_size] i32 and
 *     trace_score [max_steps,B,beam_size] f64, each or NULL: -1 / 0.0 where nothing happened
 * Refused before any device work: beam_size < 1 or > V, max_steps < 1, a NULL required pointer, a workspace that is not
 * 16-byte aligned (PPASR_EINVAL); beam_size > 32, max_steps + 1 above max_len or above 256 rows (PPASR_EUNSUPPORTED); a
 * workspace below ppasr_attention_decode_workspace_bytes (PPASR_ENOSPACE). */
PPASR_API size_t ppasr_attention_decode_workspace_bytes(ppasr_rescorer r, int B, int Tp, int beam_size, int max_steps);
PPASR_API ppasr_status ppasr_attention_decode(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp,
                                              int beam_size, int max_steps, int32_t* tokens, int32_t* lens, double* scores,
                                              int32_t* ended, int32_t* steps_run, float* token_logp, int32_t* trace_parent,
                                              int32_t* trace_token, double* trace_score, void* workspace,
                                              size_t workspace_bytes, void* stream);

/* ---- CTC-joint scoring inside the attention beam search (WeNet's ctc_weight in its attention beam search) ----
 * ppasr_attention_decode with the CTC prefix score of every candidate added inside the search:
 *   comb[v] = logp_att[v] + (float)ctc_weight * (Psi(g.v) - Psi(g)),
 * Psi(h) the log-probability, under the CTC table, that the transcript starts with h (for eos: that it IS g).  The
 * semantics are defined once, in the header comment of csrc/attn_decode_joint.hip.  One call, asynchronous on `stream`, no
 * read-back, every step enqueued.
 *   the arguments of ppasr_attention_decode, and
 *   ctc_probs [B,Tp,V_ctc] f32: the CTC head's softmax output of the same encode (frames t >= out_lens[b] are not read);
 *     V_ctc must equal the decoder's vocab_size; blank in [0, V - 1); ctc_weight >= 0
 *   token_ctc [B,beam_size,max_steps+1] f32 or NULL: Psi(g.v) - Psi(g) at every position of the final hypotheses (then
 *     token_logp holds logp_att); trace_ctc [max_steps,B,beam_size] f32 or NULL: Psi of each new row's hypothesis; 0.0
 *     where nothing happened
 * A row may offer, and an utterance may keep, fewer than beam_size finite candidates: the rest of the beam is at -inf
 * (scores -inf, lens 0, ended 0).  ctc_weight == 0 (or one that rounds to 0 in fp32): ppasr_attention_decode itself runs,
 * every output equals its output bit for bit, the workspace it needs suffices and ctc_probs may be NULL.
 * Refused before any device work, beside the refusals of ppasr_attention_decode: NULL ctc_probs with ctc_weight > 0, blank
 * outside [0, V - 1), V_ctc != vocab_size, ctc_weight negative or NaN (PPASR_EINVAL). */
PPASR_API size_t ppasr_attention_decode_joint_workspace_bytes(ppasr_rescorer r, int B, int Tp, int beam_size, int max_steps);
PPASR_API ppasr_status ppasr_attention_decode_joint(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B,
                                                    int Tp, int beam_size, int max_steps, const float* ctc_probs, int V_ctc,
                                                    int blank, double ctc_weight, int32_t* tokens, int32_t* lens,
                                                    double* scores, int32_t* ended, int32_t* steps_run, float* token_logp,
                                                    float* token_ctc, int32_t* trace_parent, int32_t* trace_token,
                                                    double* trace_score, float* trace_ctc, void* workspace,
                                                    size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PPASR_HIP_H */
