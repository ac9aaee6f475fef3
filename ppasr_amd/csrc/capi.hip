// capi.hip -- the model handle and the offline encode of the C-ABI of libppasr_hip.so (declared in include/ppasr_hip.h).
// Host side: descriptor checks and the dispatch of ppasr_create (the weights: weights.h and the families' *_create), the
// ppasr_set_* calls, the fp16 x3 mode and its range guard, workspace carving, the split / row-block rules, and the launch
// sequence of ppasr_encode (encode_impl; the frame it shares with the other walks: encode_common.h).  The decoders' entry
// points are in capi_decode.hip, the profilers in capi_profile.hip.
#include <cstdlib>

#include "capi_internal.h"

namespace ppasr {
thread_local LaunchProf g_launch_prof;  // launch.h
}

static thread_local std::string g_err;
std::string& ppasr_err_slot() { return g_err; }

// The checks of ppasr_create that need no weights, in their order of precedence; fills what they derive: m->desc (the
// Efficient-Conformer's stride layers in one representation), the route (m->generic, m->gen) and the front-end geometry.
static ppasr_status validate_desc(const ppasr_model_desc* desc, ppasr_model_s* m) {
  m->desc = *desc;
  const int F = desc->input_dim;
  if (desc->model_type == PPASR_MODEL_DEEPSPEECH2) {
    if (F > 128 || F < 7) return fail(PPASR_EUNSUPPORTED, "input_dim out of range");
    m->F1 = (F - 1) / 2;
    m->F2 = (m->F1 - 1) / 2;
    if (m->F1 > 40) return fail(PPASR_EUNSUPPORTED, "deepspeech2: input_dim <= 82 ((input_dim - 1) / 2 <= 40)");
    return PPASR_OK;
  }
  if (desc->model_type != PPASR_MODEL_CONFORMER && desc->model_type != PPASR_MODEL_SQUEEZEFORMER &&
      desc->model_type != PPASR_MODEL_EFFICIENT_CONFORMER)
    return fail(PPASR_EUNSUPPORTED, "model_type not built (conformer, efficient_conformer, squeezeformer are)");
  const bool eff = desc->model_type == PPASR_MODEL_EFFICIENT_CONFORMER;
  const unsigned smask = eff_stride_mask(*desc);
  const bool multi_stride = __builtin_popcount(smask) > 1;
  if (eff) {
    if (desc->group_layer_mask != 0 && (desc->group_size < 2 || desc->group_size > 4))
      return fail(PPASR_EUNSUPPORTED, "efficient_conformer: grouped attention is built for group_size 2, 3 and 4");
    if (desc->num_blocks > 31 || (smask >> desc->num_blocks) != 0) return fail(PPASR_EINVAL, "stride layer index out of range");
    if (smask != 0 && !multi_stride && desc->cnn_module_kernel != 15 && desc->output_size == kD)
      return fail(PPASR_EUNSUPPORTED, "efficient_conformer: cnn_module_kernel must be 15 (7 after the stride layer)");
    if ((desc->cnn_module_kernel >> __builtin_popcount(smask)) < 1)
      return fail(PPASR_EINVAL, "efficient_conformer: cnn_module_kernel halves to 0 behind the stride layers");
  }
  // output_size 256 (4 heads of 64) with the shipped constructor arguments: the fused row-block kernels.  Other multiples
  // of 256 up to 1024, non-default ConformerEncoder options (ppasr_model_desc::options), input_layer = linear or another
  // conv kernel size: the general layer route of capi_generic.hip (model_type = conformer).
  if (desc->output_size % 256 != 0 || desc->output_size < 256 || desc->output_size > 1024)
    return fail(PPASR_EUNSUPPORTED, "output_size must be 256, 512, 768 or 1024");
  if (desc->attention_heads * 64 != desc->output_size) return fail(PPASR_EUNSUPPORTED, "kernels are specialised for d_k=64");
  const bool fused_ks = desc->cnn_module_kernel == 15 || desc->cnn_module_kernel == 31 || desc->cnn_module_kernel == 7;
  const bool generic = (desc->model_type == PPASR_MODEL_CONFORMER &&
                        (desc->output_size != kD || desc->options != 0 || desc->input_layer == 1 || !fused_ks)) ||
                       ((desc->model_type == PPASR_MODEL_SQUEEZEFORMER || desc->model_type == PPASR_MODEL_EFFICIENT_CONFORMER) &&
                        desc->output_size != kD) ||
                       (eff && multi_stride) ||  // (several stride layers: kernels 15 -> 7 -> 3 ..., the general route)
                       (desc->model_type == PPASR_MODEL_SQUEEZEFORMER &&
                        (((desc->options >> PPASR_OPT_ACT_SHIFT) & PPASR_OPT_ACT_MASK) != PPASR_ACT_SWISH ||
                         (desc->options & PPASR_OPT_SQ_PRE_NORM) != 0 ||
                         (desc->options & PPASR_OPT_POS_MASK) != PPASR_OPT_POS_REL));  // (activation_type, normalize_before = True,
                                                                                       //  pos_enc_layer_type != rel_pos)
  // Squeezeformer takes two of the option fields: adaptive_scale = False and activation_type (squeezeformer/encoder.py:44-45)
  const int sq_opts = desc->model_type == PPASR_MODEL_SQUEEZEFORMER
                          ? (PPASR_OPT_SQ_NO_ADAPTIVE_SCALE | PPASR_OPT_SQ_PRE_NORM | PPASR_OPT_POS_MASK |
                             (PPASR_OPT_ACT_MASK << PPASR_OPT_ACT_SHIFT)) : 0;
  if (((desc->options & ~sq_opts) != 0 || desc->input_layer == 1) && desc->model_type != PPASR_MODEL_CONFORMER)
    return fail(PPASR_EUNSUPPORTED, "non-default encoder options / input_layer=linear are built for model_type=conformer");
  if ((desc->options & (PPASR_OPT_SQ_NO_ADAPTIVE_SCALE | PPASR_OPT_SQ_PRE_NORM)) && desc->model_type != PPASR_MODEL_SQUEEZEFORMER)
    return fail(PPASR_EINVAL, "PPASR_OPT_SQ_NO_ADAPTIVE_SCALE / PPASR_OPT_SQ_PRE_NORM are Squeezeformer options");
  if (desc->linear_units % 256 != 0 || desc->linear_units <= 0) return fail(PPASR_EUNSUPPORTED, "linear_units % 256 != 0");
  if (!generic && !fused_ks) return fail(PPASR_EUNSUPPORTED, "cnn_module_kernel must be 7, 15 or 31");
  if (generic) {
    const int ks = desc->cnn_module_kernel;
    const bool use_cnn = !(desc->options & PPASR_OPT_NO_CNN);
    if (use_cnn && (ks < 1 || ks > 63 || (!desc->causal && ks % 2 == 0)))
      return fail(PPASR_EINVAL, "cnn_module_kernel: 1..63, odd for the non-causal conv module (convolution.py:38)");
    if ((desc->options & PPASR_OPT_POS_MASK) == 3 || ((desc->options >> PPASR_OPT_ACT_SHIFT) & PPASR_OPT_ACT_MASK) > PPASR_ACT_HARDSHRINK)
      return fail(PPASR_EINVAL, "options: unknown pos_enc_layer_type / activation_type code");
  }
  if (desc->model_type == PPASR_MODEL_SQUEEZEFORMER && desc->cnn_module_kernel == 7)
    return fail(PPASR_EUNSUPPORTED, "squeezeformer: cnn_module_kernel must be 15 or 31");
  if (desc->input_dim > 128 || (desc->input_dim < 7 && desc->input_layer != 1) || desc->input_dim < 1)
    return fail(PPASR_EUNSUPPORTED, "input_dim out of range");
  if (eff) {  // one representation inside: the mask, and stride_layer_idx = its first (for the shipped shape: only) layer
    m->desc.stride_layer_mask = (int)smask;
    m->desc.stride_layer_idx = smask ? __builtin_ctz(smask) : -1;
  }
  const int il = desc->input_layer;
  if (il != 0 && il != 1 && il != 6 && il != 8)
    return fail(PPASR_EINVAL, "input_layer: 0 (conv2d), 1 (linear), 6 (conv2d6) or 8 (conv2d8)");
  m->generic = generic;
  m->gen.pos = desc->options & PPASR_OPT_POS_MASK;
  m->gen.post_norm = (desc->options & PPASR_OPT_POST_NORM) != 0;
  m->gen.concat_after = (desc->options & PPASR_OPT_CONCAT_AFTER) != 0;
  m->gen.macaron = !(desc->options & PPASR_OPT_NO_MACARON);
  m->gen.use_cnn = !(desc->options & PPASR_OPT_NO_CNN);
  m->gen.act = (desc->options >> PPASR_OPT_ACT_SHIFT) & PPASR_OPT_ACT_MASK;
  m->gen.sq_pre_norm = (desc->options & PPASR_OPT_SQ_PRE_NORM) != 0;
  if (il != 0 && desc->model_type == PPASR_MODEL_SQUEEZEFORMER)
    return fail(PPASR_EUNSUPPORTED, "squeezeformer: only the conv2d front end is built");
  m->F1 = (F - 1) / 2;
  // conv2d6's 5-wide kernel needs F1 >= 5: below that (F1 - 5) / 3 truncates toward zero to F2 = 1, and the conv would
  // read past the end of each conv1 row (the reference's conv2d raises)
  if (il == 6 && m->F1 < 5) return fail(PPASR_EINVAL, "input_dim too small for this input_layer (conv2d6: >= 11)");
  m->F2 = il == 6 ? (m->F1 - 5) / 3 + 1 : (m->F1 - 1) / 2;
  m->F3 = il == 8 ? (m->F2 - 1) / 2 : 0;
  if (il != 1 && m->F_last() < 1) return fail(PPASR_EINVAL, "input_dim too small for this input_layer");
  return PPASR_OK;
}

extern "C" {

const char* ppasr_last_error(void) { return g_err.c_str(); }
const char* ppasr_version(void) { return "ppasr_hip 0.1 (gfx950, fp32 MFMA)"; }

ppasr_status ppasr_create(const ppasr_model_desc* desc, const ppasr_weight_blob* blobs, int n_blobs, ppasr_handle* out) {
  if (!desc || !blobs || !out) return fail(PPASR_EINVAL, "null argument");
  std::unique_ptr<ppasr_model_s> m(new ppasr_model_s());
  LOAD_TRY(validate_desc(desc, m.get()));
  HIP_TRY(configure_kernels());
  if (desc->model_type != PPASR_MODEL_DEEPSPEECH2) {
    HIP_TRY(configure_generic_kernels());
    HIP_TRY(configure_squeezeformer_kernels());
  }
  const BlobMap sd = blob_map(blobs, n_blobs);
  Loader ld{m.get(), sd, ""};
  switch (desc->model_type) {
    case PPASR_MODEL_DEEPSPEECH2: LOAD_TRY(ds2_create(m.get(), ld)); break;
    case PPASR_MODEL_SQUEEZEFORMER: LOAD_TRY(squeezeformer_create(m.get(), ld)); break;
    default: LOAD_TRY(conformer_create(m.get(), ld));
  }
  HIP_TRY(hipDeviceSynchronize());
  *out = m.release();
  return PPASR_OK;
}

ppasr_status ppasr_destroy(ppasr_handle h) {
  delete h;
  return PPASR_OK;
}

int ppasr_out_frames(ppasr_handle h, int T) {
  if (T < (h ? h->min_frames() : 7)) return 0;
  int tp = h ? h->front_dims(T).Tp : ((T - 1) / 2 - 1) / 2;
  // Efficient-Conformer: the stride-2 conv layer halves the frame rate (ceil), efficient_conformer/encoder.py:252-257
  if (h)
    for (int n = __builtin_popcount(eff_stride_mask(h->desc)); n > 0; --n) tp = (tp + 1) / 2;
  return tp;
}

}  // extern "C"
WsLayout ws_layout(const ppasr_model_s* m, int B, int T) {
  if (m->generic) {
    WsLayout g{};
    g.total = generic_ws_floats(m, B, T);
    return g;
  }
  const auto fd = m->front_dims(T);
  const size_t T1 = fd.T1, Tp = fd.Tp;
  const size_t M = (size_t)B * Tp;
  auto al = [](size_t n) { return (n + 63) & ~(size_t)63; };
  WsLayout w;
  size_t o = 0;
  // Partial-sum tiles of the under-filled launches (ffn_split_for: S slices of Mi <= M rows): the default split keeps
  // S x blocks <= 256, so S Mi <= 256 x 32 rows; one forced by ppasr_set_ffn_split is S = ffn_split at any Mi.
  const size_t split_rows = m->ffn_split > 1 ? (size_t)m->ffn_split * M
                          : m->ffn_split == 0 ? 0 : std::min((size_t)8 * M, (size_t)256 * kRows);
  // (conv2d8: the third conv's output reuses it.)  Once the front end has read it, the conv1 buffer is the partial-sum
  // scratch of the layers and the head: up to 4 S tiles (the streaming chunk's two fused FFN joins of 2 S tiles each).
  // conv1's own output (T1 >= 2 T' + 1 frames of F1 bins) covers that from F1 = 16 on; at fewer bins the buffer is
  // sized for the scratch.
  w.y1 = o; o += al(std::max((size_t)B * T1 * m->F1 * kD, 4 * split_rows * kD));
  // conv2d8: once the third conv has read it, conv2's output buffer is the embed's K-split scratch (S tiles); conv2's
  // own output (T2 >= 2 T' + 1 frames of F2 bins) covers that from F2 = 4 on
  const size_t y2_floats = (size_t)B * (fd.T2 ? fd.T2 : Tp) * m->F2 * kD;
  w.y2 = o; o += al(m->desc.input_layer == 8 ? std::max(y2_floats, split_rows * kD) : y2_floats);
  w.xa = o; o += al(M * kD);
  w.xb = o; o += al(M * kD);
  w.xc = o; o += al(M * kD);
  w.qkv = o; o += al(M * 3 * kD);
  w.ctx = o; o += al(M * kD);
  w.g = o; o += al(M * kD);
  w.rmax = o; o += al(M);
  w.rsum = o; o += al(M);
  w.fa = o; o += al(M);
  w.fp = o; o += al(M);
  w.xs = o; o += al(M * kD);  // saved full-resolution activations (Squeezeformer time reduction)
  // values in fragment order for the fused attention route (VtOut): a key sub-block of 64 rows may start up to 7 rows
  // before an utterance and end up to 63 rows behind the last one
  w.vt_stride = (int)(al(M) + 128);
  w.vt = o; o += al((size_t)kD * w.vt_stride);
  w.total = o;
  return w;
}
// slices of a launch with `units` independent pieces per row block (K chunks of the input projection, vocabulary tile
// groups of the CTC head) on the split route: as many as fill the chip once, at least the feed-forward split
int wide_slices_for(const ppasr_model_s* m, int M, int units) {
  const int S = ffn_split_for(m, M);
  if (S <= 1) return S;
  const int blocks = (M + kRows - 1) / kRows;
  return std::max(S, std::min(units, 256 / blocks));
}
int ffn_split_for(const ppasr_model_s* m, int M) {
  if (m->desc.model_type == PPASR_MODEL_DEEPSPEECH2) return 1;
  const int n_chunks = m->desc.linear_units / 256;
  if (m->ffn_split >= 0) return m->ffn_split > 1 ? m->ffn_split : 1;
  const int blocks = (M + kRows - 1) / kRows;
  if (blocks > 128) return 1;
  int S = 8;
  while (S > 1 && (blocks * S > 256 || n_chunks % S != 0)) S >>= 1;
  return S;
}

bool block_tables_enabled() {
  static const bool on = [] {
    const char* e = getenv("PPASR_BLOCK_TABLE");
    return !(e && e[0] == '0');
  }();
  return on;
}

bool conv12_enabled(const ppasr_model_s* m) { return m->front_fused != 0; }  // ppasr_set_front_fused

int row_block_for(const ppasr_model_s* m, int B, int Tcur, int mul, int slack, bool skip) {
  // 32 rows on 16 waves (rbt.h kW16) in place of the 8-wave 32-row kernels: OPT-IN per handle,
  // ppasr_set_row_block(PPASR_ROW_BLOCK_32_W16).  Measured on the three bench configurations it is a wash -- the
  // feed-forward streams gain 3 % (92.6 against 89.6 % of the matrix-pipe rate, tools/phase_ts.py --t), the 16-wave
  // depthwise-conv phase requests each window row twice as often and the launch is longer: cfg2 5.99 ms against 5.92,
  // cfg4 9.10 = 9.10, cfg5 6.73 against 6.80 (NOTES.md "Measured and not adopted").
  if (m->row_block == 16 || m->row_block == 32 || m->row_block == kW16) return m->row_block;
  long long rows = (long long)B * Tcur;
  if (skip && (int)m->lens_hint.size() == B) {
    rows = 0;
    for (int b = 0; b < B; ++b) {
      const long long len = m->lens_hint[b];
      const long long need = (len > 0 ? (len + mul - 1) / mul : 0) + slack;
      rows += need < Tcur ? need : Tcur;
    }
  }
  // Rounds of one workgroup per CU: ceil(blocks / 256), a 16-row round 0.52 of a 32-row one (tools/microbench_rb16: 4.3 us
  // per 16-row GEMM unit against 8.4 us per 32-row one; tools/r04_tune_rows.py: whole-encoder timings over batch sizes).
  // 33 .. 128 blocks of 32 rows: one half-as-long round instead of a half-empty one; 257 .. 384: three short rounds instead
  // of two long ones.  Up to 32 blocks the split route (ffn_split_for: 8 hidden slices per row block) fills more CUs than
  // 2 x the blocks would.
  constexpr int min_blocks = 32;
  const long long b32 = (rows + 31) / 32, b16 = (rows + 15) / 16;
  if (b32 <= min_blocks) return 32;  // (split route: the 8-wave kernels)
  const double c32 = (double)((b32 + 255) / 256), c16 = 0.52 * (double)((b16 + 255) / 256);
  return c16 < c32 ? 16 : 32;
}

extern "C" {

ppasr_status ppasr_set_row_block(ppasr_handle h, int rows) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  if (rows != -1 && rows != 16 && rows != 32 && rows != PPASR_ROW_BLOCK_32_W16)
    return fail(PPASR_EINVAL, "row block: -1 (by grid size), 16, 32 or PPASR_ROW_BLOCK_32_W16");
  h->row_block = rows;
  return PPASR_OK;
}

ppasr_status ppasr_set_lengths_hint(ppasr_handle h, const int64_t* lens_host, int B) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  if (!lens_host || B <= 0) h->lens_hint.clear();
  else h->lens_hint.assign(lens_host, lens_host + B);
  return PPASR_OK;
}

size_t ppasr_workspace_bytes(ppasr_handle h, int B, int T) {
  if (!h || B <= 0 || T < 7) return 0;
  return ws_layout(h, B, T).total * sizeof(float);
}

ppasr_status ppasr_set_debug_taps(ppasr_handle h, float* taps, size_t n_floats) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  h->taps = taps;
  h->taps_floats = taps ? n_floats : 0;
  return PPASR_OK;
}

ppasr_status ppasr_set_memory_out(ppasr_handle h, float* memory_dev, size_t n_floats) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  if (h->desc.model_type == PPASR_MODEL_DEEPSPEECH2 && memory_dev)
    return fail(PPASR_EUNSUPPORTED, "memory output: DeepSpeech2 has no attention decoder");
  if (h->sq_final_proj && memory_dev)
    return fail(PPASR_EUNSUPPORTED, "memory output: final_proj is folded into the CTC head, its output is not formed");
  h->memory_out = memory_dev;
  h->memory_floats = memory_dev ? n_floats : 0;
  return PPASR_OK;
}

ppasr_status ppasr_set_ffn_split(ppasr_handle h, int mode) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  if (mode != -1 && mode != 0 && mode != 2 && mode != 4 && mode != 8) return fail(PPASR_EINVAL, "ffn split: -1, 0, 2, 4 or 8");
  if (mode > 0 && (h->desc.linear_units / 256) % mode != 0) return fail(PPASR_EINVAL, "ffn split must divide linear_units / 256");
  h->ffn_split = mode;
  return PPASR_OK;
}

ppasr_status ppasr_set_front_fused(ppasr_handle h, int mode) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  if (mode < -1 || mode > 1) return fail(PPASR_EINVAL, "front fused: -1 (default), 0 or 1");
  h->front_fused = mode;
  return PPASR_OK;
}

// ---- range guard of the fp16 x3 mode (csrc/h3.h): the event counters of the translation units that hold fp16 x3 kernels,
// snapshotted in stream order
struct GuardPtrs {
  const unsigned int* p[ppasr_model_s::kGuardN];
};
__global__ void k_h3_snapshot(GuardPtrs g, unsigned int* dst) {
  for (int i = 0; i < ppasr_model_s::kGuardN; ++i) dst[i] = *g.p[i];
}
static GuardPtrs guard_ptrs(ppasr_handle h) {
  GuardPtrs g;
  for (int i = 0; i < ppasr_model_s::kGuardN; ++i) g.p[i] = h->guard_ctr[i];
  return g;
}

static ppasr_status guard_alloc(ppasr_handle h) {
  if (h->guard_dev) return PPASR_OK;
  constexpr int N = ppasr_model_s::kGuardN;
  h->guard_ctr[0] = conformer_h3_ovf_counter();
  h->guard_ctr[1] = squeezeformer_h3_ovf_counter();
  h->guard_ctr[2] = front_h3_ovf_counter();
  h->guard_ctr[3] = ctc_head_h3_ovf_counter();
  h->guard_ctr[4] = split_route_h3_ovf_counter();
  for (int i = 0; i < N; ++i)
    if (!h->guard_ctr[i]) return fail(PPASR_EHIP, "fp16 x3 range guard: counter symbols not found");
  void* d = nullptr;
  LOAD_TRY(h->alloc(2 * N * sizeof(unsigned int), &d));
  h->guard_dev = static_cast<unsigned int*>(d);
  void* p = nullptr;
  HIP_TRY(hipHostMalloc(&p, 2 * N * sizeof(unsigned int), hipHostMallocDefault));
  h->guard_host = static_cast<unsigned int*>(p);
  return PPASR_OK;
}

ppasr_status ppasr_set_gemm_mode(ppasr_handle h, int mode) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  if (mode != PPASR_GEMM_F32 && mode != PPASR_GEMM_F16X3) return fail(PPASR_EINVAL, "gemm mode: PPASR_GEMM_F32 or PPASR_GEMM_F16X3");
  if (mode == PPASR_GEMM_F16X3) {
    const int mt = h->desc.model_type;
    // the layer kernels' feed-forward modules (Conformer, Efficient-Conformer) ...
    bool layers_ok = (mt == PPASR_MODEL_CONFORMER || mt == PPASR_MODEL_EFFICIENT_CONFORMER) && !h->generic && !h->layers.empty();
    for (size_t i = 0; layers_ok && i < h->layers.size(); ++i)
      layers_ok = conv_ffn_h3_supported(h->layer_ks[i]) && h->layers[i].ffm_w1 != nullptr;
    // ... and the second convolution of the 4x front end (Squeezeformer's depthwise-separable one is folded into the same
    // dense [9 * 256][256] weight at create time)
    const bool front_ok = !h->generic && mt != PPASR_MODEL_DEEPSPEECH2 && h->desc.input_layer == 0 && h->front.conv2_k == 3 &&
                          h->front.conv2_w != nullptr;
    // ... Squeezeformer: the two feed-forward modules of a layer (k_sq_mid_h3 / k_sq_tail_h3)
    const bool sq_ok = mt == PPASR_MODEL_SQUEEZEFORMER && !h->generic && !h->sq_layers.empty() &&
                       sq_h3_supported(h->desc.cnn_module_kernel, 4);
    if (!layers_ok && !front_ok && !sq_ok)
      return fail(PPASR_EUNSUPPORTED, "fp16 x3 GEMMs: built for the fused 256-wide routes (feed-forward modules of Conformer / "
                                      "Efficient-Conformer / Squeezeformer layers; conv2 of the 4x front end)");
    const int d = h->desc.output_size, H = h->desc.linear_units;
    {
      const ppasr_status g = guard_alloc(h);
      if (g != PPASR_OK) return g;
    }
    // weights are scaled by 2^8 into fp16: |w| >= 255.9 would overflow (k_repack_h3 counts such weights -- in a word of this
    // call's own, not in the run-time guard's process-wide counters, which a concurrent fp16 x3 encode on another handle
    // may raise at any time)
    unsigned int w_before = 0, w_after = 0;
    unsigned int* w_ovf = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&w_ovf), sizeof(unsigned int)));
    struct OvfFree { unsigned int* p; ~OvfFree() { (void)hipFree(p); } } w_ovf_free{w_ovf};
    HIP_TRY(hipMemset(w_ovf, 0, sizeof(unsigned int)));
    const size_t alloc_mark = h->allocs.size();  // re-packed copies made by THIS call start here (freed if the mode is refused)
    // a weight [32 n_tiles columns][8 G deep] as scaled fp16 pieces in a block of its own; *w then points at the copy
    auto repack = [&](const f32x4** w, int n_tiles, int G) -> ppasr_status {
      void* dst = nullptr;
      LOAD_TRY(h->alloc((size_t)n_tiles * G * 256 * sizeof(float), &dst));
      launch_repack_h3(*w, static_cast<f32x4*>(dst), n_tiles, G, w_ovf, nullptr);
      *w = static_cast<const f32x4*>(dst);
      return PPASR_OK;
    };
    HIP_TRY(hipDeviceSynchronize());
    if (layers_ok && h->layers_h3.empty()) {
      std::vector<LayerW> view = h->layers;
      for (LayerW& L : view) {
        // W1 [d][H]: H / 32 column tiles of d / 8 k-groups; W2 [H][d]: d / 32 tiles of H / 8 k-groups; then the d-deep
        // projections [Wq|Wk|Wv] (3d columns), linear_out, pointwise_conv1 (2d columns), pointwise_conv2
        struct { const f32x4** w; int n_tiles, G; } items[8] = {
            {&L.ffm_w1, H / 32, d / 8}, {&L.ffm_w2, d / 32, H / 8}, {&L.ff_w1, H / 32, d / 8}, {&L.ff_w2, d / 32, H / 8},
            {&L.wqkv, 3 * d / 32, d / 8}, {&L.wo, d / 32, d / 8},   {&L.pw1, 2 * d / 32, d / 8}, {&L.pw2, d / 32, d / 8}};
        for (auto& it : items) LOAD_TRY(repack(it.w, it.n_tiles, it.G));
        // the layer's projected positional table as operand planes (the fused attention's score MFMAs in the mode)
        if (L.ptab != h->zero_vec) {
          void* dst = nullptr;
          LOAD_TRY(h->alloc((size_t)h->desc.max_len * d * sizeof(float), &dst));
          launch_split_rows_h3(L.ptab, static_cast<float*>(dst), h->desc.max_len, w_ovf, nullptr);
          L.ptab = static_cast<const float*>(dst);
        }
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
      h->layers_h3 = std::move(view);
    }
    if (sq_ok && h->sq_layers_h3.empty()) {
      std::vector<SqLayerW> view = h->sq_layers;
      for (SqLayerW& L : view) {
        const f32x4** w[4] = {&L.ff1_w1, &L.ff1_w2, &L.ff2_w1, &L.ff2_w2};
        for (int j = 0; j < 4; ++j) LOAD_TRY(repack(w[j], (j & 1) ? d / 32 : H / 32, (j & 1) ? H / 8 : d / 8));
      }
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
      h->sq_layers_h3 = std::move(view);
    }
    if ((layers_ok || sq_ok || front_ok) && !h->head_w_h3 && h->head.w) {  // the CTC head of the fused routes
      const f32x4* w = h->head.w;
      LOAD_TRY(repack(&w, h->head.n_tiles, d / 8));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
      h->head_w_h3 = w;
    }
    if (front_ok && !h->conv2_w_h3) {  // K = 9 * 256
      // ... and the input projection behind it: K = F2 * 256 (a whole number of 256-deep chunks), 256 columns
      const f32x4 *wc = h->front.conv2_w, *we = h->front.embed_w;
      LOAD_TRY(repack(&wc, d / 32, 9 * d / 8));
      LOAD_TRY(repack(&we, d / 32, h->F2 * d / 8));
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipDeviceSynchronize());
      h->conv2_w_h3 = wc;
      h->embed_w_h3 = we;
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&w_after, w_ovf, sizeof(unsigned int), hipMemcpyDeviceToHost));
    if (w_after != w_before) {
      // the mode stays off, the views are dropped so that a later call re-checks, and the copies this call made are freed
      // (a retry does not pile up second copies of the weights)
      h->layers_h3.clear();
      h->sq_layers_h3.clear();
      h->head_w_h3 = h->conv2_w_h3 = h->embed_w_h3 = nullptr;
      for (size_t i = alloc_mark; i < h->allocs.size(); ++i) (void)hipFree(h->allocs[i]);
      h->allocs.resize(alloc_mark);
      return fail(PPASR_EUNSUPPORTED, "fp16 x3 GEMMs: a weight of magnitude >= 255.9 (or a positional-table entry >= 4094) does not fit the scaled fp16 pieces");
    }
    for (int i = 0; i < ppasr_model_s::kGuardN; ++i)
      HIP_TRY(hipMemcpy(&h->guard_seen[i], h->guard_ctr[i], sizeof(unsigned int), hipMemcpyDeviceToHost));
    h->gemm_coverage = (layers_ok ? PPASR_GEMM_COVERS_LAYERS : 0) | (sq_ok ? PPASR_GEMM_COVERS_LAYERS : 0) |
                       (front_ok ? PPASR_GEMM_COVERS_FRONT : 0) | (h->head_w_h3 ? PPASR_GEMM_COVERS_HEAD : 0);
  } else {
    h->gemm_coverage = 0;
  }
  h->gemm_mode = mode;
  return PPASR_OK;
}

int ppasr_gemm_coverage(ppasr_handle h) { return h ? h->gemm_coverage : 0; }

ppasr_status ppasr_set_skip_padding(ppasr_handle h, int enable) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  // the ragged mode is built into the fused 256-column kernels behind the 4x front end; other handles would silently
  // compute (and return) every padded row, which is not what the caller asked for
  if (enable && (h->desc.model_type == PPASR_MODEL_DEEPSPEECH2 || h->desc.input_layer == 1))
    return fail(PPASR_EUNSUPPORTED, "skip_padding: built behind the conv front ends (DeepSpeech2 and input_layer = linear "
                                    "compute every row)");
  h->skip_padding = enable != 0;
  return PPASR_OK;
}

static ppasr_status encode_impl(ppasr_handle h, const float* feats, const int64_t* lens, int B, int T, float* probs,
                                float* logits, int32_t* frame_argmax, float* frame_maxprob, void* workspace,
                                size_t workspace_bytes, void* stream) {
  if (!h || !feats || !workspace) return fail(PPASR_EINVAL, "null argument");
  if (B <= 0 || T < h->min_frames()) return fail(PPASR_EINVAL, "need B > 0 and T >= 7 (conv2d6: 11, conv2d8: 15) frames");
  if (h->desc.model_type == PPASR_MODEL_DEEPSPEECH2) return fail(PPASR_EINVAL, "deepspeech2 handles use ppasr_ds2_encode");
  const auto fd = h->front_dims(T);
  const int F = h->desc.input_dim, T1 = fd.T1, F1 = h->F1, Tp = fd.Tp, F2 = h->F2;
  const int sub = h->sub_rate();  // frame t of the encoder is PAD iff sub * t >= len (the reference's mask slicing)
  if (Tp >= h->desc.max_len) return fail(PPASR_EINVAL, "utterance longer than the positional table (embedding.py:64-66)");
  const int M = B * Tp;
  const WsLayout wl = ws_layout(h, B, T);
  if (workspace_bytes < wl.total * sizeof(float)) return fail(PPASR_ENOSPACE, "workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  if (h->generic)
    return h->desc.model_type == PPASR_MODEL_SQUEEZEFORMER
               ? generic_sq_encode(h, feats, lens, B, T, probs, logits, frame_argmax, frame_maxprob, ws, st)
               : generic_encode(h, feats, lens, B, T, probs, logits, frame_argmax, frame_maxprob, ws, st);
  if (h->desc.model_type == PPASR_MODEL_SQUEEZEFORMER)
    return squeezeformer_encode(h, feats, lens, B, T, probs, logits, frame_argmax, frame_maxprob, ws, wl, st);
  float *y1 = ws + wl.y1, *y2 = ws + wl.y2, *xa = ws + wl.xa, *xb = ws + wl.xb, *xc = ws + wl.xc;
  float *qkv = ws + wl.qkv, *ctx = ws + wl.ctx, *g = ws + wl.g;
  const VtOut vt_out{ws + wl.vt, wl.vt_stride};
  // the fused attention reads whole 64-row key sub-blocks of V^T: rows outside an utterance (padding behind the last
  // row, frames a ragged batch skips) are multiplied by p = 0 and must be finite
  HIP_TRY(hipMemsetAsync(ws + wl.vt, 0, (size_t)kD * wl.vt_stride * sizeof(float), st));
  Taps tap{h->taps, h->taps_floats, st};
  if (h->prof) {
    h->ev_used = 0;
    h->spans.clear();
  }
  auto timed = [&](int cls, auto&& fn) {
    if (!h->prof) {
      fn();
      return;
    }
    // every kernel launched by fn() gets its own (start, stop) events attached to its dispatch (launch.h)
    h->spans.push_back({cls, {}});
    g_launch_prof.ctx = h;
    g_launch_prof.next = [](void* ctx, const void*, hipEvent_t* s, hipEvent_t* e) {
      ppasr_model_s* m = static_cast<ppasr_model_s*>(ctx);
      *s = m->next_event();
      *e = m->next_event();
      m->spans.back().ev.emplace_back(*s, *e);
    };
    fn();
    g_launch_prof = LaunchProf{};
  };
  // ragged batches (ppasr_set_skip_padding; the rule: RaggedPlan)
  const bool eff = h->desc.model_type == PPASR_MODEL_EFFICIENT_CONFORMER;
  // (6x / 8x front ends: the LAYERS and the head skip -- frame t is valid iff 6t / 8t < len --, the front end itself
  //  computes every row: its skip rules are written for the 3x3 / 2 pair of Conv2dSubsampling4)
  const bool skip = h->skip_padding && lens && !h->taps && h->desc.input_layer != 1;
  const RaggedPlan ragged{skip, lens, h->desc.causal ? 0 : (h->desc.cnn_module_kernel - 1) / 2, eff, sub};
  // Ragged batches on the fused attention route (ppasr_set_ffn_split(0), or more than 128 row blocks): its key sub-blocks
  // read the VALUES of whole 64-row pieces of the batch's row space times p = 0, and the QKV stage writes those values
  // for every row of a 32-row block that holds one needed frame.  The rows behind the needed frames in such a block are
  // computed from what their producers left: conv2 skips by its own tiles (the embed then reads rows of y2 nobody
  // wrote), the fused attention by 32-query blocks counted from the utterance's first frame (xc / g), and behind the
  // Efficient-Conformer's stride layer the half-rate rows lie where nobody wrote at the full rate (xa).  They must be
  // finite, so the activation buffers (y2 .. g, one range of the workspace) start from zeros on this route (and on no
  // other: rowblock.h PadSkip).  The vt clear above only covers rows of blocks the QKV stage skips.
  // (tests/test_buffer_contents_gpu.py test_batched_encode[conformer-9x1000-ff], [conformer-3x131-masked-ff] and
  // [efficient-3x400-ff], routes ffn_split=0+skip: NaN in every valid row when the workspace held NaN.)
  // (fuse_rows of the M entry-rate rows: no layer has more)
  if (skip && fuse_rows(h, M)) HIP_TRY(hipMemsetAsync(y2, 0, (wl.rmax - wl.y2) * sizeof(float), st));
  BlockTables tables(skip, B, M, ws + wl.rmax, st);
  if (h->desc.input_layer == 8) {
    // Conv2dSubsampling8: conv1 -> conv2 (3x3 / 2) -> conv3 (3x3 / 2, written over conv1's output) -> linear
    timed(0, [&] { launch_conv1(feats, h->front, y1, B, T, F, T1, F1, st, PadSkip{}); });
    timed(1, [&] {
      launch_conv_stage(y1, h->front.conv2_w, h->front.conv2_b, y2, B, T1, F1, fd.T2, F2, 3, 2, st);
      launch_conv_stage(y2, h->front.conv3_w, h->front.conv3_b, y1, B, fd.T2, F2, Tp, h->F3, 3, 2, st);
    });
    timed(2, [&] { launch_embed(y1, h->front, xa, M, h->F3 * kD, sqrtf((float)kD), false, st, PadSkip{}, ffn_split_for(h, M), y2); });
  } else {
    const PadSkip ps_front = skip && h->desc.input_layer == 0 ? ragged.at(Tp, sub) : PadSkip{};  // (the front end's own kernels)
    front4_fused(h, feats, B, T, ps_front, tables.tile_tab(), /*scale_before_bias=*/false, wide_slices_for(h, M, F2), ps_front, y1,
                 y2, xa, st, timed);
  }
  tap(xa, (size_t)M * kD);
  const int n_chunks = h->desc.linear_units / 256;
  int Ti = Tp, mul = sub, pstride = 1;  // frames per utterance / pad-mask multiplier / positional stride of the current layer
  bool s1_done = false;               // this layer's S1 already ran inside the previous layer's last launch
  for (int i = 0; i < h->desc.num_blocks; ++i) {
    const LayerW& L = h->layers[i];
    const int Mi = B * Ti;
    const int grp = h->layer_group[i];
    const PadSkip ps = ragged.at(Ti, mul);
    const LayerRoute route = layer_route(h, B, Ti, mul, ps.slack, skip, i);
    const int S = route.S, form = route.form;
    const bool fuse_attn = route.fuse_attn, h3 = route.h3, h3s = route.h3s;
    const PadSkip psb = S == 1 ? tables.with_table(ps, Ti, form_rows(form)) : ps;  // (for the kernels of this layer's block size)
    const LayerW& Lk = (h3 || h3s) ? h->layers_h3[i] : L;
    // What the QKV stage that feeds layer `layer` (route r; its own S1 launch, or the NEXT tail of the layer before, which
    // runs at the same rate) leaves besides row-major qkv.  Fused attention: the values in fragment order.  In the fp16 x3
    // mode the attention's score MFMAs read K as fp16 hi / lo planes (VtOut::k_h3) and the layer's positional planes; on
    // the fp32 route it contracts 64 wide against k + p (AttnArgs::dtab), so K holds the positional rows.  Producer and
    // consumer both read r: layer j's K is planes iff j runs k_attn_out_glu_h3, holds k + p iff j runs the fp32 k_attn_out_glu.
    auto vt_for = [&](const LayerRoute& r, int layer) {
      VtOut v = r.fuse_attn ? vt_out : VtOut{};
      v.k_h3 = (r.fuse_attn && r.h3) ? 1 : 0;
      if (r.fuse_attn && !r.h3 && h->layers[layer].dtab) {
        v.kpos = h->layers[layer].ptab;  // (the fp32 table, not the h3 view's planes)
        v.kpos_stride = pstride * kD;
        v.Ti = Ti;
      }
      return v;
    };
    float* partial = y1;
    float* x3 = ctx;
    if (!s1_done) {
      if (S > 1) {
        timed(3, [&] {
          launch_ffn_split(xa, L.ln_mac_g, L.ln_mac_b, Lk.ffm_w1, L.ffm_b1, Lk.ffm_w2, L.ffm_b2, 0.5f, nullptr, nullptr, partial,
                           xb, Mi, n_chunks, S, st, ps, false, h3s);
          launch_ln_qkv(xb, qkv, Lk, Mi, st, ps, nullptr, nullptr, h3s);
        });
      } else {
        timed(3, [&] { launch_ffn_qkv(xa, xb, qkv, Lk, Mi, n_chunks, st, psb, vt_for(route, i), h3, form); });
      }
    }
    s1_done = false;
    tap(xb, (size_t)Mi * kD);
    tap(qkv, (size_t)Mi * 3 * kD);
    const int Tt = (Ti + grp - 1) / grp;  // tokens: frames, or zero-padded groups of 3 (pad4group)
    AttnArgs a{qkv, 768, qkv + 256, 768, qkv + 512, 768, Tt, Tt, 0, lens, ctx, L.pos_u, L.pos_v, (h3 && fuse_attn) ? Lk.ptab : L.ptab, pstride,
               mul * grp, Ti, Ti, grp};
    a.pad_skip = ragged.attn_pad_skip(ps);
    a.vt = vt_out.vt;
    a.vt_stride = vt_out.stride;
    if (fuse_attn && !h3) {
      a.dtab = L.dtab;
      a.dtab_len = h->desc.max_len;
    }
    if (fuse_attn) {
      timed(9, [&] { launch_attn_out_glu(a, B, xb, xc, g, Lk, st, h3); });
    } else {
      timed(4, [&] { launch_attention(a, B, h->desc.attention_heads, st); });
      tap(ctx, (size_t)Mi * kD);
      // (under-filled launch: pointwise_conv1 + GLU as its own two-column-half launch; the LayerNorm'd rows pass through
      //  xa, which is free between this layer's S1 and its output)
      timed(5, [&] {
        launch_out_glu(ctx, xb, xc, g, nullptr, h3s ? Lk : L, lens, Mi, Ti, mul, st, psb, S > 1 ? xa : nullptr, h3s, nullptr, form);
      });
    }
    tap(xc, (size_t)Mi * kD);
    tap(g, (size_t)Mi * kD);
    if (eff && i == h->desc.stride_layer_idx) {
      const int Ts = (Ti + 1) / 2;
      timed(6, [&] {
        const int Ss = form == 16 ? 1 : ffn_split_for(h, B * Ts);
        if (Ss > 1) {  // under-filled: the conv half alone (x3 -> ctx), the feed-forward module over the slices
          launch_conv_ffn_stride(g, nullptr, xc, xa, h3s ? Lk : L, lens, B, Ti, Ts, n_chunks, h->layer_ks[i], mul * 2, st,
                                 ragged.at(Ts, mul * 2), h->desc.causal != 0, h3s, ctx);
          launch_ffn_split(ctx, L.ln_ff_g, L.ln_ff_b, Lk.ff_w1, L.ff_b1, Lk.ff_w2, L.ff_b2, 0.5f, L.ln_fin_g, L.ln_fin_b, partial,
                           xa, B * Ts, n_chunks, Ss, st, ragged.at(Ts, mul * 2), false, h3s);
        } else {
          launch_conv_ffn_stride(g, nullptr, xc, xa, (h3 || h3s) ? Lk : L, lens, B, Ti, Ts, n_chunks, h->layer_ks[i], mul * 2, st,
                                 ragged.at(Ts, mul * 2), h->desc.causal != 0, h3 || h3s);
        }
      });
      Ti = Ts;  // masks[:, :, ::2], pos_emb[:, ::2]  (efficient_conformer/encoder.py:252-257)
      mul *= 2;
      pstride *= 2;
    } else if (S > 1) {
      timed(6, [&] {
        launch_conv_pre(g, nullptr, xc, x3, Lk, lens, Mi, Ti, h->layer_ks[i], mul, st, h->desc.causal != 0, ps, h3s);
        launch_ffn_split(x3, L.ln_ff_g, L.ln_ff_b, Lk.ff_w1, L.ff_b1, Lk.ff_w2, L.ff_b2, 0.5f, L.ln_fin_g, L.ln_fin_b, partial,
                         xa, Mi, n_chunks, S, st, ps, false, h3s);
      });
    } else {
      // fuse the next layer's S1 into this launch (it writes xb / qkv, which this layer no longer reads)
      const LayerW* next = (i + 1 < h->desc.num_blocks) ? (h3 ? &h->layers_h3[i + 1] : &h->layers[i + 1]) : nullptr;
      // (the next layer runs at this layer's rate: the stride layer has no NEXT tail)
      const VtOut vt_next = next ? vt_for(layer_route(h, B, Ti, mul, ps.slack, skip, i + 1), i + 1) : VtOut{};
      timed(next ? 8 : 6, [&] {
        // with the next layer's S1 fused in, the layer output itself is only read by the debug taps: skip its store
        launch_conv_ffn(g, nullptr, xc, (next && !h->taps) ? nullptr : xa, Lk, lens, Mi, Ti, n_chunks, h->layer_ks[i], mul, next,
                        xb, qkv, st, h->desc.causal != 0, psb, vt_next, h3, form);
      });
      s1_done = next != nullptr;
    }
    tap(xa, (size_t)B * Ti * kD);
  }
  const int Mo = B * Ti;
  // (under-filled launch: the vocabulary tiles are split over several workgroups per row block)
  return fused_head_tail(h, xa, probs, logits, frame_argmax, frame_maxprob, ws, wl, B, Mo,
                         wide_slices_for(h, Mo, std::min((h->head.n_tiles + 7) / 8, 32)), ragged.at(Ti, mul), st, timed);
}

ppasr_status ppasr_encode(ppasr_handle h, const float* feats, const int64_t* lens, int B, int T, float* probs,
                          float* logits, int32_t* frame_argmax, float* frame_maxprob, void* workspace,
                          size_t workspace_bytes, void* stream) {
  if (!h) return fail(PPASR_EINVAL, "null argument");
  if (h->gemm_mode != PPASR_GEMM_F16X3 || !h->gemm_guard || !h->guard_dev)
    return encode_impl(h, feats, lens, B, T, probs, logits, frame_argmax, frame_maxprob, workspace, workspace_bytes, stream);
  // fp16 x3 mode, guard on: counters before / after the call's launches (stream order), one 16-byte read-back, and on a
  // changed counter the same call again on the fp32 kernels (same weights, same workspace; the inputs are untouched)
  hipStream_t st = static_cast<hipStream_t>(stream);
  constexpr int N = ppasr_model_s::kGuardN;
  PPASR_LAUNCH(k_h3_snapshot, dim3(1), dim3(1), 0, st, guard_ptrs(h), h->guard_dev);
  ppasr_status rc = encode_impl(h, feats, lens, B, T, probs, logits, frame_argmax, frame_maxprob, workspace, workspace_bytes, stream);
  if (rc != PPASR_OK) return rc;
  PPASR_LAUNCH(k_h3_snapshot, dim3(1), dim3(1), 0, st, guard_ptrs(h), h->guard_dev + N);
  HIP_TRY(hipMemcpyAsync(h->guard_host, h->guard_dev, 2 * N * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  long long events = 0;
  for (int i = 0; i < N; ++i) {
    h->guard_seen[i] = h->guard_host[N + i];
    events += (long long)(h->guard_host[N + i] - h->guard_host[i]);
  }
  if (events == 0) return PPASR_OK;
  h->guard_events += events;
  h->guard_fallbacks += 1;
  h->gemm_mode = PPASR_GEMM_F32;
  rc = encode_impl(h, feats, lens, B, T, probs, logits, frame_argmax, frame_maxprob, workspace, workspace_bytes, stream);
  h->gemm_mode = PPASR_GEMM_F16X3;
  return rc;
}

ppasr_status ppasr_set_gemm_guard(ppasr_handle h, int enable) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  h->gemm_guard = enable != 0;
  return PPASR_OK;
}

ppasr_status ppasr_gemm_guard_stats(ppasr_handle h, long long* fallbacks_host, long long* events_host) {
  if (!h) return fail(PPASR_EINVAL, "null handle");
  if (h->guard_dev) {  // (guard off: the events since this handle last looked -- a device-wide wait, then the counters)
    HIP_TRY(hipDeviceSynchronize());
    for (int i = 0; i < ppasr_model_s::kGuardN; ++i) {
      unsigned int now = 0;
      HIP_TRY(hipMemcpy(&now, h->guard_ctr[i], sizeof(unsigned int), hipMemcpyDeviceToHost));
      h->guard_events += (long long)(now - h->guard_seen[i]);
      h->guard_seen[i] = now;
    }
  }
  if (fallbacks_host) *fallbacks_host = h->guard_fallbacks;
  if (events_host) *events_host = h->guard_events;
  return PPASR_OK;
}

}  // extern "C"
