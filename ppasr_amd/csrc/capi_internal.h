// capi_internal.h -- definitions shared by the C-ABI translation units (capi*.hip)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/ppasr_hip.h"
#include "conformer_kernels.h"
#include "launch.h"
#include "ctc_beam.h"

using namespace ppasr;

#include "squeezeformer_kernels.h"
#include "ds2_kernels.h"
#include "rescore_kernels.h"

std::string& ppasr_err_slot();  // thread-local error string (defined in capi.hip)
inline ppasr_status fail(ppasr_status s, const std::string& msg) {
  ppasr_err_slot() = msg;
  return s;
}
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) return fail(PPASR_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// the session list of a many-session call (session groups, beam pools): every index in [0, n_sessions), none twice
inline bool session_list_ok(const int* sessions, int n, int n_sessions) {
  std::vector<char> seen(n_sessions, 0);
  for (int b = 0; b < n; ++b) {
    const int s = sessions[b];
    if (s < 0 || s >= n_sessions || seen[s]) return false;
    seen[s] = 1;
  }
  return true;
}

// Per-call staging of a many-session call (session-group descriptors, beam-pool slot tables): a ring of pinned host
// buffers and their device copies, each guarded by an event, so that a call never overwrites an entry an earlier (still
// queued) call reads.  A call acquires the next entry, fills its host side, copies it to the device, launches and then
// releases the entry behind its launches; a call that fails before its launches leaves the entry unreleased (nothing
// queued reads it).
struct StagingRing {
  static constexpr int kRing = 8;
  struct Entry {
    int i;
    char* host;
    char* dev;
  };
  size_t entry_bytes = 0;
  char* host = nullptr;   // pinned [kRing][entry_bytes]
  char* dev = nullptr;    // device [kRing][entry_bytes]
  hipEvent_t ev[kRing] = {};  // (null until created)
  int next = 0;

  hipError_t alloc(size_t bytes) {
    entry_bytes = bytes;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), kRing * bytes);
    if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&host), kRing * bytes, hipHostMallocDefault);
    for (int i = 0; i < kRing && e == hipSuccess; ++i) {
      e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
      if (e != hipSuccess) ev[i] = nullptr;
    }
    return e;
  }
  // the next entry, once the call that last used it has consumed it (no wait when it was never used)
  hipError_t acquire(Entry* out) {
    const int i = next;
    next = (i + 1) % kRing;
    *out = Entry{i, host + (size_t)i * entry_bytes, dev + (size_t)i * entry_bytes};
    return hipEventSynchronize(ev[i]);
  }
  hipError_t release(const Entry& en, hipStream_t st) { return hipEventRecord(ev[en.i], st); }
  // waits for every queued call, then frees whatever exists
  void destroy() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventSynchronize(e);
    (void)hipFree(dev);
    (void)hipHostFree(host);
    for (hipEvent_t& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// The rows of many streaming sessions in pages of one slab (ppasr_prob_arena_*, capi_align.hip): CTC tables (rows V wide)
// or encoder memory (rows 256 wide).  The page lists and the free list live here, on the host; a call uploads the part of
// them its launch needs through the ring.
struct ppasr_prob_arena_s {
  int n_sessions = 0, V = 0, P = 0, n_pages = 0;
  float* slab = nullptr;                 // device [n_pages][P][V]
  std::vector<std::vector<int>> pages;   // per session, in frame order
  std::vector<long long> frames;         // per session
  std::vector<int> free_list;            // (a stack: the page freed last is handed out first)
  StagingRing ring;
  // one call's table, int32: [n_sessions] first frame (append) or frame count (align, gather), [n_sessions] rows to append,
  // [n_sessions] page_off, then the page lists.  The sessions of a call are distinct, so the lists hold at most n_pages.
  size_t table_ints() const { return 3 * (size_t)n_sessions + (size_t)n_pages; }
  ~ppasr_prob_arena_s() {
    ring.destroy();
    (void)hipFree(slab);
  }
};
// An append in two halves, so that a caller with device work of its own in between stays all-or-nothing.
// arena_plan_append: the checks of a round of rows [n][c] (frames[k] of entry k, NULL: all c) -- the session list, the
// counts, the pages the round needs against the free ones; changes nothing.  *rows_out (may be null): the rows to append.
// arena_stage_append: a planned round takes its pages, moves the sessions' frame counts on and uploads the tables of
// launch_arena_append / launch_memory_append on `st`; the caller launches, then releases tab->en behind its launch.
struct ArenaAppendTab {
  const int32_t *first, *count, *page_off, *pages;  // device
  StagingRing::Entry en;
};
ppasr_status arena_plan_append(const ppasr_prob_arena_s* a, const int* sessions, int n, int c, const int* frames, const char* who,
                               long long* rows_out);
ppasr_status arena_stage_append(ppasr_prob_arena_s* a, const int* sessions, int n, int c, const int* frames, ArenaAppendTab* tab,
                                hipStream_t st);

struct Blob {
  const float* p;
  int ndim;
  int64_t shape[4];
  size_t numel() const {
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    return n;
  }
};

// Fragment-order packing of a [K][N] weight (y = x W): for 32-column tile nt, 8-wide k-group g,
// lane l: 4 consecutive floats = W[8g + 4(l>>5) + 0..3][32 nt + (l&31)].  One wave-level
// global_load_dwordx4 then yields the B operands of 4 successive v_mfma_f32_32x32x2_f32.
template <typename Acc>
inline std::vector<float> pack_b(int K, int N, Acc w) {
  const int n_tiles = (N + 31) / 32, G = K / 8;
  std::vector<float> out((size_t)n_tiles * G * 256, 0.f);
  for (int nt = 0; nt < n_tiles; ++nt)
    for (int g = 0; g < G; ++g)
      for (int l = 0; l < 64; ++l) {
        int n = nt * 32 + (l & 31);
        if (n >= N) continue;
        float* dst = &out[(((size_t)nt * G + g) * 64 + l) * 4];
        for (int j = 0; j < 4; ++j) dst[j] = w(8 * g + 4 * (l >> 5) + j, n);
      }
  return out;
}

// conv2 of Conv2dSubsampling4 in the quad form (front_fused.hip): K = 2 stages (128-channel half) x 16 slabs x 128
// channels, packed like pack_b.  Slab 4 ft + ff is the kh factor ft times the kw factor ff, each of w0, w1, w0 + w2, w2
// (the taps {0}, {1}, {0, 2}, {2}), summed in double.  w(k, n) is the direct form's accessor (k = (kh * 3 + kw) * 256 +
// cin, as conv2_w).
template <typename Acc>
inline std::vector<float> pack_conv2_quad(int d, Acc w) {
  static const int taps[4][2] = {{0, -1}, {1, -1}, {0, 2}, {2, -1}};
  return pack_b(32 * 128, d, [&](int k, int n) {
    const int h = k / 2048, slab = (k / 128) & 15, c = h * 128 + (k & 127);
    const int* th = taps[slab >> 2];
    const int* tw = taps[slab & 3];
    double v = 0.0;
    for (int a = 0; a < 2 && th[a] >= 0; ++a)
      for (int e = 0; e < 2 && tw[e] >= 0; ++e) v += (double)w((th[a] * 3 + tw[e]) * d + c, n);
    return (float)v;
  });
}

typedef std::unordered_map<std::string, Blob> BlobMap;

// Device memory a handle owns (model, language model, fbank tables): every block is freed with the handle
struct DeviceAllocs {
  std::vector<void*> allocs;
  ppasr_status alloc(size_t bytes, void** out) {
    HIP_TRY(hipMalloc(out, bytes));
    allocs.push_back(*out);
    return PPASR_OK;
  }
  ppasr_status upload_bytes(const void* src, size_t bytes, const void** out) {
    void* d = nullptr;
    ppasr_status s = alloc(bytes, &d);
    if (s != PPASR_OK) return s;
    HIP_TRY(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
    *out = d;
    return PPASR_OK;
  }
  ~DeviceAllocs() {
    for (void* p : allocs) (void)hipFree(p);
  }
};

// Efficient-Conformer: bit i = layer i is a stride-2 layer (ppasr_model_desc::stride_layer_mask, or the single
// stride_layer_idx of the shipped configuration)
inline unsigned eff_stride_mask(const ppasr_model_desc& d) {
  if (d.model_type != PPASR_MODEL_EFFICIENT_CONFORMER) return 0u;
  if (d.stride_layer_mask != 0) return (unsigned)d.stride_layer_mask;
  return d.stride_layer_idx >= 0 ? (1u << d.stride_layer_idx) : 0u;
}
inline int eff_strides_before(const ppasr_model_desc& d, int layer) {  // stride layers among layers 0 .. layer - 1
  return __builtin_popcount(eff_stride_mask(d) & ((1u << layer) - 1u));
}

struct ppasr_model_s : DeviceAllocs {
  ppasr_model_desc desc;
  int F1, F2;
  // general layer route (capi_generic.hip): CTC head as a dense layer over the padded vocabulary
  const f32x4* gen_head_w = nullptr;
  const float* gen_head_b = nullptr;
  int gen_vpad = 0;
  int F3 = 0;  // conv2d8: feature bins behind the third conv (F2 behind the second); 0 otherwise
  // front-end geometry for T input frames (Conv2dSubsampling4 / 6 / 8, subsampling.py): frames behind conv1, behind the
  // intermediate conv (conv2d8 only, else 0) and encoder frames; F_last = feature bins entering the linear layer
  struct Front {
    int T1, T2, Tp;
  };
  int sub_rate() const { return desc.input_layer == 1 ? 1 : desc.input_layer ? desc.input_layer : 4; }
  int F_last() const { return desc.input_layer == 8 ? F3 : F2; }
  int min_frames() const { return desc.input_layer == 1 ? 1 : desc.input_layer == 6 ? 11 : desc.input_layer == 8 ? 15 : 7; }
  Front front_dims(int T) const {
    if (desc.input_layer == 1) return Front{0, 0, T};  // LinearNoSubsampling: one encoder frame per feature frame
    Front f{(T - 1) / 2, 0, 0};
    if (desc.input_layer == 6) {
      f.Tp = (f.T1 - 5) / 3 + 1;
    } else if (desc.input_layer == 8) {
      f.T2 = (f.T1 - 1) / 2;
      f.Tp = (f.T2 - 1) / 2;
    } else {
      f.Tp = (f.T1 - 1) / 2;
    }
    return f;
  }
  // ---- general layer route (capi_generic.hip): any width that is a multiple of 256 and every ConformerEncoder
  // constructor option (ppasr_model_desc::options, input_layer = linear, any conv kernel size) ----
  bool generic = false;
  struct GenOpts {
    int pos = 0;  // PPASR_OPT_POS_*
    bool post_norm = false, concat_after = false, macaron = true, use_cnn = true;
    int act = 0;  // PPASR_ACT_*
    bool sq_pre_norm = false;  // Squeezeformer normalize_before = True
  } gen;
  struct GenLayerX {  // what LayerW has no slot for
    const f32x4* wcat = nullptr;  // concat_linear [2d][d], packed
    const float* bcat = nullptr;
  };
  std::vector<GenLayerX> gen_x;
  const float* pe_dev = nullptr;    // positional table [max_len][d] (abs_pos adds it to the embedded frames)
  const float* zero_vec = nullptr;  // [d] zeros: pos_bias_u / _v and the one-row "positional table" of MultiHeadedAttention
  const float *lin_ln_g = nullptr, *lin_ln_b = nullptr;  // LinearNoSubsampling's LayerNorm (eps 1e-12)
  int lin_kpad = 0;                                      //   and its input width padded to whole 256-wide K chunks
  FrontW front;
  std::vector<LayerW> layers;
  std::vector<int> layer_ks;     // depthwise kernel size per layer (Efficient-Conformer halves it after the stride layer)
  std::vector<int> layer_group;  // 1, or 3 on grouped-attention layers
  HeadW head;
  // Squeezeformer (model_type == PPASR_MODEL_SQUEEZEFORMER)
  std::vector<SqLayerW> sq_layers;
  SqReduceW sq_reduce{};
  const f32x4* sq_wrec = nullptr;
  const float* sq_brec = nullptr;
  const float *preln_g = nullptr, *preln_b = nullptr;
  // DeepSpeech2 (model_type == PPASR_MODEL_DEEPSPEECH2)
  Ds2W ds2{};
  // single utterances: the recurrence of a layer as one persistent launch.  It needs every workgroup of its grid resident at
  // once; when a launch gives up (the chip was shared) the next `ds2_persist_hold` calls take the per-step kernels, then the
  // route is tried again (hold doubles with every give-up, 64 .. 1 024 calls)
  int ds2_persist_hold = 0, ds2_persist_giveups = 0;
  std::vector<Ds2LayerW> ds2_layers;
  float* taps = nullptr;
  size_t taps_floats = 0;
  float* memory_out = nullptr;  // ppasr_set_memory_out: the encoder output of offline encodes, [B][T'][D]
  size_t memory_floats = 0;
  bool sq_final_proj = false;  // Squeezeformer with final_proj: folded into the CTC head, its output rows are never formed
  // optional per-kernel timing (bench.py roofline leg): one event pair per launch on the caller's stream
  bool prof = false;
  int front_fused = -1;  // ppasr_set_front_fused: -1 / 1 = conv1 + conv2 of the 4x front end as one launch, 0 = two launches
  int ffn_split = -1;  // ppasr_set_ffn_split: -1 = by grid size, 0 = never, 2 / 4 / 8 = always that many slices
  bool skip_padding = false;  // ppasr_set_skip_padding: ragged batches compute only the rows valid outputs depend on
  int gemm_mode = 0;          // ppasr_set_gemm_mode: PPASR_GEMM_F32 / PPASR_GEMM_F16X3 (feed-forward GEMMs, csrc/h3.h)
  std::vector<LayerW> layers_h3;  // layers[] with the FFN weight pointers replaced by their fp16 x3 re-packing
  const f32x4* conv2_w_h3 = nullptr;  // the 4x front end's second convolution, re-packed likewise
  const f32x4* embed_w_h3 = nullptr;  // ... and its input projection
  const f32x4* head_w_h3 = nullptr;   // the CTC head's weight [256][32 * n_tiles]
  std::vector<SqLayerW> sq_layers_h3;  // Squeezeformer: sq_layers[] with the two feed-forward modules' weights re-packed
  // the fp16 x3 mode is on and this family's layers have their re-packed views
  bool h3_layers() const { return gemm_mode == PPASR_GEMM_F16X3 && !layers_h3.empty(); }
  bool h3_sq_layers() const { return gemm_mode == PPASR_GEMM_F16X3 && !sq_layers_h3.empty(); }
  int gemm_coverage = 0;      // PPASR_GEMM_COVERS_* of the current mode (ppasr_gemm_coverage)
  // range guard of the fp16 x3 mode (csrc/h3.h, ppasr_set_gemm_guard / ppasr_gemm_guard_stats)
  bool gemm_guard = true;
  static constexpr int kGuardN = 5;                 // translation units with fp16 x3 kernels (h3.h: one event counter each)
  unsigned int* guard_ctr[kGuardN] = {};            // device addresses of their counters
  unsigned int* guard_dev = nullptr;                // [kGuardN counters before the call | kGuardN after]
  unsigned int* guard_host = nullptr;               // pinned mirror
  unsigned int guard_seen[kGuardN] = {};            // counter values this handle last read
  long long guard_fallbacks = 0, guard_events = 0;
  int row_block = -1;         // ppasr_set_row_block: -1 = by grid size, 32 / 16 / kW16 = always that block form (rbt.h)
  std::vector<int64_t> lens_hint;  // ppasr_set_lengths_hint: host copy of the batch's lengths (route selection only)
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  struct Span { int cls; std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; };  // one pair per kernel launched inside the span
  std::vector<Span> spans;

  ppasr_status upload(const std::vector<float>& v, const float** out) {
    return upload_bytes(v.data(), v.size() * sizeof(float), reinterpret_cast<const void**>(out));
  }
  ppasr_status upload4(const std::vector<float>& v, const f32x4** out) {
    return upload_bytes(v.data(), v.size() * sizeof(float), reinterpret_cast<const void**>(out));
  }
  hipEvent_t next_event() {
    if (ev_used == ev_pool.size()) {
      hipEvent_t e;
      (void)hipEventCreate(&e);
      ev_pool.push_back(e);
    }
    return ev_pool[ev_used++];
  }
  ~ppasr_model_s() {
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (guard_host) (void)hipHostFree(guard_host);
  }
};


// streaming state of one session (capi_stream.hip; the general route of capi_generic.hip shares it)
struct ppasr_stream_s {
  ppasr_model_s* m;
  int D;        // model width = row stride of the caches (256 on the fused route)
  int cap;      // key capacity per layer (frames)
  int cache_t;  // cached key/value frames of the full-rate layers (cache_t1 in the reference)
  int cache_r;  // frames held by the half-rate layers
  int offset;   // encoder-output frames emitted so far (the reference's `offset` argument)
  int lo;       // longest conv left context = cnn_module_kernel - 1
  float *kc, *vc;   // [L][cap][D]
  float* xh_hist;   // [L][lo][D]  conv-module input history
  float* g_hist;    // [L][lo][256] GLU(pointwise_conv1(history)) of every layer, recomputed at the start of each chunk (fused route)
  HistLayer* hist_tab;  // device [L]: per-layer pointwise_conv1 weights / history rows for that launch (fused route)
};

// the reference's shape arithmetic for one chunk (capi_stream.hip: plan_chunk)
struct ChunkPlan {
  int c;        // full-rate frames of this chunk
  int c_r;      // half-rate frames
  int used_r;   // half-rate cache frames that take part
  int T2, T2_r; // keys of the full-rate / half-rate layers
  int ncs;      // next_cache_start
  int pos0;     // position of key 0
};

struct WsLayout {
  size_t y1, y2, xa, xb, xc, qkv, ctx, g, rmax, rsum, fa, fp, xs, vt, total;  // offsets in floats
  int vt_stride;  // row stride of the transposed values (fused attention route)
};
WsLayout ws_layout(const ppasr_model_s* m, int B, int T);
// hidden-dimension slices per row block for M rows (1 = the fused kernels), see ppasr_set_ffn_split
int ffn_split_for(const ppasr_model_s* m, int M);
int wide_slices_for(const ppasr_model_s* m, int M, int units);  // embed K chunks / head tile groups on the split route
// rows per workgroup (32 or 16) for a row-block launch over B utterances of Tcur rows each: 16 when the rows that will
// actually be computed fill at most half of the chip as 32-row blocks.  With skip_padding the computed rows are
// sum_b min(Tcur, ceil(len_b / mul) + slack) -- known on the host only through ppasr_set_lengths_hint; without a hint the
// padded count decides.
int row_block_for(const ppasr_model_s* m, int B, int Tcur, int mul, int slack, bool skip);
bool block_tables_enabled();  // active-block lists for ragged layer kernels (PPASR_BLOCK_TABLE=0: padded grids; A/B switch)
// the 4x front end as one launch (front_fused.hip)?  ppasr_set_front_fused
bool conv12_enabled(const ppasr_model_s* m);
ppasr::LayerW sq_conv_view(const ppasr::SqLayerW& W);  // capi_squeezeformer.hip

// general Conformer layer route (widths 512 / 768 / 1024, non-default constructor options): capi_generic.hip
size_t generic_ws_floats(const ppasr_model_s* m, int B, int T);
ppasr_status generic_encode(ppasr_model_s* h, const float* feats, const int64_t* lens, int B, int T, float* probs,
                            float* logits, int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st);
// one chunk of ConformerEncoder / EfficientConformerEncoder.forward_chunk (conformer/encoder.py:208-283,
// efficient_conformer/encoder.py:266-393) on the general route: the caches of `s` hold cache_t (cache_r behind the stride
// layer) frames, key 0 sits at positional row p.pos0; appends this chunk's keys / values and conv inputs
ppasr_status generic_chunk(ppasr_stream_s* s, const ChunkPlan& p, const float* feats, int T, float* probs,
                           int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st, int* frames_out);
// SqueezeformerEncoder.forward_chunk (squeezeformer/encoder.py:260-381) on the general route
ppasr_status generic_sq_chunk(ppasr_stream_s* s, const ChunkPlan& p, const float* feats, int T, float* probs,
                              int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st);
// session groups on the general route (ppasr_gen_stream_group_create): workspace of a round of n chunks of T frames, and the
// round itself -- gen_front + gen_layers over the n stacked chunks, session sess[b] (device) for chunk b; caches kc / vc
// [n_sessions][L][cap][D], conv histories xh_hist [n_sessions][L][lo][D]
size_t generic_group_ws_floats(const ppasr_model_s* m, int n, int T);
ppasr_status generic_group_chunk(ppasr_model_s* h, const SessDesc* sess, int n, float* kc, float* vc, int cap,
                                 float* xh_hist, int lo, const float* feats, int T, float* probs, int32_t* frame_argmax,
                                 float* frame_maxprob, float* ws, hipStream_t st);
hipError_t configure_generic_kernels();
// SqueezeformerEncoder.forward (squeezeformer/encoder.py:172-236) on the general route (encoder_dim 512 / 768 / 1024)
ppasr_status generic_sq_encode(ppasr_model_s* h, const float* feats, const int64_t* lens, int B, int T, float* probs,
                               float* logits, int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st);

// model-family back ends: each turns the checkpoint behind `ld` (weights.h) into the device memory of `m`
struct Loader;
ppasr_status conformer_create(ppasr_model_s* m, Loader& ld);  // capi_conformer.hip
ppasr_status ds2_create(ppasr_model_s* m, Loader& ld);
// DeepSpeech2 session groups (capi_ds2.hip): workspace of a round of n windows of T frames, and the round itself
size_t ds2_group_ws_floats(const ppasr_model_s* m, int n, int T);
ppasr_status ds2_group_round(ppasr_model_s* h, const int* slots, int n, const float* feats, int T, float* state_h,
                             float* state_c, float* probs, int32_t* frame_argmax, float* frame_maxprob, float* ws,
                             hipStream_t st);
ppasr_status squeezeformer_create(ppasr_model_s* m, Loader& ld);
ppasr_status squeezeformer_encode(ppasr_model_s* h, const float* feats, const int64_t* lens, int B, int T, float* probs,
                                  float* logits, int32_t* frame_argmax, float* frame_maxprob, float* ws,
                                  const WsLayout& wl, hipStream_t st);

#include "encode_common.h"
#include "weights.h"
