// capi_decode.hip -- the decoders' C-ABI (declared in include/ppasr_hip.h): CTC prefix beam search and the beam pools of
// session groups (ctc_beam.hip), the greedy decoder, the hypothesis records of the data-parallel path, edit distance.
#include "capi_internal.h"

extern "C" {

long long ppasr_edit_distance(const int32_t* a, int na, const int32_t* b, int nb) {
  if (na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b)) return -1;
  if (na < nb) {
    std::swap(a, b);
    std::swap(na, nb);
  }
  if (nb == 0) return na;
  std::vector<int> prev(nb + 1), cur(nb + 1);
  for (int j = 0; j <= nb; ++j) prev[j] = j;
  for (int i = 1; i <= na; ++i) {
    cur[0] = i;
    const int32_t ca = a[i - 1];
    for (int j = 1; j <= nb; ++j) {
      const int sub = prev[j - 1] + (ca != b[j - 1]);
      const int del = prev[j] + 1, ins = cur[j - 1] + 1;
      cur[j] = sub < del ? (sub < ins ? sub : ins) : (del < ins ? del : ins);
    }
    std::swap(prev, cur);
  }
  return prev[nb];
}

// =====================================================================================
// CTC prefix beam search (see ctc_beam.hip)
// =====================================================================================
static ppasr_status beam_config(int V, int beam_size, double cutoff_prob, int cutoff_top_n, int blank, int nbest,
                                int max_tokens, BeamConfig* c) {
  if (V <= 1 || V >= 16384) return fail(PPASR_EUNSUPPORTED, "beam search: vocabulary must be in (1, 16384)");
  if (beam_size < 1 || beam_size > kMaxBeam) return fail(PPASR_EUNSUPPORTED, "beam search: beam_size must be in [1, 512]");
  if (blank < 0 || blank >= V) return fail(PPASR_EINVAL, "beam search: blank id out of range");
  if (nbest < 1 || nbest > beam_size || max_tokens < 1) return fail(PPASR_EINVAL, "beam search: bad nbest / max_tokens");
  if (cutoff_top_n < 1) return fail(PPASR_EINVAL, "beam search: cutoff_top_n < 1");
  // candidates per frame: pruned to cutoff_top_n only when cutoff_prob < 1 (upstream get_pruned_log_probs); with
  // cutoff_prob >= 1 -- the default of the reference's wrappers, swig_wrapper.py:38,71 -- upstream keeps EVERY character
  // (sorted when cutoff_top_n < V, in vocabulary order otherwise), and so does the kernel: wide records and the element
  // lists they produce go through HBM scratch (ppasr_ctc_beam_scratch_bytes)
  const int n_cand = (cutoff_prob < 1.0) ? (cutoff_top_n < V ? cutoff_top_n : V) : V;
  c->V = V; c->beam = beam_size; c->blank = blank; c->cutoff_top_n = cutoff_top_n; c->cutoff_prob = cutoff_prob;
  c->n_cand_max = n_cand; c->nbest = nbest; c->max_tokens = max_tokens; c->max_nodes = 0;
  c->sorted = (cutoff_prob < 1.0 || cutoff_top_n < V) ? 1 : 0;
  {
    const char* m = getenv("PPASR_BEAM_MARGIN");  // (tuning knob: rows of the clipped element list, ctc_beam.hip)
    c->margin = m ? atoi(m) : 2;
    if (c->margin < 0) c->margin = 0;
  }
  c->list_cap = beam_list_cap(beam_size, V, n_cand, c->lm.order > 0);
  if (c->list_cap <= 0) return fail(PPASR_EUNSUPPORTED, "beam search: beam_size x vocabulary does not fit LDS");
  return PPASR_OK;
}

// state buffer = B x [header | beam arrays | arena of 1 + (F+1)*beam nodes | node table] | B status words | scratch of the
// pruning pre-pass (B x F frame records of the largest record size), F = max_frames.  The layout is recomputed from
// (state_bytes, B, beam_size) on every call, so it is the same for every chunk of a streaming decode.

// bytes of one utterance's share of the state buffer for a capacity of F frames: state block (ctc_beam.h: header, beam
// arrays, arena and node table for max_nodes = 1 + (F + 1) * beam nodes) + its status word + F pruning records
static size_t beam_max_nodes(size_t F, int beam_size) { return 1 + (F + 1) * (size_t)beam_size; }
static size_t beam_utt_bytes(size_t F, int beam_size) {
  return 4 * beam_state_words(beam_size, (int)beam_max_nodes(F, beam_size)) + 4 + F * 4 * (size_t)prune_rec_words(kSmallCand);
}
// frame capacity a state buffer of `per_utt_bytes` per utterance was sized for (0: too small for one frame)
static size_t beam_frame_capacity(size_t per_utt_bytes, int beam_size) {
  if (per_utt_bytes < beam_utt_bytes(1, beam_size)) return 0;
  const size_t per_frame = beam_utt_bytes(2, beam_size) - beam_utt_bytes(1, beam_size);
  size_t F = 1 + (per_utt_bytes - beam_utt_bytes(1, beam_size)) / per_frame;
  while (F > 1 && beam_utt_bytes(F, beam_size) > per_utt_bytes) --F;  // (the fixed part is padded to an even word)
  return F;
}

size_t ppasr_ctc_beam_state_bytes(int B, int max_frames, int beam_size) {
  if (B <= 0 || max_frames < 0 || beam_size < 1) return 0;
  return (size_t)B * beam_utt_bytes((size_t)(max_frames < 1 ? 1 : max_frames), beam_size);
}

}  // extern "C"
namespace ppasr { const LmDev* lm_device_view(ppasr_lm_handle lm); }  // lm.hip (internal: C++ linkage, not exported)
extern "C" {

ppasr_status ppasr_ctc_beam_search(const float* probs, const int32_t* frame_lens, int B, int T, int V, int beam_size,
                                   double cutoff_prob, int cutoff_top_n, int blank, int nbest, int max_tokens,
                                   int32_t* tokens, int32_t* lens, double* scores, void* state, size_t state_bytes,
                                   int init_state, void* stream) {
  return ppasr_ctc_beam_search_lm(probs, frame_lens, B, T, V, beam_size, cutoff_prob, cutoff_top_n, blank, nbest, max_tokens,
                                  tokens, lens, scores, state, state_bytes, init_state, nullptr, 0.0, 0.0, stream);
}

ppasr_status ppasr_ctc_beam_search_lm(const float* probs, const int32_t* frame_lens, int B, int T, int V, int beam_size,
                                      double cutoff_prob, int cutoff_top_n, int blank, int nbest, int max_tokens,
                                      int32_t* tokens, int32_t* lens, double* scores, void* state, size_t state_bytes,
                                      int init_state, ppasr_lm_handle lm, double alpha, double beta, void* stream) {
  return ppasr_ctc_beam_search_ws(probs, frame_lens, B, T, V, beam_size, cutoff_prob, cutoff_top_n, blank, nbest, max_tokens,
                                  tokens, lens, scores, state, state_bytes, init_state, lm, alpha, beta, nullptr, 0, stream);
}

size_t ppasr_ctc_beam_scratch_bytes(int B, int T, int V, int beam_size, double cutoff_prob, int cutoff_top_n) {
  BeamConfig c{};
  if (B <= 0 || T < 0) return 0;
  c.lm.order = 1;  // sized for a search WITH a scorer (its context summaries take LDS from the element list): enough for both
  if (beam_config(V, beam_size, cutoff_prob, cutoff_top_n, 0, 1, 1, &c) != PPASR_OK) return 0;
  return beam_scratch_bytes(c, B, T);
}

ppasr_status ppasr_ctc_beam_search_ws(const float* probs, const int32_t* frame_lens, int B, int T, int V, int beam_size,
                                      double cutoff_prob, int cutoff_top_n, int blank, int nbest, int max_tokens,
                                      int32_t* tokens, int32_t* lens, double* scores, void* state, size_t state_bytes,
                                      int init_state, ppasr_lm_handle lm, double alpha, double beta, void* scratch,
                                      size_t scratch_bytes, void* stream) {
  if (!tokens || !lens || !scores || !state || (!probs && T > 0)) return fail(PPASR_EINVAL, "null argument");
  if (B <= 0 || T < 0) return fail(PPASR_EINVAL, "empty batch");
  BeamConfig c{};
  if (lm) {  // before beam_config: the LDS budget depends on it
    c.lm = *ppasr::lm_device_view(lm);
    c.alpha = alpha;
    c.beta = beta;
  }
  ppasr_status s = beam_config(V, beam_size, cutoff_prob, cutoff_top_n, blank, nbest, max_tokens, &c);
  if (s != PPASR_OK) return s;
  c.node_table = lm && c.lm.word_based;
  {
    const char* f = getenv("PPASR_BEAM_FAST");  // (read per call: the tests run both selections in one process)
    c.fast_path = f ? (atoi(f) != 0) : 1;
  }
  const size_t per_utt_bytes = state_bytes / (size_t)B;
  const size_t F = beam_frame_capacity(per_utt_bytes, beam_size);
  if (F == 0) return fail(PPASR_ENOSPACE, "beam search: state buffer too small");
  if ((size_t)T > F) return fail(PPASR_ENOSPACE, "beam search: more frames in one call than the state buffer was sized for");
  c.max_nodes = (int)beam_max_nodes(F, beam_size);
  const size_t block_words = beam_state_words(beam_size, c.max_nodes);
  int32_t* st_words = static_cast<int32_t*>(state);
  int32_t* status = st_words + (size_t)B * block_words;
  int32_t* prune_recs = status + B;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  if (init_state) {
    HIP_TRY(hipMemsetAsync(status, 0, (size_t)B * 4, hs));
    // empty node tables (the kernel enters every prefix it creates) -- only where the search uses them: the default route
    // of scorer-less / character-LM searches never reads the table, and clearing 24 bytes per node per call is tens of MB
    // of memset on the latency-bound decoder path
    if (c.node_table) {
    const size_t tab_off = (beam_fixed_words(beam_size) + beam_arena_words(c.max_nodes)) * 4, tab_bytes = 12 * beam_table_slots(c.max_nodes);
    HIP_TRY(hipMemset2DAsync(reinterpret_cast<char*>(state) + tab_off, block_words * 4, 0, tab_bytes, (size_t)B, hs));
    }
  }
  const size_t need_scratch = beam_scratch_bytes(c, B, T);
  if (need_scratch > 0 && (!scratch || scratch_bytes < need_scratch))
    return fail(PPASR_ENOSPACE, "beam search: this pruning configuration keeps more characters per frame than the LDS-resident "
                                "search holds (cutoff_prob >= 1 keeps the whole vocabulary): call ppasr_ctc_beam_search_ws with "
                                "ppasr_ctc_beam_scratch_bytes(...) bytes of device scratch");
  HIP_TRY(launch_ctc_beam(probs, frame_lens, B, T, c, prune_recs, st_words, init_state, 1, tokens, lens, scores, status,
                          need_scratch ? scratch : nullptr, hs));
  return PPASR_OK;
}

// State layout: B blocks of (fixed + 2 * max_nodes) words (beam arrays, then the parent-pointer arena, node ids in
// creation order), B status words, the per-call pruning records.  A larger buffer therefore holds the same search once
// every block's words sit at the start of the new, longer block (the arena simply has room for more nodes behind them).
ppasr_status ppasr_ctc_beam_state_grow(const void* old_state, size_t old_bytes, void* new_state, size_t new_bytes, int B,
                                       int beam_size, void* stream) {
  if (!old_state || !new_state || B <= 0 || beam_size < 1) return fail(PPASR_EINVAL, "null argument");
  const size_t Fo = beam_frame_capacity(old_bytes / (size_t)B, beam_size), Fn = beam_frame_capacity(new_bytes / (size_t)B, beam_size);
  if (Fo == 0 || Fn == 0) return fail(PPASR_ENOSPACE, "beam search: state buffer too small");
  if (Fn < Fo) return fail(PPASR_EINVAL, "beam search: the new state buffer is smaller than the old one");
  const int mo = (int)beam_max_nodes(Fo, beam_size), mn = (int)beam_max_nodes(Fn, beam_size);
  const size_t ow = beam_state_words(beam_size, mo), nw = beam_state_words(beam_size, mn);
  const size_t head_words = beam_fixed_words(beam_size) + beam_arena_words(mo);  // header, beam arrays, arena: same offsets in both
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const int32_t* o = static_cast<const int32_t*>(old_state);
  int32_t* n = static_cast<int32_t*>(new_state);
  HIP_TRY(hipMemcpy2DAsync(n, nw * 4, o, ow * 4, head_words * 4, (size_t)B, hipMemcpyDeviceToDevice, hs));
  HIP_TRY(hipMemcpyAsync(n + (size_t)B * nw, o + (size_t)B * ow, (size_t)B * 4, hipMemcpyDeviceToDevice, hs));  // status
  // the node table is rebuilt for the new size from the arena (every node but the root is an entry)
  const size_t tab_off = (beam_fixed_words(beam_size) + beam_arena_words(mn)) * 4, tab_bytes = 12 * beam_table_slots(mn);
  HIP_TRY(hipMemset2DAsync(reinterpret_cast<char*>(new_state) + tab_off, nw * 4, 0, tab_bytes, (size_t)B, hs));
  HIP_TRY(launch_beam_rehash(n, B, beam_size, mn, hs));
  return PPASR_OK;
}

// Streaming callers of the C-ABI: the kernel flags an utterance whose prefix arena ran out (more cumulative frames than
// the state buffer was sized for) in a status word of the state buffer; this reads the B words back (synchronises the
// stream) and returns PPASR_ENOSPACE if any is set -- the hypotheses of that utterance are then truncated.
ppasr_status ppasr_ctc_beam_status(const void* state, size_t state_bytes, int B, int beam_size, int32_t* status_host,
                                   void* stream) {
  if (!state || B <= 0 || beam_size < 1) return fail(PPASR_EINVAL, "null argument");
  const size_t F = beam_frame_capacity(state_bytes / (size_t)B, beam_size);
  if (F == 0) return fail(PPASR_ENOSPACE, "beam search: state buffer too small");
  const int32_t* status = static_cast<const int32_t*>(state) + (size_t)B * beam_state_words(beam_size, (int)beam_max_nodes(F, beam_size));
  std::vector<int32_t> host(B);
  hipStream_t hs = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(host.data(), status, (size_t)B * 4, hipMemcpyDeviceToHost, hs));
  HIP_TRY(hipStreamSynchronize(hs));
  bool any = false;
  for (int b = 0; b < B; ++b) {
    if (status_host) status_host[b] = host[b];
    any |= host[b] != 0;
  }
  if (any) return fail(PPASR_ENOSPACE, "beam search: the prefix arena of at least one utterance is exhausted (state sized for fewer frames)");
  return PPASR_OK;
}

// Compaction of a streaming state buffer (ctc_beam.h: launch_beam_compact).  The live counts are the blocks' own st[1]
// afterwards (-1 where the status word is set), so the read-back needs no device array of its own.
ppasr_status ppasr_ctc_beam_state_compact(void* state, size_t state_bytes, int B, int beam_size, int rebuild_table,
                                          int32_t* live_nodes_host, void* stream) {
  if (!state || B <= 0 || beam_size < 1 || beam_size > kMaxBeam) return fail(PPASR_EINVAL, "beam search: null state, B <= 0 or bad beam_size");
  const size_t F = beam_frame_capacity(state_bytes / (size_t)B, beam_size);
  if (F == 0) return fail(PPASR_EINVAL, "beam search: state buffer too small for one frame");
  const int max_nodes = (int)beam_max_nodes(F, beam_size);
  const size_t block_words = beam_state_words(beam_size, max_nodes);
  int32_t* st_words = static_cast<int32_t*>(state);
  const int32_t* status = st_words + (size_t)B * block_words;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  HIP_TRY(launch_beam_compact(st_words, status, B, beam_size, max_nodes, rebuild_table != 0, nullptr, hs));
  if (!live_nodes_host) return PPASR_OK;
  std::vector<int32_t> stat(B);
  HIP_TRY(hipMemcpy2DAsync(live_nodes_host, 4, st_words + 1, block_words * 4, 4, (size_t)B, hipMemcpyDeviceToHost, hs));
  HIP_TRY(hipMemcpyAsync(stat.data(), status, (size_t)B * 4, hipMemcpyDeviceToHost, hs));
  HIP_TRY(hipStreamSynchronize(hs));
  for (int b = 0; b < B; ++b)
    if (stat[b] != 0) live_nodes_host[b] = -1;
  return PPASR_OK;
}

// ---- beam-search session pools (include/ppasr_hip.h: ppasr_beam_pool_*) ----
// Every session owns its state block (ctc_beam.h layout, sized for its own frame capacity) and a status word; a decode
// call builds a slot table of the listed sessions' blocks (by list position) and runs the pruning pre-pass and the search
// once for all of them.  Growth is planned on the host from the sessions' frame counters before anything is launched.
struct ppasr_beam_pool_s {
  BeamConfig cfg;  // shared configuration (max_nodes / max_tokens / fast_path set per call)
  int n_sessions;
  std::vector<int32_t*> block;   // device state block of each session
  std::vector<size_t> cap;       // frames each block is sized for
  std::vector<long long> frames; // cumulative frames decoded since the session's last reset
  // frame-equivalents of the arena in use -- what the capacity check compares: n_nodes <= 1 + used * beam.  A decode of f
  // frames adds f, a reset sets 0, a compaction that found L live nodes sets ceil((L - 1) / beam); == frames without one
  std::vector<long long> used;
  std::vector<long long> live;   // node count read back at the session's last compaction (0: none since its reset)
  bool auto_compact = false;     // ppasr_beam_arena_set_auto
  int32_t* status;               // device [n_sessions]
  // per-call slot tables + frame counts (a compaction: live counts): [n_sessions] BeamSlot, then [n_sessions] int32 per entry
  StagingRing ring;
};

namespace {
size_t pool_block_bytes(size_t F, int beam) { return 4 * beam_state_words(beam, (int)beam_max_nodes(F, beam)); }
size_t pool_rec_bytes(const BeamConfig& c, int n, int T) {  // narrow pruning records (wide ones live in the scratch)
  return c.n_cand_max > kSmallCand ? 0 : (((size_t)n * T * prune_rec_words(c.n_cand_max) * 4 + 255) & ~(size_t)255);
}
// largest capacity whose arena node count still fits the kernel's int arithmetic
bool pool_cap_ok(size_t F, int beam) { return F <= (size_t)(0x3fffffff / beam) - 2; }

// One compaction launch for the n listed sessions (checked by the caller): slot table up, live counts back, ONE
// synchronisation of `hs`, then the accounting -- used = ceil((L - 1) / beam), so that n_nodes <= 1 + used * beam still
// holds.  An exhausted session (count -1) was left as it is and keeps its accounting.  live_out [n] or null.
ppasr_status pool_compact(ppasr_beam_pool_s* p, const int* sessions, int n, long long* live_out, hipStream_t hs) {
  StagingRing::Entry en;
  HIP_TRY(p->ring.acquire(&en));
  BeamSlot* tab = reinterpret_cast<BeamSlot*>(en.host);
  const int beam = p->cfg.beam;
  for (int b = 0; b < n; ++b) {
    const int s = sessions[b];
    tab[b] = BeamSlot{p->block[s], p->status + s, (int)beam_max_nodes(p->cap[s], beam), 0};
  }
  const size_t live_off = (size_t)n * sizeof(BeamSlot);
  HIP_TRY(hipMemcpyAsync(en.dev, en.host, live_off, hipMemcpyHostToDevice, hs));
  HIP_TRY(launch_beam_compact(nullptr, nullptr, n, beam, 0, p->cfg.node_table, reinterpret_cast<int32_t*>(en.dev + live_off), hs,
                              reinterpret_cast<const BeamSlot*>(en.dev)));
  HIP_TRY(hipMemcpyAsync(en.host + live_off, en.dev + live_off, (size_t)n * 4, hipMemcpyDeviceToHost, hs));
  HIP_TRY(hipStreamSynchronize(hs));
  HIP_TRY(p->ring.release(en, hs));
  const int32_t* live = reinterpret_cast<const int32_t*>(en.host + live_off);
  for (int b = 0; b < n; ++b) {
    const int s = sessions[b];
    if (live[b] >= 1) {
      p->live[s] = live[b];
      p->used[s] = ((long long)live[b] - 1 + beam - 1) / beam;
    }
    if (live_out) live_out[b] = live[b];
  }
  return PPASR_OK;
}
}  // namespace

ppasr_status ppasr_beam_pool_create(int n_sessions, int V, int beam_size, double cutoff_prob, int cutoff_top_n, int blank,
                                    ppasr_lm_handle lm, double alpha, double beta, int init_frames, ppasr_beam_pool* out) {
  if (!out) return fail(PPASR_EINVAL, "null argument");
  *out = nullptr;
  if (n_sessions < 1 || init_frames < 1) return fail(PPASR_EINVAL, "beam pool: n_sessions and init_frames must be >= 1");
  BeamConfig c{};
  if (lm) {  // before beam_config: the LDS budget depends on it
    c.lm = *ppasr::lm_device_view(lm);
    c.alpha = alpha;
    c.beta = beta;
  }
  ppasr_status s = beam_config(V, beam_size, cutoff_prob, cutoff_top_n, blank, 1, 1, &c);
  if (s != PPASR_OK) return s;
  if (!pool_cap_ok((size_t)init_frames, beam_size)) return fail(PPASR_EINVAL, "beam pool: init_frames too large");
  c.node_table = lm && c.lm.word_based;
  auto* p = new ppasr_beam_pool_s();  // (value-initialised: every pointer and event null until it exists)
  p->cfg = c;
  p->n_sessions = n_sessions;
  p->block.assign(n_sessions, nullptr);
  p->cap.assign(n_sessions, (size_t)init_frames);
  p->frames.assign(n_sessions, 0);
  p->used.assign(n_sessions, 0);
  p->live.assign(n_sessions, 0);
  auto bail = [p](const char* what, hipError_t e) {
    (void)ppasr_beam_pool_destroy(p);
    return fail(PPASR_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  const size_t bb = pool_block_bytes((size_t)init_frames, beam_size);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->status), (size_t)n_sessions * 4);
  for (int i = 0; i < n_sessions && e == hipSuccess; ++i) e = hipMalloc(reinterpret_cast<void**>(&p->block[i]), bb);
  if (e == hipSuccess) e = p->ring.alloc(((size_t)n_sessions * (sizeof(BeamSlot) + 4) + 255) & ~(size_t)255);
  if (e != hipSuccess) return bail("allocation failed for the beam pool", e);
  for (int i = 0; i < n_sessions; ++i) {
    e = launch_beam_reset(p->block[i], p->status + i, beam_size, (int)beam_max_nodes(p->cap[i], beam_size), c.lm.bos,
                          c.node_table != 0, nullptr);
    if (e != hipSuccess) return bail("initialising the beam-pool sessions failed", e);
  }
  e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) return bail("initialising the beam-pool sessions failed", e);
  *out = p;
  return PPASR_OK;
}

ppasr_status ppasr_beam_pool_destroy(ppasr_beam_pool p) {
  if (!p) return fail(PPASR_EINVAL, "null pool");
  p->ring.destroy();
  for (int32_t* b : p->block)
    if (b) (void)hipFree(b);
  if (p->status) (void)hipFree(p->status);
  delete p;
  return PPASR_OK;
}

ppasr_status ppasr_beam_pool_reset(ppasr_beam_pool p, int session, void* stream) {
  if (!p) return fail(PPASR_EINVAL, "null pool");
  if (session >= p->n_sessions) return fail(PPASR_EINVAL, "beam pool: session out of range");
  hipStream_t hs = static_cast<hipStream_t>(stream);
  const int lo = session < 0 ? 0 : session, hi = session < 0 ? p->n_sessions : session + 1;
  for (int i = lo; i < hi; ++i) {
    HIP_TRY(launch_beam_reset(p->block[i], p->status + i, p->cfg.beam, (int)beam_max_nodes(p->cap[i], p->cfg.beam),
                              p->cfg.lm.bos, p->cfg.node_table != 0, hs));
    p->frames[i] = 0;
    p->used[i] = 0;
    p->live[i] = 0;
  }
  return PPASR_OK;
}

long long ppasr_beam_pool_frames(ppasr_beam_pool p, int session) {
  if (!p || session < 0 || session >= p->n_sessions) return -1;
  return p->frames[session];
}

long long ppasr_beam_pool_capacity(ppasr_beam_pool p, int session) {
  if (!p || session < 0 || session >= p->n_sessions) return -1;
  return (long long)p->cap[session];
}

ppasr_status ppasr_beam_pool_status(ppasr_beam_pool p, int32_t* status_host, void* stream) {
  if (!p || !status_host) return fail(PPASR_EINVAL, "null argument");
  hipStream_t hs = static_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(status_host, p->status, (size_t)p->n_sessions * 4, hipMemcpyDeviceToHost, hs));
  HIP_TRY(hipStreamSynchronize(hs));
  for (int i = 0; i < p->n_sessions; ++i)
    if (status_host[i] != 0) return fail(PPASR_ENOSPACE, "beam pool: the prefix arena of at least one session is exhausted");
  return PPASR_OK;
}

size_t ppasr_beam_pool_workspace_bytes(ppasr_beam_pool p, int n, int T) {
  if (!p || n < 1 || T < 0) return 0;
  return pool_rec_bytes(p->cfg, n, T) + beam_scratch_bytes(p->cfg, n, T);
}

// one decode call of a pool: T frames for every listed session (T = 0: none -- the search kernel loads each state block,
// stores the words it loaded back and finalizes, so the sessions stay bit for bit as they were), then the nbest best
// prefixes of each session's beam -> tokens [n][nbest][max_tokens], lens / scores [n][nbest]
static ppasr_status pool_decode(ppasr_beam_pool p, const int* sessions_host, int n, const float* probs, int T,
                                const int32_t* frame_lens_host, int nbest, int max_tokens, int32_t* tokens, int32_t* lens,
                                double* scores, void* workspace, size_t workspace_bytes, void* stream) {
  // ---- every check before any device work: a refused call changes no session ----
  if (!p || !sessions_host || !tokens || !lens || !scores || (!probs && T > 0)) return fail(PPASR_EINVAL, "null argument");
  if (n < 1 || n > p->n_sessions || T < 0 || max_tokens < 1) return fail(PPASR_EINVAL, "beam pool: bad n / T / max_tokens");
  if (!session_list_ok(sessions_host, n, p->n_sessions))
    return fail(PPASR_EINVAL, "beam pool: session index out of range or repeated");
  std::vector<int> fl(n);
  for (int b = 0; b < n; ++b) {
    fl[b] = frame_lens_host ? frame_lens_host[b] : T;
    if (fl[b] < 0 || fl[b] > T) return fail(PPASR_EINVAL, "beam pool: frame_lens must lie in [0, T]");
  }
  const size_t need = ppasr_beam_pool_workspace_bytes(p, n, T);
  if (workspace_bytes < need || (need > 0 && !workspace))
    return fail(PPASR_ENOSPACE, "beam pool: workspace smaller than ppasr_beam_pool_workspace_bytes(pool, n, T)");
  const int beam = p->cfg.beam;
  hipStream_t hs = static_cast<hipStream_t>(stream);
  // ---- automatic compaction (ppasr_beam_arena_set_auto): every listed session whose chunk does not fit is compacted, all
  // of them with one launch, before growth is planned; it then keeps its block if at least half of it stays free behind
  // this chunk, and otherwise grows from the compacted state until that holds -- so compactions of a session are at least
  // cap / 2 frames apart.  (Compaction changes no result, so a call refused below still changes no session's search.)
  std::vector<char> compacted(n, 0);
  if (p->auto_compact) {
    std::vector<int> list;
    for (int b = 0; b < n; ++b)
      if ((size_t)p->used[sessions_host[b]] + (size_t)fl[b] > p->cap[sessions_host[b]]) {
        compacted[b] = 1;
        list.push_back(sessions_host[b]);
      }
    if (!list.empty()) {
      ppasr_status rc = pool_compact(p, list.data(), (int)list.size(), nullptr, hs);
      if (rc != PPASR_OK) return rc;
    }
  }
  std::vector<size_t> new_cap(n, 0);  // 0: no growth
  for (int b = 0; b < n; ++b) {
    const int s = sessions_host[b];
    const size_t want = ((size_t)p->used[s] + (size_t)fl[b]) * (compacted[b] ? 2 : 1);
    if (want <= p->cap[s]) continue;
    size_t c = p->cap[s];
    while (c < want) c *= 2;
    if (!pool_cap_ok(c, beam)) return fail(PPASR_ENOSPACE, "beam pool: a session's stream is too long for one prefix arena");
    new_cap[b] = c;
  }
  // ---- growth: the session's block moves into one sized for twice the frames (doubling until the chunk fits).  Header,
  // beam arrays and arena keep their offsets (ppasr_ctc_beam_state_grow); the node table, where the search uses one, is
  // rebuilt for its new size.  The replaced blocks are freed after ONE stream synchronisation that covers every copy of
  // this call (growth is rare: a session's capacity doubles, so a stream of F frames grows log2(F / init_frames) times).
  std::vector<int32_t*> retired;
  for (int b = 0; b < n; ++b) {
    if (!new_cap[b]) continue;
    const int s = sessions_host[b];
    const int mo = (int)beam_max_nodes(p->cap[s], beam), mn = (int)beam_max_nodes(new_cap[b], beam);
    int32_t* nb = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&nb), pool_block_bytes(new_cap[b], beam)));
    const size_t head_words = beam_fixed_words(beam) + beam_arena_words(mo);
    hipError_t e = hipMemcpyAsync(nb, p->block[s], head_words * 4, hipMemcpyDeviceToDevice, hs);
    if (e == hipSuccess && p->cfg.node_table) {
      const size_t tab_off = (beam_fixed_words(beam) + beam_arena_words(mn)) * 4, tab_bytes = 12 * beam_table_slots(mn);
      e = hipMemsetAsync(reinterpret_cast<char*>(nb) + tab_off, 0, tab_bytes, hs);
      if (e == hipSuccess) e = launch_beam_rehash(nb, 1, beam, mn, hs);
    }
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(hs);
      (void)hipFree(nb);
      return fail(PPASR_EHIP, std::string("beam pool: growing a session failed: ") + hipGetErrorString(e));
    }
    retired.push_back(p->block[s]);
    p->block[s] = nb;
    p->cap[s] = new_cap[b];
  }
  if (!retired.empty()) {
    HIP_TRY(hipStreamSynchronize(hs));
    for (int32_t* o : retired) (void)hipFree(o);
  }
  // ---- the slot table and frame counts of this call ----
  StagingRing::Entry en;
  HIP_TRY(p->ring.acquire(&en));
  BeamSlot* tab = reinterpret_cast<BeamSlot*>(en.host);
  int32_t* fl_host = reinterpret_cast<int32_t*>(en.host + (size_t)n * sizeof(BeamSlot));
  for (int b = 0; b < n; ++b) {
    const int s = sessions_host[b];
    tab[b] = BeamSlot{p->block[s], p->status + s, (int)beam_max_nodes(p->cap[s], beam), 0};
    fl_host[b] = fl[b];
  }
  const size_t used = (size_t)n * (sizeof(BeamSlot) + 4);
  HIP_TRY(hipMemcpyAsync(en.dev, en.host, used, hipMemcpyHostToDevice, hs));
  BeamConfig c = p->cfg;
  c.max_tokens = max_tokens;
  c.nbest = nbest;
  c.max_nodes = 0;  // (per session: the slot table)
  {
    const char* f = getenv("PPASR_BEAM_FAST");  // (read per call, as ppasr_ctc_beam_search_ws does)
    c.fast_path = f ? (atoi(f) != 0) : 1;
  }
  char* ws = static_cast<char*>(workspace);
  const size_t rec_bytes = pool_rec_bytes(c, n, T), scratch_bytes = beam_scratch_bytes(c, n, T);
  int32_t* recs = rec_bytes ? reinterpret_cast<int32_t*>(ws) : nullptr;
  void* scratch = scratch_bytes ? ws + rec_bytes : nullptr;
  HIP_TRY(launch_ctc_beam(probs, reinterpret_cast<const int32_t*>(en.dev + (size_t)n * sizeof(BeamSlot)), n, T, c, recs,
                          nullptr, 0, 1, tokens, lens, scores, nullptr, scratch, hs, reinterpret_cast<const BeamSlot*>(en.dev)));
  HIP_TRY(p->ring.release(en, hs));
  for (int b = 0; b < n; ++b) {
    p->frames[sessions_host[b]] += fl[b];
    p->used[sessions_host[b]] += fl[b];
  }
  return PPASR_OK;
}

ppasr_status ppasr_beam_pool_decode(ppasr_beam_pool p, const int* sessions_host, int n, const float* probs, int T,
                                    const int32_t* frame_lens_host, int max_tokens, int32_t* tokens, int32_t* lens,
                                    double* scores, void* workspace, size_t workspace_bytes, void* stream) {
  return pool_decode(p, sessions_host, n, probs, T, frame_lens_host, 1, max_tokens, tokens, lens, scores, workspace,
                     workspace_bytes, stream);
}

ppasr_status ppasr_beam_sessions_nbest(ppasr_beam_pool p, const int* sessions_host, int n, int nbest, int max_tokens, int32_t* tokens,
                                   int32_t* lens, double* scores, void* workspace, size_t workspace_bytes, void* stream) {
  if (p && (nbest < 1 || nbest > p->cfg.beam)) return fail(PPASR_EINVAL, "beam pool: nbest must lie in [1, beam_size]");
  return pool_decode(p, sessions_host, n, nullptr, 0, nullptr, nbest, max_tokens, tokens, lens, scores, workspace, workspace_bytes,
                     stream);
}

// ---- compaction of the pool's prefix arenas (include/ppasr_hip.h: ppasr_beam_arena_*) ----
ppasr_status ppasr_beam_arena_compact(ppasr_beam_pool p, const int* sessions_host, int n, long long* live_nodes_host, void* stream) {
  if (!p) return fail(PPASR_EINVAL, "null pool");
  std::vector<int> all;
  if (!sessions_host || n < 0) {
    all.resize(p->n_sessions);
    for (int i = 0; i < p->n_sessions; ++i) all[i] = i;
    sessions_host = all.data();
    n = p->n_sessions;
  }
  if (n < 1 || n > p->n_sessions) return fail(PPASR_EINVAL, "beam pool: bad n");
  if (!session_list_ok(sessions_host, n, p->n_sessions))
    return fail(PPASR_EINVAL, "beam pool: session index out of range or repeated");
  return pool_compact(p, sessions_host, n, live_nodes_host, static_cast<hipStream_t>(stream));
}

ppasr_status ppasr_beam_arena_set_auto(ppasr_beam_pool p, int enable) {
  if (!p) return fail(PPASR_EINVAL, "null pool");
  p->auto_compact = enable != 0;
  return PPASR_OK;
}

long long ppasr_beam_arena_live_nodes(ppasr_beam_pool p, int session) {
  if (!p || session < 0 || session >= p->n_sessions) return -1;
  return p->live[session];
}

size_t ppasr_beam_arena_bytes(ppasr_beam_pool p) {
  if (!p) return 0;
  size_t total = 0;
  for (size_t c : p->cap) total += pool_block_bytes(c, p->cfg.beam);
  return total;
}

ppasr_status ppasr_ctc_collapse(const int32_t* frame_argmax, const float* frame_maxprob, const int32_t* frame_lens, int B,
                                int Tp, int blank, int32_t* tokens, int32_t* n_tokens, double* score, void* stream) {
  if (!frame_argmax || !frame_maxprob || !tokens || !n_tokens || !score) return fail(PPASR_EINVAL, "null argument");
  if (B <= 0 || Tp <= 0) return fail(PPASR_EINVAL, "empty batch");
  launch_ctc_collapse(frame_argmax, frame_maxprob, frame_lens, B, Tp, blank, tokens, n_tokens, score,
                      static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

ppasr_status ppasr_ctc_greedy(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank,
                              int32_t* tokens, int32_t* n_tokens, double* score, void* workspace, size_t workspace_bytes,
                              void* stream) {
  if (!probs || !tokens || !n_tokens || !score || !workspace) return fail(PPASR_EINVAL, "null argument");
  if (B <= 0 || Tp <= 0 || V <= 0) return fail(PPASR_EINVAL, "empty batch");
  const size_t n = (size_t)B * Tp;
  if (workspace_bytes < n * (sizeof(int32_t) + sizeof(float))) return fail(PPASR_ENOSPACE, "workspace too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* fa = static_cast<int32_t*>(workspace);
  float* fp = reinterpret_cast<float*>(fa + n);
  launch_frame_argmax(probs, fa, fp, B * Tp, V, st);
  launch_ctc_collapse(fa, fp, frame_lens, B, Tp, blank, tokens, n_tokens, score, st);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

// ---- hypothesis records of the data-parallel path (ppasr_amd/parallel.py): int32 rows
// tokens[cols] (-1 padded) | n_tokens | score (f64 as two words) [| utterance index].  One launch packs a batch's
// hypotheses into its rows of the rank's record, one launch restores the caller's utterance order after the all-gather --
// the record never passes through torch's indexing / elementwise kernels. ----
}  // extern "C"
namespace {
__global__ __launch_bounds__(256) void k_hyp_pack(const int32_t* __restrict__ tokens, long long token_stride, int L,
                                                  const int32_t* __restrict__ n, long long n_stride,
                                                  const double* __restrict__ score, long long score_stride,
                                                  const int32_t* __restrict__ index, int k, int32_t* __restrict__ rec,
                                                  int row0, int cols, int extra) {
  const int W = cols + extra;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)k * W) return;
  const int r = (int)(i / W), j = (int)(i - (long long)r * W);
  int32_t v;
  if (j < cols) {
    v = j < L ? tokens[r * token_stride + j] : -1;
  } else if (j == cols) {
    v = n[r * n_stride];
  } else if (j <= cols + 2) {
    const long long bits = __double_as_longlong(score[r * score_stride]);
    v = (int32_t)(j == cols + 1 ? (uint32_t)bits : (uint32_t)((unsigned long long)bits >> 32));
  } else {
    v = index ? index[r] : -1;
  }
  rec[(size_t)(row0 + r) * W + j] = v;
}
__global__ __launch_bounds__(256) void k_hyp_unpack(const int32_t* __restrict__ rec, const int64_t* __restrict__ order, int N,
                                                    int cols, int extra, int32_t* __restrict__ tokens, int32_t* __restrict__ n,
                                                    double* __restrict__ score, int32_t* __restrict__ index) {
  const int W = cols + extra;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * (cols + 1)) return;
  const int r = (int)(i / (cols + 1)), j = (int)(i - (long long)r * (cols + 1));
  const int32_t* src = rec + (size_t)(order ? order[r] : r) * W;
  if (j < cols) {
    tokens[(size_t)r * cols + j] = src[j];
  } else {
    n[r] = src[cols];
    const unsigned long long bits = (unsigned long long)(uint32_t)src[cols + 1] | ((unsigned long long)(uint32_t)src[cols + 2] << 32);
    score[r] = __longlong_as_double((long long)bits);
    if (index) index[r] = extra > 3 ? src[cols + 3] : -1;
  }
}
}  // namespace
extern "C" {

ppasr_status ppasr_hyp_pack(const int32_t* tokens, long long token_stride, int L, const int32_t* n_tokens, long long n_stride,
                            const double* score, long long score_stride, const int32_t* index, int k, int32_t* rec, int row0,
                            int cols, int extra, void* stream) {
  if (!tokens || !n_tokens || !score || !rec) return fail(PPASR_EINVAL, "null argument");
  if (k <= 0 || cols <= 0 || L < 0 || row0 < 0 || (extra != 3 && extra != 4)) return fail(PPASR_EINVAL, "hyp_pack: bad shape");
  const long long total = (long long)k * (cols + extra);
  PPASR_LAUNCH(k_hyp_pack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), tokens,
               token_stride, L, n_tokens, n_stride, score, score_stride, index, k, rec, row0, cols, extra);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

ppasr_status ppasr_hyp_unpack(const int32_t* rec, const int64_t* order, int N, int cols, int extra, int32_t* tokens,
                              int32_t* n_tokens, double* score, int32_t* index, void* stream) {
  if (!rec || !tokens || !n_tokens || !score) return fail(PPASR_EINVAL, "null argument");
  if (N <= 0 || cols <= 0 || (extra != 3 && extra != 4)) return fail(PPASR_EINVAL, "hyp_unpack: bad shape");
  const long long total = (long long)N * (cols + 1);
  PPASR_LAUNCH(k_hyp_unpack, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), rec, order,
               N, cols, extra, tokens, n_tokens, score, index);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // extern "C"
