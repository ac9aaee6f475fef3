// capi_align.hip -- C-ABI of CTC forced alignment: ppasr_ctc_align_workspace_bytes and ppasr_ctc_align (ctc_align.hip),
// and of the CTC negative log-likelihood over the same trellis: ppasr_ctc_loss_workspace_bytes and ppasr_ctc_loss
// (ctc_loss.hip).
#include "capi_internal.h"
#include "ctc_align.h"
#include "ctc_loss.h"

#include <algorithm>

// ---- the two halves of an append (capi_internal.h): ppasr_prob_arena_append and the encoder rounds that keep their memory ----
ppasr_status arena_plan_append(const ppasr_prob_arena_s* a, const int* sessions, int n, int c, const int* frames, const char* who,
                               long long* rows_out) {
  const std::string w(who);
  if (!session_list_ok(sessions, n, a->n_sessions))
    return fail(PPASR_EINVAL, w + ": sessions must be distinct indices in [0, n_sessions)");
  const int P = a->P;
  long long need = 0, rows = 0;
  for (int k = 0; k < n; ++k) {
    const int f = frames ? frames[k] : c;
    if (f < 0 || f > c) return fail(PPASR_EINVAL, w + ": frames[k] outside [0, c]");
    need += (a->frames[sessions[k]] + f + P - 1) / P - (long long)a->pages[sessions[k]].size();
    rows += f;
  }
  if (need > (long long)a->free_list.size())
    return fail(PPASR_ENOSPACE, w + ": the round needs " + std::to_string(need) + " pages, " +
                                    std::to_string(a->free_list.size()) + " are free");
  if (rows_out) *rows_out = rows;
  return PPASR_OK;
}

ppasr_status arena_stage_append(ppasr_prob_arena_s* a, const int* sessions, int n, int c, const int* frames, ArenaAppendTab* tab,
                                hipStream_t st) {
  const int P = a->P;
  HIP_TRY(a->ring.acquire(&tab->en));
  int32_t* h = reinterpret_cast<int32_t*>(tab->en.host);
  int32_t *first = h, *count = h + a->n_sessions, *page_off = h + 2 * a->n_sessions, *pages = h + 3 * a->n_sessions;
  int used = 0;
  for (int k = 0; k < n; ++k) {
    const int s = sessions[k], f = frames ? frames[k] : c;
    std::vector<int>& pg = a->pages[s];
    const long long f0 = a->frames[s];
    while ((long long)pg.size() * P < f0 + f) {
      pg.push_back(a->free_list.back());
      a->free_list.pop_back();
    }
    first[k] = (int)f0;
    count[k] = f;
    page_off[k] = used;
    // the pages this entry's frames f0 .. f0 + f - 1 touch (at most n_pages over the whole call: sessions are distinct)
    if (f > 0)
      for (long long j = f0 / P; j <= (f0 + f - 1) / P; ++j) pages[used++] = pg[j];
    a->frames[s] = f0 + f;
  }
  const size_t bytes = (size_t)(3 * a->n_sessions + used) * sizeof(int32_t);
  HIP_TRY(hipMemcpyAsync(tab->en.dev, tab->en.host, bytes, hipMemcpyHostToDevice, st));
  const int32_t* d = reinterpret_cast<const int32_t*>(tab->en.dev);
  tab->first = d;
  tab->count = d + a->n_sessions;
  tab->page_off = d + 2 * a->n_sessions;
  tab->pages = d + 3 * a->n_sessions;
  return PPASR_OK;
}

extern "C" {

size_t ppasr_ctc_align_workspace_bytes(int B, int Tp, int max_tokens) {
  if (B <= 0 || Tp < 0 || max_tokens < 0 || max_tokens > kAlignMaxTokens) return 0;
  return align_layout(B, Tp, max_tokens).total;
}

ppasr_status ppasr_ctc_align(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank,
                             const int32_t* tokens, const int32_t* n_tokens, int max_tokens, int32_t* frame_token, int32_t* begin,
                             int32_t* end, int32_t* peak, float* conf, float* score, int32_t* status, void* workspace,
                             size_t workspace_bytes, void* stream) {
  if (B <= 0 || Tp < 0 || V < 2 || max_tokens < 0) return fail(PPASR_EINVAL, "ctc_align: bad shape (B > 0, Tp >= 0, V >= 2, max_tokens >= 0)");
  if (blank < 0 || blank >= V) return fail(PPASR_EINVAL, "ctc_align: blank outside [0, V)");
  if (max_tokens > kAlignMaxTokens)
    return fail(PPASR_EUNSUPPORTED, "ctc_align: max_tokens exceeds the 255 tokens per utterance the kernel is built for");
  if (!n_tokens || !score || !status || !workspace || (Tp > 0 && (!probs || !frame_token)) || (max_tokens > 0 && !tokens))
    return fail(PPASR_EINVAL, "ctc_align: null argument");
  if ((size_t)B * Tp > (size_t)1 << 26) return fail(PPASR_EUNSUPPORTED, "ctc_align: batch too large (B * Tp > 2^26)");
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(PPASR_EINVAL, "ctc_align: workspace must be 16-byte aligned");
  if (workspace_bytes < ppasr_ctc_align_workspace_bytes(B, Tp, max_tokens))
    return fail(PPASR_EINVAL, "ctc_align: workspace too small (ppasr_ctc_align_workspace_bytes)");
  launch_ctc_align(probs, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, frame_token, begin, end, peak, conf, score,
                   status, workspace, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

// ---- probability arena ----
ppasr_status ppasr_prob_arena_create(int n_sessions, int V, int page_frames, int n_pages, ppasr_prob_arena* out) {
  if (!out) return fail(PPASR_EINVAL, "prob_arena_create: null argument");
  *out = nullptr;
  if (n_sessions < 1 || V < 2 || page_frames < 1 || n_pages < 1)
    return fail(PPASR_EINVAL, "prob_arena_create: bad shape (n_sessions >= 1, V >= 2, page_frames >= 1, n_pages >= 1)");
  if (n_sessions > (1 << 20) || n_pages > (1 << 24) || (long long)n_pages * page_frames > (1ll << 30) ||
      (double)n_pages * page_frames * V * sizeof(float) >= (double)((size_t)1 << 40))
    return fail(PPASR_EINVAL, "prob_arena_create: arena too large (slab below 2^40 bytes, n_pages <= 2^24, n_pages * "
                              "page_frames <= 2^30, n_sessions <= 2^20)");
  std::unique_ptr<ppasr_prob_arena_s> a(new ppasr_prob_arena_s());
  a->n_sessions = n_sessions;
  a->V = V;
  a->P = page_frames;
  a->n_pages = n_pages;
  a->pages.resize(n_sessions);
  a->frames.assign(n_sessions, 0);
  a->free_list.resize(n_pages);
  for (int i = 0; i < n_pages; ++i) a->free_list[i] = n_pages - 1 - i;  // (page 0 is handed out first)
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&a->slab), (size_t)n_pages * page_frames * V * sizeof(float)));
  HIP_TRY(a->ring.alloc(a->table_ints() * sizeof(int32_t)));
  *out = a.release();
  return PPASR_OK;
}

ppasr_status ppasr_prob_arena_destroy(ppasr_prob_arena arena) {
  delete arena;
  return PPASR_OK;
}

ppasr_status ppasr_prob_arena_append(ppasr_prob_arena a, const int* sessions, int n, const float* probs, int c, const int* frames,
                                     void* stream) {
  if (!a || !sessions) return fail(PPASR_EINVAL, "prob_arena_append: null argument");
  if (n < 1 || c < 0) return fail(PPASR_EINVAL, "prob_arena_append: n >= 1 and c >= 0");
  if (!session_list_ok(sessions, n, a->n_sessions))
    return fail(PPASR_EINVAL, "prob_arena_append: sessions must be distinct indices in [0, n_sessions)");
  if (c > 0 && !probs) return fail(PPASR_EINVAL, "prob_arena_append: null argument");
  if ((long long)n * c > (1ll << 30)) return fail(PPASR_EUNSUPPORTED, "prob_arena_append: round too large (n * c > 2^30)");
  long long rows = 0;
  ppasr_status r = arena_plan_append(a, sessions, n, c, frames, "prob_arena_append", &rows);
  if (r != PPASR_OK) return r;
  if (rows == 0) return PPASR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ArenaAppendTab tab{};
  r = arena_stage_append(a, sessions, n, c, frames, &tab, st);
  if (r != PPASR_OK) return r;
  launch_arena_append(probs, n, c, a->V, a->P, tab.first, tab.count, tab.page_off, tab.pages, a->slab, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(a->ring.release(tab.en, st));
  return PPASR_OK;
}

ppasr_status ppasr_prob_arena_reset(ppasr_prob_arena a, int session) {
  if (!a) return fail(PPASR_EINVAL, "prob_arena_reset: null argument");
  if (session >= a->n_sessions) return fail(PPASR_EINVAL, "prob_arena_reset: session out of range");
  for (int s = session < 0 ? 0 : session; s < (session < 0 ? a->n_sessions : session + 1); ++s) {
    std::vector<int>& pg = a->pages[s];
    for (size_t i = pg.size(); i-- > 0;) a->free_list.push_back(pg[i]);
    pg.clear();
    a->frames[s] = 0;
  }
  return PPASR_OK;
}

long long ppasr_prob_arena_frames(ppasr_prob_arena a, int session) {
  return (!a || session < 0 || session >= a->n_sessions) ? -1 : a->frames[session];
}

long long ppasr_prob_arena_free_pages(ppasr_prob_arena a) { return a ? (long long)a->free_list.size() : -1; }

ppasr_status ppasr_prob_arena_read(ppasr_prob_arena a, int session, float* dense, void* stream) {
  if (!a) return fail(PPASR_EINVAL, "prob_arena_read: null argument");
  if (session < 0 || session >= a->n_sessions) return fail(PPASR_EINVAL, "prob_arena_read: session out of range");
  const long long T = a->frames[session];
  if (T == 0) return PPASR_OK;
  if (!dense) return fail(PPASR_EINVAL, "prob_arena_read: null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  StagingRing::Entry en;
  HIP_TRY(a->ring.acquire(&en));
  const std::vector<int>& pg = a->pages[session];
  std::memcpy(en.host, pg.data(), pg.size() * sizeof(int32_t));
  HIP_TRY(hipMemcpyAsync(en.dev, en.host, pg.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  launch_arena_read(a->slab, a->V, a->P, reinterpret_cast<const int32_t*>(en.dev), (int)T, dense, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(a->ring.release(en, st));
  return PPASR_OK;
}

ppasr_status ppasr_prob_arena_read_many(ppasr_prob_arena a, const int* sessions, int n, int Tp, float* dense, int32_t* lens,
                                        void* stream) {
  if (!a || !sessions || !lens) return fail(PPASR_EINVAL, "prob_arena_read_many: null argument");
  if (n < 1 || Tp < 0) return fail(PPASR_EINVAL, "prob_arena_read_many: n >= 1 and Tp >= 0");
  if (!session_list_ok(sessions, n, a->n_sessions))
    return fail(PPASR_EINVAL, "prob_arena_read_many: sessions must be distinct indices in [0, n_sessions)");
  for (int k = 0; k < n; ++k)
    if (a->frames[sessions[k]] > Tp) return fail(PPASR_EINVAL, "prob_arena_read_many: Tp below the longest listed session");
  if (Tp > 0 && !dense) return fail(PPASR_EINVAL, "prob_arena_read_many: null argument");
  if ((long long)n * Tp > (1ll << 30)) return fail(PPASR_EUNSUPPORTED, "prob_arena_read_many: gather too large (n * Tp > 2^30)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  StagingRing::Entry en;
  HIP_TRY(a->ring.acquire(&en));
  int32_t* h = reinterpret_cast<int32_t*>(en.host);
  int32_t *count = h, *page_off = h + 2 * a->n_sessions, *pages = h + 3 * a->n_sessions;
  int used = 0;
  for (int k = 0; k < n; ++k) {
    const std::vector<int>& pg = a->pages[sessions[k]];
    count[k] = (int)a->frames[sessions[k]];
    page_off[k] = used;
    std::memcpy(pages + used, pg.data(), pg.size() * sizeof(int32_t));
    used += (int)pg.size();
  }
  HIP_TRY(hipMemcpyAsync(en.dev, en.host, (size_t)(3 * a->n_sessions + used) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int32_t* d = reinterpret_cast<const int32_t*>(en.dev);
  launch_arena_read_many(a->slab, a->V, a->P, d, d + 2 * a->n_sessions, d + 3 * a->n_sessions, n, Tp, dense, lens, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(a->ring.release(en, st));
  return PPASR_OK;
}

size_t ppasr_ctc_align_arena_workspace_bytes(int n, int Tp, int max_tokens) {
  return ppasr_ctc_align_workspace_bytes(n, Tp, max_tokens);
}

ppasr_status ppasr_ctc_align_arena(ppasr_prob_arena a, const int* sessions, int n, int blank, const int32_t* tokens,
                                   const int32_t* n_tokens, int max_tokens, int32_t* frame_token, int32_t* begin, int32_t* end,
                                   int32_t* peak, float* conf, float* score, int32_t* status, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!a || !sessions) return fail(PPASR_EINVAL, "ctc_align_arena: null argument");
  if (n < 1 || max_tokens < 0) return fail(PPASR_EINVAL, "ctc_align_arena: n >= 1 and max_tokens >= 0");
  if (!session_list_ok(sessions, n, a->n_sessions))
    return fail(PPASR_EINVAL, "ctc_align_arena: sessions must be distinct indices in [0, n_sessions)");
  if (blank < 0 || blank >= a->V) return fail(PPASR_EINVAL, "ctc_align_arena: blank outside [0, V)");
  if (max_tokens > kAlignMaxTokens)
    return fail(PPASR_EUNSUPPORTED, "ctc_align_arena: max_tokens exceeds the 255 tokens per utterance the kernel is built for");
  long long Tp = 0;
  for (int k = 0; k < n; ++k) Tp = std::max(Tp, a->frames[sessions[k]]);
  if (!n_tokens || !score || !status || !workspace || (Tp > 0 && !frame_token) || (max_tokens > 0 && !tokens))
    return fail(PPASR_EINVAL, "ctc_align_arena: null argument");
  if ((unsigned long long)n * Tp > 1ull << 26) return fail(PPASR_EUNSUPPORTED, "ctc_align_arena: batch too large (n * Tp > 2^26)");
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0)
    return fail(PPASR_EINVAL, "ctc_align_arena: workspace must be 16-byte aligned");
  if (workspace_bytes < ppasr_ctc_align_arena_workspace_bytes(n, (int)Tp, max_tokens))
    return fail(PPASR_ENOSPACE, "ctc_align_arena: workspace too small (ppasr_ctc_align_arena_workspace_bytes)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  StagingRing::Entry en;
  HIP_TRY(a->ring.acquire(&en));
  int32_t* h = reinterpret_cast<int32_t*>(en.host);
  int32_t *lens = h, *page_off = h + 2 * a->n_sessions, *pages = h + 3 * a->n_sessions;
  int used = 0;
  for (int k = 0; k < n; ++k) {
    const std::vector<int>& pg = a->pages[sessions[k]];
    lens[k] = (int)a->frames[sessions[k]];
    page_off[k] = used;
    std::memcpy(pages + used, pg.data(), pg.size() * sizeof(int32_t));
    used += (int)pg.size();
  }
  HIP_TRY(hipMemcpyAsync(en.dev, en.host, (size_t)(3 * a->n_sessions + used) * sizeof(int32_t), hipMemcpyHostToDevice, st));
  const int32_t* d = reinterpret_cast<const int32_t*>(en.dev);
  launch_ctc_align_paged(a->slab, a->V, a->P, d + 2 * a->n_sessions, d + 3 * a->n_sessions, d, n, (int)Tp, blank, tokens, n_tokens,
                         max_tokens, frame_token, begin, end, peak, conf, score, status, workspace, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(a->ring.release(en, st));
  return PPASR_OK;
}

size_t ppasr_ctc_loss_workspace_bytes(int B, int Tp, int max_tokens) {
  if (B <= 0 || Tp < 0 || max_tokens < 0 || max_tokens > kAlignMaxTokens) return 0;
  return ctc_loss_workspace(B, Tp, max_tokens);
}

ppasr_status ppasr_ctc_loss(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                            const int32_t* n_tokens, int max_tokens, float* nll, int32_t* status, void* workspace,
                            size_t workspace_bytes, void* stream) {
  if (B <= 0 || Tp < 0 || V < 2 || max_tokens < 0) return fail(PPASR_EINVAL, "ctc_loss: bad shape (B > 0, Tp >= 0, V >= 2, max_tokens >= 0)");
  if (blank < 0 || blank >= V) return fail(PPASR_EINVAL, "ctc_loss: blank outside [0, V)");
  if (max_tokens > kAlignMaxTokens)
    return fail(PPASR_EUNSUPPORTED, "ctc_loss: max_tokens exceeds the 255 tokens per utterance the kernel is built for");
  if (!n_tokens || !nll || !status || !workspace || (Tp > 0 && !probs) || (max_tokens > 0 && !tokens))
    return fail(PPASR_EINVAL, "ctc_loss: null argument");
  if ((size_t)B * Tp > (size_t)1 << 26) return fail(PPASR_EUNSUPPORTED, "ctc_loss: batch too large (B * Tp > 2^26)");
  if (reinterpret_cast<uintptr_t>(workspace) % 16 != 0) return fail(PPASR_EINVAL, "ctc_loss: workspace must be 16-byte aligned");
  if (workspace_bytes < ppasr_ctc_loss_workspace_bytes(B, Tp, max_tokens))
    return fail(PPASR_EINVAL, "ctc_loss: workspace too small (ppasr_ctc_loss_workspace_bytes)");
  launch_ctc_loss(probs, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, nll, status, workspace,
                  static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // extern "C"
