// ctc_align.hip -- CTC forced alignment on the device: the Viterbi path of a token sequence through a [B, Tp, V] table of
// CTC probabilities, and from it per-token frames and confidences.
//
// DEFINITION (the one tests/align_oracle.py restates in numpy).
//   Inputs: probs [B, Tp, V] f32; frame_lens [B] i32 or NULL (= Tp), clamped to [0, Tp]; tokens [B, max_tokens] i32;
//   n_tokens [B] i32.  For utterance b let T = frame_lens[b], L = n_tokens[b], tok = tokens[b, 0..L).
//   Bad input (status 2): L outside [0, max_tokens], or a tok[l] outside [0, V) or equal to `blank`.  Nothing is clamped.
//   Trellis: states s = 0 .. 2L; even states are blank, odd state 2l+1 is token l; label(s) = blank or tok[l].
//     e(t, s) = logf(max(p[t, label(s)], FLT_MIN))      accurate logf; the clamp makes 0 and denormals finite
//   Transitions into s at frame t: from s (stay), from s-1 (step), and from s-2 (skip) for odd s with label(s) != label(s-2).
//   Start in state 0 or 1, end in state 2L or (L > 0) 2L-1.
//     a(0, s) = e(0, s) for s in {0, 1}, -inf elsewhere;   a(t, s) = max over the transitions of a(t-1, .) + e(t, s)
//   fp32, one add per frame.  Ties: the first of stay, step, skip that attains the maximum (a candidate replaces the
//   running best only when strictly greater); at the end 2L unless a(T-1, 2L-1) is strictly greater.
//   Feasible iff T >= L + #{l >= 1 : tok[l] == tok[l-1]}; otherwise status 1.  L = 0 with T = 0 is feasible: score 0.
//   Outputs (status 0): frame_token [Tp] = l where the path sits in state 2l+1, -1 on blank frames and for t >= T;
//   begin[l] / end[l] = first frame of token l / one past its last; conf[l] = max of p[t, tok[l]] over begin <= t < end,
//   copied from the table; peak[l] = the first such t; score = a(T-1, final state); entries l >= L are -1 (conf 0.0).
//   Status 1 or 2: score -inf and every entry -1 (conf 0.0).
//
// FORM.  Two launches.
//   align_gather_kernel: one wave per (b, t) row writes e(t, .) of the utterance's tokens and of blank into a dense row of
//     the workspace (ctc_align.h: align_row_stride), so that the chain reads 16 contiguous bytes per lane and frame
//     and not scattered words of a V-wide row.  Only rows t < T and tokens l < L are read and written.
//   align_chain_kernel: one wave per utterance.  Lane i owns the (blank 2l, token 2l+1) pairs l = 4i .. 4i+3 in
//     registers; the only value a lane needs from outside is the score of token 4i-1, one DPP wave_shr:1 move per frame.
//     No LDS and no barrier on the chain; emission rows are loaded kAhead = 16 frames ahead.  Each lane stores the 2-bit
//     back-pointers of its 8 states as one 16-bit word (128 bytes per frame).  After the last frame lane 0 walks the
//     back-pointers, 64 frames at a time through an 8 KB LDS copy (a dependent LDS read per frame, not a dependent global
//     one), then the wave fills begin / end over frames and peak / conf over tokens in parallel.
//   Nothing is accumulated with atomics, and no word of the workspace or of an output is read before this call wrote it.
//
// PAGED TABLES (ppasr_prob_arena_*, capi_align.hip).  A stream's table grows by one chunk per round, so it is kept in pages
//   of page_frames rows inside one slab: frame t of session b is row t % page_frames of page pages[page_off[b] + t /
//   page_frames].  arena_append_kernel copies one round's rows of every listed session behind their last frames with one
//   launch (one workgroup per row; words, so every bit pattern survives).  align_gather_paged_kernel is the gather above
//   with the row found through the page list, and the chain is the same kernel: the only place where it reads the table
//   itself (peak / conf) finds the row through DenseRows or PagedRows.  Rows behind a session's last frame are never read.
#include "ctc_align.h"

#include "launch.h"

namespace ppasr {
namespace {

constexpr int kAhead = 16;  // frames of emissions in flight per lane (5 registers each)

__global__ __launch_bounds__(256) void align_gather_kernel(const float* __restrict__ probs, const int32_t* __restrict__ frame_lens,
                                                           long long rows, int Tp, int V, int blank,
                                                           const int32_t* __restrict__ tokens,
                                                           const int32_t* __restrict__ n_tokens, int max_tokens, int stride,
                                                           float* __restrict__ emis) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / Tp), t = (int)(row - (long long)b * Tp);
  if (t >= clamp_frames(frame_lens, b, Tp)) return;
  const int L = n_tokens[b];
  if (L < 0 || L > max_tokens) return;
  const float* p = probs + (size_t)row * V;
  float* e = emis + (size_t)row * stride;
  if (lane == 0) e[stride - 4] = emission(p[blank]);
  for (int l = lane; l < L; l += 64) {
    const int tok = tokens[(size_t)b * max_tokens + l];
    if ((unsigned)tok < (unsigned)V) e[l] = emission(p[tok]);  // (an id outside the table makes the utterance status 2)
  }
}

// where row t of utterance b lies: a dense [B][Tp][V] table, or the pages of a probability arena
struct DenseRows {
  const float* probs;
  int Tp, V;
  __device__ __forceinline__ const float* row(int b, int t) const { return probs + ((size_t)b * Tp + t) * V; }
};
struct PagedRows {
  const float* slab;         // [n_pages][P][V]
  const int32_t* page_off;   // [B]: where utterance b's page list starts in `pages`
  const int32_t* pages;      // page of frames jP .. jP + P - 1 of utterance b at [page_off[b] + j]
  int P, V;
  __device__ __forceinline__ const float* row(int b, int t) const {
    return slab + ((size_t)pages[page_off[b] + t / P] * P + t % P) * V;
  }
};

// align_gather_kernel over an arena: frame_lens [B] are the sessions' own frame counts (never NULL, all <= Tp)
__global__ __launch_bounds__(256) void align_gather_paged_kernel(PagedRows table, const int32_t* __restrict__ frame_lens,
                                                                 long long rows, int Tp, int blank,
                                                                 const int32_t* __restrict__ tokens,
                                                                 const int32_t* __restrict__ n_tokens, int max_tokens,
                                                                 int stride, float* __restrict__ emis) {
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int b = (int)(row / Tp), t = (int)(row - (long long)b * Tp);
  if (t >= clamp_frames(frame_lens, b, Tp)) return;
  const int L = n_tokens[b];
  if (L < 0 || L > max_tokens) return;
  const float* p = table.row(b, t);
  float* e = emis + (size_t)row * stride;
  if (lane == 0) e[stride - 4] = emission(p[blank]);
  for (int l = lane; l < L; l += 64) {
    const int tok = tokens[(size_t)b * max_tokens + l];
    if ((unsigned)tok < (unsigned)table.V) e[l] = emission(p[tok]);
  }
}

// One round's rows into the arena: workgroup (k, r) copies row r of entry k to frame first[k] + r of its session, whose
// pages from page first[k] / P on are pages[page_off[k] ..].  Rows r >= count[k] are not appended.
__global__ __launch_bounds__(256) void arena_append_kernel(const uint32_t* __restrict__ probs, int c, int V, int P,
                                                           const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ page_off,
                                                           const int32_t* __restrict__ pages, uint32_t* __restrict__ slab) {
  const int k = blockIdx.x / c, r = blockIdx.x - k * c;
  if (r >= count[k]) return;
  const int f = first[k] + r;
  const int page = pages[page_off[k] + f / P - first[k] / P];
  const uint32_t* src = probs + (size_t)blockIdx.x * V;
  uint32_t* dst = slab + ((size_t)page * P + f % P) * V;
  for (int v = threadIdx.x; v < V; v += 256) dst[v] = src[v];
}

// a session's pages as one dense [T][V] table: workgroup t copies frame t
__global__ __launch_bounds__(256) void arena_read_kernel(const uint32_t* __restrict__ slab, int V, int P,
                                                         const int32_t* __restrict__ pages, uint32_t* __restrict__ dense) {
  const int t = blockIdx.x;
  const uint32_t* src = slab + ((size_t)pages[t / P] * P + t % P) * V;
  uint32_t* dst = dense + (size_t)t * V;
  for (int v = threadIdx.x; v < V; v += 256) dst[v] = src[v];
}

// the pages of n sessions as one dense [n][Tp][V] table: workgroup (k, t) copies frame t of entry k, or writes zeros when
// the session holds no such frame; the workgroup of frame 0 also writes the session's frame count (grid n * max(Tp, 1))
__global__ __launch_bounds__(256) void arena_read_many_kernel(const uint32_t* __restrict__ slab, int V, int P,
                                                              const int32_t* __restrict__ count,
                                                              const int32_t* __restrict__ page_off,
                                                              const int32_t* __restrict__ pages, int Tp,
                                                              uint32_t* __restrict__ dense, int32_t* __restrict__ lens) {
  const int span = Tp > 0 ? Tp : 1;
  const int k = blockIdx.x / span, t = blockIdx.x - k * span;
  const int T = count[k];
  if (t == 0 && threadIdx.x == 0) lens[k] = T;
  if (t >= Tp) return;
  uint32_t* dst = dense + ((size_t)k * Tp + t) * V;
  if (t >= T) {
    for (int v = threadIdx.x; v < V; v += 256) dst[v] = 0u;
    return;
  }
  const uint32_t* src = slab + ((size_t)pages[page_off[k] + t / P] * P + t % P) * V;
  for (int v = threadIdx.x; v < V; v += 256) dst[v] = src[v];
}

struct Emis {
  float4 v;  // e(t, token 4i .. 4i+3) of lane i
  float eb;  // e(t, blank)
};

template <class Rows>
__global__ __launch_bounds__(64) void align_chain_kernel(const Rows table, const int32_t* __restrict__ frame_lens,
                                                         int Tp, int V, int blank, const int32_t* __restrict__ tokens,
                                                         const int32_t* __restrict__ n_tokens, int max_tokens, int stride,
                                                         const float* emis, uint16_t* bp, int32_t* span, int32_t* frame_token,
                                                         int32_t* begin, int32_t* end, int32_t* peak, float* conf, float* score,
                                                         int32_t* status) {
  __shared__ uint4 sbp[64 * 8];  // back-pointers of 64 frames, for the walk
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = clamp_frames(frame_lens, b, Tp);
  const int Lraw = n_tokens[b];
  const bool len_bad = Lraw < 0 || Lraw > max_tokens;
  const int L = len_bad ? 0 : Lraw;
  const int32_t* tk = tokens + (size_t)b * max_tokens;  // (never dereferenced when L == 0)

  int tok[4];
  bool bad = false;
  int reps = 0;
  unsigned skip_ok = 0;  // bit k: token 4i+k differs from the token before it (the skip into its state is allowed)
  int before = (4 * lane >= 1 && 4 * lane - 1 < L) ? tk[4 * lane - 1] : -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int l = 4 * lane + k;
    tok[k] = l < L ? tk[l] : -1;
    if (l < L) {
      if ((unsigned)tok[k] >= (unsigned)V || tok[k] == blank) bad = true;
      if (l >= 1) {
        if (tok[k] == before) ++reps;
        else skip_ok |= 1u << k;
      }
    }
    before = tok[k];
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) reps += __shfl_xor(reps, o);
  const int st = (len_bad || __ballot(bad) != 0ull) ? 2 : (T < L + reps ? 1 : 0);

  int32_t* ft = frame_token + (size_t)b * Tp;
  const size_t tb = (size_t)b * max_tokens;
  // per-token outputs of the tokens that do not exist: l >= l0
  auto clear_tokens = [&](int l0) {
    for (int l = l0 + lane; l < max_tokens; l += 64) {
      if (begin) begin[tb + l] = -1;
      if (end) end[tb + l] = -1;
      if (peak) peak[tb + l] = -1;
      if (conf) conf[tb + l] = 0.f;
    }
  };
  if (st != 0 || T == 0) {
    for (int t = lane; t < Tp; t += 64) ft[t] = -1;
    clear_tokens(0);
    if (lane == 0) {
      score[b] = st != 0 ? kNegInf : 0.f;
      status[b] = st;
    }
    return;
  }

  // ---- the chain ----
  const float* erow = emis + (size_t)b * Tp * stride;
  uint16_t* bprow = bp + (size_t)b * Tp * 64;
  const int off = 4 * lane < L ? 4 * lane : stride - 4;  // (a lane without tokens reads the blank's slot; never used)
  auto load = [&](int t) {
    const float* r = erow + (size_t)t * stride;
    Emis e;
    e.v = *reinterpret_cast<const float4*>(r + off);
    e.eb = r[stride - 4];
    return e;
  };
  bool tok_on[4], blank_on[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    tok_on[k] = 4 * lane + k < L;
    blank_on[k] = 4 * lane + k <= L;
  }
  float ab[4], at[4];
  {
    const Emis e0 = load(0);
#pragma unroll
    for (int k = 0; k < 4; ++k) ab[k] = at[k] = kNegInf;
    if (lane == 0) {
      ab[0] = e0.eb;
      if (L > 0) at[0] = e0.v.x;
    }
  }
  Emis buf[kAhead];
#pragma unroll
  for (int u = 0; u < kAhead; ++u) buf[u] = load(min(1 + u, T - 1));
  for (int t0 = 1; t0 < T; t0 += kAhead) {
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const int t = t0 + u;
      if (t >= T) break;
      const Emis cur = buf[u];
      buf[u] = load(min(t + kAhead, T - 1));
      const float ev[4] = {cur.v.x, cur.v.y, cur.v.z, cur.v.w};
      const float in = lane_shr1(at[3], kNegInf);  // token 4i-1 at frame t-1
      unsigned bits = 0;
#pragma unroll
      for (int k = 3; k >= 0; --k) {  // (descending: at[k-1] is still frame t-1's when pair k reads it)
        const float prev_tok = k ? at[k - 1] : in;
        const float ob = ab[k], ot = at[k];
        const bool step_b = prev_tok > ob;
        const float nb = step_b ? prev_tok : ob;
        float best = ot;
        unsigned c = 0;
        if (ob > best) {
          best = ob;
          c = 1;
        }
        if (((skip_ok >> k) & 1u) && prev_tok > best) {
          best = prev_tok;
          c = 2;
        }
        bits |= ((unsigned)step_b << (4 * k)) | (c << (4 * k + 2));
        ab[k] = blank_on[k] ? nb + cur.eb : kNegInf;
        at[k] = tok_on[k] ? best + ev[k] : kNegInf;
      }
      bprow[(size_t)t * 64 + lane] = (uint16_t)bits;
    }
  }

  // ---- the end: state 2L, or 2L-1 when strictly better ----
  auto pick = [](const float (&a)[4], int k) { return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3]; };
  const float fin_b = __shfl(pick(ab, L & 3), L >> 2);
  const float fin_t = L > 0 ? __shfl(pick(at, (L - 1) & 3), (L - 1) >> 2) : kNegInf;
  int s = fin_t > fin_b ? 2 * L - 1 : 2 * L;
  if (lane == 0) {
    score[b] = fin_t > fin_b ? fin_t : fin_b;
    status[b] = 0;
  }

  // ---- the walk (lane 0), 64 frames of back-pointers at a time ----
  __threadfence();
  __syncthreads();
  for (int hi = T - 1; hi >= 1; hi -= 64) {
    const int lo = max(1, hi - 63);
    const uint4* src = reinterpret_cast<const uint4*>(bprow + (size_t)lo * 64);
    for (int i = lane; i < (hi - lo + 1) * 8; i += 64) sbp[i] = src[i];
    __syncthreads();
    if (lane == 0) {
      const uint16_t* w = reinterpret_cast<const uint16_t*>(sbp);
      for (int t = hi; t >= lo; --t) {
        ft[t] = (s & 1) ? (s >> 1) : -1;
        s -= (w[(t - lo) * 64 + (s >> 3)] >> ((s & 7) * 2)) & 3;
      }
    }
    __syncthreads();
  }
  if (lane == 0) ft[0] = (s & 1) ? (s >> 1) : -1;
  for (int t = T + lane; t < Tp; t += 64) ft[t] = -1;
  __threadfence();
  __syncthreads();

  // ---- begin / end over frames: every token of a feasible path has exactly one first and one last frame ----
  int32_t* sb = span + (size_t)b * 2 * max_tokens;
  int32_t* se = sb + max_tokens;
  for (int t = lane; t < T; t += 64) {
    const int f = ft[t];
    if (f < 0) continue;
    if (t == 0 || ft[t - 1] != f) sb[f] = t;
    if (t == T - 1 || ft[t + 1] != f) se[f] = t + 1;
  }
  __threadfence();
  __syncthreads();

  // ---- peak / conf over tokens ----
  for (int l = lane; l < L; l += 64) {
    const int t0 = min(max(sb[l], 0), T - 1), t1 = min(se[l], T);  // (in range as written; the clamp bounds the reads below)
    const int id = tk[l];
    float best = table.row(b, t0)[id];
    int at_t = t0;
    for (int t = t0 + 1; t < t1; ++t) {
      const float p = table.row(b, t)[id];
      if (p > best) {
        best = p;
        at_t = t;
      }
    }
    if (begin) begin[tb + l] = t0;
    if (end) end[tb + l] = t1;
    if (peak) peak[tb + l] = at_t;
    if (conf) conf[tb + l] = best;
  }
  clear_tokens(L);
}

}  // namespace

void launch_ctc_gather(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                       const int32_t* n_tokens, int max_tokens, float* emis, hipStream_t st) {
  const long long rows = (long long)B * Tp;
  if (rows > 0)
    PPASR_LAUNCH(align_gather_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, probs, frame_lens, rows, Tp, V, blank,
                 tokens, n_tokens, max_tokens, align_row_stride(max_tokens), emis);
}

namespace {
template <class Rows>
void launch_ctc_chain(const Rows& table, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                      const int32_t* n_tokens, int max_tokens, int32_t* frame_token, int32_t* begin, int32_t* end, int32_t* peak,
                      float* conf, float* score, int32_t* status, void* workspace, hipStream_t st) {
  const AlignLayout l = align_layout(B, Tp, max_tokens);
  char* ws = static_cast<char*>(workspace);
  PPASR_LAUNCH(align_chain_kernel<Rows>, dim3(B), dim3(64), 0, st, table, frame_lens, Tp, V, blank, tokens, n_tokens, max_tokens,
               align_row_stride(max_tokens), reinterpret_cast<const float*>(ws + l.emis), reinterpret_cast<uint16_t*>(ws + l.bp),
               reinterpret_cast<int32_t*>(ws + l.span), frame_token, begin, end, peak, conf, score, status);
}
}  // namespace

void launch_ctc_align(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                      const int32_t* n_tokens, int max_tokens, int32_t* frame_token, int32_t* begin, int32_t* end, int32_t* peak,
                      float* conf, float* score, int32_t* status, void* workspace, hipStream_t st) {
  float* emis = reinterpret_cast<float*>(static_cast<char*>(workspace) + align_layout(B, Tp, max_tokens).emis);
  launch_ctc_gather(probs, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, emis, st);
  launch_ctc_chain(DenseRows{probs, Tp, V}, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, frame_token, begin, end,
                   peak, conf, score, status, workspace, st);
}

void launch_ctc_align_paged(const float* slab, int V, int P, const int32_t* page_off, const int32_t* pages,
                            const int32_t* frame_lens, int B, int Tp, int blank, const int32_t* tokens, const int32_t* n_tokens,
                            int max_tokens, int32_t* frame_token, int32_t* begin, int32_t* end, int32_t* peak, float* conf,
                            float* score, int32_t* status, void* workspace, hipStream_t st) {
  float* emis = reinterpret_cast<float*>(static_cast<char*>(workspace) + align_layout(B, Tp, max_tokens).emis);
  const PagedRows table{slab, page_off, pages, P, V};
  const long long rows = (long long)B * Tp;
  if (rows > 0)
    PPASR_LAUNCH(align_gather_paged_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, table, frame_lens, rows, Tp, blank,
                 tokens, n_tokens, max_tokens, align_row_stride(max_tokens), emis);
  launch_ctc_chain(table, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, frame_token, begin, end, peak, conf, score,
                   status, workspace, st);
}

void launch_arena_append(const float* probs, int n, int c, int V, int P, const int32_t* first, const int32_t* count,
                         const int32_t* page_off, const int32_t* pages, float* slab, hipStream_t st) {
  PPASR_LAUNCH(arena_append_kernel, dim3((unsigned)n * c), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(probs), c, V, P,
               first, count, page_off, pages, reinterpret_cast<uint32_t*>(slab));
}

void launch_arena_read(const float* slab, int V, int P, const int32_t* pages, int T, float* dense, hipStream_t st) {
  PPASR_LAUNCH(arena_read_kernel, dim3((unsigned)T), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(slab), V, P, pages,
               reinterpret_cast<uint32_t*>(dense));
}

void launch_arena_read_many(const float* slab, int V, int P, const int32_t* count, const int32_t* page_off, const int32_t* pages,
                            int n, int Tp, float* dense, int32_t* lens, hipStream_t st) {
  PPASR_LAUNCH(arena_read_many_kernel, dim3((unsigned)n * (Tp > 0 ? Tp : 1)), dim3(256), 0, st,
               reinterpret_cast<const uint32_t*>(slab), V, P, count, page_off, pages, Tp, reinterpret_cast<uint32_t*>(dense), lens);
}

}  // namespace ppasr
