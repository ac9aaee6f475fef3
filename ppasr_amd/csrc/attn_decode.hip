// attn_decode.hip -- attention beam-search decoding (WeNet's `attention` decode mode, `recognize`) with the checkpoint's
// left decoder (transformer/decoder.py of the reference: TransformerDecoder.forward_one_step, which the reference ships
// and never calls).  One ppasr_attention_decode call enqueues every step on the caller's stream and reads nothing back.
//
// SEMANTICS (the tests hold the code to these)
//   Setup.  Per utterance b there are N = beam_size rows.  sos = eos = V - 1.  Only the left decoder runs.  Row k holds
//     tokens hyp[k] (initially empty, decoder input [sos]), a score s[k] (f64) and a flag ended[k].  Initially s[0] = 0,
//     s[k > 0] = -inf, nothing ended.
//   Step i = 1 .. max_steps.  A live row (not ended, finite score) gets logp = log_softmax(output_layer(after_norm(x_last)))
//     over v < V, in fp32, from the decoder over [sos] + hyp[k] and the utterance's memory frames t < out_lens[b].  It
//     offers its N largest entries as candidates (k, j), j = 0 .. N - 1, largest first, lower token id first on equal
//     values, each with score s[k] + (double)logp[v].  An ended row offers one candidate (k, 0) = (eos, s[k]).  A row at
//     -inf offers nothing.
//   Selection.  The N best candidates of the utterance become the new rows in that order; on equal scores the lower
//     k * N + j goes first.  (Fewer than N finite candidates cannot occur: beam_size <= V.)  The new row copies its
//     parent's tokens; if the parent had not ended it appends the candidate's token; ended = parent ended, or the token
//     is eos.
//   Stopping.  An utterance whose rows have all ended does no more work: its rows, scores and order stay as they are
//     while others continue, and its trace entries of later steps stay at "nothing happened".  The search stops when
//     every utterance is done or after max_steps steps; the steps enqueued behind that point change nothing.
//   Outputs.  tokens [B, N, max_steps] i32: the tokens before the first eos, -1 behind them.  lens [B, N] i32.  scores
//     [B, N] f64, best first, the eos term included when the row ended.  ended [B, N] i32: 0 marks a hypothesis cut at
//     max_steps.  steps_run (one i32): the step at which the last row ended, or max_steps.
//   Taps (optional; 0.0 / -1 where nothing happened).  token_logp [B, N, max_steps + 1] f32: the summand of every
//     position of the final hypotheses, eos included.  trace_parent / trace_token / trace_score [max_steps, B, N]
//     i32 / i32 / f64: per step and new row its parent row, its candidate's token (eos for a carried-over ended row) and
//     its score.
//
// LAUNCHES.  Before the first step: k_dec_kv of rescore_kernels.hip over the left decoder's layer slots (the
// cross-attention keys / values, shared by the N rows of an utterance) and k_ad_init.  Per step, for L = num_blocks layers:
//   k_ad_qkv          (layer 0: embedding * 16 + pe of the row's newest token) LayerNorm -> q, and k | v of the NEW
//                     position only into the cache
//   k_ad_attn<true>   self-attention, one query per (row, head) over the prefix's cached keys
//   k_ad_selfout_q    output projection + residual + LayerNorm + cross query
//   k_ad_attn<false>  cross-attention, one query per (row, head) over the utterance's out_lens[b] keys
//   k_ad_crossout_ffn output projection + residual + feed-forward
// then k_ad_output (after_norm + the [256, Vp] output GEMM), k_ad_topn (log-softmax and the row's N largest) and
// k_ad_select (per utterance: selection, ancestry, end flags): 5 L + 3 launches per step, and k_ad_finish once at the end.
// launch_attention_decode is the one loop of both modes: with joint buffers it adds the CTC prefix launches of
// attn_decode_joint.hip (k_aj_init once, k_aj_psi and k_aj_update per step: 5 L + 5) and runs the three search kernels as
// <true>.
//
// ROWS are dense: r = b * N + k, 32 per MFMA tile whatever utterance they belong to (the dense layers are row-local, and
// the one-query attentions do not need rows of one utterance in one tile).  A row's result depends on its own inputs only:
// the same inputs give the same bytes wherever the row sits in a tile.
// CACHE: addressed by (layer, position, utterance, slot); at position p row k writes slot k.  Nothing is copied when the
// beam reorders: every row carries an ancestry list anc[row][j] = slot of its ancestor at position j (one byte each,
// double-buffered because the selection reads the old beam while it writes the new one).
// DONE: the selection keeps live[r] per row and utt_live[b] per utterance.  Every step kernel's workgroup looks at the
// flags of its own rows first and returns at once when none is live, so the steps behind the end of the search cost a
// launch and one flag read per workgroup; that is the device-side "all done" test, held per tile, and nothing is read
// back.  No result depends on what the workspace or the outputs held: every word that is read was written by this call.
#include "attn_decode.h"

#include <math.h>

#include "attn_decode_dev.h"
#include "dec_tile.h"
#include "launch.h"

namespace ppasr {
namespace {

// does tile t hold a live row?  (a barrier: every thread of the workgroup calls it)
__device__ __forceinline__ bool tile_live(const int32_t* __restrict__ live, int R, int t) {
  const int r = t * 32 + (int)threadIdx.x;
  return __syncthreads_or(threadIdx.x < 32 && r < R && live[r] != 0) != 0;
}

__global__ __launch_bounds__(256) void k_ad_init(AttDecDims d, AttDecBufs bf, int V) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < d.Rp()) {
    const bool first = r < d.R() && r % d.N == 0;
    bf.live[r] = first ? 1 : 0;
    bf.last_tok[r] = V - 1;
    if (r < d.R()) {
      bf.score[0][r] = first ? 0.0 : -INFINITY;
      bf.ended[0][r] = 0;
    }
  }
  if (r < d.B) {
    bf.utt_live[r] = 1;
    bf.utt_steps[r] = 0;
  }
}

// ---- LayerNorm -> q, and k | v of the new position into the cache ------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_ad_qkv(RescoreW W, AttDecDims d, AttDecBufs bf, int layer, int p) {
  __shared__ float a[kTileLds];
  __shared__ int s_live[32];
  const int t = blockIdx.x;
  if (!tile_live(bf.live, d.R(), t)) return;
  const DecSideW& S = W.side[0];
  const DecLayerW lw = S.layers[layer];
  const int lane = lane_id(), w = wave_id();
  if (threadIdx.x < 32) {
    const int r = t * 32 + threadIdx.x;
    s_live[threadIdx.x] = r < d.R() && bf.live[r] != 0;
  }
  if (layer == 0) {  // the row's newest token at position p; rows that do not run are 0
    for (int i = w; i < 32; i += kWaves) {
      const int r = t * 32 + i;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < d.R() && bf.live[r] != 0) {
        const int tok = min(max(bf.last_tok[r], 0), W.V - 1);
        const f32x4 e = *reinterpret_cast<const f32x4*>(S.embed + (size_t)tok * kD + 4 * lane);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(W.pe + (size_t)p * kD + 4 * lane);
        v = e * 16.0f + pe;  // sqrt(256)
      }
      *reinterpret_cast<f32x4*>(a + i * kLda + 4 * lane) = v;
      *reinterpret_cast<f32x4*>(bf.x + (size_t)r * kD + 4 * lane) = v;
    }
  } else {
    rb_load_rows(a, kLda, bf.x + (size_t)t * 32 * kD, 32, 32);
  }
  __syncthreads();
  rb_layernorm(a, a, kLda, 32, lw.n1g, lw.n1b, kLnEps);
  __syncthreads();
  float* cache_p = bf.cache + ((size_t)layer * d.P + p) * d.R() * 512;
  for (int j = 0; j < 3; ++j) {
    f32x16 acc[1][1];
    const int nt = j * 8 + w;
    gemm256(a, lw.wqkv + (size_t)nt * kTs256, acc);
    const int col = nt * 32 + (lane & 31);
    const float bias = lw.bqkv[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, lane);
      const float v = acc[0][0][r] + bias;
      if (j == 0)
        bf.q[((size_t)t * 32 + row) * kD + col] = v;
      else if (s_live[row])
        cache_p[((size_t)t * 32 + row) * 512 + (col - 256)] = v;
    }
  }
}

// ---- one-query attention of a (row, head): a wave per head, a key per lane 64 at a time, online softmax ------------------
// kSelf: keys 0 .. p of the row's prefix, key j in the cache slot anc[row][j] (j == p: the row's own slot).
// !kSelf: keys t < out_lens[b] of the utterance's cross-attention k | v.
template <bool kSelf>
__global__ __launch_bounds__(256) void k_ad_attn(AttDecDims d, AttDecBufs bf, int layer, int p, int cur, int n_left,
                                                 const int32_t* __restrict__ out_lens) {
  __shared__ float s_p[4][64];
  __shared__ size_t s_off[4][64];
  const int r = blockIdx.x;
  if (bf.live[r] == 0) return;
  const int b = r / d.N, lane = lane_id(), head = wave_id();
  const int n = kSelf ? p + 1 : (out_lens ? min(max(out_lens[b], 0), d.Tp) : d.Tp);
  const float* base = kSelf ? bf.cache : bf.kv;
  float q[64];
  {
    const float* qp = (kSelf ? bf.q : bf.qc) + (size_t)r * kD + head * 64;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + c);
      q[c] = v[0] * 0.125f; q[c + 1] = v[1] * 0.125f; q[c + 2] = v[2] * 0.125f; q[c + 3] = v[3] * 0.125f;
    }
  }
  float m = -INFINITY, s = 0.f, acc = 0.f;  // acc: channel `lane` of the head
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int nj = min(64, n - j0), j = j0 + lane;
    float sc = -INFINITY;
    size_t off = 0;
    if (j < n) {
      if (kSelf) {
        const int slot = j == p ? r - b * d.N : (int)bf.anc[cur][(size_t)r * 256 + j];
        off = (((size_t)layer * d.P + j) * d.R() + (size_t)b * d.N + slot) * 512 + head * 64;
      } else {
        off = ((size_t)b * d.Tp + j) * (512 * (size_t)n_left) + (size_t)layer * 512 + head * 64;
      }
      const float* kp = base + off;
      sc = 0.f;
#pragma unroll
      for (int c = 0; c < 64; c += 4) {
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(kp + c);
        sc = fmaf(q[c], k4[0], sc); sc = fmaf(q[c + 1], k4[1], sc); sc = fmaf(q[c + 2], k4[2], sc); sc = fmaf(q[c + 3], k4[3], sc);
      }
    }
    const float mn = fmaxf(m, wave_max(sc));  // finite: lane 0's key exists
    const float f = expf(m - mn), pj = j < n ? expf(sc - mn) : 0.f;
    __syncthreads();  // (the loop count is the row's: the same for the four heads)
    s_p[head][lane] = pj;
    s_off[head][lane] = off + 256;
    __syncthreads();
    float ps = 0.f;
    acc *= f;
    for (int jj = 0; jj < nj; ++jj) {  // keys in order: the sums do not depend on the lane
      const float pv = s_p[head][jj];
      ps += pv;
      acc = fmaf(pv, base[s_off[head][jj] + lane], acc);
    }
    s = s * f + ps;
    m = mn;
  }
  bf.ctx[(size_t)r * kD + head * 64 + lane] = s > 0.f ? acc / s : 0.f;  // no valid frame: attends to nothing
}

// x += self_attn.linear_out(ctx); qc = src_attn.linear_q(norm2(x))
__global__ __launch_bounds__(kThreads) void k_ad_selfout_q(RescoreW W, AttDecDims d, AttDecBufs bf, int layer) {
  __shared__ float a[kTileLds];
  const int t = blockIdx.x;
  if (!tile_live(bf.live, d.R(), t)) return;
  dec_selfout_q_tile(W.side[0].layers[layer], a, bf.ctx, bf.x, bf.qc, t);
}

// x += src_attn.linear_out(ctx); x += w_2(relu(w_1(norm3(x)))) with the hidden layer 256 units at a time through LDS
__global__ __launch_bounds__(kThreads) void k_ad_crossout_ffn(RescoreW W, AttDecDims d, AttDecBufs bf, int layer) {
  extern __shared__ float lds[];
  float* a = lds;
  float* hb = lds + kTileLds;
  const int t = blockIdx.x;
  if (!tile_live(bf.live, d.R(), t)) return;
  dec_crossout_ffn_tile(W.side[0].layers[layer], W.U, a, hb, bf.ctx, bf.x, t);
}

// after_norm -> 256 columns of output_layer per workgroup: logits [Rp][Vp] (columns v < V only)
__global__ __launch_bounds__(kThreads) void k_ad_output(RescoreW W, AttDecDims d, AttDecBufs bf) {
  __shared__ float a[kTileLds];
  const int t = blockIdx.x;
  if (!tile_live(bf.live, d.R(), t)) return;
  const DecSideW& S = W.side[0];
  const int lane = lane_id(), w = wave_id();
  rb_load_rows(a, kLda, bf.x + (size_t)t * 32 * kD, 32, 32);
  __syncthreads();
  rb_layernorm(a, a, kLda, 32, S.ang, S.anb, kLnEps);
  __syncthreads();
  f32x16 acc[1][1];
  const int nt = blockIdx.y * 8 + w;
  gemm256(a, S.wout + (size_t)nt * kTs256, acc);
  const int col = nt * 32 + (lane & 31);
  if (col < W.V) {
    const float bias = S.bout[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) bf.logits[((size_t)t * 32 + acc_row(r, lane)) * W.Vp + col] = acc[0][0][r] + bias;
  }
}

// The three search kernels serve both modes: kJoint = false is the search of the SEMANTICS above, kJoint = true the
// CTC-joint one (attn_decode_joint.hip says what differs); jb is read only when kJoint.

// log-softmax over v < V of a live row and its N largest entries, largest first, lower id first on equal values.
// The rounds compare the raw logit (the same order as lg - lse, without its rounding); kJoint: comb, finite entries only
template <bool kJoint>
__global__ __launch_bounds__(256) void k_ad_topn(AttDecDims d, AttDecBufs bf, AttJointBufs jb, int step, int V, int Vp) {
  __shared__ float s_v[4];
  __shared__ int s_i[4];
  __shared__ float s_sum[256];
  const int r = blockIdx.x;
  if (bf.live[r] == 0) return;
  const float* lg = bf.logits + (size_t)r * Vp;
  float mv = -INFINITY;
  int mi = V;
  for (int v = threadIdx.x; v < V; v += 256) {
    const float x = lg[v];
    if (cand_before(x, v, mv, mi)) {
      mv = x;
      mi = v;
    }
  }
  block_first(mv, mi, s_v, s_i);
  const float M = mv;
  float sum = 0.f;
  for (int v = threadIdx.x; v < V; v += 256) sum += expf(lg[v] - M);
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {  // a fixed tree: the sum depends on the row's logits only
    if ((int)threadIdx.x < o) s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
    __syncthreads();
  }
  const float lse = M + logf(s_sum[0]);
  const float* cp = kJoint ? jb.cpsi + (size_t)r * Vp : nullptr;
  const float psig = kJoint ? jb.psi[(step - 1) & 1][r] : 0.f;
  auto key = [&](int v) {
    if constexpr (kJoint)
      return __fadd_rn(lg[v] - lse, __fmul_rn(jb.weight, cp[v] - psig));
    else
      return lg[v];
  };
  // round j takes the first entry behind round j - 1's in the order (plain: round 0 is the maximum found above)
  float pv = kJoint ? INFINITY : mv;
  int pi = kJoint ? -1 : mi;
  for (int j = 0; j < d.N; ++j) {
    if (kJoint || j > 0) {
      float bv = -INFINITY;
      int bi = V;
      for (int v = threadIdx.x; v < V; v += 256) {
        const float x = key(v);
        if ((!kJoint || x > -INFINITY) && cand_before(pv, pi, x, v) && cand_before(x, v, bv, bi)) {
          bv = x;
          bi = v;
        }
      }
      block_first(bv, bi, s_v, s_i);
      pv = bv;
      pi = bi;
    }
    if (threadIdx.x == 0) {
      const size_t ci = (size_t)r * d.N + j;
      const int tok = min(pi, V - 1);
      bf.cand_lp[ci] = kJoint ? pv : pv - lse;  // kJoint: -inf when nothing is left to offer
      bf.cand_tok[ci] = tok;
      if constexpr (kJoint) {
        jb.cand_att[ci] = lg[tok] - lse;
        jb.cand_psi[ci] = cp[tok];
      }
    }
  }
}

// per utterance: the N best of its candidates become the new rows (state buffer nw = step & 1 from cur = (step - 1) & 1).
// kJoint: fewer than N finite candidates leave rows at -inf (`some`), Psi of the new rows and the two summands
template <bool kJoint>
__global__ __launch_bounds__(1024) void k_ad_select(AttDecDims d, AttDecBufs bf, AttJointBufs jb, int step, int V,
                                                    AttDecOut out) {
  __shared__ double s_sc[kAttDecMaxBeam * kAttDecMaxBeam];
  __shared__ int s_par[kAttDecMaxBeam], s_nlive[kAttDecMaxBeam];
  const int b = blockIdx.x;
  if (bf.utt_live[b] == 0) return;
  const int N = d.N, NN = N * N, R = d.R(), p = step - 1;
  const int cur = (step - 1) & 1, nw = step & 1;
  const int c = threadIdx.x, k = c / N, j = c - k * N;
  double val = -INFINITY;
  int tok = V - 1, was_ended = 0;
  float lp = 0.f;  // the attention summand
  [[maybe_unused]] float cpsi = 0.f, psig = 0.f;
  if (c < NN) {
    const int r = b * N + k;
    const double s = bf.score[cur][r];
    was_ended = bf.ended[cur][r];
    if (was_ended) {
      if (j == 0) {
        val = s;
        if constexpr (kJoint) psig = jb.psi[cur][r];
      }
    } else if (s > -INFINITY) {
      const float key = bf.cand_lp[(size_t)r * N + j];
      if (!kJoint || key > -INFINITY) {
        tok = bf.cand_tok[(size_t)r * N + j];
        if constexpr (kJoint) {
          lp = jb.cand_att[(size_t)r * N + j];
          cpsi = jb.cand_psi[(size_t)r * N + j];
          psig = jb.psi[cur][r];
        } else {
          lp = key;
        }
        val = s + (double)key;
      }
    }
    s_sc[c] = val;
  }
  __syncthreads();
  if (c < NN) {
    int rank = 0;
    for (int o = 0; o < NN; ++o) {
      const double v = s_sc[o];
      rank += (v > val || (v == val && o < c)) ? 1 : 0;
    }
    if (rank < N) {
      const int nr = b * N + rank;
      const bool some = kJoint ? val > -INFINITY : true;
      const int e = (some && (was_ended || tok == V - 1)) ? 1 : 0;
      const int lv = (!e && val > -INFINITY) ? 1 : 0;
      bf.score[nw][nr] = val;
      bf.ended[nw][nr] = e;
      bf.live[nr] = lv;
      bf.last_tok[nr] = some ? tok : V - 1;
      const size_t ti = (size_t)p * R + nr;
      bf.tr_par[ti] = k;
      bf.tr_tok[ti] = some ? tok : V - 1;
      bf.tr_lp[ti] = (some && !was_ended) ? lp : 0.f;
      [[maybe_unused]] float npsi = 0.f;
      if constexpr (kJoint) {
        npsi = some ? (was_ended ? psig : cpsi) : 0.f;
        jb.psi[nw][nr] = npsi;
        jb.tr_ctc[ti] = (some && !was_ended) ? cpsi - psig : 0.f;
      }
      if (some) {
        if (out.trace_parent) out.trace_parent[ti] = k;
        if (out.trace_token) out.trace_token[ti] = tok;
        if (out.trace_score) out.trace_score[ti] = val;
        if constexpr (kJoint)
          if (jb.trace_ctc) jb.trace_ctc[ti] = npsi;
      }
      s_par[rank] = k;
      s_nlive[rank] = lv;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N * (p + 1); i += blockDim.x) {
    const int kn = i / (p + 1), jj = i - kn * (p + 1), par = s_par[kn];
    bf.anc[nw][((size_t)b * N + kn) * 256 + jj] = jj < p ? bf.anc[cur][((size_t)b * N + par) * 256 + jj] : (uint8_t)par;
  }
  if (threadIdx.x == 0) {
    int nl = 0;
    for (int i = 0; i < N; ++i) nl += s_nlive[i];
    bf.utt_live[b] = nl;
    bf.utt_steps[b] = step;
  }
}

// the final hypotheses, read from the back-pointers; kJoint: a row at -inf has an empty hypothesis, and the CTC tap
template <bool kJoint>
__global__ __launch_bounds__(64) void k_ad_finish(AttDecDims d, AttDecBufs bf, AttJointBufs jb, int V, AttDecOut out) {
  const int b = blockIdx.x, N = d.N, R = d.R(), P = d.P;
  const int steps = bf.utt_steps[b], buf = steps & 1;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const int r = b * N + k;
    const double sc = bf.score[buf][r];
    const int from = kJoint ? (sc > -INFINITY ? steps : 0) : steps;
    out.scores[r] = sc;
    out.ended[r] = bf.ended[buf][r];
    for (int i = from; i < P; ++i) out.tokens[(size_t)r * P + i] = -1;
    if (out.token_logp)
      for (int i = from; i <= P; ++i) out.token_logp[(size_t)r * (P + 1) + i] = 0.f;
    if constexpr (kJoint)
      if (jb.token_ctc)
        for (int i = from; i <= P; ++i) jb.token_ctc[(size_t)r * (P + 1) + i] = 0.f;
    int curk = k, len = 0;
    for (int i = from; i >= 1; --i) {
      const size_t ti = (size_t)(i - 1) * R + b * N + curk;
      const int tok = bf.tr_tok[ti];
      out.tokens[(size_t)r * P + i - 1] = tok != V - 1 ? tok : -1;
      len += tok != V - 1 ? 1 : 0;
      if (out.token_logp) out.token_logp[(size_t)r * (P + 1) + i - 1] = bf.tr_lp[ti];
      if constexpr (kJoint)
        if (jb.token_ctc) jb.token_ctc[(size_t)r * (P + 1) + i - 1] = jb.tr_ctc[ti];
      curk = bf.tr_par[ti];
    }
    out.lens[r] = len;
  }
  if (b == 0 && threadIdx.x == 0) {
    int mx = 0;
    for (int i = 0; i < d.B; ++i) mx = max(mx, bf.utt_steps[i]);
    out.steps_run[0] = mx;
  }
}

template <bool kJoint>
void launch_search(const RescoreW& W, const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs& jb, int step,
                   const AttDecOut& out, hipStream_t st) {
  PPASR_LAUNCH(k_ad_topn<kJoint>, dim3(d.R()), dim3(256), 0, st, d, bf, jb, step, W.V, W.Vp);
  PPASR_LAUNCH(k_ad_select<kJoint>, dim3(d.B), dim3(1024), 0, st, d, bf, jb, step, W.V, out);
}

}  // namespace

void launch_attention_decode(const RescoreW& W, const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs* joint,
                             const float* memory, const int32_t* out_lens, const AttDecOut& out, hipStream_t st) {
  const AttJointBufs jb = joint ? *joint : AttJointBufs{};
  const int L = W.n_left, R = d.R(), tiles = d.Rp() / 32;
  launch_dec_kv(W, d.B, d.Tp, L, memory, out_lens, bf.kv, st);
  PPASR_LAUNCH(k_ad_init, dim3(((d.Rp() > d.B ? d.Rp() : d.B) + 255) / 256), dim3(256), 0, st, d, bf, W.V);
  if (joint) launch_aj_init(d, jb, st);
  for (int step = 1; step <= d.P; ++step) {
    const int p = step - 1, cur = (step - 1) & 1;
    for (int l = 0; l < L; ++l) {
      PPASR_LAUNCH(k_ad_qkv, dim3(tiles), dim3(kThreads), 0, st, W, d, bf, l, p);
      PPASR_LAUNCH(k_ad_attn<true>, dim3(R), dim3(256), 0, st, d, bf, l, p, cur, L, out_lens);
      PPASR_LAUNCH(k_ad_selfout_q, dim3(tiles), dim3(kThreads), 0, st, W, d, bf, l);
      PPASR_LAUNCH(k_ad_attn<false>, dim3(R), dim3(256), 0, st, d, bf, l, p, cur, L, out_lens);
      PPASR_LAUNCH(k_ad_crossout_ffn, dim3(tiles), dim3(kThreads), kFfnLds, st, W, d, bf, l);
    }
    PPASR_LAUNCH(k_ad_output, dim3(tiles, W.Vp / 256), dim3(kThreads), 0, st, W, d, bf);
    if (joint) {
      launch_aj_psi(d, bf, jb, step, W.Vp, st);
      launch_search<true>(W, d, bf, jb, step, out, st);
      launch_aj_update(d, bf, jb, step, st);
    } else {
      launch_search<false>(W, d, bf, jb, step, out, st);
    }
  }
  if (joint)
    PPASR_LAUNCH(k_ad_finish<true>, dim3(d.B), dim3(64), 0, st, d, bf, jb, W.V, out);
  else
    PPASR_LAUNCH(k_ad_finish<false>, dim3(d.B), dim3(64), 0, st, d, bf, jb, W.V, out);
}

hipError_t configure_attention_decode_kernels() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_ad_crossout_ffn), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kFfnLds);
}

}  // namespace ppasr
