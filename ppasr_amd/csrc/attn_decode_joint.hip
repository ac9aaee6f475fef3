// attn_decode_joint.hip -- CTC-joint scoring inside the attention beam search (WeNet's `ctc_weight` in its attention beam
// search, its CTCPrefixScorer; ESPnet's joint decoding).  ppasr_attention_decode_joint is ppasr_attention_decode with one
// more term per candidate: how probable it is, under the CTC head, that the transcript STARTS with the candidate's
// hypothesis.  The kernels and the launch loop are those of attn_decode.hip (its top-N pass, selection and finish in their
// kJoint = true instantiation); here are the CTC prefix kernels that loop launches beside them.
//
// SEMANTICS (the tests hold the code to these; everything not said here is the header comment of attn_decode.hip)
//   Emissions.  ctc_probs [B, Tp, V] f32 is the head's softmax output, `blank` its blank column.  For utterance b,
//     T = clamp(out_lens[b], 0, Tp) (Tp when out_lens is NULL: the out_lens of the cross-attention) and
//     x[t][v] = logf(max(p[t][v], FLT_MIN)), the emission of ctc_loss.hip.  Nothing at t >= T is read.
//   State of a hypothesis g (length L, last token `last`).  For t < T, rn[t] and rb[t] are the log-probabilities of all
//     alignments of frames 0 .. t that collapse to exactly g and end in a non-blank / in blank.  For the empty g:
//     rn[t] = -inf, rb[t] = sum_{tau <= t} x[tau][blank], Psi(empty) = 0.
//   Extension by a token c, c != blank and c != eos.
//     phi[t]  = rb[t] if c == last, else lse(rn[t], rb[t]);  phi[-1] = 0 if L == 0, else -inf
//     rn'[t]  = lse(rn'[t-1], phi[t-1]) + x[t][c]
//     rb'[t]  = lse(rn'[t-1], rb'[t-1]) + x[t][blank]         rn'[-1] = rb'[-1] = -inf
//     Psi(g.c) = lse_{t = 0 .. T-1} (phi[t-1] + x[t][c])
//     lse of nothing, or of terms that are all -inf, is -inf, never NaN.  exp Psi(g.c) is the probability that the
//     collapsed transcript starts with g.c, and exp Psi(g) = P_ctc(g) + sum_{c != blank} exp Psi(g.c).
//   Special candidates.  Psi(g.blank) = -inf.  Psi(g.eos) = lse(rn[T-1], rb[T-1]) = log P_ctc(g); at T == 0 it is 0 for
//     the empty g and -inf otherwise.  Column V - 1 of the table is never read as a token.
//   The step.  A live row k with hypothesis g computes in fp32, with logp_att the log-softmax of attn_decode.hip,
//       comb[v] = logp_att[v] + (float)ctc_weight * (Psi(g.v) - Psi(g))          (one multiply, then one add)
//     and offers its N largest FINITE entries, largest first, lower id first on equal values, each with score
//     s[k] + (double)comb[v].  Entries at -inf are not offered: a row may offer fewer than N candidates, and an utterance
//     may select fewer than N finite ones.  The remaining new rows are at -inf, not ended and not live, with an empty
//     hypothesis in the outputs, and their trace entries stay at "nothing happened".  Ended rows, the selection, the tie
//     rule on k * N + j, stopping and the outputs are those of attn_decode.hip.  A reported score is therefore
//     sum logp_att + ctc_weight * Psi(final hypothesis), the eos terms included.
//   Taps.  token_logp holds the ATTENTION summand logp_att[v] of every position, token_ctc [B, N, max_steps + 1] f32 the
//     CTC difference Psi(g.v) - Psi(g) of the same position (before the weight), so that
//     score = sum (token_logp + (float)ctc_weight * token_ctc) up to the rounding of comb.  trace_ctc [max_steps, B, N]
//     f32: Psi of each new row's hypothesis (a carried-over ended row keeps its own); 0.0 where nothing happened.
//   ctc_weight == 0.  launch_attention_decode runs, nothing else: no CTC kernel is launched, no 0 * inf is formed, and
//     every output equals ppasr_attention_decode's bit for bit (token_ctc and trace_ctc are 0.0 throughout).
//
// LAUNCHES.  Before the first step, k_aj_init (the empty hypothesis' state of row 0 of every utterance) beside those of
// attn_decode.hip.  Per step, behind the decoder's 5 L + 1 launches:
//   k_aj_psi     Psi(g.v) of every (live row, v): the hot pass.  A workgroup owns one utterance and 256 vocabulary
//                columns.  Per utterance this is an [N, T] x [T, V] contraction in the log semiring: phi of the N rows is
//                staged in LDS kFrames frames at a time, a thread owns one column v, reads x[t][v] once per frame
//                (coalesced over the workgroup) and keeps the running maximum and the scaled sum of all N rows in
//                registers: one expf per term.  The column v == last of a row takes rb in place of phi.
//                Why the log domain: a probability-domain product scaled by the row's largest phi loses every term whose
//                phi lies more than e^-87 below it, and a candidate whose emission is FLT_MIN exactly where phi peaks
//                gets its whole mass from such terms (the "extreme" table of the tests).
//   k_ad_topn<true>    the log-softmax as in the plain mode, comb, and the row's N largest finite entries
//   k_ad_select<true>  the selection with rows at -inf, Psi of the new rows and the two summands
//   k_aj_update  rn' / rb' of the new live rows only: the N chosen (parent, token) pairs, one wave each, the frames in
//                order (the recurrence is sequential in t)
// and k_ad_finish<true> once at the end.  No atomics; a row's result depends on its own inputs only; every word that is
// read was written by this call; a workgroup of a finished utterance returns at its first flag read.
#include <float.h>
#include <math.h>

#include "attn_decode.h"
#include "launch.h"

namespace ppasr {
namespace {

constexpr int kFrames = 64;  // frames of phi staged in LDS at a time

__device__ __forceinline__ float emission(float p) { return logf(p >= FLT_MIN ? p : FLT_MIN); }  // (a denormal clamps too)

__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (!(m > -INFINITY)) return -INFINITY;
  return m + log1pf(expf(fminf(a, b) - m));
}

// one more term `a` into the running (maximum m, sum s of exp(term - m)): one expf
__device__ __forceinline__ void lse_push(float& m, float& s, float a) {
  const float e = expf(-fabsf(a - m));  // (NaN when both are -inf: not selected below)
  const bool gt = a > m;
  s = gt ? fmaf(s, e, 1.0f) : (a > -INFINITY ? s + e : s);
  m = gt ? a : m;
}

__device__ __forceinline__ int frames_of(const int32_t* __restrict__ out_lens, int b, int Tp) {
  return out_lens ? min(max(out_lens[b], 0), Tp) : Tp;
}

// the empty hypothesis: row 0 of every utterance, state buffer 0
__global__ __launch_bounds__(64) void k_aj_init(AttDecDims d, AttJointBufs jb) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = frames_of(jb.out_lens, b, d.Tp);
  for (int k = lane; k < d.N; k += 64) jb.psi[0][b * d.N + k] = 0.f;
  float* st = jb.state[0] + (size_t)b * d.N * d.Tp * 2;
  const float* pb = jb.probs + (size_t)b * d.Tp * jb.V + jb.blank;
  float acc = 0.f;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int nt = min(64, T - t0);
    const float x = lane < nt ? emission(pb[(size_t)(t0 + lane) * jb.V]) : 0.f;
    float mine = 0.f;
    for (int j = 0; j < nt; ++j) {  // frames in order: one add per frame
      acc += __shfl(x, j);
      if (j == lane) mine = acc;
    }
    if (lane < nt) {
      st[(size_t)(t0 + lane) * 2] = -INFINITY;
      st[(size_t)(t0 + lane) * 2 + 1] = mine;
    }
  }
}

// Psi(g.v) of every live row of utterance blockIdx.x and the 256 columns of blockIdx.y; NR: rows held in registers
template <int NR>
__global__ __launch_bounds__(256) void k_aj_psi(AttDecDims d, AttDecBufs bf, AttJointBufs jb, int step, int Vp) {
  __shared__ float2 s_ph[kFrames][NR];  // (phi[t-1], rb[t-1]) of frame t and live row k
  __shared__ int s_row[NR], s_last[NR];
  __shared__ int s_nl;
  const int b = blockIdx.x;
  if (bf.utt_live[b] == 0) return;
  const int N = d.N, V = jb.V, Tp = d.Tp, cur = (step - 1) & 1;
  const int T = frames_of(jb.out_lens, b, Tp);
  const int v = blockIdx.y * 256 + (int)threadIdx.x;
  if (threadIdx.x == 0) {  // the live rows, in row order
    int nl = 0;
    for (int k = 0; k < N; ++k)
      if (bf.live[b * N + k] != 0) {
        s_row[nl] = b * N + k;
        s_last[nl] = bf.last_tok[b * N + k];
        ++nl;
      }
    s_nl = nl;
  }
  __syncthreads();
  const int nl = s_nl;
  const float first = step == 1 ? 0.f : -INFINITY;  // phi[-1]: the hypotheses of step i have i - 1 tokens
  float m[NR], s[NR];
  bool is_last[NR];
#pragma unroll
  for (int k = 0; k < NR; ++k) {
    m[k] = -INFINITY;
    s[k] = 0.f;
    is_last[k] = k < nl && s_last[k] == v;
  }
  const float* pv = jb.probs + (size_t)b * Tp * V + min(v, V - 1);
  for (int t0 = 0; t0 < T; t0 += kFrames) {
    const int nt = min(kFrames, T - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < nt * nl; i += 256) {
      const int tt = i / nl, k = i - tt * nl, t = t0 + tt;
      float2 ph = {first, first};
      if (t > 0) {
        const float2 st = *reinterpret_cast<const float2*>(jb.state[cur] + ((size_t)s_row[k] * Tp + (t - 1)) * 2);
        ph.x = lse2(st.x, st.y);
        ph.y = st.y;
      }
      s_ph[tt][k] = ph;
    }
    __syncthreads();
    for (int tt = 0; tt < nt; ++tt) {
      const float x = emission(pv[(size_t)(t0 + tt) * V]);
#pragma unroll
      for (int k = 0; k < NR; ++k)
        if (k < nl) {
          const float2 ph = s_ph[tt][k];
          lse_push(m[k], s[k], (is_last[k] ? ph.y : ph.x) + x);
        }
    }
  }
  if (v >= V) return;
#pragma unroll
  for (int k = 0; k < NR; ++k)
    if (k < nl) {
      float psi = m[k] > -INFINITY ? m[k] + logf(s[k]) : -INFINITY;
      if (v == jb.blank) psi = -INFINITY;
      if (v == V - 1) {  // eos: log P_ctc(g)
        if (T == 0) {
          psi = first;
        } else {
          const float2 st = *reinterpret_cast<const float2*>(jb.state[cur] + ((size_t)s_row[k] * Tp + (T - 1)) * 2);
          psi = lse2(st.x, st.y);
        }
      }
      jb.cpsi[(size_t)s_row[k] * Vp + v] = psi;
    }
}

// rn' / rb' of a new live row from its parent's state and its token: a wave per row, the frames in order
__global__ __launch_bounds__(64) void k_aj_update(AttDecDims d, AttDecBufs bf, AttJointBufs jb, int step) {
  const int nr = blockIdx.x;
  if (bf.live[nr] == 0) return;
  const int N = d.N, R = d.R(), Tp = d.Tp, V = jb.V, p = step - 1, lane = threadIdx.x;
  const int b = nr / N, cur = (step - 1) & 1, nw = step & 1;
  const int par = b * N + bf.tr_par[(size_t)p * R + nr];
  const int c = bf.last_tok[nr];
  const int last = p > 0 ? bf.tr_tok[(size_t)(p - 1) * R + par] : -1;  // the parent's newest token
  const int T = frames_of(jb.out_lens, b, Tp);
  const float* sp = jb.state[cur] + (size_t)par * Tp * 2;
  float* sn = jb.state[nw] + (size_t)nr * Tp * 2;
  const float* pb = jb.probs + (size_t)b * Tp * V;
  float rn = -INFINITY, rb = -INFINITY, phi = p == 0 ? 0.f : -INFINITY;  // index t - 1
  for (int t0 = 0; t0 < T; t0 += 64) {
    const int nt = min(64, T - t0), t = t0 + lane;
    float xc = 0.f, xb = 0.f, ph = 0.f;
    if (lane < nt) {
      xc = emission(pb[(size_t)t * V + c]);
      xb = emission(pb[(size_t)t * V + jb.blank]);
      const float2 st = *reinterpret_cast<const float2*>(sp + (size_t)t * 2);
      ph = c == last ? st.y : lse2(st.x, st.y);
    }
    float my_rn = 0.f, my_rb = 0.f;
    for (int j = 0; j < nt; ++j) {
      const float n_rn = lse2(rn, phi) + __shfl(xc, j);
      const float n_rb = lse2(rn, rb) + __shfl(xb, j);
      rn = n_rn;
      rb = n_rb;
      phi = __shfl(ph, j);
      if (j == lane) {
        my_rn = rn;
        my_rb = rb;
      }
    }
    if (lane < nt) *reinterpret_cast<float2*>(sn + (size_t)t * 2) = float2{my_rn, my_rb};
  }
}

template <int NR>
void launch_psi(const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs& jb, int step, int Vp, hipStream_t st) {
  PPASR_LAUNCH(k_aj_psi<NR>, dim3(d.B, (jb.V + 255) / 256), dim3(256), 0, st, d, bf, jb, step, Vp);
}

}  // namespace

void launch_aj_init(const AttDecDims& d, const AttJointBufs& jb, hipStream_t st) {
  PPASR_LAUNCH(k_aj_init, dim3(d.B), dim3(64), 0, st, d, jb);
}

void launch_aj_psi(const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs& jb, int step, int Vp, hipStream_t st) {
  if (d.N <= 8)
    launch_psi<8>(d, bf, jb, step, Vp, st);
  else if (d.N <= 16)
    launch_psi<16>(d, bf, jb, step, Vp, st);
  else
    launch_psi<32>(d, bf, jb, step, Vp, st);
}

void launch_aj_update(const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs& jb, int step, hipStream_t st) {
  PPASR_LAUNCH(k_aj_update, dim3(d.R()), dim3(64), 0, st, d, bf, jb, step);
}

}  // namespace ppasr
