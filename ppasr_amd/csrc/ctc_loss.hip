// ctc_loss.hip -- CTC negative log-likelihood on the device: -log of the summed probability of every alignment of a token
// sequence through a [B, Tp, V] table of CTC probabilities (the forward half of the reference's CTCLoss; no backward pass).
//
// DEFINITION (the one tests/loss_oracle.py restates in numpy).  It is ctc_align.hip's with the maximum replaced by a log-sum.
//   Inputs: probs [B, Tp, V] f32; frame_lens [B] i32 or NULL (= Tp), clamped to [0, Tp]; tokens [B, max_tokens] i32;
//   n_tokens [B] i32.  For utterance b let T = frame_lens[b], L = n_tokens[b], tok = tokens[b, 0..L).
//   Bad input (status 2): L outside [0, max_tokens], or a tok[l] outside [0, V) or equal to `blank`.  Nothing is clamped.
//   Trellis: states s = 0 .. 2L; even states are blank, odd state 2l+1 is token l; label(s) = blank or tok[l].
//     e(t, s) = logf(max(p[t, label(s)], FLT_MIN))      accurate logf; the clamp makes 0 and denormals finite
//   Transitions into s at frame t: from s (stay), from s-1 (step), and from s-2 (skip) for odd s with label(s) != label(s-2).
//   Start in state 0 or 1, end in state 2L or (L > 0) 2L-1.
//     a(0, s) = e(0, s) for s in {0, 1}, -inf elsewhere
//     a(t, s) = log sum exp over the transitions of a(t-1, .), plus e(t, s)
//     nll = -log(exp a(T-1, 2L) + exp a(T-1, 2L-1))
//   The value is the float64 one; fp32 here, accurate expf / logf, log-sum as m + logf(sum expf(x - m)) around the largest
//   term m, and -inf when every term is -inf (never NaN).
//   Feasible iff T >= L + #{l >= 1 : tok[l] == tok[l-1]}; otherwise status 1.  L = 0 with T = 0 is feasible: nll 0.
//   Status 1 or 2: nll = +inf.
//
// FORM.  Two launches.
//   The alignment's gather (ctc_align.hip, launch_ctc_gather) writes e(t, .) of the utterance's tokens and of blank into a
//     dense row of the workspace.
//   loss_chain_kernel: one wave per utterance, as align_chain_kernel.  Lane i owns the (blank 2l, token 2l+1) pairs
//     l = 4i .. 4i+3 in registers; the score of token 4i-1 arrives by one DPP wave_shr:1 move per frame.  No back-pointers,
//     no LDS and no barrier; emission rows are loaded kAhead = 16 frames ahead.  Per frame and lane: 8 log-sums
//     (5 or 6 expf and 2 logf per pair).
//   A result is a function of its own utterance only: no atomics, and no word of the workspace or of an output is read
//   before this call wrote it.
#include "ctc_loss.h"

#include "launch.h"

namespace ppasr {
namespace {

constexpr int kAhead = 16;  // frames of emissions in flight per lane (5 registers each)

__device__ __forceinline__ float lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == kNegInf) return kNegInf;
  return m + logf(expf(a - m) + expf(b - m));
}
__device__ __forceinline__ float lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c);
  if (m == kNegInf) return kNegInf;
  return m + logf(expf(a - m) + expf(b - m) + expf(c - m));
}

struct Emis {
  float4 v;  // e(t, token 4i .. 4i+3) of lane i
  float eb;  // e(t, blank)
};

__global__ __launch_bounds__(64) void loss_chain_kernel(const int32_t* __restrict__ frame_lens, int Tp, int V, int blank,
                                                        const int32_t* __restrict__ tokens, const int32_t* __restrict__ n_tokens,
                                                        int max_tokens, int stride, const float* __restrict__ emis,
                                                        float* __restrict__ nll, int32_t* __restrict__ status) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int T = clamp_frames(frame_lens, b, Tp);
  const int Lraw = n_tokens[b];
  const bool len_bad = Lraw < 0 || Lraw > max_tokens;
  const int L = len_bad ? 0 : Lraw;
  const int32_t* tk = tokens + (size_t)b * max_tokens;  // (never dereferenced when L == 0)

  bool bad = false;
  int reps = 0;
  unsigned skip_ok = 0;  // bit k: token 4i+k differs from the token before it (the skip into its state is allowed)
  int before = (4 * lane >= 1 && 4 * lane - 1 < L) ? tk[4 * lane - 1] : -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int l = 4 * lane + k;
    const int tok = l < L ? tk[l] : -1;
    if (l < L) {
      if ((unsigned)tok >= (unsigned)V || tok == blank) bad = true;
      if (l >= 1) {
        if (tok == before) ++reps;
        else skip_ok |= 1u << k;
      }
    }
    before = tok;
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) reps += __shfl_xor(reps, o);
  const int st = (len_bad || __ballot(bad) != 0ull) ? 2 : (T < L + reps ? 1 : 0);
  if (st != 0 || T == 0) {
    if (lane == 0) {
      nll[b] = st != 0 ? -kNegInf : 0.f;
      status[b] = st;
    }
    return;
  }

  // ---- the chain ----
  const float* erow = emis + (size_t)b * Tp * stride;
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
#pragma unroll
      for (int k = 3; k >= 0; --k) {  // (descending: at[k-1] is still frame t-1's when pair k reads it)
        const float prev_tok = k ? at[k - 1] : in;
        const float ob = ab[k], ot = at[k];
        const float nb = lse2(ob, prev_tok);
        const float nt = lse3(ot, ob, ((skip_ok >> k) & 1u) ? prev_tok : kNegInf);
        ab[k] = blank_on[k] ? nb + cur.eb : kNegInf;
        at[k] = tok_on[k] ? nt + ev[k] : kNegInf;
      }
    }
  }

  // ---- the end: states 2L and 2L-1 ----
  auto pick = [](const float (&a)[4], int k) { return k == 0 ? a[0] : k == 1 ? a[1] : k == 2 ? a[2] : a[3]; };
  const float fin_b = __shfl(pick(ab, L & 3), L >> 2);
  const float fin_t = L > 0 ? __shfl(pick(at, (L - 1) & 3), (L - 1) >> 2) : kNegInf;
  if (lane == 0) {
    nll[b] = -lse2(fin_b, fin_t);
    status[b] = 0;
  }
}

}  // namespace

void launch_ctc_loss(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                     const int32_t* n_tokens, int max_tokens, float* nll, int32_t* status, void* workspace, hipStream_t st) {
  float* emis = static_cast<float*>(workspace);
  launch_ctc_gather(probs, frame_lens, B, Tp, V, blank, tokens, n_tokens, max_tokens, emis, st);
  PPASR_LAUNCH(loss_chain_kernel, dim3(B), dim3(64), 0, st, frame_lens, Tp, V, blank, tokens, n_tokens, max_tokens,
               align_row_stride(max_tokens), emis, nll, status);
}

}  // namespace ppasr
