// attn_decode.h -- attention beam-search decoding with the left decoder (attn_decode.hip, capi_attdecode.hip): the
// workspace views and the launcher of one ppasr_attention_decode / ppasr_attention_decode_joint call.  Semantics: header
// comments of attn_decode.hip and attn_decode_joint.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rescore_kernels.h"

namespace ppasr {

constexpr int kAttDecMaxBeam = 32;

struct AttDecDims {
  int B, Tp, N, P;  // utterances, memory frames, beam_size, max_steps
  __host__ __device__ int R() const { return B * N; }                   // rows, dense: r = b * N + k
  __host__ __device__ int Rp() const { return (B * N + 31) / 32 * 32; }  // rows of the activation buffers (whole tiles)
};

struct AttDecBufs {
  float *x, *q, *ctx, *qc;   // [Rp][256]: the new position's activations
  float* kv;                 // [B * Tp][512 * n_left]: cross-attention k | v per layer
  float* cache;              // [n_left][P][R][512]: self-attention k | v by (layer, position, utterance, slot)
  float* logits;             // [Rp][Vp]
  float* cand_lp;            // [R][N] the row's N largest log-probabilities, largest first
  int32_t* cand_tok;         // [R][N]
  double* score[2];          // [R]   (beam state, double-buffered: step i reads (i - 1) & 1 and writes i & 1)
  int32_t* ended[2];         // [R]
  uint8_t* anc[2];           // [R][256]: slot of the row's ancestor at every earlier position
  int32_t *live, *last_tok;  // [Rp]: row runs the decoder at this step / its newest token
  int32_t *utt_live, *utt_steps;  // [B]: live rows of the utterance / steps it has run
  int32_t *tr_par, *tr_tok;  // [P][R]: the back-pointers the final hypotheses are read from
  float* tr_lp;              // [P][R]: the summand of that step (0 on a carried-over ended row)
};

struct AttDecOut {
  int32_t *tokens, *lens;
  double* scores;
  int32_t *ended, *steps_run;
  float* token_logp;                      // or nullptr
  int32_t *trace_parent, *trace_token;    // or nullptr
  double* trace_score;                    // or nullptr
};

// the joint mode's share of the workspace and its taps (attn_decode_joint.hip)
struct AttJointBufs {
  const float* probs;   // [B][Tp][V] the CTC head's softmax output
  const int32_t* out_lens;
  int V, blank;
  float weight;         // (float)ctc_weight
  float* state[2];      // [R][Tp][2]: (rn, rb) of the row's hypothesis per frame, double-buffered like the scores
  float* psi[2];        // [R]: Psi of the row's hypothesis
  float* cpsi;          // [R][Vp]: Psi(g . v) of every candidate of a live row
  float *cand_att, *cand_psi;  // [R][N]: the attention log-probability and Psi(g . v) of the row's offers
  float* tr_ctc;        // [P][R]: Psi(g . v) - Psi(g) of that step (0 on a carried-over ended row); tr_lp: logp_att
  float *token_ctc, *trace_ctc;  // taps, or nullptr
};

hipError_t configure_attention_decode_kernels();
// every launch of one call; joint == nullptr: the plain search
void launch_attention_decode(const RescoreW& W, const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs* joint,
                             const float* memory, const int32_t* out_lens, const AttDecOut& out, hipStream_t st);
// the joint mode's own kernels (attn_decode_joint.hip), for that loop: the empty hypothesis' state before the first step,
// Psi(g . v) of every candidate behind the output GEMM, and the new rows' states behind the selection
void launch_aj_init(const AttDecDims& d, const AttJointBufs& jb, hipStream_t st);
void launch_aj_psi(const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs& jb, int step, int Vp, hipStream_t st);
void launch_aj_update(const AttDecDims& d, const AttDecBufs& bf, const AttJointBufs& jb, int step, hipStream_t st);

}  // namespace ppasr
