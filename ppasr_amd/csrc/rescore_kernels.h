// rescore_kernels.h -- attention rescoring of CTC n-best lists (rescore_kernels.hip, capi_rescore.hip): device-side
// weight views of the reference's BiTransformerDecoder and the launchers of one ppasr_rescore call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rowblock.h"

namespace ppasr {

// one DecoderLayer (transformer/decoder.py:273): pre-norm self-attention, cross-attention, feed-forward
struct DecLayerW {
  const float *n1g, *n1b, *n2g, *n2b, *n3g, *n3b;
  const f32x4 *wqkv, *wo;   // self_attn: [256][768] q|k|v, linear_out
  const float *bqkv, *bo;
  const f32x4 *wq2, *wo2;   // src_attn: linear_q, linear_out (its keys / values: RescoreW::wkv)
  const float *bq2, *bo2;
  const f32x4 *w1, *w2;     // feed_forward [256][U], [U][256]
  const float *b1, *b2;
};
struct DecSideW {  // one TransformerDecoder (left or right)
  const float* embed;          // [V][256]
  const float *ang, *anb;      // after_norm
  const f32x4* wout;           // output_layer, packed [256][Vp]
  const float* bout;           // [Vp]
  const DecLayerW* layers;     // device array [nblk]
  int nblk;
};
struct RescoreW {
  DecSideW side[2];
  const f32x4* wkv;   // [256][512 * (L + R)]: per layer slot (left 0 .. L-1, right L .. L+R-1) the src_attn k | v
  const float* bkv;
  const float* pe;    // [max_len][256]
  int V, Vp, U, n_left;
};

// Packed rows: one row per (direction, utterance, hypothesis, position) that exists.  The rows of one (direction,
// utterance) group are contiguous and the group starts at a multiple of 32, so that a 32-row tile has one set of
// cross-attention keys.  Built on the device from `lens` (k_row_table); nothing of it is read back.
struct RowTab {
  int* counts;     // [0] = active tiles
  int* tile_info;  // [tiles_cap]: dir * B + b
  int2* row_info;  // [rows_cap]: (b * nbest + n, position) or (-1, 0) on a fill row
  int* hyp_row0;   // [2][B * nbest]: first row of the hypothesis in that direction, -1: absent
};
struct RescoreDims {
  int B, Tp, nbest, max_tokens, ndir;
  __host__ __device__ int L() const { return max_tokens + 1; }
  __host__ __device__ int group_cap() const { return (nbest * L() + 31) / 32 * 32; }  // rows of one (direction, utterance) group at most
  __host__ __device__ int rows_cap() const { return ndir * B * group_cap(); }
  __host__ __device__ int tiles_cap() const { return rows_cap() / 32; }
};
constexpr int kRescoreMaxRows = 256;  // rows per hypothesis (max_tokens + 1) the self-attention kernel is built for

struct RescoreBufs {
  float *x, *qkv, *ctx, *qc, *kv, *logp;
  RowTab tab;
};

// ppasr_set_memory_out: out [M][D] = LayerNorm(x) (g == nullptr: x itself); ragged batches (ps.lens): 0 behind the valid frames
// ppasr_rescorer_loss: what launch_rescore computes in place of the hypothesis scores (nbest = 1; the labels are `tokens`)
struct RescoreLoss {
  double lsm_weight;
  float* stat;         // workspace [rows_cap][2]: per row the logit sum over v < V and the log-sum-exp
  double *att_kl, *r_att_kl;  // [B]
  int32_t* rows;       // [B]
};

void launch_memory_out(const float* x, const float* g, const float* b, float* out, int M, int D, const PadSkip& ps,
                       hipStream_t st);
// the same rows of a streaming round, x [n][c][D] (n * c > 0), into a row arena of width D (slab [n_pages][P][D]): rows
// 0 .. count[k] - 1 of list position k become frames first[k] .. of its session, whose pages from page first[k] / P on are
// pages[page_off[k] ..] (the tables of launch_arena_append, ctc_align.h; device arrays).  One launch
void launch_memory_append(const float* x, const float* g, const float* b, int n, int c, int D, int P, const int32_t* first,
                          const int32_t* count, const int32_t* page_off, const int32_t* pages, float* slab, hipStream_t st);
hipError_t configure_rescore_kernels();
// k_dec_kv alone, over the first `slots` layer slots (the left decoder's when slots = n_left): kv [B * Tp][512 * slots]
void launch_dec_kv(const RescoreW& W, int B, int Tp, int slots, const float* memory, const int32_t* out_lens, float* kv,
                   hipStream_t st);
void launch_rescore(const RescoreW& W, const RescoreDims& d, const RescoreBufs& bf, const float* memory, const int32_t* out_lens,
                    const int32_t* tokens, const int32_t* lens, const double* ctc_scores, double ctc_weight,
                    double reverse_weight, double* att, double* r_att, double* total, int32_t* best, float* token_logp,
                    float* logits_tap, const RescoreLoss* loss, hipStream_t st);

}  // namespace ppasr
