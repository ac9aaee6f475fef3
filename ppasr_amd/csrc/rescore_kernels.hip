// rescore_kernels.hip -- the attention decoder of attention rescoring (transformer/decoder.py of the reference:
// BiTransformerDecoder) over PACKED rows: one row per (direction, utterance, hypothesis, position) that exists.
//
// One ppasr_rescore call launches, for L = max(num_blocks, r_num_blocks) layers:
//   k_row_table (1)   lens -> row table (groups of one direction + utterance, 32-row aligned)
//   k_dec_kv (1)      memory [B*Tp, 256] x [256, 512 (L + R)] -> cross-attention keys / values of EVERY layer, once
//   k_dec_embed (1)   embedding * sqrt(d) + pe
//   per layer: k_dec_self_qkv, k_dec_self_attn, k_dec_selfout_q, k_dec_cross_attn, k_dec_crossout_ffn
//   k_dec_output (1)  after_norm -> output_layer with running max / sum over the vocabulary tiles; keeps the target's
//                     log-probability only (the logits leave the chip only into the parity tests' tap)
//   k_dec_score (1)   per-hypothesis sums in double, the combine with the CTC score and the argmax
// ppasr_rescorer_loss makes the same walk with nbest = 1 and ends in k_dec_output<true> + k_dec_loss instead.
// Left and right decoder share every launch (a tile belongs to one direction and reads that direction's weights).
// Grids are sized from B * nbest * 2 * (max_tokens + 1); blocks behind the device-side tile count exit.
// Dense layers: rowblock.h (exact fp32 on the matrix core, weights streamed in fragment order).
#include "rescore_kernels.h"

#include <math.h>

#include "dec_tile.h"
#include "launch.h"

namespace ppasr {
namespace {

// ---- row table ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_row_table(const int32_t* __restrict__ lens, RescoreDims d, RowTab tab) {
  const int H = d.B * d.nbest;
  __shared__ int s_rows;
  if (threadIdx.x == 0) {
    int row = 0, tile = 0;
    for (int dir = 0; dir < d.ndir; ++dir)
      for (int b = 0; b < d.B; ++b) {
        for (int n = 0; n < d.nbest; ++n) {
          const int h = b * d.nbest + n;
          const int len = min(lens[h], d.max_tokens);
          tab.hyp_row0[dir * H + h] = len < 0 ? -1 : row;
          if (len >= 0) row += len + 1;
        }
        for (; tile * 32 < row; ++tile) tab.tile_info[tile] = dir * d.B + b;
        row = tile * 32;
      }
    tab.counts[0] = tile;
    s_rows = row;
  }
  __syncthreads();
  const int rows = s_rows;
  for (int r = threadIdx.x; r < rows; r += blockDim.x) tab.row_info[r] = make_int2(-1, 0);
  __syncthreads();
  for (int i = threadIdx.x; i < d.ndir * H; i += blockDim.x) {
    const int h = i % H, r0 = tab.hyp_row0[i];
    if (r0 < 0) continue;
    const int len = min(lens[h], d.max_tokens);
    for (int p = 0; p <= len; ++p) tab.row_info[r0 + p] = make_int2(h, p);
  }
}

// input token of a row: sos = V - 1 at position 0, else the hypothesis read forwards (left) or backwards (right)
__device__ __forceinline__ int clamp_tok(int t, int V) { return min(max(t, 0), V - 1); }

// ---- embedding ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dec_embed(RescoreW W, RescoreDims d, RowTab tab, const int32_t* __restrict__ tokens,
                                                   const int32_t* __restrict__ lens, float* __restrict__ x) {
  const int t = blockIdx.x;
  if (t >= tab.counts[0]) return;
  const int dir = tab.tile_info[t] / d.B;
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x >> 6; i < 32; i += 4) {
    const int r = t * 32 + i;
    const int2 ri = tab.row_info[r];
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ri.x >= 0) {
      const int n = min(lens[ri.x], d.max_tokens);
      int tok = W.V - 1;
      if (ri.y > 0) tok = clamp_tok(tokens[(size_t)ri.x * d.max_tokens + (dir ? n - ri.y : ri.y - 1)], W.V);
      const f32x4 e = *reinterpret_cast<const f32x4*>(W.side[dir].embed + (size_t)tok * kD + 4 * lane);
      const f32x4 p = *reinterpret_cast<const f32x4*>(W.pe + (size_t)ri.y * kD + 4 * lane);
      v = e * 16.0f + p;  // sqrt(256)
    }
    *reinterpret_cast<f32x4*>(x + (size_t)r * kD + 4 * lane) = v;
  }
}

// ---- cross-attention keys / values of every layer --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_dec_kv(RescoreW W, RescoreDims d, const float* __restrict__ memory,
                                                     const int32_t* __restrict__ out_lens, int kvw, float* __restrict__ kv) {
  __shared__ float a[kTileLds];
  const int M = d.B * d.Tp, m0 = blockIdx.x * 32;
  const int lane = lane_id(), w = wave_id();
  for (int i = w; i < 32; i += kWaves) {
    const int r = m0 + i;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (r < M) {
      const int b = r / d.Tp, tt = r - b * d.Tp;
      if (!out_lens || tt < out_lens[b]) v = *reinterpret_cast<const f32x4*>(memory + (size_t)r * kD + 4 * lane);
    }
    *reinterpret_cast<f32x4*>(a + i * kLda + 4 * lane) = v;
  }
  __syncthreads();
  f32x16 acc[1][1];
  const int nt = blockIdx.y * 8 + w;
  gemm256(a, W.wkv + (size_t)nt * kTs256, acc);
  const int col = nt * 32 + (lane & 31);
  const float bias = W.bkv[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + acc_row(r, lane);
    if (row < M) kv[(size_t)row * kvw + col] = acc[0][0][r] + bias;
  }
}

// ---- self-attention: LayerNorm -> q | k | v -----------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_dec_self_qkv(RescoreW W, RescoreDims d, RowTab tab, int layer,
                                                           const float* __restrict__ x, float* __restrict__ qkv) {
  __shared__ float a[kTileLds];
  const int t = blockIdx.x;
  if (t >= tab.counts[0]) return;
  const DecSideW& S = W.side[tab.tile_info[t] / d.B];
  if (layer >= S.nblk) return;
  const DecLayerW lw = S.layers[layer];
  const int lane = lane_id(), w = wave_id();
  rb_load_rows(a, kLda, x + (size_t)t * 32 * kD, 32, 32);
  __syncthreads();
  rb_layernorm(a, a, kLda, 32, lw.n1g, lw.n1b, kLnEps);
  __syncthreads();
  for (int j = 0; j < 3; ++j) {
    f32x16 acc[1][1];
    const int nt = j * 8 + w;
    gemm256(a, lw.wqkv + (size_t)nt * kTs256, acc);
    const int col = nt * 32 + (lane & 31);
    const float bias = lw.bqkv[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) qkv[((size_t)t * 32 + acc_row(r, lane)) * 768 + col] = acc[0][0][r] + bias;
  }
}

// causal self-attention of one (hypothesis, direction, head): at most 256 positions, one thread per query row, keys and
// values through LDS 64 at a time, online softmax
__global__ __launch_bounds__(256) void k_dec_self_attn(RescoreW W, RescoreDims d, RowTab tab, int layer,
                                                       const int32_t* __restrict__ lens, const float* __restrict__ qkv,
                                                       float* __restrict__ ctx) {
  __shared__ float ks[64 * 64], vs[64 * 64];
  const int h = blockIdx.x, dir = blockIdx.y, head = blockIdx.z;
  if (layer >= W.side[dir].nblk) return;
  const int row0 = tab.hyp_row0[dir * d.B * d.nbest + h];
  if (row0 < 0) return;
  const int n = min(lens[h], d.max_tokens) + 1;
  const int i = threadIdx.x;
  float q[64], acc[64];
  float m = -INFINITY, s = 0.f;
  if (i < n) {
    const float* qp = qkv + (size_t)(row0 + i) * 768 + head * 64;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + c);
      q[c] = v[0] * 0.125f; q[c + 1] = v[1] * 0.125f; q[c + 2] = v[2] * 0.125f; q[c + 3] = v[3] * 0.125f;
    }
  }
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = 0.f;
  for (int j0 = 0; j0 < n; j0 += 64) {
    const int nj = min(64, n - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < nj * 16; e += 256) {
      const int j = e >> 4, c = (e & 15) * 4;
      const float* p = qkv + (size_t)(row0 + j0 + j) * 768 + head * 64 + c;
      *reinterpret_cast<f32x4*>(ks + j * 64 + c) = *reinterpret_cast<const f32x4*>(p + 256);
      *reinterpret_cast<f32x4*>(vs + j * 64 + c) = *reinterpret_cast<const f32x4*>(p + 512);
    }
    __syncthreads();
    if (i < n) {
      const int jmax = min(nj, i - j0 + 1);  // keys j0 + j <= i
      for (int j = 0; j < jmax; ++j) {
        float sc = 0.f;
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
          const f32x4 k4 = *reinterpret_cast<const f32x4*>(ks + j * 64 + c);
          sc = fmaf(q[c], k4[0], sc); sc = fmaf(q[c + 1], k4[1], sc); sc = fmaf(q[c + 2], k4[2], sc); sc = fmaf(q[c + 3], k4[3], sc);
        }
        const float mn = fmaxf(m, sc);
        const float f = expf(m - mn), p = expf(sc - mn);
        s = s * f + p;
        m = mn;
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
          const f32x4 v4 = *reinterpret_cast<const f32x4*>(vs + j * 64 + c);
          acc[c] = fmaf(p, v4[0], acc[c] * f); acc[c + 1] = fmaf(p, v4[1], acc[c + 1] * f);
          acc[c + 2] = fmaf(p, v4[2], acc[c + 2] * f); acc[c + 3] = fmaf(p, v4[3], acc[c + 3] * f);
        }
      }
    }
  }
  if (i < n) {
    const float inv = 1.0f / s;  // key 0 is always visible: s >= 1
    float* op = ctx + (size_t)(row0 + i) * kD + head * 64;
#pragma unroll
    for (int c = 0; c < 64; c += 4)
      *reinterpret_cast<f32x4*>(op + c) = f32x4{acc[c] * inv, acc[c + 1] * inv, acc[c + 2] * inv, acc[c + 3] * inv};
  }
}

// x += self_attn.linear_out(ctx); q2 = src_attn.linear_q(norm2(x))
__global__ __launch_bounds__(kThreads) void k_dec_selfout_q(RescoreW W, RescoreDims d, RowTab tab, int layer,
                                                            const float* __restrict__ ctx, float* __restrict__ x,
                                                            float* __restrict__ qc) {
  __shared__ float a[kTileLds];
  const int t = blockIdx.x;
  if (t >= tab.counts[0]) return;
  const DecSideW& S = W.side[tab.tile_info[t] / d.B];
  if (layer >= S.nblk) return;
  dec_selfout_q_tile(S.layers[layer], a, ctx, x, qc, t);
}

// Cross-attention of one 32-row tile and head over the utterance's valid memory frames.  A tile of 64 keys / values staged
// in LDS serves all 32 rows (every hypothesis of the utterance the tile holds); each row is worked on by 8 adjacent lanes
// that take every 8th key with an online softmax of their own and are merged with lane shuffles at the end.
constexpr int kKvLd = 68;  // LDS row stride: the 8 key slices of a wave read 8 distinct bank groups
__global__ __launch_bounds__(256) void k_dec_cross_attn(RescoreW W, RescoreDims d, RowTab tab, int layer,
                                                        const int32_t* __restrict__ out_lens, const float* __restrict__ qc,
                                                        const float* __restrict__ kv, int kvw, float* __restrict__ ctx) {
  __shared__ float ks[64 * kKvLd], vs[64 * kKvLd];
  const int t = blockIdx.x, head = blockIdx.y;
  if (t >= tab.counts[0]) return;
  const int g = tab.tile_info[t], dir = g / d.B, b = g - dir * d.B;
  if (layer >= W.side[dir].nblk) return;
  const int klen = out_lens ? min(max(out_lens[b], 0), d.Tp) : d.Tp;
  const int slot = dir ? W.n_left + layer : layer;
  const float* kvb = kv + (size_t)b * d.Tp * kvw + slot * 512 + head * 64;
  const int row = threadIdx.x >> 3, sl = threadIdx.x & 7;
  float q[64], acc[64];
  {
    const float* qp = qc + ((size_t)t * 32 + row) * kD + head * 64;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(qp + c);
      q[c] = v[0] * 0.125f; q[c + 1] = v[1] * 0.125f; q[c + 2] = v[2] * 0.125f; q[c + 3] = v[3] * 0.125f;
    }
  }
#pragma unroll
  for (int c = 0; c < 64; ++c) acc[c] = 0.f;
  float m = -INFINITY, s = 0.f;
  for (int j0 = 0; j0 < klen; j0 += 64) {
    const int nj = min(64, klen - j0);
    __syncthreads();
    for (int e = threadIdx.x; e < nj * 16; e += 256) {
      const int j = e >> 4, c = (e & 15) * 4;
      const float* p = kvb + (size_t)(j0 + j) * kvw + c;
      *reinterpret_cast<f32x4*>(ks + j * kKvLd + c) = *reinterpret_cast<const f32x4*>(p);
      *reinterpret_cast<f32x4*>(vs + j * kKvLd + c) = *reinterpret_cast<const f32x4*>(p + 256);
    }
    __syncthreads();
    for (int j = sl; j < nj; j += 8) {
      float sc = 0.f;
#pragma unroll
      for (int c = 0; c < 64; c += 4) {
        const f32x4 k4 = *reinterpret_cast<const f32x4*>(ks + j * kKvLd + c);
        sc = fmaf(q[c], k4[0], sc); sc = fmaf(q[c + 1], k4[1], sc); sc = fmaf(q[c + 2], k4[2], sc); sc = fmaf(q[c + 3], k4[3], sc);
      }
      const float mn = fmaxf(m, sc);
      const float f = expf(m - mn), p = expf(sc - mn);
      s = s * f + p;
      m = mn;
#pragma unroll
      for (int c = 0; c < 64; c += 4) {
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(vs + j * kKvLd + c);
        acc[c] = fmaf(p, v4[0], acc[c] * f); acc[c + 1] = fmaf(p, v4[1], acc[c + 1] * f);
        acc[c + 2] = fmaf(p, v4[2], acc[c + 2] * f); acc[c + 3] = fmaf(p, v4[3], acc[c + 3] * f);
      }
    }
  }
  // merge the 8 key slices of the row (a slice that saw no key has m = -inf, s = 0, acc = 0)
  float M = m;
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) M = fmaxf(M, __shfl_xor(M, o));
  const float f = (m == -INFINITY) ? 0.f : expf(m - M);
  s *= f;
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o);
  const float inv = s > 0.f ? 1.0f / s : 0.f;  // no valid frame: the reference's masked softmax attends to nothing
  float out[8];
#pragma unroll
  for (int c = 0; c < 64; ++c) {
    float v = acc[c] * f;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) v += __shfl_xor(v, o);
    if ((c >> 3) == sl) out[c & 7] = v * inv;
  }
  float* op = ctx + ((size_t)t * 32 + row) * kD + head * 64 + sl * 8;
  *reinterpret_cast<f32x4*>(op) = f32x4{out[0], out[1], out[2], out[3]};
  *reinterpret_cast<f32x4*>(op + 4) = f32x4{out[4], out[5], out[6], out[7]};
}

// x += src_attn.linear_out(ctx); x += w_2(relu(w_1(norm3(x)))) with the hidden layer 256 units at a time through LDS
__global__ __launch_bounds__(kThreads) void k_dec_crossout_ffn(RescoreW W, RescoreDims d, RowTab tab, int layer,
                                                               const float* __restrict__ ctx, float* __restrict__ x) {
  extern __shared__ float lds[];
  float* a = lds;
  float* hb = lds + kTileLds;
  const int t = blockIdx.x;
  if (t >= tab.counts[0]) return;
  const DecSideW& S = W.side[tab.tile_info[t] / d.B];
  if (layer >= S.nblk) return;
  dec_crossout_ffn_tile(S.layers[layer], W.U, a, hb, ctx, x, t);
}

// after_norm -> output_layer over the vocabulary 256 columns at a time; per row only the running max / sum and the target's
// logit are kept.  tap (parity tests): the logits themselves, [B * nbest][2][L][V].
// kLoss (ppasr_rescorer_loss): the row also keeps X, the sum of its logits over the real columns v < V, and writes
// stat [row][2] = (X, log-sum-exp); the padded columns up to Vp never enter X.  Lanes are summed as a tree, waves in order.
template <bool kLoss>
__global__ __launch_bounds__(kThreads) void k_dec_output(RescoreW W, RescoreDims d, RowTab tab, const float* __restrict__ x,
                                                         const int32_t* __restrict__ tokens, const int32_t* __restrict__ lens,
                                                         float* __restrict__ logp, float* __restrict__ tap,
                                                         float* __restrict__ stat) {
  __shared__ float a[kTileLds];
  __shared__ int s_tgt[32], s_hyp[32], s_pos[32];
  __shared__ float s_tv[32], s_m[kWaves][32], s_s[kWaves][32];
  __shared__ float s_x[kLoss ? kWaves : 1][32];
  const int t = blockIdx.x;
  if (t >= tab.counts[0]) return;
  const int dir = tab.tile_info[t] / d.B;
  const DecSideW& S = W.side[dir];
  const int lane = lane_id(), w = wave_id();
  rb_load_rows(a, kLda, x + (size_t)t * 32 * kD, 32, 32);
  if (threadIdx.x < 32) {
    const int2 ri = tab.row_info[t * 32 + threadIdx.x];
    int tgt = -1;
    if (ri.x >= 0) {
      const int n = min(lens[ri.x], d.max_tokens);
      tgt = ri.y == n ? W.V - 1 : clamp_tok(tokens[(size_t)ri.x * d.max_tokens + (dir ? n - 1 - ri.y : ri.y)], W.V);
    }
    s_tgt[threadIdx.x] = tgt;
    s_hyp[threadIdx.x] = ri.x;
    s_pos[threadIdx.x] = ri.y;
    s_tv[threadIdx.x] = 0.f;
  }
  __syncthreads();
  rb_layernorm(a, a, kLda, 32, S.ang, S.anb, kLnEps);
  __syncthreads();
  float m[16], s[16];
  [[maybe_unused]] float xs[16];
  int tgt[16];
  size_t tap_row[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = acc_row(r, lane);
    m[r] = -INFINITY;
    s[r] = 0.f;
    if constexpr (kLoss) xs[r] = 0.f;
    tgt[r] = s_tgt[row];
    tap_row[r] = (((size_t)max(s_hyp[row], 0) * 2 + dir) * d.L() + s_pos[row]) * W.V;
  }
  const bool has_tap = tap != nullptr;
  for (int vt = 0; vt < W.Vp / 256; ++vt) {
    f32x16 acc[1][1];
    const int nt = vt * 8 + w;
    gemm256(a, S.wout + (size_t)nt * kTs256, acc);
    const int col = nt * 32 + (lane & 31);
    if (col < W.V) {
      const float bias = S.bout[col];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[0][0][r] + bias;
        if (col == tgt[r]) s_tv[acc_row(r, lane)] = v;
        if (has_tap && tgt[r] >= 0) tap[tap_row[r] + col] = v;
        const float mn = fmaxf(m[r], v);
        s[r] = s[r] * expf(m[r] - mn) + expf(v - mn);
        m[r] = mn;
        if constexpr (kLoss) xs[r] += v;
      }
    }
  }
  // merge the 32 column lanes of a row, then the 8 waves
#pragma unroll
  for (int r = 0; r < 16; ++r) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
      const float m2 = __shfl_xor(m[r], o), s2 = __shfl_xor(s[r], o);
      const float mn = fmaxf(m[r], m2);
      const float f1 = m[r] == -INFINITY ? 0.f : expf(m[r] - mn), f2 = m2 == -INFINITY ? 0.f : expf(m2 - mn);
      s[r] = s[r] * f1 + s2 * f2;
      m[r] = mn;
      if constexpr (kLoss) xs[r] += __shfl_xor(xs[r], o);
    }
    if ((lane & 31) == 0) {
      s_m[w][acc_row(r, lane)] = m[r];
      s_s[w][acc_row(r, lane)] = s[r];
      if constexpr (kLoss) s_x[w][acc_row(r, lane)] = xs[r];
    }
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    const int row = threadIdx.x;
    float M = -INFINITY;
    for (int k = 0; k < kWaves; ++k) M = fmaxf(M, s_m[k][row]);
    float sum = 0.f;
    for (int k = 0; k < kWaves; ++k) sum += s_m[k][row] == -INFINITY ? 0.f : s_s[k][row] * expf(s_m[k][row] - M);
    logp[t * 32 + row] = s_tgt[row] >= 0 ? s_tv[row] - (M + logf(sum)) : 0.f;
    if constexpr (kLoss) {
      float X = 0.f;
      for (int k = 0; k < kWaves; ++k) X += s_x[k][row];
      stat[(size_t)(t * 32 + row) * 2] = s_tgt[row] >= 0 ? X : 0.f;
      stat[(size_t)(t * 32 + row) * 2 + 1] = s_tgt[row] >= 0 ? M + logf(sum) : 0.f;
    }
  }
}

// ppasr_rescorer_loss: per utterance (nbest = 1) and direction the label-smoothing KL of its L + 1 target rows, summed in
// double in row order.  With c = 1 - s:  kl_row = c ln c + s ln(s / (V - 1)) - c logp_y - s / (V - 1) (X - x_y - (V - 1) lse),
// 0 ln 0 = 0, and x_y = logp_y + lse.  At s = 0 the row term is -logp_y exactly.
__global__ __launch_bounds__(64) void k_dec_loss(RescoreDims d, RowTab tab, const int32_t* __restrict__ lens,
                                                 const float* __restrict__ logp, const float* __restrict__ stat, int V, double lsm,
                                                 double* __restrict__ att_kl, double* __restrict__ r_att_kl,
                                                 int32_t* __restrict__ rows) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= d.B) return;
  const int len = min(lens[b], d.max_tokens);
  const double c = 1.0 - lsm, low = lsm / (double)(V - 1);
  const double k0 = (c > 0.0 ? c * log(c) : 0.0) + (lsm > 0.0 ? lsm * log(low) : 0.0);
  double kl[2] = {0.0, 0.0};
  for (int dir = 0; dir < d.ndir; ++dir) {
    const int r0 = len >= 0 ? tab.hyp_row0[dir * d.B + b] : -1;
    if (r0 < 0) continue;
    for (int p = 0; p <= len; ++p) {
      const double lp = (double)logp[r0 + p];
      double row = k0 - c * lp;
      if (lsm > 0.0) {
        const double X = (double)stat[(size_t)(r0 + p) * 2], lse = (double)stat[(size_t)(r0 + p) * 2 + 1];
        row -= low * (X - lp - (double)V * lse);
      }
      kl[dir] += row;
    }
  }
  att_kl[b] = kl[0];
  r_att_kl[b] = kl[1];
  rows[b] = len >= 0 ? len + 1 : 0;
}

// per-hypothesis sums (double), total = (1 - rw) att + rw r_att - cw ctc, best = first largest total; also the
// per-position log-probabilities [B][nbest][2][L] (0 where there is no row)
__global__ __launch_bounds__(64) void k_dec_score(RescoreDims d, RowTab tab, const int32_t* __restrict__ lens,
                                                  const float* __restrict__ logp, const double* __restrict__ ctc,
                                                  double cw, double rw, double* __restrict__ att, double* __restrict__ r_att,
                                                  double* __restrict__ total, int32_t* __restrict__ best,
                                                  float* __restrict__ token_logp) {
  const int b = blockIdx.x, H = d.B * d.nbest, L = d.L();
  for (int n = threadIdx.x; n < d.nbest; n += blockDim.x) {
    const int h = b * d.nbest + n;
    const int len = min(lens[h], d.max_tokens);
    double sc[2] = {0.0, 0.0};
    for (int dir = 0; dir < 2; ++dir) {
      const int r0 = (len >= 0 && dir < d.ndir) ? tab.hyp_row0[dir * H + h] : -1;
      for (int p = 0; p < L; ++p) {
        const float v = (r0 >= 0 && p <= len) ? logp[r0 + p] : 0.f;
        sc[dir] += (double)v;
        if (token_logp) token_logp[((size_t)h * 2 + dir) * L + p] = v;
      }
    }
    att[h] = sc[0];
    r_att[h] = sc[1];
    total[h] = len < 0 ? -INFINITY : (1.0 - rw) * sc[0] + rw * sc[1] + cw * (-ctc[h]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int bi = 0;
    double bv = -INFINITY;
    for (int n = 0; n < d.nbest; ++n) {
      const double v = total[b * d.nbest + n];
      if (v > bv) {
        bv = v;
        bi = n;
      }
    }
    best[b] = bi;
  }
}

// one row of the encoder output, by one wave: o = LayerNorm(xr) over D (encoder.after_norm; g == nullptr: a copy).  Shared
// by the offline and the streaming kernel below, so that a frame's memory is the same bits on either path
__device__ __forceinline__ void memory_row(const float* __restrict__ xr, const float* __restrict__ g,
                                           const float* __restrict__ bta, float* __restrict__ o, int D, int lane) {
  if (!g) {
    for (int c = lane; c < D; c += 64) o[c] = xr[c];
    return;
  }
  float sum = 0.f;
  for (int c = lane; c < D; c += 64) sum += xr[c];
  const float mean = wave_sum(sum) / (float)D;
  float sq = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float dlt = xr[c] - mean;
    sq = fmaf(dlt, dlt, sq);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + 1e-5f);
  for (int c = lane; c < D; c += 64) o[c] = (xr[c] - mean) * rstd * g[c] + bta[c];
}

// encoder output of an offline encode (ppasr_set_memory_out): memory_row of the rows the CTC head reads, one wave per
// row; ragged batches: rows behind the valid frames are 0
__global__ __launch_bounds__(256) void k_memory_out(const float* __restrict__ x, const float* __restrict__ g,
                                                    const float* __restrict__ bta, float* __restrict__ out, int M, int D,
                                                    const int64_t* __restrict__ lens, int Tp, int mul) {
  const int row = blockIdx.x * 4 + wave_id();
  if (row >= M) return;
  const int lane = lane_id();
  float* o = out + (size_t)row * D;
  if (lens) {
    const int b = row / Tp, t = row - b * Tp;
    if ((int64_t)mul * t >= lens[b]) {
      for (int c = lane; c < D; c += 64) o[c] = 0.f;
      return;
    }
  }
  memory_row(x + (size_t)row * D, g, bta, o, D, lane);
}

// encoder output of a streaming round (ppasr_encode_chunk_group_mem / ppasr_encode_chunk_mem): memory_row of row r of list
// position k (x [n][c][D]) goes to frame first[k] + r of its session in a row arena of width D -- the page addressing of
// arena_append_kernel (ctc_align.hip): the session's pages from page first[k] / P on are pages[page_off[k] ..].  One wave
// per row; rows r >= count[k] are not kept.
__global__ __launch_bounds__(256) void k_memory_append(const float* __restrict__ x, const float* __restrict__ g,
                                                       const float* __restrict__ bta, int M, int c, int D, int P,
                                                       const int32_t* __restrict__ first, const int32_t* __restrict__ count,
                                                       const int32_t* __restrict__ page_off,
                                                       const int32_t* __restrict__ pages, float* __restrict__ slab) {
  const int row = blockIdx.x * 4 + wave_id();
  if (row >= M) return;
  const int k = row / c, r = row - k * c;
  if (r >= count[k]) return;
  const int f = first[k] + r;
  const int page = pages[page_off[k] + f / P - first[k] / P];
  memory_row(x + (size_t)row * D, g, bta, slab + ((size_t)page * P + f % P) * D, D, lane_id());
}

}  // namespace

void launch_memory_out(const float* x, const float* g, const float* b, float* out, int M, int D, const PadSkip& ps,
                       hipStream_t st) {
  PPASR_LAUNCH(k_memory_out, dim3((M + 3) / 4), dim3(256), 0, st, x, g, b, out, M, D, ps.lens, ps.Tp, ps.mul);
}

void launch_memory_append(const float* x, const float* g, const float* b, int n, int c, int D, int P, const int32_t* first,
                          const int32_t* count, const int32_t* page_off, const int32_t* pages, float* slab, hipStream_t st) {
  const int M = n * c;
  PPASR_LAUNCH(k_memory_append, dim3((M + 3) / 4), dim3(256), 0, st, x, g, b, M, c, D, P, first, count, page_off, pages, slab);
}

void launch_dec_kv(const RescoreW& W, int B, int Tp, int slots, const float* memory, const int32_t* out_lens, float* kv,
                   hipStream_t st) {
  const RescoreDims d{B, Tp, 1, 0, 1};
  PPASR_LAUNCH(k_dec_kv, dim3((B * Tp + 31) / 32, 2 * slots), dim3(kThreads), 0, st, W, d, memory, out_lens, 512 * slots, kv);
}

hipError_t configure_rescore_kernels() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_dec_crossout_ffn), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)kFfnLds);
}

void launch_rescore(const RescoreW& W, const RescoreDims& d, const RescoreBufs& bf, const float* memory, const int32_t* out_lens,
                    const int32_t* tokens, const int32_t* lens, const double* ctc_scores, double ctc_weight,
                    double reverse_weight, double* att, double* r_att, double* total, int32_t* best, float* token_logp,
                    float* logits_tap, const RescoreLoss* loss, hipStream_t st) {
  const int tiles = d.tiles_cap();
  const int slots = W.n_left + (d.ndir == 2 ? W.side[1].nblk : 0);
  const int kvw = 512 * (W.n_left + W.side[1].nblk);
  const int layers = d.ndir == 2 ? (W.side[0].nblk > W.side[1].nblk ? W.side[0].nblk : W.side[1].nblk) : W.side[0].nblk;
  PPASR_LAUNCH(k_row_table, dim3(1), dim3(1024), 0, st, lens, d, bf.tab);
  PPASR_LAUNCH(k_dec_kv, dim3((d.B * d.Tp + 31) / 32, 2 * slots), dim3(kThreads), 0, st, W, d, memory, out_lens, kvw, bf.kv);
  PPASR_LAUNCH(k_dec_embed, dim3(tiles), dim3(256), 0, st, W, d, bf.tab, tokens, lens, bf.x);
  for (int l = 0; l < layers; ++l) {
    PPASR_LAUNCH(k_dec_self_qkv, dim3(tiles), dim3(kThreads), 0, st, W, d, bf.tab, l, bf.x, bf.qkv);
    PPASR_LAUNCH(k_dec_self_attn, dim3(d.B * d.nbest, d.ndir, 4), dim3(256), 0, st, W, d, bf.tab, l, lens, bf.qkv, bf.ctx);
    PPASR_LAUNCH(k_dec_selfout_q, dim3(tiles), dim3(kThreads), 0, st, W, d, bf.tab, l, bf.ctx, bf.x, bf.qc);
    PPASR_LAUNCH(k_dec_cross_attn, dim3(tiles, 4), dim3(256), 0, st, W, d, bf.tab, l, out_lens, bf.qc, bf.kv, kvw, bf.ctx);
    PPASR_LAUNCH(k_dec_crossout_ffn, dim3(tiles), dim3(kThreads), kFfnLds, st, W, d, bf.tab, l, bf.ctx, bf.x);
  }
  if (loss) {  // ppasr_rescorer_loss: the same walk (nbest = 1), the row statistics of the smoothed target on top
    PPASR_LAUNCH(k_dec_output<true>, dim3(tiles), dim3(kThreads), 0, st, W, d, bf.tab, bf.x, tokens, lens, bf.logp, logits_tap,
                 loss->stat);
    PPASR_LAUNCH(k_dec_loss, dim3((d.B + 63) / 64), dim3(64), 0, st, d, bf.tab, lens, bf.logp, loss->stat, W.V, loss->lsm_weight,
                 loss->att_kl, loss->r_att_kl, loss->rows);
    return;
  }
  PPASR_LAUNCH(k_dec_output<false>, dim3(tiles), dim3(kThreads), 0, st, W, d, bf.tab, bf.x, tokens, lens, bf.logp, logits_tap,
               static_cast<float*>(nullptr));
  PPASR_LAUNCH(k_dec_score, dim3(d.B), dim3(64), 0, st, d, bf.tab, lens, bf.logp, ctc_scores, ctc_weight, reverse_weight, att,
               r_att, total, best, token_logp);
}

}  // namespace ppasr
