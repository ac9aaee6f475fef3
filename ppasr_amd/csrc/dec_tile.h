// dec_tile.h -- device helpers shared by the attention decoder's kernel files (rescore_kernels.hip: teacher-forced
// rescoring and losses; attn_decode.hip: the incremental step of the beam search).
#pragma once
#include "rescore_kernels.h"
#include "rowblock.h"

namespace ppasr {

constexpr float kLnEps = 1e-12f;  // LayerNorm(epsilon=1e-12) of decoder.py
constexpr int kTileLds = kRows * kLda;  // floats of one [32][256] LDS tile
constexpr size_t kFfnLds = 2 * (size_t)kTileLds * sizeof(float);  // dynamic LDS of the kernels of dec_crossout_ffn_tile

// acc = A[32 x 256] (LDS) x one 32-column tile of a packed K = 256 weight (positioned at the tile)
__device__ __forceinline__ void gemm256(const float* a, const f32x4* __restrict__ wtile, f32x16 (&acc)[1][1]) {
  BRing<1> ring;
  acc_zero<1, 1>(acc);
  ring_prime<1, kPF>(ring, wtile, 0);
  rb_gemm<1, 1, kG256>(a, kLda, wtile, 0, nullptr, 0, ring, acc);
}

// The two dense stages of a decoder layer over one 32-row tile: everything behind the calling kernel's early-exit guard
// (k_dec_* of rescore_kernels.hip, k_ad_* of attn_decode.hip).  ctx / x / qc are the [rows][256] activation buffers, t the
// tile (rows 32 t .. 32 t + 31); every thread of the workgroup calls.  layer_w is the layer's entry in device memory: the
// functions copy it themselves, first thing, so that its pointers are loaded ahead of every store (a copy made by the
// caller and handed in by reference cost the k_dec_* kernels their global-address loads of the small vectors: NOTES 39).

// x += self_attn.linear_out(ctx); qc = src_attn.linear_q(norm2(x)).  a: one LDS tile
__device__ __forceinline__ void dec_selfout_q_tile(const DecLayerW& layer_w, float* a, const float* ctx, float* x,
                                                   float* qc, int t) {
  const DecLayerW lw = layer_w;  // the layer's pointers, read once before anything is written
  const int lane = lane_id(), w = wave_id();
  rb_load_rows(a, kLda, ctx + (size_t)t * 32 * kD, 32, 32);
  __syncthreads();
  f32x16 acc[1][1];
  gemm256(a, lw.wo + (size_t)w * kTs256, acc);
  const int col = w * 32 + (lane & 31);
  __syncthreads();  // every wave is done reading the context tile
  {
    const float bias = lw.bo[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, lane);
      const size_t gi = ((size_t)t * 32 + row) * kD + col;
      const float v = acc[0][0][r] + bias + x[gi];
      x[gi] = v;
      a[row * kLda + col] = v;
    }
  }
  __syncthreads();
  rb_layernorm(a, a, kLda, 32, lw.n2g, lw.n2b, kLnEps);
  __syncthreads();
  gemm256(a, lw.wq2 + (size_t)w * kTs256, acc);
  const float bias = lw.bq2[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) qc[((size_t)t * 32 + acc_row(r, lane)) * kD + col] = acc[0][0][r] + bias;
}

// x += src_attn.linear_out(ctx); x += w_2(relu(w_1(norm3(x)))) with the hidden layer (U units) 256 at a time through LDS.
// a, hb: two LDS tiles (kFfnLds bytes)
__device__ __forceinline__ void dec_crossout_ffn_tile(const DecLayerW& layer_w, int U, float* a, float* hb, const float* ctx,
                                                      float* x, int t) {
  const DecLayerW lw = layer_w;  // the layer's pointers, read once before anything is written
  const int lane = lane_id(), w = wave_id();
  rb_load_rows(a, kLda, ctx + (size_t)t * 32 * kD, 32, 32);
  __syncthreads();
  f32x16 acc[1][1], xa;
  gemm256(a, lw.wo2 + (size_t)w * kTs256, acc);
  const int col = w * 32 + (lane & 31);
  __syncthreads();
  {
    const float bias = lw.bo2[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, lane);
      xa[r] = acc[0][0][r] + bias + x[((size_t)t * 32 + row) * kD + col];
      a[row * kLda + col] = xa[r];
    }
  }
  __syncthreads();
  rb_layernorm(a, a, kLda, 32, lw.n3g, lw.n3b, kLnEps);
  __syncthreads();
  f32x16 out[1][1];
  acc_zero<1, 1>(out);
  const int G2 = U / 8;  // k-groups of w_2
  for (int ch = 0; ch < U / 256; ++ch) {
    gemm256(a, lw.w1 + (size_t)(ch * 8 + w) * kTs256, acc);
    const float b1 = lw.b1[ch * 256 + col];
#pragma unroll
    for (int r = 0; r < 16; ++r) hb[acc_row(r, lane) * kLda + col] = fmaxf(acc[0][0][r] + b1, 0.f);
    __syncthreads();
    const f32x4* w2t = lw.w2 + ((size_t)w * G2 + ch * kG256) * 64;
    BRing<1> ring;
    ring_prime<1, kPF>(ring, w2t, 0);
    rb_gemm<1, 1, kG256>(hb, kLda, w2t, 0, nullptr, 0, ring, out);
    __syncthreads();
  }
  const float b2 = lw.b2[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) x[((size_t)t * 32 + acc_row(r, lane)) * kD + col] = xa[r] + out[0][0][r] + b2;
}

}  // namespace ppasr
