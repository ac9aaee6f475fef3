// dec_tile.h -- device helpers shared by the attention decoder's kernel files (rescore_kernels.hip: teacher-forced
// rescoring and losses; attn_decode.hip: the incremental step of the beam search).
#pragma once
#include "rowblock.h"

namespace ppasr {

constexpr float kLnEps = 1e-12f;  // LayerNorm(epsilon=1e-12) of decoder.py
constexpr int kTileLds = kRows * kLda;  // floats of one [32][256] LDS tile

// acc = A[32 x 256] (LDS) x one 32-column tile of a packed K = 256 weight (positioned at the tile)
__device__ __forceinline__ void gemm256(const float* a, const f32x4* __restrict__ wtile, f32x16 (&acc)[1][1]) {
  BRing<1> ring;
  acc_zero<1, 1>(acc);
  ring_prime<1, kPF>(ring, wtile, 0);
  rb_gemm<1, 1, kG256>(a, kLda, wtile, 0, nullptr, 0, ring, acc);
}

}  // namespace ppasr
