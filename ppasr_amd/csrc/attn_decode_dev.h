// attn_decode_dev.h -- device helpers of the top-N pass of attn_decode.hip (both of its instantiations).
#pragma once
#include <hip/hip_runtime.h>

#include "rowblock.h"

namespace ppasr {

// (value, id) pairs ordered by larger value, then lower id
__device__ __forceinline__ bool cand_before(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

// the first pair of the workgroup's 256 in that order, to every thread (id V: none)
__device__ __forceinline__ void block_first(float& v, int& id, float* s_v, int* s_i) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v2 = __shfl_xor(v, o);
    const int i2 = __shfl_xor(id, o);
    if (cand_before(v2, i2, v, id)) {
      v = v2;
      id = i2;
    }
  }
  __syncthreads();
  if (lane_id() == 0) {
    s_v[threadIdx.x >> 6] = v;
    s_i[threadIdx.x >> 6] = id;
  }
  __syncthreads();
  v = s_v[0];
  id = s_i[0];
  for (int k = 1; k < 4; ++k)
    if (cand_before(s_v[k], s_i[k], v, id)) {
      v = s_v[k];
      id = s_i[k];
    }
}

}  // namespace ppasr
