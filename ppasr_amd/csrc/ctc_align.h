// ctc_align.h -- CTC forced alignment (ctc_align.hip): the workspace layout and the launcher behind ppasr_ctc_align.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ppasr {

constexpr int kAlignMaxTokens = 255;  // 64 lanes x 4 (blank, token) pairs = 256 pairs: L tokens and the L + 1 blanks

// One emission row of the workspace: e(t, token l) at [l] for l < max_tokens, then padding up to a multiple of 4, then
// e(t, blank) at [stride - 4] (a lane reads its four tokens as one 16-byte word; the blank is one wave-uniform word).
inline int align_row_stride(int max_tokens) { return (max_tokens + 3) / 4 * 4 + 4; }

// workspace offsets in bytes (every part 256-byte aligned)
struct AlignLayout {
  size_t emis;   // f32 [B][Tp][stride]
  size_t bp;     // u16 [B][Tp][64]: 2-bit back-pointers of a lane's 8 states, 128 bytes per frame
  size_t span;   // i32 [B][2][max_tokens]: begin / end, kept here because the caller may not want them
  size_t total;
};
inline AlignLayout align_layout(int B, int Tp, int max_tokens) {
  auto al = [](size_t n) { return (n + 255) / 256 * 256; };
  AlignLayout l;
  size_t o = 0;
  l.emis = o;
  o += al((size_t)B * Tp * align_row_stride(max_tokens) * sizeof(float));
  l.bp = o;
  o += al((size_t)B * Tp * 64 * sizeof(uint16_t));
  l.span = o;
  o += al((size_t)B * 2 * max_tokens * sizeof(int32_t));
  l.total = o > 0 ? o : 256;
  return l;
}

// Queues the gather and the chain on `st`.  Arguments as ppasr_ctc_align (include/ppasr_hip.h), already validated.
void launch_ctc_align(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                      const int32_t* n_tokens, int max_tokens, int32_t* frame_token, int32_t* begin, int32_t* end, int32_t* peak,
                      float* conf, float* score, int32_t* status, void* workspace, hipStream_t st);

}  // namespace ppasr
