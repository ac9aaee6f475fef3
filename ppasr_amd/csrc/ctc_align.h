// ctc_align.h -- CTC forced alignment (ctc_align.hip): the workspace layout and the launcher behind ppasr_ctc_align.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
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

// ---- what the alignment (ctc_align.hip) and the loss (ctc_loss.hip) share: the emission, the frame clamp, the lane move ----
#if defined(__HIPCC__)
constexpr float kNegInf = -__builtin_huge_valf();

__device__ __forceinline__ float emission(float p) { return logf(fmaxf(p, FLT_MIN)); }

__device__ __forceinline__ int clamp_frames(const int32_t* frame_lens, int b, int Tp) {
  const int T = frame_lens ? frame_lens[b] : Tp;
  return min(max(T, 0), Tp);
}

// lane i <- lane i-1 across the whole wave (DPP wave_shr:1); lane 0 gets `edge`
__device__ __forceinline__ float lane_shr1(float x, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(x), 0x138, 0xf, 0xf, false));
}
#endif

// Queues the gather alone: emis [B][Tp][align_row_stride(max_tokens)] = e(t, .) of every row t < T and token l < L.
void launch_ctc_gather(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                       const int32_t* n_tokens, int max_tokens, float* emis, hipStream_t st);

// Queues the gather and the chain on `st`.  Arguments as ppasr_ctc_align (include/ppasr_hip.h), already validated.
void launch_ctc_align(const float* probs, const int32_t* frame_lens, int B, int Tp, int V, int blank, const int32_t* tokens,
                      const int32_t* n_tokens, int max_tokens, int32_t* frame_token, int32_t* begin, int32_t* end, int32_t* peak,
                      float* conf, float* score, int32_t* status, void* workspace, hipStream_t st);

// ---- probability arena (ppasr_prob_arena_*): a slab [n_pages][P][V]; every table below is a device array ----
// The alignment of B sessions held in pages: utterance b has frame_lens[b] <= Tp frames, frame t in row t % P of page
// pages[page_off[b] + t / P].  The paged gather, then the chain of launch_ctc_align; same workspace, same outputs.
void launch_ctc_align_paged(const float* slab, int V, int P, const int32_t* page_off, const int32_t* pages,
                            const int32_t* frame_lens, int B, int Tp, int blank, const int32_t* tokens, const int32_t* n_tokens,
                            int max_tokens, int32_t* frame_token, int32_t* begin, int32_t* end, int32_t* peak, float* conf,
                            float* score, int32_t* status, void* workspace, hipStream_t st);
// One launch: rows 0 .. count[k] - 1 of probs[k] ([n][c][V], n * c > 0) become frames first[k] .. of entry k's session, whose
// pages from page first[k] / P on are pages[page_off[k] ..].
void launch_arena_append(const float* probs, int n, int c, int V, int P, const int32_t* first, const int32_t* count,
                         const int32_t* page_off, const int32_t* pages, float* slab, hipStream_t st);
// dense [T][V] (T > 0) = the frames held in pages[0 .. (T - 1) / P]
void launch_arena_read(const float* slab, int V, int P, const int32_t* pages, int T, float* dense, hipStream_t st);
// dense [n][Tp][V] = the count[k] <= Tp frames of entry k (pages[page_off[k] ..]), zeros behind them; lens [n] = count
void launch_arena_read_many(const float* slab, int V, int P, const int32_t* count, const int32_t* page_off, const int32_t* pages,
                            int n, int Tp, float* dense, int32_t* lens, hipStream_t st);

}  // namespace ppasr
