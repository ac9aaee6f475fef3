// front_fused.hip -- Conv2dSubsampling4's second convolution in the quad form, with conv1 fused in (conformer/subsampling.py:84-88):
//   y2[b][t'][f2][c2] = relu(b2 + sum_{kh,kw,c} W2[c2][c][kh][kw] * y1[b][2t'+kh][2f2+kw][c]),
//   y1[b][t1][f1][c]  = relu(b1 + sum_{i,j} W1[c][i][j] * cmvn(x)[b][2t1+i][2f1+j]).
//
// Quad form (Winograd F(2x2, 2x2)).  A quad is output frames 2p, 2p + 1 x output bins 2q, 2q + 1; it reads the 5 x 5 y1
// values at frames 4p .. 4p + 4 and columns 4q .. 4q + 4.  Along each axis, with d0, d1, d2 = y1[0], y1[2], y1[4] and
// o0, o1 = y1[1], y1[3] of that axis, F(2,2) with points 0, 1, inf:
//   A = (d0 - d1) w0 + o0 w1,   S = d1 (w0 + w2),   B = (d2 - d1) w2 + o1 w1,   out[0] = A + S,   out[1] = S + B.
// In 2-D the 3 x 3 points XY' need 25 K=256 products per quad (the pair form over time: 30, the direct form: 36), and
//   y[0][0] = AA' + AS' + SA' + SS',  y[0][1] = AS' + AB' + SS' + SB',  y[1][0] = SA' + SS' + BA' + BS',
//   y[1][1] = SS' + SB' + BS' + BB',  each then relu(. + b2).
// A product is an input tile (a time transform D01 = d0 - d1, O0 = o0, D1 = d1, D21 = d2 - d1, O1 = o1 of the frequency
// transform D01', O0', D1', D21', O1' of the y1 patch: constants +-1) times one of 16 weight slabs
// {w0, w1, w0 + w2, w2} (kh) x {w0, w1, w0 + w2, w2} (kw) of W2[c2][c][kh][kw], summed at load (capi_internal.h
// pack_conv2_quad).  A GEMM row is a (utterance, pair, q) quad; quads never straddle utterances.  An odd Tp leaves the
// last pair's second frame dead and an odd F2 the last quad's second column: computed from clamped or zero inputs, never
// written (the live outputs read none of those inputs).
//
// Output-domain accumulation: y00, y01, y10, y11 take the 16 single-output products (AA', AB', BA', BB') directly; the
// 9 shared-point products (SS', SA', SB', AS', BS') go through two temporary sets, which VALU adds fold into the outputs
// they feed during a later chunk that writes neither those outputs nor that set: 6 x 16 accumulator registers.
// The contraction runs in 2 stages (128-channel halves) of 25 chunks, one product each, with its own 32-row LDS A tile
// and 128 x 256 weight slab; the tile of chunk j + 1 is produced while the matrix pipe works on chunk j (rb_gemm Side;
// double-buffered LDS).  Chunk order: time groups D1, D01, O0, D21, O1, each over the frequency taps D1', D01', O0',
// D21', O1'.  Every chunk then needs one new y1 value per row (25 per quad and channel, no recomputation): the d1 frame's
// 5 values (in LDS, private to the thread) and the group's centre value (in registers) are kept for the chunks that
// use them.
//
// k_conv12 computes the y1 values from the features held in LDS (the tile's input frames, normalised once) and conv1's
// weights, also in LDS; each thread owns 4 channels and 2 rows -- y1 never leaves the chip.  k_conv2_pair is its
// two-launch twin (behind k_conv1, ppasr_set_front_fused(0)): the same body with the y1 values read from HBM.  k_conv1
// runs the same fmaf chain per y1 element, and the chunk / MFMA / fold / epilogue order is shared: the two routes are
// bit-identical.
#include <utility>

#include "conformer_kernels.h"
#include "launch.h"

namespace ppasr {

namespace {
// Chunk t of a stage = time group t / 5 (D1, D01, O0, D21, O1) x frequency tap t % 5 (D1', D01', O0', D21', O1').
constexpr int kGroupRow[5] = {2, 0, 1, 4, 3};  // the y1 frame of the patch a time group evaluates
constexpr int kTapCol[5] = {2, 0, 1, 4, 3};    // the y1 column of the patch a frequency tap evaluates
constexpr int kFactor[5] = {2, 0, 1, 3, 1};    // the weight factor of a transform: 0 w0, 1 w1, 2 w0 + w2, 3 w2
constexpr int quad_slab(int t) { return 4 * kFactor[t / 5] + kFactor[t % 5]; }
// accumulator of chunk t: 0..3 = y00, y01, y10, y11; 4, 5 = the temporary sets
//   D1 x D1' = SS' -> 4; D1 x {D01', O0'} = SA' -> 5; D1 x {D21', O1'} = SB' -> 4;
//   {D01, O0} x D1' = AS' -> 5, x {D01', O0'} -> y00, x {D21', O1'} -> y01;
//   {D21, O1} x D1' = BS' -> 4, x {D01', O0'} -> y10, x {D21', O1'} -> y11
constexpr int quad_target(int t) {
  const int g = t / 5, k = t % 5;
  if (g == 0) return k == 0 ? 4 : k <= 2 ? 5 : 4;
  const int a = (g == 1 || g == 2) ? 0 : 2;
  return k == 0 ? (a == 0 ? 5 : 4) : k <= 2 ? a : a + 1;
}
// folds during chunk t (a set's last product is behind; chunk t writes neither the set nor the outputs it is folded
// into): the set, the outputs (bit mask over y00, y01, y10, y11), and whether the set is cleared for its next point
constexpr int quad_fold_src(int t) {
  return t == 1 || t == 5 || t == 21 || t == 23 ? 4 : t == 3 || t == 11 || t == 13 ? 5 : -1;
}
constexpr int quad_fold_mask(int t) {
  return t == 1 ? 0xf : t == 3 ? 0x5 : t == 5 ? 0xa : t == 11 ? 0x2 : t == 13 ? 0x1 : t == 21 ? 0x8 : t == 23 ? 0x4 : 0;
}
constexpr bool quad_fold_clear(int t) { return t == 1 || t == 3 || t == 5 || t == 13 || t == 23; }
static_assert(quad_target(0) == 4 && quad_target(2) == 5 && quad_target(10) == 5 && quad_target(12) == 0 &&
                  quad_target(14) == 1 && quad_target(20) == 4 && quad_target(22) == 2 && quad_target(24) == 3,
              "chunk targets");

template <typename Fn, int... I>
__device__ __forceinline__ void static_for(std::integer_sequence<int, I...>, Fn&& fn) {
  (fn(std::integral_constant<int, I>{}), ...);
}

// row stride of the fused route's feature patch: the last quad's dead column reads bins up to 8 Q + 2 (zeros past F)
__host__ __device__ inline int quad_xs_stride(int F, int Q) { return F > 8 * Q + 3 ? F : 8 * Q + 3; }
}  // namespace

// FROM_Y1 = false: src = features [B][T][F] (T, F: feature frames / bins); true: src = y1 [B][T][F][256] (T1, F1)
template <bool FROM_Y1>
__device__ __forceinline__ void conv2_quad_body(const float* __restrict__ src, const FrontW& fw, float* __restrict__ out,
                                                int T, int F, int Tp, int F2, int M, int m0, const PadSkip& ps,
                                                const int* __restrict__ tile_tab) {
  constexpr int BP = 32, KC = 128, LD = KC + 4, G = KC / 8, NL = 2, N_CHUNKS = 25;
  constexpr int SLOT = BP * LD;      // one A buffer
  const int P = (Tp + 1) >> 1;       // pairs per utterance
  const int Q = (F2 + 1) >> 1;       // quads per pair; M = B * P * Q rows
  // tile -> rows: as k_gemm_stream (ragged batches: the t-th ACTIVE tile of the table, cut per utterance)
  int r0 = m0 + blockIdx.x * BP, Mlim = M;
  if (tile_tab) {
    const int t = blockIdx.x, nb = tile_tab[0];
    const int* pre = tile_tab + 1;
    if (t >= pre[nb]) return;
    int lo = 0, hi = nb;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pre[mid] <= t) lo = mid;
      else hi = mid;
    }
    const int S = ps.Tp * ps.unit;
    r0 = lo * S + (t - pre[lo]) * BP;
    Mlim = min(M, (lo + 1) * S);
  } else if (pad_block_skippable(ps, r0, BP, M)) {
    return;
  }
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* const slot0 = smem;
  float* const slot1 = smem + SLOT;
  f32x4* const y2s = reinterpret_cast<f32x4*>(smem + 2 * SLOT);  // the D1 group's y1 values, [5][NL][kThreads]
  float* const w1s = smem + 2 * SLOT + 5 * NL * 4 * kThreads;     // fused: conv1's weights [9][256] and bias [256]
  float* const xs = w1s + 10 * 256;    // fused: the tile's feature patch
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  constexpr int tile_stride = 2 * 16 * G * 64;  // 2 stages x 16 slabs of G k-groups
  const f32x4* wbase = fw.conv2_wp + (size_t)wave * tile_stride;  // (wave-uniform)
  auto seg = [&](int h, int slab) { return wbase + (size_t)(16 * h + slab) * G * 64; };
  BRing<1> ring;
  ring_prime(ring, seg(0, quad_slab(0)), 0);
  const int c4 = tid & 31, rbase = tid >> 5;  // this thread's channel quad and first row (rows rbase + 16 i, i < NL)
  const int bp0 = r0 / Q;                     // first (utterance, pair) of the tile
  // ---- per-row state: where row i's y1 values come from ----
  // fused: the row's window inside xs (the tile's input frames 8p .. 8p + 10 of each pair, row stride FX), two 16-bit
  // offsets per register (0xffff: a zero row); twin: the row's first y1 frame b T1 + 4p, the frame 4p and 4q (-1: a
  // zero row)
  const int FX = quad_xs_stride(F, Q);
  uint32_t pb = 0;
  int yrow[FROM_Y1 ? NL : 1], yp4[FROM_Y1 ? NL : 1], yq4[FROM_Y1 ? NL : 1];
  if constexpr (!FROM_Y1) {
    for (int idx = tid; idx < 10 * 256; idx += kThreads) w1s[idx] = idx < 9 * 256 ? fw.conv1_w[idx] : fw.conv1_b[idx - 9 * 256];
    const int nbp = (min(r0 + BP, Mlim) - 1) / Q - bp0 + 1;
    for (int idx = tid; idx < nbp * 11 * FX; idx += kThreads) {
      const int fr_row = idx / FX, f = idx - fr_row * FX;
      const int bpl = fr_row / 11, fr = fr_row - 11 * bpl;
      const int bp = bp0 + bpl, b = bp / P, p = bp - b * P;
      const int t = min(8 * p + fr, T - 1);  // (< T except for the dead second frame of an odd Tp's last pair)
      xs[idx] = f < F ? (src[((size_t)b * T + t) * F + f] - fw.cmvn_mean[f]) * fw.cmvn_istd[f] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int m = r0 + rbase + 16 * i;
      const int bp = m / Q, q = m - bp * Q;
      const uint32_t v = m < Mlim ? (uint32_t)((bp - bp0) * 11 * FX + 8 * q) : 0xffffu;
      pb |= v << (16 * i);
    }
  } else {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int m = r0 + rbase + 16 * i;
      const int bp = m / Q, q = m - bp * Q, b = bp / P, p = bp - b * P;
      yrow[i] = b * T + 4 * p;
      yp4[i] = 4 * p;
      yq4[i] = m < Mlim ? 4 * q : -1;
    }
  }
  auto pbase = [&](int i) { return (int)((pb >> (16 * i)) & 0xffffu); };
  const int lds_off0 = rbase * LD + 4 * c4;  // row i of this thread: + i * 16 * LD
  float xv[9];
  f32x4 wv[3], bv, ya, yv;
  // y1 value of row i at patch frame r, column c, channels h * 128 + 4 c4 .. + 3, in 4 steps (one per k-group):
  // 0 the request (LDS window / HBM) and conv1 taps 0..2's weights, 1..3 k_conv1's fmaf chain over taps 3 (step - 1)
  // .. + 2 (fused), the bias and ReLU in step 3
  auto y1_step = [&](int i, int h, int r, int c, int step) {
    const int cc = h * 128 + 4 * c4;
    if constexpr (!FROM_Y1) {
      if (step == 0) {
        const int o = pbase(i);
        const float* p = xs + (o == 0xffff ? 0 : o) + 2 * r * FX + 2 * c;
#pragma unroll
        for (int ii = 0; ii < 3; ++ii)
#pragma unroll
          for (int jj = 0; jj < 3; ++jj) xv[ii * 3 + jj] = p[ii * FX + jj];
        ya = f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
#pragma unroll
        for (int j = 3 * (step - 1); j < 3 * step; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) ya[e] = fmaf(wv[j % 3][e], xv[j], ya[e]);
        if (step == 3) {
          ya += bv;
#pragma unroll
          for (int e = 0; e < 4; ++e) ya[e] = pbase(i) != 0xffff ? fmaxf(ya[e], 0.f) : 0.f;
        }
      }
      if (step < 3) {  // the next step's weights
#pragma unroll
        for (int j = 0; j < 3; ++j) wv[j] = *reinterpret_cast<const f32x4*>(w1s + (3 * step + j) * 256 + cc);
        if (step == 2) bv = *reinterpret_cast<const f32x4*>(w1s + 9 * 256 + cc);
      }
    } else {
      if (step == 0) {
        // (zero rows, the frames behind T1 that only the dead second frame of an odd Tp's last pair reads, and the
        // columns behind F1 that only the dead second column of an odd F2's last quad reads)
        yv = f32x4{0.f, 0.f, 0.f, 0.f};
        if (yq4[i] >= 0 && yp4[i] + r < T && yq4[i] + c < F)
          yv = *reinterpret_cast<const f32x4*>(src + ((size_t)(yrow[i] + r) * F + yq4[i] + c) * 256 + cc);
      } else if (step == 3) {
        ya = yv;
      }
    }
  };
  auto put = [&](float* buf, int i, const f32x4& v) { *reinterpret_cast<f32x4*>(buf + lds_off0 + i * 16 * LD) = v; };
  // the D1 group's y1 values (used by D01 and D21: private to the thread, kept in LDS), the group's centre value
  auto y2row = [&](int c, int i) -> f32x4& { return y2s[(c * NL + i) * kThreads + tid]; };
  f32x4 z2[NL];
  // k-group g < 4 NL of a chunk: step g & 3 of row g >> 2 of tile n (stage h) into buf
  auto build = [&](auto nc, int g, int h, float* buf) {
    constexpr int n = decltype(nc)::value, grp = n / 5, k = n % 5, r = kGroupRow[grp], c = kTapCol[k];
    const int i = g >> 2, step = g & 3;
    y1_step(i, h, r, c, step);
    if (step != 3) return;
    f32x4 v = ya;
    if constexpr (grp == 0) y2row(c, i) = ya;
    if constexpr (grp == 1 || grp == 3) v = ya - y2row(c, i);
    if constexpr (k == 0) {
      z2[i] = v;
      put(buf, i, v);
    } else if constexpr (k == 1 || k == 3) {
      put(buf, i, v - z2[i]);
    } else {
      put(buf, i, v);
    }
  };
  f32x16 acc[6][1][1];
#pragma unroll
  for (int a = 0; a < 6; ++a) acc_zero(acc[a]);
  auto fold = [&](auto tc, int g) {  // k-groups 4 NL .. of chunk t: one output per k-group, then the clear
    constexpr int t = decltype(tc)::value, fs = quad_fold_src(t), mask = quad_fold_mask(t);
    if constexpr (fs >= 0) {
      const int j = g - 4 * NL;
      int seen = 0;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        if (!((mask >> o) & 1)) continue;
        if (seen++ == j) {  // (in place: a plain vector add is given fresh registers beside the accumulators)
#pragma unroll
          for (int e = 0; e < 16; ++e) asm volatile("v_add_f32 %0, %0, %1" : "+v"(acc[o][0][0][e]) : "v"(acc[fs][0][0][e]));
        }
      }
      if (quad_fold_clear(t) && j == 4) acc_zero(acc[fs]);
    }
  };
  __syncthreads();  // xs, w1s complete
#pragma unroll
  for (int g = 0; g < 4 * NL; ++g) {
    build(std::integral_constant<int, 0>{}, g, 0, slot0);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  for (int h = 0; h < 2; ++h) {
    // (opaque per stage: keeps the compiler from hoisting the 25 chunks' y1 addresses and weight resources out of the
    // stage loop, where they would stay live -- and spill -- across it)
    asm volatile("" : "+s"(wbase));
    if constexpr (!FROM_Y1) {
      asm volatile("" : "+v"(pb));
    } else {
#pragma unroll
      for (int i = 0; i < NL; ++i) asm volatile("" : "+v"(yrow[i]), "+v"(yp4[i]), "+v"(yq4[i]));
    }
    static_for(std::make_integer_sequence<int, N_CHUNKS>{}, [&](auto tc) {
      constexpr int t = decltype(tc)::value;
      // slot of chunk 25 h + t: (t + h) & 1
      float* const cur = ((t + h) & 1) ? slot1 : slot0;
      float* const nxb = ((t + h) & 1) ? slot0 : slot1;
      const f32x4* nseg = t + 1 < N_CHUNKS ? seg(h, quad_slab(t + 1)) : (h == 0 ? seg(1, quad_slab(0)) : nullptr);
      auto side = [&](int g) {
        if (g < 4 * NL) {
          if constexpr (t + 1 < N_CHUNKS) build(std::integral_constant<int, t + 1>{}, g, h, nxb);
          else if (h == 0) build(std::integral_constant<int, 0>{}, g, 1, nxb);
        } else {
          fold(tc, g);
        }
      };
      rb_gemm<1, 1, G, kPF, decltype(side)>(cur, LD, seg(h, quad_slab(t)), 0, nseg, 0, ring, acc[quad_target(t)], side);
      __syncthreads();
    });
  }
  const int col = wave * 32 + (lane & 31);
  const float b2 = fw.conv2_b[col];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = r0 + acc_row(r, lane);
    if (m >= Mlim) continue;
    const int bp = m / Q, q = m - bp * Q, b = bp / P, t0 = 2 * (bp - b * P), f0 = 2 * q;
    float* o = out + ((size_t)(b * Tp + t0) * F2 + f0) * 256 + col;
    const bool f1 = f0 + 1 < F2, t1 = t0 + 1 < Tp;
    o[0] = fmaxf(acc[0][0][0][r] + b2, 0.f);
    if (f1) o[256] = fmaxf(acc[1][0][0][r] + b2, 0.f);
    if (t1) o[(size_t)F2 * 256] = fmaxf(acc[2][0][0][r] + b2, 0.f);
    if (t1 && f1) o[(size_t)F2 * 256 + 256] = fmaxf(acc[3][0][0][r] + b2, 0.f);
  }
}

__global__ __launch_bounds__(kThreads) void k_conv12(const float* __restrict__ feats, FrontW fw, float* __restrict__ out,
                                                     int T, int F, int Tp, int F2, int M, int m0, PadSkip ps,
                                                     const int* __restrict__ tile_tab) {
  conv2_quad_body<false>(feats, fw, out, T, F, Tp, F2, M, m0, ps, tile_tab);
}
// (the name of the two-launch twin is kept from the pair form)
__global__ __launch_bounds__(kThreads) void k_conv2_pair(const float* __restrict__ y1, FrontW fw, float* __restrict__ out,
                                                         int T1, int F1, int Tp, int F2, int M, int m0, PadSkip ps,
                                                         const int* __restrict__ tile_tab) {
  conv2_quad_body<true>(y1, fw, out, T1, F1, Tp, F2, M, m0, ps, tile_tab);
}

static int quad_tile_pairs(int Q) { return 31 / Q + 2; }  // (utterance, pair)s a 32-row tile touches, at most
static size_t quad_lds(bool fused, int F, int F2) {
  const int Q = (F2 + 1) / 2;
  return ((size_t)2 * 32 * 132 + (size_t)5 * 2 * 4 * 512 + (fused ? (size_t)10 * 256 + (size_t)quad_tile_pairs(Q) * 11 * quad_xs_stride(F, Q) : 0)) *
         sizeof(float);
}
bool conv2_quad_supported(const FrontW& fw) { return fw.conv2_wp && fw.conv2_k == 3 && fw.conv2_s == 2; }
bool conv12_supported(const FrontW& fw, int F, int F2) {
  // the quad form's weights, and the tile's features + conv1's weights + the A double buffer must fit the CU's LDS
  const int Q = (F2 + 1) / 2;
  return conv2_quad_supported(fw) && F2 >= 1 && quad_lds(true, F, F2) <= 160 * 1024 &&
         (size_t)quad_tile_pairs(Q) * 11 * quad_xs_stride(F, Q) < 0xffff;  // (16-bit window offsets)
}

// tile_prefix_launch: the ragged launch's tile table (front_kernels.hip k_tile_prefix)
void launch_tile_prefix(const PadSkip& ps, int B, int BM, int* tab, hipStream_t st);

// rows are (utterance, pair, q): B * ceil(Tp / 2) * ceil(F2 / 2) of them.  Pair p holds frames 2p, 2p + 1 = input
// frames 8p .., so the ragged-batch rule of the frames (need = ceil(len / 4) + slack frames) becomes ceil(len / 8) +
// ceil(slack / 2) pairs (a superset: ceil((a + s) / 2) <= ceil(a / 2) + ceil(s / 2)).
static void launch_quad(bool fused, const float* src, const FrontW& fw, float* y2, int B, int T, int F, int Tp, int F2,
                        hipStream_t st, const PadSkip& ps_frames, int* tile_scratch) {
  const int P = (Tp + 1) / 2, Q = (F2 + 1) / 2;
  PadSkip ps = ps_frames;
  ps.Tp = P;
  ps.mul = 2 * ps_frames.mul;
  ps.slack = (ps_frames.slack + 1) / 2;
  ps.unit = Q;
  const int M = B * P * Q;
  const int* no_tab = nullptr;
#define QUAD(GRID, TAB)                                                                                                  \
  do {                                                                                                                 \
    if (fused)                                                                                                         \
      PPASR_LAUNCH(k_conv12, dim3(GRID), dim3(kThreads), quad_lds(true, F, F2), st, src, fw, y2, T, F, Tp, F2, M, 0, ps, \
                   TAB);                                                                                               \
    else                                                                                                               \
      PPASR_LAUNCH(k_conv2_pair, dim3(GRID), dim3(kThreads), quad_lds(false, F, F2), st, src, fw, y2, T, F, Tp, F2, M, 0, \
                   ps, TAB);                                                                                           \
  } while (0)
  // 32-row tiles: 6 x 16 accumulator registers; ragged batches: the active tiles in front of one grid
  if (ps.lens && tile_scratch) {
    launch_tile_prefix(ps, B, 32, tile_scratch, st);
    QUAD(B * ((P * Q + 31) / 32), (const int*)tile_scratch);
    return;
  }
  QUAD((M + 31) / 32, no_tab);
#undef QUAD
}

void launch_conv12(const float* feats, const FrontW& fw, float* y2, int B, int T, int F, int Tp, int F2, hipStream_t st,
                   const PadSkip& ps_frames, int* tile_scratch) {
  launch_quad(true, feats, fw, y2, B, T, F, Tp, F2, st, ps_frames, tile_scratch);
}
void launch_conv2_quad(const float* y1, const FrontW& fw, float* y2, int B, int T1, int F1, int Tp, int F2, hipStream_t st,
                       const PadSkip& ps_frames, int* tile_scratch) {
  launch_quad(false, y1, fw, y2, B, T1, F1, Tp, F2, st, ps_frames, tile_scratch);
}

hipError_t configure_front_fused_kernels() {
  hipError_t e;
#define SET_LDS(fn)                                                                                              \
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
  if (e != hipSuccess) return e;
  SET_LDS(k_conv12);
  SET_LDS(k_conv2_pair);
#undef SET_LDS
  return hipSuccess;
}

}  // namespace ppasr
