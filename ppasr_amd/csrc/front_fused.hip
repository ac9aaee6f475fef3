// front_fused.hip -- Conv2dSubsampling4's second convolution in the pair form, with conv1 fused in (conformer/subsampling.py:84-88):
//   y2[b][t'][f2][c2] = relu(b2 + sum_{kh,kw,c} W2[c2][c][kh][kw] * y1[b][2t'+kh][2f2+kw][c]),
//   y1[b][t1][f1][c]  = relu(b1 + sum_{i,j} W1[c][i][j] * cmvn(x)[b][2t1+i][2f1+j]).
//
// Pair form (Winograd F(2,2) over time).  Output frames t0 = 2p and t0 + 1 read y1 frames 4p .. 4p + 4.  With
// d0, d1, d2 = y1 frames 4p, 4p + 2, 4p + 4, o0, o1 = y1 frames 4p + 1, 4p + 3 and g0, g1 = W2[kh=0], W2[kh=2]:
//   A = (d0 - d1) g0 + o0 W2[kh=1],   S = d1 (g0 + g1),   B = (d2 - d1) g1 + o1 W2[kh=1],
//   y2[t0] = relu(A + S + b2),        y2[t0 + 1] = relu(S + B + b2)
// (each product a K = 3 x 256 contraction over (kw, c)): 5 K=256 tap-GEMMs per pair of output frames instead of 6, and
// 5 y1 frames instead of 6.  The transform constants are +-1; g0 + g1 is folded into the weights at load
// (capi_internal.h pack_conv2_pair).  A GEMM row is a (pair, f2) position; pairs never straddle utterances (an odd Tp
// leaves the last pair's second frame dead: computed from clamped inputs, never written).
//
// The contraction runs in 6 stages (kw, 128-channel half), each as 4 chunks with their own LDS A tile and weight slab:
//   D01 = d0 - d1 (x g0 -> A),  O = [o0; o1] (x W2[kh=1] -> A and B: one weight slab, two row tiles),
//   D1 = d1 (x (g0 + g1) -> S), D21 = d2 - d1 (x g1 -> B).
// The tile of chunk j + 1 is produced while the matrix pipe works on chunk j (rb_gemm Side; double-buffered LDS).
//
// k_conv12 computes the y1 values from the features held in LDS (the tile's input frames, normalised once; each thread
// owns 4 channels and 2 MT rows, d1 is kept in registers between the chunks that use it) -- y1 never leaves the chip.
// k_conv2_pair is its two-launch twin (behind k_conv1, ppasr_set_front_fused(0)): the same body with the y1 values read
// from HBM.  k_conv1 runs the same fmaf chain per y1 element, and the chunk / MFMA / epilogue order is shared: the two
// routes are bit-identical.
#include "conformer_kernels.h"
#include "launch.h"

namespace ppasr {

// FROM_Y1 = false: src = features [B][T][F] (T, F: feature frames / bins); true: src = y1 [B][T][F][256] (T1, F1)
template <int MT, bool FROM_Y1>
__device__ __forceinline__ void conv2_pair_body(const float* __restrict__ src, const FrontW& fw, float* __restrict__ out,
                                                int T, int F, int Tp, int F2, int M, int m0, const PadSkip& ps,
                                                const int* __restrict__ tile_tab) {
  constexpr int BP = 32 * MT, KC = 128, LD = KC + 4, G = KC / 8, NL = 2 * MT, N_STAGES = 6, N_CHUNKS = 4 * N_STAGES;
  constexpr int SLOT = 2 * BP * LD;  // one A buffer: the O chunk's 2 BP rows
  const int P = (Tp + 1) >> 1;       // pairs per utterance; M = B * P * F2 rows
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
  const int tid = threadIdx.x, lane = lane_id(), wave = wave_id();
  constexpr int tile_stride = N_CHUNKS * G * 64;
  const f32x4* wbase = fw.conv2_wp + (size_t)wave * tile_stride;
  BRing<1> ring;
  ring_prime(ring, wbase, 0);
  const int c4 = tid & 31, rbase = tid >> 5;  // this thread's channel quad and first row (rows rbase + 16 i, i < NL)
  const int bp0 = r0 / F2;                    // first (utterance, pair) of the tile
  // ---- per-row state: where row i's y1 values come from ----
  // fused: the row's window inside xs (the tile's input frames 8p .. 8p + 10 of each pair), two 16-bit offsets per
  // register (0xffff: a zero row); twin: the row's first y1 frame b T1 + 4p, the frame 4p and 2 f2 (-1: a zero row)
  float* xs = smem + 2 * SLOT;
  uint32_t pb[MT];
  int yrow[FROM_Y1 ? NL : 1], yp4[FROM_Y1 ? NL : 1], yf[FROM_Y1 ? NL : 1];
  if constexpr (!FROM_Y1) {
    const int nbp = (min(r0 + BP, Mlim) - 1) / F2 - bp0 + 1;
    for (int idx = tid; idx < nbp * 11 * F; idx += kThreads) {
      const int q = idx / F, f = idx - q * F;
      const int bpl = q / 11, fr = q - 11 * bpl;
      const int bp = bp0 + bpl, b = bp / P, p = bp - b * P;
      const int t = min(8 * p + fr, T - 1);  // (< T except for the dead second frame of an odd Tp's last pair)
      xs[idx] = (src[((size_t)b * T + t) * F + f] - fw.cmvn_mean[f]) * fw.cmvn_istd[f];
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int m = r0 + rbase + 16 * i;
      const int bp = m / F2, f2 = m - bp * F2;
      const uint32_t v = m < Mlim ? (uint32_t)((bp - bp0) * 11 * F + 4 * f2) : 0xffffu;
      pb[i >> 1] = (i & 1) ? (pb[i >> 1] | (v << 16)) : v;
    }
  } else {
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int m = r0 + rbase + 16 * i;
      const int bp = m / F2, f2 = m - bp * F2, b = bp / P, p = bp - b * P;
      yrow[i] = b * T + 4 * p;
      yp4[i] = 4 * p;
      yf[i] = m < Mlim ? 2 * f2 : -1;
    }
  }
  auto pbase = [&](int i) { return (int)((i & 1) ? (pb[i >> 1] >> 16) : (pb[i >> 1] & 0xffffu)); };
  const int lds_off0 = rbase * LD + 4 * c4;  // row i of this thread: + i * 16 * LD
  f32x4 wv[FROM_Y1 ? 1 : 9], bv;
  float xv[9];
  f32x4 yv;
  auto load_w = [&](int s) {  // conv1 weights of the 4 channels this thread produces in stage s
    if constexpr (!FROM_Y1) {
      const int c = (s & 1) * 128 + 4 * c4;
#pragma unroll
      for (int j = 0; j < 9; ++j) wv[j] = *reinterpret_cast<const f32x4*>(fw.conv1_w + j * 256 + c);
      bv = *reinterpret_cast<const f32x4*>(fw.conv1_b + c);
    }
  };
  // y1 frame 4p + j of row i at column 2 f2 + kw, channels (s & 1) * 128 + 4 c4 .. + 3, in two steps: the request
  // (LDS window / HBM) during one k-group, the value during the next
  auto y1_read = [&](int i, int s, int j) {
    const int kw = s >> 1;
    if constexpr (!FROM_Y1) {
      const int o = pbase(i);
      const float* p = xs + (o == 0xffff ? 0 : o) + 2 * j * F + 2 * kw;
#pragma unroll
      for (int ii = 0; ii < 3; ++ii)
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) xv[ii * 3 + jj] = p[ii * F + jj];
    } else {
      // (zero rows, and the frames behind T1 that only the dead second frame of an odd Tp's last pair reads)
      yv = f32x4{0.f, 0.f, 0.f, 0.f};
      if (yf[i] >= 0 && yp4[i] + j < T)
        yv = *reinterpret_cast<const f32x4*>(src + ((size_t)(yrow[i] + j) * F + yf[i] + kw) * 256 + (s & 1) * 128 + 4 * c4);
    }
  };
  auto y1_value = [&](int i) {  // k_conv1's arithmetic (fused) / the value read (twin)
    if constexpr (!FROM_Y1) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 9; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] = fmaf(wv[j][e], xv[j], a[e]);
      a += bv;
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = pbase(i) != 0xffff ? fmaxf(a[e], 0.f) : 0.f;
      return a;
    } else {
      return yv;
    }
  };
  auto put = [&](float* buf, int row16, const f32x4& v) {  // row16: this thread's row index (+ NL for O's second half)
    *reinterpret_cast<f32x4*>(buf + lds_off0 + row16 * 16 * LD) = v;
  };
  f32x4 d1c[NL], d0;  // d1 of the stage's rows (used by D01, D1 and D21); d0 until its d1 is there
  // the chunks' tiles; y1 value number e (read during k-group 2e, used during 2e + 1)
  auto side_d01 = [&](int s, int g) {  // D01 of stage s into slot 0
    const int e = g >> 1, i = e >> 1;
    if (e >= 2 * NL) return;
    if ((g & 1) == 0) {
      y1_read(i, s, (e & 1) ? 2 : 0);
    } else if ((e & 1) == 0) {
      d0 = y1_value(i);
    } else {
      d1c[i] = y1_value(i);
      put(slot0, i, d0 - d1c[i]);
    }
  };
  auto side_o = [&](int s, int g) {  // O of stage s into slot 1: o0 in rows [0, BP), o1 in rows [BP, 2 BP)
    const int e = g >> 1, hi = e >= NL, i = e - (hi ? NL : 0);
    if (e >= 2 * NL) return;
    if ((g & 1) == 0) y1_read(i, s, hi ? 3 : 1);
    else put(slot1, hi ? NL + i : i, y1_value(i));
  };
  auto side_d1 = [&](int g) {  // D1 into slot 0
    if (g < NL) put(slot0, g, d1c[g]);
  };
  auto side_d21 = [&](int s, int g) {  // D21 of stage s into slot 1
    const int e = g >> 1;
    if (e >= NL) return;
    if ((g & 1) == 0) y1_read(e, s, 4);
    else put(slot1, e, y1_value(e) - d1c[e]);
  };
  load_w(0);
  __syncthreads();  // xs complete
#pragma unroll
  for (int g = 0; g < 2 * G; ++g) {
    side_d01(0, g);
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  f32x16 accA[MT][1], accB[MT][1], accS[MT][1];
  acc_zero(accA);
  acc_zero(accB);
  acc_zero(accS);
  for (int s = 0; s < N_STAGES; ++s) {
    const f32x4* seg = wbase + (size_t)(4 * s) * G * 64;
    {
      auto side = [&](int g) { side_o(s, g); };
      rb_gemm<MT, 1, G, kPF, decltype(side)>(slot0, LD, seg, 0, seg + G * 64, 0, ring, accA, side);
    }
    __syncthreads();
    {  // (the W2[kh=1] slab is streamed twice: o0 -> A, then o1 -> B)
      auto side = [&](int g) { side_d1(g); };
      rb_gemm<MT, 1, G, kPF, decltype(side)>(slot1, LD, seg + G * 64, 0, seg + G * 64, 0, ring, accA, side);
      rb_gemm<MT, 1, G>(slot1 + BP * LD, LD, seg + G * 64, 0, seg + 2 * G * 64, 0, ring, accB);
    }
    __syncthreads();
    {
      auto side = [&](int g) { side_d21(s, g); };
      rb_gemm<MT, 1, G, kPF, decltype(side)>(slot0, LD, seg + 2 * G * 64, 0, seg + 3 * G * 64, 0, ring, accS, side);
    }
    __syncthreads();
    if (s + 1 < N_STAGES) {
      load_w(s + 1);
      auto side = [&](int g) { side_d01(s + 1, g); };
      rb_gemm<MT, 1, G, kPF, decltype(side)>(slot1, LD, seg + 3 * G * 64, 0, seg + 4 * G * 64, 0, ring, accB, side);
    } else {
      rb_gemm<MT, 1, G>(slot1, LD, seg + 3 * G * 64, 0, nullptr, 0, ring, accB);
    }
    __syncthreads();
  }
  const int col = wave * 32 + (lane & 31);
  const float b2 = fw.conv2_b[col];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = r0 + mt * 32 + acc_row(r, lane);
      if (m >= Mlim) continue;
      const int bp = m / F2, f2 = m - bp * F2, b = bp / P, t0 = 2 * (bp - b * P);
      const float s = accS[mt][0][r];
      float* o = out + ((size_t)(b * Tp + t0) * F2 + f2) * 256 + col;
      o[0] = fmaxf(accA[mt][0][r] + s + b2, 0.f);
      if (t0 + 1 < Tp) o[(size_t)F2 * 256] = fmaxf(s + accB[mt][0][r] + b2, 0.f);
    }
}

template <int MT>
__global__ __launch_bounds__(kThreads) void k_conv12(const float* __restrict__ feats, FrontW fw, float* __restrict__ out,
                                                     int T, int F, int Tp, int F2, int M, int m0, PadSkip ps,
                                                     const int* __restrict__ tile_tab) {
  conv2_pair_body<MT, false>(feats, fw, out, T, F, Tp, F2, M, m0, ps, tile_tab);
}
template <int MT>
__global__ __launch_bounds__(kThreads) void k_conv2_pair(const float* __restrict__ y1, FrontW fw, float* __restrict__ out,
                                                         int T1, int F1, int Tp, int F2, int M, int m0, PadSkip ps,
                                                         const int* __restrict__ tile_tab) {
  conv2_pair_body<MT, true>(y1, fw, out, T1, F1, Tp, F2, M, m0, ps, tile_tab);
}

static size_t pair_lds(int mt, bool fused, int F, int F2) {
  const int bp = 32 * mt, nbp = (bp - 1) / F2 + 2;
  return ((size_t)2 * 2 * bp * 132 + (fused ? (size_t)nbp * 11 * F : 0)) * sizeof(float);
}
bool conv2_pair_supported(const FrontW& fw) { return fw.conv2_wp && fw.conv2_k == 3 && fw.conv2_s == 2; }
bool conv12_supported(const FrontW& fw, int F, int F2) {
  // the pair form's weights, and the tile's features + A double buffer must fit the CU's LDS
  return conv2_pair_supported(fw) && F2 >= 1 && pair_lds(1, true, F, F2) <= 160 * 1024 &&
         (size_t)((31 / F2) + 2) * 11 * F < 0xffff;  // (16-bit window offsets)
}

// tile_prefix_launch: the ragged launch's tile table (front_kernels.hip k_tile_prefix)
void launch_tile_prefix(const PadSkip& ps, int B, int BM, int* tab, hipStream_t st);

// rows are (utterance, pair, f2): B * ceil(Tp / 2) * F2 of them.  Pair p holds frames 2p, 2p + 1 = input frames 8p ..,
// so the ragged-batch rule of the frames (need = ceil(len / 4) + slack frames) becomes ceil(len / 8) + ceil(slack / 2)
// pairs (a superset: ceil((a + s) / 2) <= ceil(a / 2) + ceil(s / 2)).
static void launch_pair(bool fused, const float* src, const FrontW& fw, float* y2, int B, int T, int F, int Tp, int F2,
                        hipStream_t st, const PadSkip& ps_frames, int* tile_scratch) {
  const int P = (Tp + 1) / 2;
  PadSkip ps = ps_frames;
  ps.Tp = P;
  ps.mul = 2 * ps_frames.mul;
  ps.slack = (ps_frames.slack + 1) / 2;
  ps.unit = F2;
  const int M = B * P * F2;
  const int* no_tab = nullptr;
#define PAIR(MTA, GRID, M0, TAB)                                                                                        \
  do {                                                                                                                 \
    if (fused)                                                                                                         \
      PPASR_LAUNCH(k_conv12<MTA>, dim3(GRID), dim3(kThreads), pair_lds(MTA, true, F, F2), st, src, fw, y2, T, F, Tp, F2, \
                   M, M0, ps, TAB);                                                                                    \
    else                                                                                                               \
      PPASR_LAUNCH(k_conv2_pair<MTA>, dim3(GRID), dim3(kThreads), pair_lds(MTA, false, F, F2), st, src, fw, y2, T, F,   \
                   Tp, F2, M, M0, ps, TAB);                                                                            \
  } while (0)
  // 32-row tiles (MT = 2 would need 96 accumulator registers besides conv1's weights and operands: more than the 256 a
  // lane of a two-waves-per-SIMD workgroup has).  Ragged batches: the active tiles in front of one grid.
  if (ps.lens && tile_scratch) {
    launch_tile_prefix(ps, B, 32, tile_scratch, st);
    PAIR(1, B * ((P * F2 + 31) / 32), 0, (const int*)tile_scratch);
    return;
  }
  PAIR(1, (M + 31) / 32, 0, no_tab);
#undef PAIR
}

void launch_conv12(const float* feats, const FrontW& fw, float* y2, int B, int T, int F, int Tp, int F2, hipStream_t st,
                   const PadSkip& ps_frames, int* tile_scratch) {
  launch_pair(true, feats, fw, y2, B, T, F, Tp, F2, st, ps_frames, tile_scratch);
}
void launch_conv2_pair(const float* y1, const FrontW& fw, float* y2, int B, int T1, int F1, int Tp, int F2, hipStream_t st,
                       const PadSkip& ps_frames, int* tile_scratch) {
  launch_pair(false, y1, fw, y2, B, T1, F1, Tp, F2, st, ps_frames, tile_scratch);
}

hipError_t configure_front_fused_kernels() {
  hipError_t e;
#define SET_LDS(fn)                                                                                              \
  e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); \
  if (e != hipSuccess) return e;
  SET_LDS(k_conv12<1>);
  SET_LDS(k_conv2_pair<1>);
#undef SET_LDS
  return hipSuccess;
}

}  // namespace ppasr
