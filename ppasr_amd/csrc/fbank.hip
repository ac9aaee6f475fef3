// fbank.hip -- Kaldi-compatible log-mel filterbank front-end on the GPU (the step BEFORE the
// encoder).  Replaces AudioFeaturizer.featurize (ppasr/data_utils/featurizer/audio_featurizer.py:37-67,120-138):
//   AudioSegment.normalize(target_dB)           data_utils/audio.py:287-304   gain = 10^((target - rms_dB)/20)
//   AudioSegment.to('int16')                    data_utils/audio.py:244       clip, truncate to int16
//   paddleaudio.compliance.kaldi.fbank(...)     third-party (paddleaudio>=1.0.1, requirements.txt:14; not in the tree):
//       snip_edges framing (25 ms / 10 ms), remove_dc_offset, pre-emphasis 0.97 (first sample against itself),
//       povey window = hann(periodic=False)^0.85, zero-pad to 512, power spectrum, 80 triangular mel bins on the mel
//       scale 1127 ln(1 + f/700) from 20 Hz to Nyquist over FFT bins 0..255, log(max(e, FLT_EPSILON)), dither 0.
// One 256-thread workgroup per frame: the frame lives in LDS from the raw samples to the 80 log-mel values
// (radix-2 FFT, one butterfly per thread per stage); HBM traffic = the samples once (L2 absorbs the 2.5x frame
// overlap) + 320 B per frame out.  HBM- / latency-bound: 4 B * 160 new samples + 320 B out per frame.
// MFCC form (ppasr_mfcc_create; paddleaudio.compliance.kaldi.mfcc with use_energy False, subtract_mean False, lifter 22):
// the same frame kernel, compiled a second time with one more stage -- the log-mel values go to LDS instead of HBM, and
// n_mfcc threads contract them with the orthonormal DCT-II table and apply the lifter.  No further launch.
#include "launch.h"
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

#include "capi_internal.h"

namespace {

constexpr int kFT = 256;       // threads per frame
constexpr int kNfftMax = 512;  // 25 ms at <= 16 kHz (20.48 kHz would still fit)

struct FbankTables {
  const float* window;   // [win]
  const float* tw_re;    // [nfft/2] cos(-2 pi k / nfft)
  const float* tw_im;    // [nfft/2] sin(-2 pi k / nfft)
  const float* bank;     // [n_mels][nfft/2]
  const int* bank_lo;    // [n_mels] first bin with a non-zero weight
  const int* bank_hi;    // [n_mels] one past the last
};

// The MFCC form's own tables, a trailing kernel argument of their own: the fbank form's argument layout stays as it is.
struct MfccTables {
  const float* dct;     // [n_mels][n_mfcc] D[m][k]: column k is read by thread k, so a row is one coalesced load
  const float* lifter;  // [n_mfcc] L[k]
  int n_mfcc;
};

// ---- mean square of AudioSegment.rms_db (audio.py:526: np.mean(self._samples ** 2) on float32 samples) ----
// numpy reduces a contiguous float32 array in chunks of 8192 elements (the ufunc buffer size), res = 0; res += S(chunk),
// and S is its pairwise sum: n <= 128 -> eight running sums r[j] += a[8i + j], ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)),
// then the n % 8 tail element by element; n > 128 -> S(first n2) + S(rest), n2 = n/2 rounded down to a multiple of 8.
// All float32, squares rounded before they are added (x ** 2 is an array of its own).  The oracle calls np.mean, so the
// kernel has to reproduce this order bit for bit: one ulp of the mean square moves the gain and with it one int16 sample
// in a few thousand by one LSB (tests/test_fbank_gpu.py, the 10 s case).
// One workgroup per chunk: heap node h (root 1) of the chunk's tree = 8 lanes (the eight running sums of a leaf).
constexpr int kPwChunk = 8192, kPwLeaf = 128;
// A FULL chunk is 2^6 leaves of 128.  A shorter last chunk can be one level deeper: the "rest" half keeps up to 7 extra
// elements per split (8191 -> 4103 -> 2055 -> 1031 -> 519 -> 263 -> 135 -> 71), so 135 > 128 at depth 6 splits once more.
// Depth 7 is the bound for every n <= 8192 (tests/test_fbank_cpu.py walks all 8192 lengths): 256 heap slots.
constexpr int kPwDepth = 7, kPwSlots = 1 << (kPwDepth + 1);

// node h of the pairwise tree over n elements: its range; false when an ancestor is already a leaf
__host__ __device__ __forceinline__ bool pw_node(int h, int n, int& off, int& len) {
  off = 0;
  len = n;
  int top = 0;
  while ((h >> (top + 1)) != 0) ++top;  // depth of h (root 1 = depth 0)
  for (int d = top - 1; d >= 0; --d) {
    if (len <= kPwLeaf) return false;
    int n2 = len / 2;
    n2 -= n2 % 8;
    if ((h >> d) & 1) {
      off += n2;
      len -= n2;
    } else {
      len = n2;
    }
  }
  return true;
}

// The tree of one chunk: `a` = its first sample, `cn` = its length (1 .. 8192); all 1024 threads of the workgroup call it,
// thread 0 gets the chunk's sum.
__device__ __forceinline__ float sumsq_chunk(const float* __restrict__ a, int cn) {
  // numpy rounds every square before it is added (x ** 2 is an array of its own): no fused multiply-add here.  hipcc
  // contracts a * b + c -- also when written __fadd_rn(c, __fmul_rn(a, b)): the header's operations carry the contract
  // flag -- into v_fma_f32 under its default -ffp-contract=fast (found in round 6: one ulp of the sum for ~1 length in
  // 3), so this function uses plain operators with contraction switched off.
#pragma clang fp contract(off)
  __shared__ float val[kPwSlots];
  __shared__ unsigned char inner[kPwSlots];  // 1: node with two children
  const int j = threadIdx.x & 7;  // 8 lanes per heap slot; 128 slots per pass, two passes
  for (int h = threadIdx.x >> 3; h < kPwSlots; h += 128) {
    int off = 0, len = 0;
    const bool node = h >= 1 && pw_node(h, cn, off, len);
    const bool leaf = node && len <= kPwLeaf;
    float r = 0.f;
    if (leaf && len >= 8) {
      const int full = len - (len % 8);
      float v = a[off + j];
      r = v * v;
      for (int i = 8; i < full; i += 8) {
        v = a[off + i + j];
        r = r + v * v;
      }
    }
    // ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)): a butterfly over the 8 lanes (float addition commutes)
    r = r + __shfl_xor(r, 1);
    r = r + __shfl_xor(r, 2);
    r = r + __shfl_xor(r, 4);
    if (j == 0) {
      inner[h] = node && !leaf;
      if (leaf) {
        int i = len - (len % 8);
        if (len < 8) {
          r = 0.f;
          i = 0;
        }
        for (; i < len; ++i) {
          const float v = a[off + i];
          r = r + v * v;
        }
        val[h] = r;
      }
    }
  }
  __syncthreads();
  for (int d = kPwDepth - 1; d >= 0; --d) {  // inner nodes of depth d: slots [2^d, 2^(d+1))
    const int h = (1 << d) + (int)threadIdx.x;
    if ((int)threadIdx.x < (1 << d) && inner[h]) val[h] = val[2 * h] + val[2 * h + 1];
    __syncthreads();
  }
  return val[1];
}

__global__ __launch_bounds__(1024) void k_sumsq(const float* __restrict__ x, int n, float* __restrict__ chunk_sum) {
  const int c0 = blockIdx.x * kPwChunk, cn = min(kPwChunk, n - c0);
  const float r = sumsq_chunk(x + c0, cn);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = r;
}

// ---- segment-table (batch) forms: one launch covers n independent waveforms packed back to back in `x` ----
// The last segment whose first chunk / first frame is <= key: the segment that owns chunk / frame `key` (segments
// without chunks / frames share their successor's prefix value and are passed over).  key < the total, so it exists.
template <int ppasr_fbank_segment::*kFirst>
__device__ __forceinline__ int segment_of(const ppasr_fbank_segment* __restrict__ seg, int n_seg, int key) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid].*kFirst <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// grid = the total number of chunks; chunk numbering restarts in every segment (numpy's order is per waveform)
__global__ __launch_bounds__(1024) void k_sumsq_batch(const float* __restrict__ x, const ppasr_fbank_segment* __restrict__ seg,
                                                      int n_seg, float* __restrict__ chunk_sum) {
  __shared__ long long s_first;
  __shared__ int s_cn;
  if (threadIdx.x == 0) {
    const ppasr_fbank_segment g = seg[segment_of<&ppasr_fbank_segment::first_chunk>(seg, n_seg, (int)blockIdx.x)];
    const int c0 = ((int)blockIdx.x - g.first_chunk) * kPwChunk;
    s_first = g.first_sample + c0;
    s_cn = min(kPwChunk, g.n_samples - c0);
  }
  __syncthreads();
  const float r = sumsq_chunk(x + s_first, s_cn);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = r;
}

// gain of AudioSegment.normalize (audio.py:287-304, gain_db :256-264): the chunk sums of one waveform of n samples, added in
// chunk order -> out[0] the linear gain, out[1] the gain in dB
__device__ __forceinline__ void gain_of(const float* __restrict__ sums, int n_chunks, int n, float target_db,
                                        float* __restrict__ out) {
  float s = 0.f;
  for (int c = 0; c < n_chunks; ++c) s = __fadd_rn(s, sums[c]);
  // the scalar types numpy 1.x gives the reference here (oracle/fbank_oracle.py; pinned by tests/golden/ref_wav.npz): the
  // mean square and its log10 are float32, 10 * log10, target_db - rms_db and the power are float64, the gain is rounded
  // to float32 when it scales the float32 samples.  (n == 0, a segment of the batch form only: rms_db 0 like silence)
  const float ms = n > 0 ? (float)((double)s / (double)n) : 0.f;
  const double rms_db = ms != 0.f ? 10.0 * (double)(float)log10((double)ms) : 0.0;
  out[0] = (float)pow(10.0, ((double)target_db - rms_db) / 20.0);
  out[1] = (float)((double)target_db - rms_db);  // the host raises beyond max_gain_db = 300 like audio.py:301
}

// once per call: ws[n_chunks], ws[n_chunks + 1] <- the gain, the gain in dB
__global__ void k_gain(float* __restrict__ ws, int n_chunks, int n, float target_db) {
  gain_of(ws, n_chunks, n, target_db, ws + n_chunks);
}

// one thread per segment: gains[2 s], gains[2 s + 1] <- the gain of segment s, its gain in dB
__global__ __launch_bounds__(64) void k_gain_batch(const float* __restrict__ chunk_sum,
                                                   const ppasr_fbank_segment* __restrict__ seg, int n_seg, float target_db,
                                                   float* __restrict__ gains) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= n_seg) return;
  const ppasr_fbank_segment g = seg[s];
  gain_of(chunk_sum + g.first_chunk, (g.n_samples + kPwChunk - 1) / kPwChunk, g.n_samples, target_db, gains + 2 * (size_t)s);
}

// One frame, by the 256 threads of a workgroup: `src` = its first sample, `gain` = its waveform's gain (1 without dB
// normalisation), `out` = its n_mels log-mel values (kMfcc: its mc.n_mfcc cepstral coefficients; `mc` is not read otherwise).
template <bool kMfcc>
__device__ __forceinline__ void fbank_frame(const float* __restrict__ src, float gain, const FbankTables& tb, int win,
                                            int nfft, int log2n, int n_mels, float* __restrict__ out, const MfccTables& mc) {
  __shared__ float re[kNfftMax], im[kNfftMax];
  __shared__ double dred[4];
  __shared__ float s_mean;
  const int tid = threadIdx.x;
  // ---- load: float -> gain -> int16 (clip, truncate) ----
  for (int i = tid; i < nfft; i += kFT) {
    float v = 0.f;
    if (i < win) {
      float t = (src[i] * gain) * 32768.0f;
      t = fminf(fmaxf(t, -32768.f), 32767.f);
      v = truncf(t);
    }
    re[i] = v;
  }
  __syncthreads();
  // ---- remove_dc_offset ----
  {
    double s = 0.0;
    for (int i = tid; i < win; i += kFT) s += (double)re[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) dred[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) s_mean = (float)((dred[0] + dred[1] + dred[2] + dred[3]) / (double)win);
    __syncthreads();
  }
  const float mean = s_mean;
  // ---- pre-emphasis + window, written in bit-reversed order for the in-place DIT FFT ----
  float y[2];
  int dst[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int i = tid + q * kFT;
    float v = 0.f;
    if (i < win && i < nfft) {
      const float cur = re[i] - mean;
      const float prev = re[i > 0 ? i - 1 : 0] - mean;
      v = (cur - 0.97f * prev) * tb.window[i];
    }
    y[q] = v;
    dst[q] = (int)(__brev((unsigned)i) >> (32 - log2n));
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int i = tid + q * kFT;
    if (i < nfft) {
      re[dst[q]] = y[q];
      im[dst[q]] = 0.f;
    }
  }
  __syncthreads();
  // ---- radix-2 decimation-in-time FFT: nfft/2 butterflies per stage, one (or fewer) per thread ----
  for (int s = 1; s <= log2n; ++s) {
    const int half = 1 << (s - 1);
    for (int bfly = tid; bfly < nfft / 2; bfly += kFT) {
      const int grp = bfly >> (s - 1), k = bfly & (half - 1);
      const int i0 = (grp << s) + k, i1 = i0 + half;
      const int tw = k << (log2n - s);
      const float wr = tb.tw_re[tw], wi = tb.tw_im[tw];
      const float xr = re[i1], xi = im[i1];
      const float tr = wr * xr - wi * xi, ti = wr * xi + wi * xr;
      const float ur = re[i0], ui = im[i0];
      re[i0] = ur + tr; im[i0] = ui + ti;
      re[i1] = ur - tr; im[i1] = ui - ti;
    }
    __syncthreads();
  }
  // ---- power spectrum of bins 0 .. nfft/2-1 (the Nyquist bin is not used by the mel banks) ----
  for (int k = tid; k < nfft / 2; k += kFT) {
    const float p = re[k] * re[k] + im[k] * im[k];
    re[k] = p;
  }
  __syncthreads();
  if (tid < n_mels) {
    const float* w = tb.bank + (size_t)tid * (nfft / 2);
    float e = 0.f;
    for (int k = tb.bank_lo[tid]; k < tb.bank_hi[tid]; ++k) e = fmaf(re[k], w[k], e);
    const float v = logf(fmaxf(e, 1.1920928955078125e-07f));
    if constexpr (kMfcc) im[tid] = v;  // (im[] is free since the power spectrum went to re[]; n_mels <= kFT <= kNfftMax)
    else out[tid] = v;
  }
  if constexpr (kMfcc) {
    // ---- DCT-II over the mel axis + lifter: thread k forms coefficient k.  im[m] is one address for the whole wave (an
    // LDS broadcast), D's row m is n_mfcc consecutive floats (<= 256 KB in all, shared by every frame: it stays in L2) ----
    __syncthreads();
    if (tid < mc.n_mfcc) {
      const float* d = mc.dct + tid;
      float a = 0.f;
#pragma unroll 8  // eight table loads in flight per wait: the loop is bound by their L2 latency, not by the fma chain
      for (int m = 0; m < n_mels; ++m) a = fmaf(im[m], d[(size_t)m * mc.n_mfcc], a);
      out[tid] = a * mc.lifter[tid];
    }
  }
}

template <bool kMfcc>
__global__ __launch_bounds__(kFT) void k_fbank(const float* __restrict__ x, int n, const float* __restrict__ gain_p,
                                               int use_db, float target_db, FbankTables tb, int win, int shift,
                                               int nfft, int log2n, int n_mels, float* __restrict__ feats, MfccTables mc) {
  __shared__ float s_gain;
  const int frame = blockIdx.x;
  if (threadIdx.x == 0) s_gain = use_db ? *gain_p : 1.0f;
  __syncthreads();
  const int row = kMfcc ? mc.n_mfcc : n_mels;
  fbank_frame<kMfcc>(x + (size_t)frame * shift, s_gain, tb, win, nfft, log2n, n_mels, feats + (size_t)frame * row, mc);
}

// grid = the total number of frames (the compact numbering); a frame's output row = its segment's out_row + its number
// inside the segment, so the same kernel writes a compact [sum frames][n_mels] or a padded [B][Tmax][n_mels] array
// (kMfcc: rows of n_mfcc floats)
template <bool kMfcc>
__global__ __launch_bounds__(kFT) void k_fbank_batch(const float* __restrict__ x, const ppasr_fbank_segment* __restrict__ seg,
                                                     int n_seg, const float* __restrict__ gains, int use_db, FbankTables tb,
                                                     int win, int shift, int nfft, int log2n, int n_mels,
                                                     float* __restrict__ feats, MfccTables mc) {
  __shared__ long long s_src, s_row;
  __shared__ float s_gain;
  if (threadIdx.x == 0) {
    const int s = segment_of<&ppasr_fbank_segment::first_frame>(seg, n_seg, (int)blockIdx.x);
    const ppasr_fbank_segment g = seg[s];
    const int local = (int)blockIdx.x - g.first_frame;
    s_src = g.first_sample + (long long)local * shift;
    s_row = g.out_row + local;
    s_gain = use_db ? gains[2 * (size_t)s] : 1.0f;
  }
  __syncthreads();
  const int row = kMfcc ? mc.n_mfcc : n_mels;
  fbank_frame<kMfcc>(x + s_src, s_gain, tb, win, nfft, log2n, n_mels, feats + (size_t)s_row * row, mc);
}

}  // namespace

struct ppasr_fbank_s : DeviceAllocs {
  int sample_rate, n_mels, win, shift, nfft, log2n;
  FbankTables tb;
  MfccTables mc = {nullptr, nullptr, 0};  // n_mfcc == 0: the fbank form
};

// What ppasr_mfcc_create and ppasr_mfcc_tables refuse beyond ppasr_fbank_create's own refusals
static ppasr_status mfcc_check(int n_mels, int n_mfcc, float cepstral_lifter) {
  if (n_mels < 1 || n_mels > kFT || n_mfcc < 1 || n_mfcc > n_mels || !(cepstral_lifter >= 0.f) || std::isinf(cepstral_lifter))
    return fail(PPASR_EINVAL, "mfcc: needs 1 <= n_mfcc <= n_mels <= 256 and a finite cepstral_lifter >= 0");
  return PPASR_OK;
}

// The tables of the MFCC stage (ppasr_mfcc_create uploads them, ppasr_mfcc_tables hands them out): computed in double,
// rounded to float once.
static void mfcc_host_tables(int n_mels, int n_mfcc, float cepstral_lifter, float* dct, float* lifter) {
  const double pi = 3.14159265358979323846, q = (double)cepstral_lifter;
  for (int m = 0; m < n_mels; ++m) {  // orthonormal DCT-II: D^T D = I for n_mfcc == n_mels
    dct[(size_t)m * n_mfcc] = (float)sqrt(1.0 / n_mels);
    for (int k = 1; k < n_mfcc; ++k) dct[(size_t)m * n_mfcc + k] = (float)(sqrt(2.0 / n_mels) * cos(pi / n_mels * (m + 0.5) * k));
  }
  for (int k = 0; k < n_mfcc; ++k) lifter[k] = q > 0.0 ? (float)(1.0 + 0.5 * q * sin(pi * k / q)) : 1.0f;
}

// What ppasr_fbank_create and ppasr_mfcc_create share: the frame geometry and the tables of the log-mel stage.
static ppasr_status fbank_build(int sample_rate, int n_mels, float frame_length_ms, float frame_shift_ms,
                                std::unique_ptr<ppasr_fbank_s>& f) {
  if (sample_rate <= 0 || n_mels < 1 || n_mels > kFT) return fail(PPASR_EINVAL, "fbank: bad arguments");
  f = std::make_unique<ppasr_fbank_s>();
  f->sample_rate = sample_rate;
  f->n_mels = n_mels;
  f->win = (int)(sample_rate * 0.001 * frame_length_ms);
  f->shift = (int)(sample_rate * 0.001 * frame_shift_ms);
  if (f->win < 2 || f->shift < 1) return fail(PPASR_EINVAL, "fbank: frame length / shift too small");
  int nfft = 1, l2 = 0;
  while (nfft < f->win) { nfft <<= 1; ++l2; }
  if (nfft > kNfftMax) return fail(PPASR_EUNSUPPORTED, "fbank: frame longer than 512 samples");
  f->nfft = nfft;
  f->log2n = l2;
  const int nb = nfft / 2;
  std::vector<float> window(f->win), twr(nb), twi(nb), bank((size_t)n_mels * nb, 0.f);
  std::vector<int> lo(n_mels), hi(n_mels);
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < f->win; ++i)  // povey: hann (symmetric) ^ 0.85
    window[i] = (float)pow(0.5 - 0.5 * cos(2.0 * pi * i / (f->win - 1)), 0.85);
  for (int k = 0; k < nb; ++k) {
    twr[k] = (float)cos(-2.0 * pi * k / nfft);
    twi[k] = (float)sin(-2.0 * pi * k / nfft);
  }
  // get_mel_banks: low 20 Hz, high = Nyquist, no VTLN; weights in float32 on the mel scale
  auto mel = [](double hz) { return 1127.0 * log(1.0 + hz / 700.0); };
  const double mel_lo = mel(20.0), mel_hi = mel(0.5 * sample_rate);
  const double delta = (mel_hi - mel_lo) / (n_mels + 1);
  const double bin_w = (double)sample_rate / nfft;
  for (int m = 0; m < n_mels; ++m) {
    const double left = mel_lo + m * delta, center = left + delta, right = center + delta;
    int first = -1, last = -1;
    for (int k = 0; k < nb; ++k) {
      const double mk = mel(bin_w * k);
      const double up = (mk - left) / (center - left), down = (right - mk) / (right - center);
      const double w = std::max(0.0, std::min(up, down));
      bank[(size_t)m * nb + k] = (float)w;
      if (w > 0.0) {
        if (first < 0) first = k;
        last = k;
      }
    }
    lo[m] = first < 0 ? 0 : first;
    hi[m] = first < 0 ? 0 : last + 1;
  }
  auto up = [&](const void* src, size_t bytes, const void** dst) { return f->upload_bytes(src, bytes, dst); };
  const void* p = nullptr;
  ppasr_status s;
  if ((s = up(window.data(), window.size() * 4, &p)) != PPASR_OK) return s;
  f->tb.window = static_cast<const float*>(p);
  if ((s = up(twr.data(), twr.size() * 4, &p)) != PPASR_OK) return s;
  f->tb.tw_re = static_cast<const float*>(p);
  if ((s = up(twi.data(), twi.size() * 4, &p)) != PPASR_OK) return s;
  f->tb.tw_im = static_cast<const float*>(p);
  if ((s = up(bank.data(), bank.size() * 4, &p)) != PPASR_OK) return s;
  f->tb.bank = static_cast<const float*>(p);
  if ((s = up(lo.data(), lo.size() * 4, &p)) != PPASR_OK) return s;
  f->tb.bank_lo = static_cast<const int*>(p);
  if ((s = up(hi.data(), hi.size() * 4, &p)) != PPASR_OK) return s;
  f->tb.bank_hi = static_cast<const int*>(p);
  return PPASR_OK;
}

extern "C" {

ppasr_status ppasr_fbank_create(int sample_rate, int n_mels, float frame_length_ms, float frame_shift_ms,
                                ppasr_fbank_handle* out) {
  if (!out) return fail(PPASR_EINVAL, "fbank: bad arguments");
  std::unique_ptr<ppasr_fbank_s> f;
  ppasr_status s = fbank_build(sample_rate, n_mels, frame_length_ms, frame_shift_ms, f);
  if (s != PPASR_OK) return s;
  *out = f.release();
  return PPASR_OK;
}

ppasr_status ppasr_mfcc_tables(int n_mels, int n_mfcc, float cepstral_lifter, float* dct, float* lifter) {
  if (!dct || !lifter) return fail(PPASR_EINVAL, "mfcc: null argument");
  ppasr_status s = mfcc_check(n_mels, n_mfcc, cepstral_lifter);
  if (s == PPASR_OK) mfcc_host_tables(n_mels, n_mfcc, cepstral_lifter, dct, lifter);
  return s;
}

ppasr_status ppasr_mfcc_create(int sample_rate, int n_mels, int n_mfcc, float frame_length_ms, float frame_shift_ms,
                               float cepstral_lifter, ppasr_fbank_handle* out) {
  if (!out) return fail(PPASR_EINVAL, "mfcc: null argument");
  ppasr_status s = mfcc_check(n_mels, n_mfcc, cepstral_lifter);  // (refused before any allocation or device call)
  if (s != PPASR_OK) return s;
  std::vector<float> dct((size_t)n_mels * n_mfcc), lifter(n_mfcc);
  mfcc_host_tables(n_mels, n_mfcc, cepstral_lifter, dct.data(), lifter.data());
  std::unique_ptr<ppasr_fbank_s> f;
  if ((s = fbank_build(sample_rate, n_mels, frame_length_ms, frame_shift_ms, f)) != PPASR_OK) return s;
  const void* p = nullptr;
  if ((s = f->upload_bytes(dct.data(), dct.size() * 4, &p)) != PPASR_OK) return s;
  f->mc.dct = static_cast<const float*>(p);
  if ((s = f->upload_bytes(lifter.data(), lifter.size() * 4, &p)) != PPASR_OK) return s;
  f->mc.lifter = static_cast<const float*>(p);
  f->mc.n_mfcc = n_mfcc;
  *out = f.release();
  return PPASR_OK;
}

int ppasr_fbank_feature_dim(ppasr_fbank_handle f) { return !f ? 0 : f->mc.n_mfcc > 0 ? f->mc.n_mfcc : f->n_mels; }

ppasr_status ppasr_fbank_destroy(ppasr_fbank_handle f) {
  delete f;
  return PPASR_OK;
}

int ppasr_fbank_frames(ppasr_fbank_handle f, int n_samples) {
  if (!f || n_samples < f->win) return 0;
  return 1 + (n_samples - f->win) / f->shift;  // snip_edges
}

static size_t fbank_ws_bytes(int n_samples) {
  // one float per 8192-sample chunk of the mean square + the gain + the gain in dB; never less than the 8 KiB earlier
  // versions asked for
  const size_t chunks = n_samples > 0 ? ((size_t)n_samples + kPwChunk - 1) / kPwChunk : 0;
  return std::max<size_t>(8192, (chunks + 2) * sizeof(float));
}

size_t ppasr_fbank_workspace_bytes(ppasr_fbank_handle f, int n_samples) { return f ? fbank_ws_bytes(n_samples) : 0; }

ppasr_status ppasr_fbank_compute(ppasr_fbank_handle f, const float* samples, int n_samples, int use_db_norm,
                                 float target_db, float* feats, void* workspace, size_t workspace_bytes, void* stream) {
  if (!f || !samples || !feats || !workspace) return fail(PPASR_EINVAL, "fbank: null argument");
  if (workspace_bytes < fbank_ws_bytes(n_samples)) return fail(PPASR_ENOSPACE, "fbank: workspace too small");
  const int frames = ppasr_fbank_frames(f, n_samples);
  if (frames <= 0) return PPASR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  const int chunks = (n_samples + kPwChunk - 1) / kPwChunk;
  if (use_db_norm) {
    PPASR_LAUNCH(k_sumsq, dim3(chunks), dim3(1024), 0, st, samples, n_samples, ws);
    PPASR_LAUNCH(k_gain, dim3(1), dim3(1), 0, st, ws, chunks, n_samples, target_db);
  }
  if (f->mc.n_mfcc > 0)
    PPASR_LAUNCH(k_fbank<true>, dim3(frames), dim3(kFT), 0, st, samples, n_samples, ws + chunks, use_db_norm, target_db, f->tb,
                 f->win, f->shift, f->nfft, f->log2n, f->n_mels, feats, f->mc);
  else
    PPASR_LAUNCH(k_fbank<false>, dim3(frames), dim3(kFT), 0, st, samples, n_samples, ws + chunks, use_db_norm, target_db, f->tb,
                 f->win, f->shift, f->nfft, f->log2n, f->n_mels, feats, f->mc);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

// ---- batch form: n waveforms ("segments") packed back to back, one set of launches ----
ppasr_status ppasr_fbank_plan_batch(int sample_rate, float frame_length_ms, float frame_shift_ms, const int* n_samples,
                                    int n, int t_max, ppasr_fbank_segment* table, int* total_chunks, int* total_frames) {
  if (n < 0 || (n > 0 && (!n_samples || !table)) || !total_chunks || !total_frames || sample_rate <= 0 || t_max < 0)
    return fail(PPASR_EINVAL, "fbank plan: bad arguments");
  const int win = (int)(sample_rate * 0.001 * frame_length_ms), shift = (int)(sample_rate * 0.001 * frame_shift_ms);
  if (win < 2 || shift < 1) return fail(PPASR_EINVAL, "fbank plan: frame length / shift too small");
  long long sample = 0, chunk = 0, frame = 0;
  for (int b = 0; b < n; ++b) {
    const int ns = n_samples[b];
    if (ns < 0) return fail(PPASR_EINVAL, "fbank plan: negative sample count");
    const int frames = ns < win ? 0 : 1 + (ns - win) / shift;  // snip_edges
    if (t_max > 0 && frames > t_max) return fail(PPASR_EINVAL, "fbank plan: a segment has more frames than the row stride");
    if (chunk > INT_MAX || frame > INT_MAX) return fail(PPASR_EINVAL, "fbank plan: more than 2^31 - 1 chunks or frames");
    table[b].first_sample = sample;
    table[b].out_row = t_max > 0 ? (long long)b * t_max : frame;
    table[b].n_samples = ns;
    table[b].first_chunk = (int)chunk;
    table[b].first_frame = (int)frame;
    table[b].reserved = 0;
    sample += ns;
    chunk += (ns + kPwChunk - 1) / kPwChunk;
    frame += frames;
  }
  if (chunk > INT_MAX || frame > INT_MAX) return fail(PPASR_EINVAL, "fbank plan: more than 2^31 - 1 chunks or frames");
  *total_chunks = (int)chunk;
  *total_frames = (int)frame;
  return PPASR_OK;
}

static size_t fbank_batch_ws_bytes(int n, int total_chunks) {
  // one float per chunk, then {gain, gain in dB} per segment; never nothing, so that the pointer is a real one
  return std::max<size_t>(256, ((size_t)std::max(total_chunks, 0) + 2 * (size_t)std::max(n, 0)) * sizeof(float));
}

size_t ppasr_fbank_batch_workspace_bytes(int n, int total_chunks) { return fbank_batch_ws_bytes(n, total_chunks); }

ppasr_status ppasr_fbank_compute_batch(ppasr_fbank_handle f, const float* samples, const ppasr_fbank_segment* table_dev,
                                       int n, int total_chunks, int total_frames, int use_db_norm, float target_db,
                                       float* feats, void* workspace, size_t workspace_bytes, void* stream) {
  if (!f || !samples || !table_dev || !feats || !workspace) return fail(PPASR_EINVAL, "fbank batch: null argument");
  if (n < 0 || total_chunks < 0 || total_frames < 0) return fail(PPASR_EINVAL, "fbank batch: negative count");
  if (workspace_bytes < fbank_batch_ws_bytes(n, total_chunks)) return fail(PPASR_ENOSPACE, "fbank batch: workspace too small");
  if (n == 0) return PPASR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = static_cast<float*>(workspace);
  float* gains = ws + total_chunks;
  if (use_db_norm) {
    if (total_chunks > 0) PPASR_LAUNCH(k_sumsq_batch, dim3(total_chunks), dim3(1024), 0, st, samples, table_dev, n, ws);
    PPASR_LAUNCH(k_gain_batch, dim3((n + 63) / 64), dim3(64), 0, st, ws, table_dev, n, target_db, gains);
  }
  if (total_frames > 0 && f->mc.n_mfcc > 0)
    PPASR_LAUNCH(k_fbank_batch<true>, dim3(total_frames), dim3(kFT), 0, st, samples, table_dev, n, gains, use_db_norm, f->tb,
                 f->win, f->shift, f->nfft, f->log2n, f->n_mels, feats, f->mc);
  else if (total_frames > 0)
    PPASR_LAUNCH(k_fbank_batch<false>, dim3(total_frames), dim3(kFT), 0, st, samples, table_dev, n, gains, use_db_norm, f->tb,
                 f->win, f->shift, f->nfft, f->log2n, f->n_mels, feats, f->mc);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // extern "C"
