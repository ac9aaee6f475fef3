// resample.hip -- polyphase FIR resampler on the GPU: AudioSegment.resample (data_utils/audio.py:306-317), the step BEFORE
// the fbank front-end for audio that is not at the model's rate (audio_featurizer.py:46-47).  The filter is the one the host
// route (data_utils/featurizer.py::resample) gets from scipy.signal.resample_poly(x, up, down, window=("kaiser", beta)):
//   g = gcd(in_rate, out_rate), up = out_rate / g, down = in_rate / g, half_len = 10 max(up, down), L = 2 half_len + 1,
//   h = up * firwin(L, 1 / max(up, down), kaiser beta)   (windowed sinc, scaled to unit gain at 0 Hz),
//   n_pre_pad = down - half_len % down, n_pre_remove = (half_len + n_pre_pad) / down, hp = [0] * n_pre_pad + h,
//   y[m] = sum_i hp[(m + n_pre_remove) down - i up] x[i],   0 <= m < ceil(n_in up / down),   x = 0 outside the stream.
// With k = (m + n_pre_remove) down, q = k / up and p = k % up this is y[m] = sum_t table[p][t] x[q - t], t = 0 .. T - 1,
// table[p][t] = hp[p + t up] (0 past hp's end), T = ceil((L + n_pre_pad) / up): one row of T taps per phase.
// The kernel is stateless and addressed by ABSOLUTE stream position: one thread per output, one fp32 accumulator, the T
// taps in ascending t with fmaf -- an order that depends on the output's absolute index alone.  A whole utterance, a
// segment of a packed batch and a packet of a stream (its kept tail + the new samples) therefore give the same bytes.
// Memory-bound and small: the stores are coalesced, the loads of one tap step are neighbouring samples (stride down / up)
// and both the samples and the table (<= 54 KB for the standard rates) are served by L1 / L2.  Not tuned further.
#include "launch.h"
#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

#include "capi_internal.h"

namespace {

constexpr int kTile = PPASR_RESAMPLE_TILE;  // outputs (= threads) per workgroup
constexpr int kMaxRatio = 1024;             // max(up, down) the library accepts
constexpr double kKaiserBeta = 14.769656459379492;

struct Geometry {
  int up, down, taps, n_pre_pad, n_pre_remove, L;
};

ppasr_status geometry_of(int in_rate, int out_rate, Geometry* g) {
  if (in_rate <= 0 || out_rate <= 0) return fail(PPASR_EINVAL, "resampler: rates must be positive");
  if (in_rate == out_rate) return fail(PPASR_EINVAL, "resampler: equal rates need no resampler");
  int a = in_rate, b = out_rate;
  while (b != 0) {
    const int r = a % b;
    a = b;
    b = r;
  }
  g->up = out_rate / a;
  g->down = in_rate / a;
  const int mx = std::max(g->up, g->down);
  if (mx > kMaxRatio) return fail(PPASR_EUNSUPPORTED, "resampler: max(up, down) > 1024 after reducing the two rates");
  const int half_len = 10 * mx;
  g->L = 2 * half_len + 1;
  g->n_pre_pad = g->down - half_len % g->down;
  g->n_pre_remove = (half_len + g->n_pre_pad) / g->down;
  g->taps = (g->L + g->n_pre_pad + g->up - 1) / g->up;
  return PPASR_OK;
}

// modified Bessel function I0 by its power series: every term is positive, so there is no cancellation (x <= 15 here)
double bessel_i0(double x) {
  const double y = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= y / ((double)k * (double)k);
    sum += term;
    if (term < 1e-20 * sum) break;
  }
  return sum;
}

// table [up][taps]: firwin's windowed sinc in double (pass_zero, scaled to unit gain at 0 Hz), times up, rounded to float once
void host_table(const Geometry& g, float* table) {
  const double pi = 3.14159265358979323846;
  const int L = g.L;
  const double alpha = 0.5 * (L - 1), fc = 1.0 / std::max(g.up, g.down), i0b = bessel_i0(kKaiserBeta);
  std::vector<double> h(L);
  double sum = 0.0;
  for (int n = 0; n < L; ++n) {
    const double m = n - alpha, x = pi * fc * m;
    const double sinc = x == 0.0 ? 1.0 : sin(x) / x;
    const double r = m / alpha;
    const double w = bessel_i0(kKaiserBeta * sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    h[n] = fc * sinc * w;
    sum += h[n];
  }
  for (int p = 0; p < g.up; ++p)
    for (int t = 0; t < g.taps; ++t) {
      const long long j = (long long)p + (long long)t * g.up - g.n_pre_pad;  // index into h
      table[(size_t)p * g.taps + t] = j >= 0 && j < L ? (float)((double)g.up * (h[j] / sum)) : 0.f;
    }
}

struct ResampleParams {
  const float* table;  // [up][taps]
  int up, down, taps, n_pre_remove;
};

// Output j of one segment by one thread.  Index arithmetic in 64 bits: (m + n_pre_remove) * down passes 2^31 on long streams.
__device__ __forceinline__ void resample_one(const ResampleParams& rp, const float* __restrict__ in, long long in_first,
                                             long long n_in, float* __restrict__ out, long long out_first, long long n_out,
                                             long long j) {
  if (j >= n_out) return;
  const long long k = (out_first + j + rp.n_pre_remove) * (long long)rp.down;
  const long long q = k / rp.up;
  const int p = (int)(k - q * rp.up);
  const float* __restrict__ row = rp.table + (size_t)p * rp.taps;
  const long long i0 = q - in_first;  // tap t reads sample i0 - t of `in`
  float acc = 0.f;
  // (a sample outside the call's window is a zero that is still multiplied and added: the chain of T fmaf is the same
  //  whichever samples the window holds)
#pragma unroll 4  // four pairs of loads in flight per wait; the fmaf chain keeps its order
  for (int t = 0; t < rp.taps; ++t) {
    const long long i = i0 - t;
    const float x = (i >= 0 && i < n_in) ? in[i] : 0.f;
    acc = fmaf(row[t], x, acc);
  }
  out[j] = acc;
}

__global__ __launch_bounds__(kTile) void k_resample(ResampleParams rp, const float* __restrict__ in, long long in_first,
                                                    long long n_in, float* __restrict__ out, long long out_first,
                                                    long long n_out) {
  resample_one(rp, in, in_first, n_in, out, out_first, n_out, (long long)blockIdx.x * kTile + threadIdx.x);
}

// grid = (tiles of the longest segment, segments): a workgroup past its segment's last tile has nothing to do
__global__ __launch_bounds__(kTile) void k_resample_batch(ResampleParams rp, const float* __restrict__ in,
                                                          const ppasr_resample_segment* __restrict__ seg,
                                                          float* __restrict__ out) {
  const ppasr_resample_segment g = seg[blockIdx.y];
  resample_one(rp, in + g.in_offset, g.in_first, g.n_in, out + g.out_offset, g.out_first, g.n_out,
               (long long)blockIdx.x * kTile + threadIdx.x);
}

}  // namespace

struct ppasr_resampler_s : DeviceAllocs {
  Geometry g;
  ResampleParams rp;
};

extern "C" {

ppasr_status ppasr_resampler_geometry(int in_rate, int out_rate, int* up, int* down, int* taps_per_phase, int* n_pre_pad,
                                      int* n_pre_remove) {
  if (!up || !down || !taps_per_phase || !n_pre_pad || !n_pre_remove) return fail(PPASR_EINVAL, "resampler: null argument");
  Geometry g;
  ppasr_status s = geometry_of(in_rate, out_rate, &g);
  if (s != PPASR_OK) return s;
  *up = g.up;
  *down = g.down;
  *taps_per_phase = g.taps;
  *n_pre_pad = g.n_pre_pad;
  *n_pre_remove = g.n_pre_remove;
  return PPASR_OK;
}

ppasr_status ppasr_resampler_table(int in_rate, int out_rate, float* table) {
  if (!table) return fail(PPASR_EINVAL, "resampler: null argument");
  Geometry g;
  ppasr_status s = geometry_of(in_rate, out_rate, &g);
  if (s == PPASR_OK) host_table(g, table);
  return s;
}

long long ppasr_resampler_out_len(int in_rate, int out_rate, long long n_in) {
  Geometry g;
  if (geometry_of(in_rate, out_rate, &g) != PPASR_OK) return -1;
  if (n_in < 0 || n_in > PPASR_RESAMPLE_MAX_SAMPLES) {
    fail(PPASR_EINVAL, "resampler: sample count outside 0 .. 2^40");
    return -1;
  }
  return (n_in * g.up + g.down - 1) / g.down;
}

long long ppasr_resampler_ready(int in_rate, int out_rate, long long n_in_total) {
  const long long n_out = ppasr_resampler_out_len(in_rate, out_rate, n_in_total);
  if (n_out < 0) return -1;
  Geometry g;
  (void)geometry_of(in_rate, out_rate, &g);
  // output m reads samples up to q(m) = (m + n_pre_remove) down / up; q(m) < n  <=>  m + n_pre_remove < ceil(n up / down)
  return std::max(0LL, n_out - g.n_pre_remove);
}

long long ppasr_resampler_first_needed(int in_rate, int out_rate, long long m) {
  Geometry g;
  if (geometry_of(in_rate, out_rate, &g) != PPASR_OK) return -1;
  if (m < 0 || m > PPASR_RESAMPLE_MAX_SAMPLES) {
    fail(PPASR_EINVAL, "resampler: output index outside 0 .. 2^40");
    return -1;
  }
  const long long q = (m + g.n_pre_remove) * (long long)g.down / g.up;
  return std::max(0LL, q - (g.taps - 1));
}

ppasr_status ppasr_resampler_create(int in_rate, int out_rate, ppasr_resampler_handle* out) {
  if (!out) return fail(PPASR_EINVAL, "resampler: null argument");
  Geometry g;
  ppasr_status s = geometry_of(in_rate, out_rate, &g);  // (refused before any allocation or device call)
  if (s != PPASR_OK) return s;
  std::vector<float> table((size_t)g.up * g.taps);
  host_table(g, table.data());
  auto r = std::make_unique<ppasr_resampler_s>();
  r->g = g;
  const void* p = nullptr;
  if ((s = r->upload_bytes(table.data(), table.size() * sizeof(float), &p)) != PPASR_OK) return s;
  r->rp = ResampleParams{static_cast<const float*>(p), g.up, g.down, g.taps, g.n_pre_remove};
  *out = r.release();
  return PPASR_OK;
}

ppasr_status ppasr_resampler_destroy(ppasr_resampler_handle r) {
  delete r;
  return PPASR_OK;
}

ppasr_status ppasr_resample_compute(ppasr_resampler_handle r, const float* in, long long in_first, long long n_in, float* out,
                                    long long out_first, long long n_out, void* stream) {
  if (!r) return fail(PPASR_EINVAL, "resample: null handle");
  if (in_first < 0 || n_in < 0 || out_first < 0 || n_out < 0 || in_first > PPASR_RESAMPLE_MAX_SAMPLES ||
      n_in > PPASR_RESAMPLE_MAX_SAMPLES || out_first > PPASR_RESAMPLE_MAX_SAMPLES || n_out > PPASR_RESAMPLE_MAX_SAMPLES)
    return fail(PPASR_EINVAL, "resample: positions and counts must lie in 0 .. 2^40");
  if ((n_in > 0 && !in) || (n_out > 0 && !out)) return fail(PPASR_EINVAL, "resample: null buffer");
  if (n_out == 0) return PPASR_OK;
  const long long tiles = (n_out + kTile - 1) / kTile;
  if (tiles > 0x7fffffffLL) return fail(PPASR_EINVAL, "resample: more than 2^31 - 1 tiles of outputs in one call");
  PPASR_LAUNCH(k_resample, dim3((unsigned)tiles), dim3(kTile), 0, static_cast<hipStream_t>(stream), r->rp, in, in_first, n_in,
               out, out_first, n_out);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

ppasr_status ppasr_resample_compute_batch(ppasr_resampler_handle r, const float* in, const ppasr_resample_segment* segments_dev,
                                          int n, long long max_n_out, float* out, void* stream) {
  if (!r) return fail(PPASR_EINVAL, "resample batch: null handle");
  if (n < 0 || n > 65535 || max_n_out < 0) return fail(PPASR_EINVAL, "resample batch: needs 0 <= n <= 65535 and max_n_out >= 0");
  if (n == 0 || max_n_out == 0) return PPASR_OK;
  if (!in || !segments_dev || !out) return fail(PPASR_EINVAL, "resample batch: null argument");
  const long long tiles = (max_n_out + kTile - 1) / kTile;
  if (tiles > 0x7fffffffLL) return fail(PPASR_EINVAL, "resample batch: more than 2^31 - 1 tiles of outputs in a segment");
  PPASR_LAUNCH(k_resample_batch, dim3((unsigned)tiles, (unsigned)n), dim3(kTile), 0, static_cast<hipStream_t>(stream), r->rp, in,
               segments_dev, out);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // extern "C"
