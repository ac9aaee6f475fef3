// weights.h -- the one place where a checkpoint becomes device memory (host only; included by capi_internal.h).
// ppasr_create builds the blob map once and hands a Loader to the family's *_create; the recipes every family shares
// are written once here, the family-specific arithmetic (adaptive-scale vectors, gate packing, final_proj) stays with
// the family and goes through the same lookups and uploads.
#pragma once

inline BlobMap blob_map(const ppasr_weight_blob* blobs, int n_blobs) {
  BlobMap sd;
  for (int i = 0; i < n_blobs; ++i) {
    Blob b{blobs[i].data_host, blobs[i].ndim, {0, 0, 0, 0}};
    for (int j = 0; j < blobs[i].ndim && j < 4; ++j) b.shape[j] = blobs[i].shape[j];
    sd[blobs[i].name] = b;
  }
  return sd;
}

inline std::vector<float> vec_of(const float* p, size_t n) { return std::vector<float>(p, p + n); }

// `return` the status of a fallible step unless it is PPASR_OK
#define LOAD_TRY(expr)                    \
  do {                                    \
    ppasr_status _s = (expr);             \
    if (_s != PPASR_OK) return _s;        \
  } while (0)
// a host pointer to the named tensor, or the loader's error: nothing behind it runs with a failed lookup
#define GETW(var, name, numel)                      \
  const float* var = ld.get(name, (size_t)(numel)); \
  if (!var) return ld.emissing()

struct Loader {
  ppasr_model_s* m;
  const BlobMap& sd;
  std::string missing;  // the FIRST name a lookup did not find, or found with another element count
  // (a method that uses GETW names itself `ld`, like the code of a family does)

  bool has(const std::string& name) const { return sd.find(name) != sd.end(); }
  const float* get(const std::string& name, size_t numel) {
    auto it = sd.find(name);
    if (it == sd.end() || it->second.numel() != numel) {
      if (missing.empty()) missing = name;
      return nullptr;
    }
    return it->second.p;
  }
  // a tensor that exists in one of two shapes: the second lookup, made after the first one failed, decides
  const float* get_either(const std::string& name, size_t numel_a, size_t numel_b, bool* is_b) {
    const std::string before = missing;
    const float* p = get(name, numel_a);
    *is_b = !p;
    if (!p) {
      missing = before;
      p = get(name, numel_b);
    }
    return p;
  }
  ppasr_status emissing() const { return fail(PPASR_EMISSING, "missing or mis-shaped weight: " + missing); }

  ppasr_status up(const std::vector<float>& v, const float** dst) { return m->upload(v, dst); }
  ppasr_status up4(const std::vector<float>& v, const f32x4** dst) { return m->upload4(v, dst); }
  // the named tensor as it is
  ppasr_status vec(const std::string& name, size_t n, const float** dst) {
    Loader& ld = *this;
    GETW(p, name, n);
    return up(vec_of(p, n), dst);
  }
  // a [K][N] matrix y = x W from its accessor w(k, n), in fragment order (pack_b)
  template <typename Acc>
  ppasr_status packed(int K, int N, Acc w, const f32x4** dst) {
    return up4(pack_b(K, N, w), dst);
  }

  // ---- the recipes ----
  ppasr_status cmvn(int F, const float** mean, const float** istd) {
    LOAD_TRY(vec("encoder.global_cmvn.mean", F, mean));
    return vec("encoder.global_cmvn.istd", F, istd);
  }
  // positional table [max_len][d]: the checkpoint's own, or PositionalEncoding.__init__ (embedding.py:38-53)
  ppasr_status pe_table(const float** pe_dev) {
    const int d = m->desc.output_size > 0 ? m->desc.output_size : kD;
    const int max_len = m->desc.max_len > 0 ? m->desc.max_len : 5000;
    m->desc.max_len = max_len;
    std::vector<float> pe((size_t)max_len * d);
    auto it = sd.find("__pe_table__");
    if (it != sd.end() && it->second.numel() == pe.size()) {
      std::memcpy(pe.data(), it->second.p, pe.size() * sizeof(float));
    } else {
      for (int i = 0; i < d / 2; ++i) {
        float div = expf((float)(2 * i) * (float)(-(std::log(10000.0) / d)));
        for (int pos = 0; pos < max_len; ++pos) {
          float a = (float)pos * div;
          pe[(size_t)pos * d + 2 * i] = sinf(a);
          pe[(size_t)pos * d + 2 * i + 1] = cosf(a);
        }
      }
    }
    return up(pe, pe_dev);
  }
  // LayerNorm: `prefix`.weight / .bias
  ppasr_status norm(const std::string& prefix, int n, const float** g, const float** b) {
    LOAD_TRY(vec(prefix + ".weight", n, g));
    return vec(prefix + ".bias", n, b);
  }
  // ConvolutionModule.norm (convolution.py:65-71): nn.LayerNorm, or nn.BatchNorm1D (cnn_module_norm: batch_norm), which
  // at inference is the per-channel affine y = (x - _mean) / sqrt(_variance + 1e-5) * weight + bias: folded here into
  // scale / shift vectors in the LayerNorm slots, marked by cm_eps < 0 (ln_rows_inreg then skips the row statistics)
  ppasr_status conv_module_norm(const std::string& prefix, int d, const float** g, const float** b, float* cm_eps) {
    Loader& ld = *this;
    *cm_eps = 1e-5f;
    if (!has(prefix + "._mean")) return norm(prefix, d, g, b);
    GETW(mean, prefix + "._mean", d);
    GETW(var, prefix + "._variance", d);
    GETW(gw, prefix + ".weight", d);
    GETW(gb, prefix + ".bias", d);
    std::vector<float> sc(d), sh(d);
    for (int c = 0; c < d; ++c) {
      sc[c] = gw[c] / std::sqrt(var[c] + 1e-5f);
      sh[c] = gb[c] - mean[c] * sc[c];
    }
    *cm_eps = -1.f;
    LOAD_TRY(up(sc, g));
    return up(sh, b);
  }
  // conv taps [C][k] -> tap-major [k][C] (conv1 of the front ends, the depthwise convs, the time-reduction conv)
  ppasr_status taps(const float* w, int C, int k, const float** dst) {
    std::vector<float> t((size_t)k * C);
    for (int c = 0; c < C; ++c)
      for (int j = 0; j < k; ++j) t[(size_t)j * C + c] = w[(size_t)c * k + j];
    return up(t, dst);
  }
  ppasr_status taps(const std::string& name, int C, int k, const float** dst) {
    Loader& ld = *this;
    GETW(w, name, (size_t)C * k);
    return taps(w, C, k, dst);
  }
  // a dense Conv2D weight [cout][cin][kh][kw] as the GEMM accessor w(k, n): k = (kh * kw_n + kw) * d + cin
  static auto dense_conv(const float* w, int d, int n_taps) {
    return [=](int k, int n) { return w[((size_t)n * d + (k % d)) * n_taps + (k / d)]; };
  }
  // the front ends' second convolution from its accessor; `quad`: also the quad form of batched calls (front_fused.hip)
  template <typename Acc>
  ppasr_status conv2(int d, int n_taps, Acc w, bool quad, const f32x4** dst, const f32x4** dst_quad) {
    LOAD_TRY(packed(n_taps * d, d, w, dst));
    *dst_quad = nullptr;
    return quad ? up4(pack_conv2_quad(d, w), dst_quad) : PPASR_OK;
  }
  // the projection behind the convs: our K index = f * d + c; Paddle's = c * F2 + f (subsampling.py:113 transpose + reshape)
  ppasr_status embed(const std::string& prefix, int F2, int d, const f32x4** w, const float** b) {
    Loader& ld = *this;
    GETW(ew, prefix + ".weight", (size_t)d * F2 * d);
    LOAD_TRY(packed(F2 * d, d, [&](int k, int n) { return ew[((size_t)(k % d) * F2 + (k / d)) * d + n]; }, w));
    return vec(prefix + ".bias", d, b);
  }
  // A dense layer [K][N] from its accessor at(k, n) behind an optional per-channel input scale / bias (Squeezeformer's
  // adaptive scale):  (s.x + a) W + b = x (diag(s) W) + (a W + b), the bias in double.  Without a fold (as = ab = NULL) it
  // is the plain packing and the bias as it is.
  template <typename Acc>
  ppasr_status linear(Acc at, const float* bias, int K, int N, const float* as, const float* ab, const f32x4** wd,
                      const float** bd) {
    if (!as) {
      LOAD_TRY(packed(K, N, at, wd));
      return up(vec_of(bias, N), bd);
    }
    LOAD_TRY(packed(K, N, [&](int k, int n) { return as[k] * at(k, n); }, wd));
    std::vector<float> bf(N);
    for (int n = 0; n < N; ++n) {
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc += (double)ab[k] * (double)at(k, n);
      bf[n] = (float)((double)bias[n] + acc);
    }
    return up(bf, bd);
  }
  // PositionwiseFeedForward: `prefix`.w_1 / .w_2, the fold on w_1
  ppasr_status ffn(const std::string& prefix, int d, int H, const float* as, const float* ab, const f32x4** w1,
                   const float** b1, const f32x4** w2, const float** b2) {
    Loader& ld = *this;
    GETW(a1, prefix + ".w_1.weight", (size_t)d * H);
    GETW(c1, prefix + ".w_1.bias", H);
    GETW(a2, prefix + ".w_2.weight", (size_t)H * d);
    GETW(c2, prefix + ".w_2.bias", d);
    LOAD_TRY(linear([=](int k, int n) { return a1[(size_t)k * H + n]; }, c1, d, H, as, ab, w1, b1));
    return linear([=](int k, int n) { return a2[(size_t)k * d + n]; }, c2, H, d, nullptr, nullptr, w2, b2);
  }
  // attention projections: [Wq|Wk|Wv] as one [d][3d] matrix (the fold on its input) and linear_out
  ppasr_status qkv_out(const std::string& prefix, int d, const float* as, const float* ab, const f32x4** wqkv,
                       const float** bqkv, const f32x4** wo, const float** bo) {
    Loader& ld = *this;
    const float* ws[3];
    std::vector<float> b(3 * d);
    const char* names[3] = {"linear_q", "linear_k", "linear_v"};
    for (int j = 0; j < 3; ++j) {
      GETW(wj, prefix + names[j] + ".weight", (size_t)d * d);
      GETW(bj, prefix + names[j] + ".bias", d);
      ws[j] = wj;
      std::memcpy(&b[j * d], bj, d * sizeof(float));
    }
    GETW(ow, prefix + "linear_out.weight", (size_t)d * d);
    GETW(ob, prefix + "linear_out.bias", d);
    LOAD_TRY(linear([&](int k, int n) { return ws[n / d][(size_t)k * d + (n % d)]; }, b.data(), d, 3 * d, as, ab, wqkv, bqkv));
    return linear([=](int k, int n) { return ow[(size_t)k * d + n]; }, ob, d, d, nullptr, nullptr, wo, bo);
  }
  // the layer's projected positional table pe[0 .. max_len) W_pos (+ b_pos: grouped and Squeezeformer attention)
  ppasr_status pos_table(const std::string& prefix, int d, bool bias, const float* pe_dev, const float** ptab) {
    const float *w_dev = nullptr, *b_dev = nullptr;
    LOAD_TRY(vec(prefix + "linear_pos.weight", (size_t)d * d, &w_dev));
    if (bias) LOAD_TRY(vec(prefix + "linear_pos.bias", d, &b_dev));
    void* pt = nullptr;
    LOAD_TRY(m->alloc((size_t)m->desc.max_len * d * sizeof(float), &pt));
    launch_posproj(pe_dev, w_dev, b_dev, static_cast<float*>(pt), m->desc.max_len, nullptr, d);
    HIP_TRY(hipGetLastError());
    *ptab = static_cast<const float*>(pt);
    return PPASR_OK;
  }
  // the conv module's pointwise pair: Conv1D weights [out][in][1], W[k][n] = w[n][k]; GLU value = channels [0, d), gate =
  // [d, 2d).  Zero-padded / PAD frames see pointwise_conv1(0) = the ORIGINAL bias (a mask is applied behind the scale),
  // so the GLU pad vector comes from it whatever the fold.
  ppasr_status conv_pointwise(const std::string& prefix, int d, const float* as, const float* ab, const f32x4** pw1,
                              const float** pw1_b, const float** glu_pad, const f32x4** pw2, const float** pw2_b) {
    Loader& ld = *this;
    GETW(p1w, prefix + "pointwise_conv1.weight", (size_t)2 * d * d);
    GETW(p1b, prefix + "pointwise_conv1.bias", 2 * d);
    GETW(p2w, prefix + "pointwise_conv2.weight", (size_t)d * d);
    GETW(p2b, prefix + "pointwise_conv2.bias", d);
    LOAD_TRY(linear([=](int k, int n) { return p1w[(size_t)n * d + k]; }, p1b, d, 2 * d, as, ab, pw1, pw1_b));
    std::vector<float> gp(d);
    for (int c = 0; c < d; ++c) gp[c] = p1b[c] * (1.0f / (1.0f + expf(-p1b[c + d])));
    LOAD_TRY(up(gp, glu_pad));
    return linear([=](int k, int n) { return p2w[(size_t)n * d + k]; }, p2b, d, d, nullptr, nullptr, pw2, pw2_b);
  }
  // an output layer [K][V] with its columns zero-padded to a multiple of `mult` (32: the CTC head's tiles; 256: a dense
  // layer's column blocks)
  ppasr_status head(const float* w, const float* bias, int K, int V, int mult, const f32x4** wd, const float** bd) {
    const int Vp = (V + mult - 1) / mult * mult;
    LOAD_TRY(packed(K, Vp, [&](int k, int n) { return n < V ? w[(size_t)k * V + n] : 0.f; }, wd));
    std::vector<float> bp(Vp, 0.f);
    std::memcpy(bp.data(), bias, V * sizeof(float));
    return up(bp, bd);
  }
};
