// capi_stream.hip -- streaming entry points: <Family>Encoder.forward_chunk with the attention K/V cache and the
// conv-module cache resident on the device inside a stream-state object (the reference round-trips both through the
// host on every chunk, infer_utils/inference_predictor.py:196-210).
//   Conformer            conformer/encoder.py:208-283
//   Squeezeformer        squeezeformer/encoder.py:260-381   (time-reduced layers 5..10, recover at 11)
//   Efficient-Conformer  efficient_conformer/encoder.py:266-393 (grouped attention 0..3, stride layer 3, 7-tap convs after)
//
// Cache bookkeeping.  Every layer owns K and V caches [cap][256] (row = frame) and a conv-module input history
// [lo_max][256] (the reference's cnn_cache, frame-major; its first lo_i rows are used, lo_i = kernel_i - 1).
// Layers that run at half rate (after a time reduction / the stride layer) hold each cached frame ONCE; the reference
// stores those caches repeat_interleave'd to the full rate and reads them back with [::2], which is the identity on
// the values.  The frame COUNTS follow the reference's slicing exactly (including Squeezeformer's trim of the reduced
// cache to len(pos_emb) - len(xs) and of the exported cache to the first layer's length); a combination for which the
// reference itself fails with a shape error (odd cache lengths) is refused with PPASR_EINVAL.
#include <algorithm>

#include "capi_internal.h"

namespace {

inline bool is_sq(const ppasr_model_s* h) { return h->desc.model_type == PPASR_MODEL_SQUEEZEFORMER; }
inline bool is_eff(const ppasr_model_s* h) { return h->desc.model_type == PPASR_MODEL_EFFICIENT_CONFORMER; }

// calculate_downsampling_factor (squeezeformer/encoder.py:246-258, efficient_conformer/encoder.py:205-210)
inline int layer_factor(const ppasr_model_s* h, int i) {
  if (is_sq(h)) return (h->desc.reduce_idx >= 0 && i >= h->desc.reduce_idx && !(h->desc.recover_idx >= 0 && i >= h->desc.recover_idx)) ? 2 : 1;
  if (is_eff(h)) return (h->desc.stride_layer_idx >= 0 && i > h->desc.stride_layer_idx) ? 2 : 1;
  return 1;
}
inline int layer_lo(const ppasr_model_s* h, int i) {
  return (is_sq(h) ? h->desc.cnn_module_kernel : h->layer_ks[i]) - 1;
}
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

// keep rows [from, from+keep) of a [cap][256] cache at its start
ppasr_status shift_cache(float* buf, int from, int keep, float* tmp, hipStream_t st, int D = kD) {
  if (keep <= 0 || from <= 0) return PPASR_OK;
  const size_t bytes = (size_t)keep * D * sizeof(float);
  HIP_TRY(hipMemcpyAsync(tmp, buf + (size_t)from * D, bytes, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(buf, tmp, bytes, hipMemcpyDeviceToDevice, st));
  return PPASR_OK;
}


// the reference's shape arithmetic for one chunk of c frames on a session whose caches hold cache_t (full-rate layers) /
// cache_r (half-rate layers) frames, `offset` frames emitted so far and room for `cap` keys per layer; shared by the
// stream handles and the Squeezeformer / Efficient-Conformer session groups
ppasr_status plan_chunk_for(const ppasr_model_s* h, int cache_t, int cache_r, int offset, int cap, int c,
                            int required_cache_size, ChunkPlan* p) {
  p->c = c;
  p->c_r = ceil_div(c, 2);  // Conv1D(k=1, s=2) / stride-2 depthwise conv + ceil-mode AvgPool
  p->T2 = cache_t + c;
  const int pos_len_r = ceil_div(cache_t + c, 2);  // pos_emb[:, ::2]
  if (is_sq(h)) {
    // att_cache[i][:, :, ::2][:, :, :pos_len - xs_len] of a cache exported as repeat_interleave(...)[:max_att_len]
    const int avail = ceil_div(std::min(2 * cache_r, cache_t), 2);
    p->used_r = std::min(avail, pos_len_r - p->c_r);
  } else {
    p->used_r = cache_r;  // att_cache[i][:, :, ::2], no trim
  }
  p->T2_r = p->used_r + p->c_r;
  const bool has_half = is_sq(h) ? h->desc.reduce_idx >= 0 : (is_eff(h) && h->desc.stride_layer_idx >= 0);
  if (has_half && p->T2_r != pos_len_r)
    return fail(PPASR_EINVAL, "half-rate attention cache does not line up with the strided positional table "
                              "(the reference fails on matrix_ac + matrix_bd here): keep cache lengths even");
  if (required_cache_size < 0) p->ncs = 0;
  else if (required_cache_size == 0) p->ncs = p->T2;
  else p->ncs = std::max(p->T2 - required_cache_size, 0);
  // efficient_conformer/encoder.py:305: offset *= calculate_downsampling_factor(num_blocks + 1)
  const int off = is_eff(h) && h->desc.stride_layer_idx >= 0 ? 2 * offset : offset;
  p->pos0 = off - cache_t;
  if (p->pos0 < 0) return fail(PPASR_EINVAL, "offset smaller than the attention cache length");
  if (p->pos0 + p->T2 >= h->desc.max_len) return fail(PPASR_EINVAL, "offset + chunk exceeds the positional table (max_len)");
  if (p->T2 > cap) return fail(PPASR_EINVAL, "attention cache capacity exceeded");
  return PPASR_OK;
}
ppasr_status plan_chunk(const ppasr_stream_s* s, int c, int required_cache_size, ChunkPlan* p) {
  return plan_chunk_for(s->m, s->cache_t, s->cache_r, s->offset, s->cap, c, required_cache_size, p);
}

ppasr_status finish_chunk(ppasr_stream_s* s, const ChunkPlan& p, float* shift_tmp, hipStream_t st) {
  ppasr_model_s* h = s->m;
  const int keep = p.T2 - p.ncs;
  const int from_r = p.ncs / 2;
  const int keep_r = std::max(p.T2_r - from_r, 0);
  if (h->desc.num_blocks <= 64 && s->D % 4 == 0 && s->D <= 1024) {  // one launch for every layer's K and V cache
    unsigned long long half_mask = 0;
    for (int i = 0; i < h->desc.num_blocks; ++i)
      if (layer_factor(h, i) == 2) half_mask |= 1ull << i;
    if ((p.ncs > 0 && keep > 0) || (half_mask && from_r > 0 && keep_r > 0))
      launch_shift_caches(s->kc, s->vc, (long long)s->cap * s->D, s->D, h->desc.num_blocks, p.ncs, keep, from_r, keep_r, half_mask, st);
    s->cache_t = keep;
    s->cache_r = keep_r;
    return PPASR_OK;
  }
  for (int i = 0; i < h->desc.num_blocks; ++i) {
    float* bufs[2] = {s->kc + (size_t)i * s->cap * s->D, s->vc + (size_t)i * s->cap * s->D};
    const bool half = layer_factor(h, i) == 2;
    for (float* b : bufs) {
      ppasr_status r = half ? shift_cache(b, from_r, keep_r, shift_tmp, st, s->D) : shift_cache(b, p.ncs, keep, shift_tmp, st, s->D);
      if (r != PPASR_OK) return r;
    }
  }
  s->cache_t = keep;
  s->cache_r = keep_r;
  return PPASR_OK;
}

// ---- the rows a streaming round runs on ----
// n chunks of c frames each (c_r behind a time reduction / the stride layer), stacked: ONE chunk of a stream handle, or the
// chunks of the sessions a group round lists.  The layer walks below are written once against this view; what differs by
// caller -- where the caches live and who moves them on -- is behind its helpers.
struct StreamRows {
  int n, c, c_r;
  float *kc, *vc;       // K / V caches [session][L][cap][256]
  int cap;
  long long kv_sess;    // floats from one session's caches to the next's
  float* xh_hist;       // conv-module input histories [session][L][lo][256]
  int lo;
  long long hist_sess;
  // GLU(pointwise_conv1(history)) scratch.  hist_tab (device [L]): every layer's in one launch ahead of the walk, layer i's
  // slab [n * lo][256] at i * n * lo rows.  No table (the Conformer group): layer i gathers its sessions' histories to
  // [n][lo][256] at g_hist and GLUs them to the [n][lo][256] behind, inside the walk
  float* g_hist;
  const HistLayer* hist_tab;
  int cache_t, used_r, pos0;      // a stream handle: cached frames of the full-rate / half-rate layers, position of key 0
  const SessDesc *full, *half;    // a session group: the round's device descriptors of the full-rate / half-rate layers

  bool handle() const { return !full; }
  float* k_of(int i) const { return kc + (size_t)i * cap * kD; }
  float* v_of(int i) const { return vc + (size_t)i * cap * kD; }
  float* hist_of(int i) const { return xh_hist + (size_t)i * lo * kD; }
  const SessDesc* desc(bool half_rate) const { return half_rate ? half : full; }
  int cached(bool half_rate) const { return half_rate ? used_r : cache_t; }
  // Where the launch that makes layer i's qkv writes the K / V rows.  A handle: straight behind the cached frames of its
  // cache.  A group: nowhere (they stay in qkv), kv_append scatters them to the listed sessions
  float* k_dst(int i, bool half_rate) const { return handle() ? k_of(i) + (size_t)cached(half_rate) * kD : nullptr; }
  float* v_dst(int i, bool half_rate) const { return handle() ? v_of(i) + (size_t)cached(half_rate) * kD : nullptr; }
  void kv_append(const float* qkv, int i, bool half_rate, int Ti, hipStream_t st) const {
    if (handle()) launch_kv_append(qkv, k_dst(i, half_rate), v_dst(i, half_rate), Ti, st);
    else launch_kv_append_group(qkv, k_of(i), v_of(i), kv_sess, desc(half_rate), n, Ti, st);
  }
  // the cache half of a layer's attention (a: built for Ti query frames in tokens of grp frames, no cache).  A handle:
  // cache + chunk frames re-cut into tokens from the START of the cache (pad4group on the concatenated keys,
  // efficient_conformer/attention.py:160-175).  A group: the same per session, from its descriptor (k_attention_t)
  void attn_cache(AttnArgs& a, bool half_rate, int Ti, int grp) const {
    if (handle()) {
      a.kv_frames = cached(half_rate) + Ti;
      a.T2 = ceil_div(a.kv_frames, grp);
      a.pos0 = pos0;
    } else {
      a.sess = desc(half_rate);
      a.sess_stride = kv_sess;
    }
  }
  // pointwise_conv1 + GLU of the cached conv inputs: the histories are last chunk's state (hist_step of layer i runs after
  // layer i has consumed its slab)
  void glu_histories(int L, hipStream_t st) const {
    if (!hist_tab) return;
    if (handle()) launch_pw1_glu_layers(xh_hist, g_hist, hist_tab, L, lo, st);
    else launch_pw1_glu_layers_group(xh_hist, hist_sess, full, g_hist, hist_tab, L, n, lo, st);
  }
  void glu_layer_history(int i, const LayerW& W, hipStream_t st) const {
    if (hist_tab) return;
    launch_hist_gather(hist_of(i), hist_sess, full, g_hist, n, lo, st);
    launch_pw1_glu(g_hist, g_hist_of(i), W, n * lo, st);
  }
  float* g_hist_of(int i) const { return g_hist + (size_t)(hist_tab ? i : 1) * n * lo * kD; }  // (list position b at row b * lo_i)
  // layer i's histories move on by the chunk's Ti rows of xhat (moved: a handle's launch did it on the side -- HistMove,
  // launch_pw1_glu_cols_16)
  void hist_step(int i, bool half_rate, const float* xhat, int Ti, int lo_i, bool moved, hipStream_t st) const {
    if (!handle()) launch_hist_update_group(hist_of(i), hist_sess, desc(half_rate), xhat, n, Ti, lo_i, st);
    else if (!moved) launch_hist_update(hist_of(i), xhat, Ti, lo_i, st);
  }
};

StreamRows handle_rows(const ppasr_stream_s* s, const ChunkPlan& p) {
  return StreamRows{1, p.c, p.c_r, s->kc, s->vc, s->cap, 0, s->xh_hist, s->lo, 0, s->g_hist, s->hist_tab, s->cache_t, p.used_r,
                    p.pos0, nullptr, nullptr};
}

// the buffers of a round in its workspace: the batched layout for B = n and, behind it, the conv-module input rows
// xhat [rows][256] of this chunk; `behind` = the first float past them (64-float aligned), the caller's own scratch
struct StreamWs {
  float *y1, *y2, *xa, *xb, *xc, *qkv, *ctx, *g, *xs, *rmax, *rsum, *fa, *fp, *xhat, *behind;
};
StreamWs carve_ws(float* ws, const WsLayout& wl, int rows) {
  float* xhat = ws + wl.total;
  return StreamWs{ws + wl.y1, ws + wl.y2, ws + wl.xa, ws + wl.xb, ws + wl.xc, ws + wl.qkv, ws + wl.ctx, ws + wl.g, ws + wl.xs,
                  ws + wl.rmax, ws + wl.rsum, ws + wl.fa, ws + wl.fp, xhat, xhat + (((size_t)rows * kD + 63) & ~(size_t)63)};
}

// conv front end + input projection of the n chunks of T frames -> w.xa [n * c][256].
// The caller is a stream handle: ONE row block, so
//   - conv2 splits its taps (K) over workgroups, scratch at conv2_part (behind the handle's shift scratch);
//   - up to 32 rows the input projection runs a workgroup per 256-wide K chunk -- F2 of them -- instead of 8 workgroups of
//     2 - 3 chunks;
//   - the conv2d6 / conv2d8 front ends exist (Conformer handles only; groups are built for conv2d).
void stream_front(const ppasr_model_s* h, const StreamRows& v, const StreamWs& w, const float* feats, int T, float* conv2_part,
                  hipStream_t st) {
  const auto fd = h->front_dims(T);
  const int F1 = h->F1, F2 = h->F2, M = v.n * v.c, S = ffn_split_for(h, M);
  launch_conv1(feats, h->front, w.y1, v.n, T, h->desc.input_dim, fd.T1, F1, st);
  if (h->desc.input_layer == 8) {  // Conv2dSubsampling8: three 3x3 / 2 convs, the third one over conv1's output buffer
    launch_conv_stage(w.y1, h->front.conv2_w, h->front.conv2_b, w.y2, 1, fd.T1, F1, fd.T2, F2, 3, 2, st);
    launch_conv_stage(w.y2, h->front.conv3_w, h->front.conv3_b, w.y1, 1, fd.T2, F2, v.c, h->F3, 3, 2, st);
    launch_embed(w.y1, h->front, w.xa, v.c, h->F3 * kD, sqrtf((float)kD), false, st, PadSkip{}, S, w.y2);
    return;
  }
  // (3x3 / 2, or conv2d6's 5x5 / 3: FrontW::conv2_k / _s)
  launch_conv2(w.y1, h->front, w.y2, v.n, fd.T1, F1, v.c, F2, st, PadSkip{}, nullptr, nullptr, conv2_part,
               conv2_part ? conv_stage_part_floats(v.c * F2) : 0);
  launch_embed(w.y2, h->front, w.xa, M, F2 * kD, sqrtf((float)kD), /*scale_before_bias=*/is_sq(h), st, PadSkip{},
               (v.handle() && v.c <= 32 && S > 1) ? F2 : S, w.y1);
}

// CTC head over the n * frames encoder rows x.  The caller is a stream handle: up to 32 rows are one row block, which takes
// as many column slices as give every wave ONE 32-column vocabulary tile -- 17 at V = 4233 -- not 8
void stream_head(const ppasr_model_s* h, const StreamRows& v, const StreamWs& w, const float* x, int frames, float* probs,
                 int32_t* frame_argmax, float* frame_maxprob, hipStream_t st) {
  const int M = v.n * frames, S = ffn_split_for(h, M);
  int32_t* fa = frame_argmax ? frame_argmax : reinterpret_cast<int32_t*>(w.fa);
  float* fp = frame_maxprob ? frame_maxprob : w.fp;
  const int slices = (v.handle() && frames <= 32 && S > 1) ? std::min((h->head.n_tiles + 7) / 8, 32) : S;
  launch_ctc_head(x, h->head, probs, fa, fp, w.rmax, w.rsum, M, st, PadSkip{}, slices, w.y1);
  if (probs) launch_softmax_from_stats(probs, w.rmax, w.rsum, M, h->head.V, st);
}

// ---- Conformer / Efficient-Conformer: the layers of a streaming round over the rows of v, w.xa -> w.xa; returns the
// frames each chunk leaves with (c_r behind a stride layer).  Few rows are an under-filled grid: the split route
// (ppasr_set_ffn_split) runs the feed-forward modules over S workgroups per row block, partial sums in w.y1 (the conv1
// buffer, free after the front end); S == 1 runs the fused kernels.
// ppasr_set_gemm_mode(h, PPASR_GEMM_F16X3) puts the split route's GEMM units on the fp16 x3 route (Lk = the layer's h3 view: the
// same LayerNorm / bias pointers, re-packed weights; its ptab are operand planes, so the attention keeps L's); the fused
// kernels stay fp32.  Out-of-range activations are saturated and counted (ppasr_gemm_guard_stats); a chunk is not re-run.
int conformer_stream_layers(const ppasr_model_s* h, const StreamRows& v, const StreamWs& w, hipStream_t st) {
  const int n_chunks = h->desc.linear_units / 256, H = h->desc.attention_heads, n = v.n;
  const bool h3_mode = h->h3_layers();
  float *xa = w.xa, *xb = w.xb, *xc = w.xc, *qkv = w.qkv, *ctx = w.ctx, *g = w.g, *xhat = w.xhat, *partial = w.y1;
  int Ti = v.c, mul = 4, pstride = 1;
  bool half = false;
  v.glu_histories(h->desc.num_blocks, st);
  // Consumer-side joins (conformer_kernels.h JoinIn; a stream handle's chunk on the fp32 route, <= 16 rows): a feed-forward
  // module leaves 2 S partial tiles and a PENDING join that the next launch computes in its prologue.  Macaron slices go to
  // partial, final slices to the tiles behind them (the pending final join of block i is read while block i + 1's macaron
  // slices are written).  Single-session kernels: a group never takes them, whatever its rows.
  JoinIn pending;
  auto flush = [&](int M) {  // a launch that cannot take a pending join in: the join alone
    if (pending.partial) launch_join16(pending, M, st);
    pending = JoinIn{};
  };
  for (int i = 0; i < h->desc.num_blocks; ++i) {
    const LayerW& L = h->layers[i];
    const int grp = h->layer_group[i], KS = h->layer_ks[i], lo_i = layer_lo(h, i), M = n * Ti;
    const int S = ffn_split_for(h, M);
    const bool h3 = S > 1 && h3_mode;
    const LayerW& Lk = h3 ? h->layers_h3[i] : L;
    const bool fused_joins = v.handle() && !h3 && ffn_half16_route(Ti, S, n_chunks);
    if (fused_joins) {
      launch_ffn_half16(xa, pending, L.ln_mac_g, L.ln_mac_b, L.ffm_w1, L.ffm_b1, L.ffm_w2, partial, Ti, n_chunks, st);
      const JoinIn mac{partial, 2 * S, L.ffm_b2, 0.5f, xa, nullptr, nullptr, xb};
      launch_join_ln_qkv16(mac, qkv, L, Ti, st, v.k_dst(i, half), v.v_dst(i, half));
      pending = JoinIn{};
    } else if (S > 1) {
      flush(M);
      launch_ffn_split(xa, L.ln_mac_g, L.ln_mac_b, Lk.ffm_w1, L.ffm_b1, Lk.ffm_w2, L.ffm_b2, 0.5f, nullptr, nullptr, partial, xb,
                       M, n_chunks, S, st, PadSkip{}, false, h3);
      launch_ln_qkv(xb, qkv, Lk, M, st, PadSkip{}, v.k_dst(i, half), v.v_dst(i, half), h3);
    } else {
      flush(M);
      launch_ffn_qkv(xa, xb, qkv, L, M, n_chunks, st);
    }
    if (S == 1 || !v.handle()) v.kv_append(qkv, i, half, Ti, st);  // (a handle's split-route launches wrote them in place)
    const int Tq = ceil_div(Ti, grp);
    AttnArgs a{qkv, 768, v.k_of(i), kD, v.v_of(i), kD, Tq, Tq, 0, nullptr, ctx, L.pos_u, L.pos_v, L.ptab, pstride, mul * grp,
               Ti, Ti, grp};
    v.attn_cache(a, half, Ti, grp);
    launch_attention(a, n, H, st);
    v.glu_layer_history(i, L, st);
    float* gh = v.g_hist_of(i);
    HistMove hm{v.hist_of(i), lo_i, false};  // (a handle's out_glu launch may move the history on the side)
    launch_out_glu(ctx, xb, xc, g, xhat, Lk, nullptr, M, Ti, mul, st, PadSkip{}, S > 1 ? xhat : nullptr, h3,
                   v.handle() ? &hm : nullptr);
    if (is_eff(h) && i == h->desc.stride_layer_idx) {
      const int Ts = ceil_div(Ti, 2), Ms = n * Ts, Ss = ffn_split_for(h, Ms);
      // the fp16 x3 view of the stride layer: a handle keeps the layer's (from S), a group decides by the strided rows (Ss)
      const bool h3s = v.handle() ? h3 : (Ss > 1 && h3_mode);
      const LayerW& Ls = h3s ? h->layers_h3[i] : L;
      // Ss > 1: the conv half of the stride layer alone (x3 -> ctx), its feed-forward module over the slices
      launch_conv_ffn_stride(g, gh, xc, xa, Ls, nullptr, n, Ti, Ts, n_chunks, KS, mul * 2, st, PadSkip{}, true, h3s,
                             Ss > 1 ? ctx : nullptr);
      if (Ss > 1)
        launch_ffn_split(ctx, L.ln_ff_g, L.ln_ff_b, Ls.ff_w1, L.ff_b1, Ls.ff_w2, L.ff_b2, 0.5f, L.ln_fin_g, L.ln_fin_b, partial, xa,
                         Ms, n_chunks, Ss, st, PadSkip{}, false, h3s);
      v.hist_step(i, half, xhat, Ti, lo_i, hm.done, st);
      Ti = Ts;  // masks[:, :, ::2], pos_emb[:, ::2]  (efficient_conformer/encoder.py:252-257)
      mul *= 2;
      pstride *= 2;
      half = true;
      continue;
    }
    if (fused_joins) {
      launch_conv_pre(g, gh, xc, ctx, L, nullptr, Ti, Ti, KS, mul, st, true, PadSkip{}, false);
      float* part_fin = partial + (size_t)2 * S * Ti * kD;  // (behind the macaron module's 2 S tiles of Ti rows)
      launch_ffn_half16(ctx, JoinIn{}, L.ln_ff_g, L.ln_ff_b, L.ff_w1, L.ff_b1, L.ff_w2, part_fin, Ti, n_chunks, st);
      pending = JoinIn{part_fin, 2 * S, L.ff_b2, 0.5f, ctx, L.ln_fin_g, L.ln_fin_b, xa};
    } else if (S > 1) {
      launch_conv_pre(g, gh, xc, ctx, Lk, nullptr, M, Ti, KS, mul, st, true, PadSkip{}, h3);
      launch_ffn_split(ctx, L.ln_ff_g, L.ln_ff_b, Lk.ff_w1, L.ff_b1, Lk.ff_w2, L.ff_b2, 0.5f, L.ln_fin_g, L.ln_fin_b, partial, xa,
                       M, n_chunks, S, st, PadSkip{}, false, h3);
    } else {
      launch_conv_ffn(g, gh, xc, xa, L, nullptr, M, Ti, n_chunks, KS, mul, nullptr, nullptr, nullptr, st);
    }
    v.hist_step(i, half, xhat, Ti, lo_i, hm.done, st);
  }
  flush(n * Ti);  // (the last block's final join)
  return Ti;
}

// ---- Squeezeformer: the layers of a streaming round over the rows of v (n * c full-rate rows, n * c_r half-rate rows
// between reduce_idx and recover_idx), w.xa -> *x_final.  Split route and fp16 x3 mode as in conformer_stream_layers: the
// mode covers the feed-forward slices of the split route, a layer whose rows leave it (ffn_split_for = 1: more than 4 096
// stacked rows at the default setting, or ppasr_set_ffn_split(0)) runs the fused fp32 kernels in either mode.
ppasr_status sq_stream_layers(const ppasr_model_s* h, const StreamRows& v, const StreamWs& w, float** x_final, hipStream_t st) {
  const int L = h->desc.num_blocks, H = h->desc.attention_heads, n = v.n;
  const int n_chunks = h->desc.linear_units / 256, KS = h->desc.cnn_module_kernel;
  float *xc = w.xc, *qkv = w.qkv, *ctx = w.ctx, *g = w.g, *xhat = w.xhat, *partial = w.y1;
  launch_ln_rows(w.xa, h->preln_g, h->preln_b, n * v.c, st);
  v.glu_histories(L, st);
  float* x = w.xa;
  float* other = w.xb;
  bool reduced = false, have_qkv = false;
  // A stream handle on the split route (fp32) runs the layer's single-unit launches on the Conformer's 16-row kernels through
  // weight views -- Q / K / V thirds (no LayerNorm: ln_mha_g = nullptr; K and V straight into the cache rows), out-projection
  // + LayerNorm, pointwise_conv1 + GLU over two column halves (which also moves the SCALED conv-input history on).
  // Single-session launches: a group runs launch_sq_qkv / _oproj / _pw1glu, whatever its rows
  bool kv_in_cache = false;  // this layer's K / V rows were written to its cache by the launch that made its qkv
  auto qkv_view = [](const SqLayerW& W) {
    LayerW view{};
    view.wqkv = W.wqkv;
    view.bqkv = W.bqkv;
    return view;
  };
  for (int i = 0; i < L; ++i) {
    const SqLayerW& W = h->sq_layers[i];
    if (i == h->desc.reduce_idx) {
      HIP_TRY(hipMemcpyAsync(w.xs, x, (size_t)n * v.c * kD * sizeof(float), hipMemcpyDeviceToDevice, st));
      launch_sq_reduce(x, other, qkv, h->sq_reduce, W.wqkv, W.bqkv, nullptr, n, v.c, v.c_r, st);
      std::swap(x, other);
      reduced = true;
      have_qkv = true;
    }
    if (i == h->desc.recover_idx && reduced) {
      launch_sq_recover(x, w.xs, other, qkv, h->sq_wrec, h->sq_brec, W.wqkv, W.bqkv, n, v.c, v.c_r, st);
      std::swap(x, other);
      reduced = false;
      have_qkv = true;
    }
    const int Ti = reduced ? v.c_r : v.c, M = n * Ti;
    const int mul = reduced ? 8 : 4;
    const int S = ffn_split_for(h, M);
    const bool h3s = S > 1 && h->h3_sq_layers();  // (the FFN slices in the mode)
    const bool r16 = v.handle() && S > 1 && !h3s && Ti <= kSplitRows16Max;
    if (!have_qkv) {
      if (r16) {
        launch_ln_qkv(x, qkv, qkv_view(W), Ti, st, PadSkip{}, v.k_dst(i, reduced), v.v_dst(i, reduced), false);
        kv_in_cache = true;
      } else {
        launch_sq_qkv(x, qkv, W.wqkv, W.bqkv, M, st);
      }
    }
    if (!kv_in_cache) v.kv_append(qkv, i, reduced, Ti, st);
    kv_in_cache = false;
    AttnArgs a{qkv, 768, v.k_of(i), kD, v.v_of(i), kD, Ti, Ti, 0, nullptr, ctx, W.pos_u, W.pos_v, W.ptab, reduced ? 2 : 1, mul,
               Ti, Ti, 1};
    v.attn_cache(a, reduced, Ti, 1);
    launch_attention(a, n, H, st);
    float* gh = v.g_hist_of(i);
    const bool fuse_next = (i + 1 < L) && (i + 1 != h->desc.reduce_idx) && !(i + 1 == h->desc.recover_idx && reduced);
    const SqLayerW* Wn = fuse_next ? &h->sq_layers[i + 1] : nullptr;
    bool hist_moved = false;
    if (S > 1) {
      const SqLayerW& Ws = h3s ? h->sq_layers_h3[i] : W;
      if (r16) {  // x1 = LN1(x + ctx Wo + bo) (the plain sum goes to g, dead until pointwise_conv1 writes it)
        LayerW vo{};
        vo.wo = W.wo; vo.bo = W.bo; vo.ln_conv_g = W.ln1_g; vo.ln_conv_b = W.ln1_b;
        launch_oproj_ln_16(ctx, x, g, other, vo, Ti, st);
      } else {
        launch_sq_oproj(ctx, x, other, W, M, st);
      }
      launch_ffn_split(other, nullptr, nullptr, Ws.ff1_w1, W.ff1_b1, Ws.ff1_w2, W.ff1_b2, 1.0f, W.ln2_g, W.ln2_b, partial, xc, M,
                       n_chunks, S, st, PadSkip{}, false, h3s);
      if (r16 && KS - 1 <= 30) {
        LayerW vp{};
        vp.pw1 = W.pw1; vp.pw1_b = W.pw1_b;
        launch_pw1_glu_cols_16(xc, g, vp, Ti, st, v.hist_of(i), KS - 1, W.cm_scale, W.cm_bias);
        hist_moved = true;
      } else {
        launch_sq_pw1glu(xc, g, xhat, W, nullptr, M, Ti, mul, st);
      }
      launch_conv_pre(g, gh, xc, ctx, sq_conv_view(W), nullptr, M, Ti, KS, mul, st);
      launch_ffn_split(ctx, W.ln3_g, W.ln3_b, Ws.ff2_w1, W.ff2_b1, Ws.ff2_w2, W.ff2_b2, 1.0f, W.ln4_g, W.ln4_b, partial, other, M,
                       n_chunks, S, st, PadSkip{}, /*residual_is_normed=*/true, h3s);
      if (Wn && r16) {  // (fuse_next: layer i + 1 runs at this layer's rate -- same rows, same cache length)
        launch_ln_qkv(other, qkv, qkv_view(*Wn), Ti, st, PadSkip{}, v.k_dst(i + 1, reduced), v.v_dst(i + 1, reduced), false);
        kv_in_cache = true;
      } else if (Wn) {
        launch_sq_qkv(other, qkv, Wn->wqkv, Wn->bqkv, M, st);
      }
    } else {
      launch_sq_mid(ctx, x, xc, g, xhat, W, nullptr, M, Ti, mul, n_chunks, st);
      launch_sq_tail(g, gh, xc, other, qkv, W, Wn ? Wn->wqkv : nullptr, Wn ? Wn->bqkv : nullptr, nullptr, M, Ti, mul, n_chunks,
                     KS, st);
    }
    v.hist_step(i, reduced, xhat, Ti, KS - 1, hist_moved, st);
    std::swap(x, other);
    have_qkv = fuse_next;
  }
  *x_final = x;
  return PPASR_OK;
}

// Where a round keeps its encoder output (ppasr_encode_chunk_mem / ppasr_encode_chunk_group_mem): list position k's rows go
// behind the last frame arena session sessions[k] holds, frames[k] of them (null: all).  No arena: nowhere, no launch.
struct MemOut {
  ppasr_prob_arena_s* arena;
  const int* sessions;
  const int* frames;
};

// what a round with a memory arena needs, checked before any device work: a model whose head rows become the encoder
// output through after_norm on the fused route (the set ppasr_set_memory_out serves, without the general route; the
// Squeezeformer's and the Efficient-Conformer's streams are not built: DESIGN section 8), an arena of 256-wide rows with
// a slot for every session, and the pages of this round (arena_plan_append: PPASR_ENOSPACE, nothing changed)
ppasr_status mem_check(const ppasr_model_s* h, const MemOut& mem, int n, int n_sessions, int c, const char* who) {
  const std::string w(who);
  if (h->desc.model_type != PPASR_MODEL_CONFORMER || h->generic)
    return fail(PPASR_EUNSUPPORTED, w + ": a memory arena is built for Conformer streams on the fused 256-wide route "
                                        "(not DeepSpeech2, the general route, the Squeezeformer or the Efficient-Conformer)");
  if (mem.arena->V != kD) return fail(PPASR_EINVAL, w + ": the memory arena must hold rows of 256 floats");
  if (mem.arena->n_sessions < n_sessions) return fail(PPASR_EINVAL, w + ": the memory arena has fewer sessions than the caller");
  return arena_plan_append(mem.arena, mem.sessions, n, c, mem.frames, who, nullptr);
}

// the round's encoder output: after_norm of the rows x the head reads, [n][frames][256], into the arena's pages; one launch
ppasr_status keep_memory(const ppasr_model_s* h, const MemOut& mem, int n, const float* x, int frames, hipStream_t st) {
  ArenaAppendTab tab{};
  ppasr_status r = arena_stage_append(mem.arena, mem.sessions, n, frames, mem.frames, &tab, st);
  if (r != PPASR_OK) return r;
  launch_memory_append(x, h->head.ln_g, h->head.ln_b, n, frames, kD, mem.arena->P, tab.first, tab.count, tab.page_off, tab.pages,
                       mem.arena->slab, st);
  HIP_TRY(mem.arena->ring.release(tab.en, st));
  return PPASR_OK;
}

// One streaming round on the fused 256-wide route -- a stream handle's chunk or a session group's listed chunks: front
// end, the family's layers, head and, with a memory arena, the encoder output.  *frames = the encoder frames each chunk
// leaves with
ppasr_status stream_round(const ppasr_model_s* h, const StreamRows& v, const StreamWs& w, const float* feats, int T,
                          float* conv2_part, float* probs, int32_t* frame_argmax, float* frame_maxprob, hipStream_t st,
                          int* frames, const MemOut& mem) {
  stream_front(h, v, w, feats, T, conv2_part, st);
  float* x_final = w.xa;
  *frames = v.c;
  if (is_sq(h)) {
    ppasr_status r = sq_stream_layers(h, v, w, &x_final, st);
    if (r != PPASR_OK) return r;
  } else {
    *frames = conformer_stream_layers(h, v, w, st);
  }
  stream_head(h, v, w, x_final, *frames, probs, frame_argmax, frame_maxprob, st);
  return mem.arena ? keep_memory(h, mem, v.n, x_final, *frames, st) : PPASR_OK;
}

// every layer's pointwise_conv1 and history rows (kernel_i - 1) for k_pw1_glu_layers -> tab_dev [L] (the general route
// recomputes the history's GLU inside the layer: null entries)
hipError_t upload_hist_table(const ppasr_model_s* h, HistLayer* tab_dev) {
  const int L = h->desc.num_blocks;
  std::vector<HistLayer> tab(L, HistLayer{nullptr, nullptr, 0, 0});
  for (int i = 0; i < L && !h->generic; ++i)
    tab[i] = is_sq(h) ? HistLayer{h->sq_layers[i].pw1_raw, h->sq_layers[i].pw1_b_raw, layer_lo(h, i), 0}
                      : HistLayer{h->layers[i].pw1, h->layers[i].pw1_b, layer_lo(h, i), 0};
  return hipMemcpy(tab_dev, tab.data(), L * sizeof(HistLayer), hipMemcpyHostToDevice);
}

// which of the chunk-round paths a session group takes (the family of the handle it was built for)
// (kGeneral: a Conformer handle on the general layer route, capi_generic.hip)
enum class GroupFamily { kConformer, kSqueezeformer, kEfficientConformer, kDeepSpeech2, kGeneral };
// families with full- and half-rate layers and per-layer conv histories
inline bool is_layered(GroupFamily f) { return f == GroupFamily::kSqueezeformer || f == GroupFamily::kEfficientConformer; }

}  // namespace

extern "C" {

ppasr_status ppasr_stream_create(ppasr_handle h, ppasr_stream* out) {
  if (!h || !out) return fail(PPASR_EINVAL, "null argument");
  if (h->desc.model_type == PPASR_MODEL_DEEPSPEECH2)
    return fail(PPASR_EUNSUPPORTED, "deepspeech2 streams carry their state in the h/c boxes of ppasr_ds2_encode");
  if (!h->desc.causal)
    return fail(PPASR_EUNSUPPORTED, "forward_chunk needs the causal conv module (a streaming=True model)");
  if (h->generic && h->desc.input_layer == 1)
    return fail(PPASR_EUNSUPPORTED, "stream handles are built for the conv front ends (input_layer=linear: batched encode)");
  if (__builtin_popcount(eff_stride_mask(h->desc)) > 1)
    return fail(PPASR_EUNSUPPORTED, "stream handles are built for one stride layer (several: batched encode)");
  if (h->desc.input_layer != 0 && h->desc.model_type != PPASR_MODEL_CONFORMER)
    return fail(PPASR_EUNSUPPORTED, "stream handles with the conv2d6 / conv2d8 front ends are built for model_type=conformer");
  auto* s = new ppasr_stream_s();
  s->m = h;
  s->D = h->desc.output_size;
  s->cap = h->desc.max_len;
  s->lo = (h->generic && !h->gen.use_cnn) ? 0 : h->desc.cnn_module_kernel - 1;
  const size_t L = h->desc.num_blocks;
  const size_t D = s->D, lo_alloc = s->lo > 0 ? s->lo : 1;
  hipError_t e1 = hipMalloc(reinterpret_cast<void**>(&s->kc), L * s->cap * D * sizeof(float));
  hipError_t e2 = hipMalloc(reinterpret_cast<void**>(&s->vc), L * s->cap * D * sizeof(float));
  hipError_t e3 = hipMalloc(reinterpret_cast<void**>(&s->xh_hist), L * lo_alloc * D * sizeof(float));
  hipError_t e4 = hipMalloc(reinterpret_cast<void**>(&s->g_hist), L * lo_alloc * D * sizeof(float));
  s->hist_tab = nullptr;
  if (e4 == hipSuccess) e4 = hipMalloc(reinterpret_cast<void**>(&s->hist_tab), L * sizeof(HistLayer));
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess) {
    (void)hipFree(s->kc); (void)hipFree(s->vc); (void)hipFree(s->xh_hist); (void)hipFree(s->g_hist);
    (void)hipFree(s->hist_tab);
    delete s;
    return fail(PPASR_EHIP, "hipMalloc failed for the stream caches");
  }
  s->cache_t = 0;
  s->cache_r = 0;
  s->offset = 0;
  hipError_t e5 = hipMemset(s->xh_hist, 0, L * lo_alloc * D * sizeof(float));
  if (e5 == hipSuccess) e5 = upload_hist_table(h, s->hist_tab);
  // (hipMemset on device memory and a pageable upload go to the null stream and may return before they have landed; the
  // first chunk runs on the caller's stream, which need not wait for the null stream: create-time only)
  if (e5 == hipSuccess) e5 = hipStreamSynchronize(nullptr);
  if (e5 != hipSuccess) {
    (void)ppasr_stream_destroy(s);
    return fail(PPASR_EHIP, "initialising the stream caches failed");
  }
  *out = s;
  return PPASR_OK;
}

ppasr_status ppasr_stream_destroy(ppasr_stream s) {
  if (!s) return PPASR_OK;
  (void)hipFree(s->kc); (void)hipFree(s->vc); (void)hipFree(s->xh_hist); (void)hipFree(s->g_hist);
  (void)hipFree(s->hist_tab);
  delete s;
  return PPASR_OK;
}

// InferencePredictor.reset_stream (inference_predictor.py:215-220): empty caches, offset 0
ppasr_status ppasr_stream_reset(ppasr_stream s, void* stream) {
  if (!s) return fail(PPASR_EINVAL, "null stream");
  s->cache_t = 0;
  s->cache_r = 0;
  s->offset = 0;
  HIP_TRY(hipMemsetAsync(s->xh_hist, 0, (size_t)s->m->desc.num_blocks * s->lo * s->D * sizeof(float),
                         static_cast<hipStream_t>(stream)));
  return PPASR_OK;
}

int ppasr_stream_offset(ppasr_stream s) { return s ? s->offset : -1; }
int ppasr_stream_cache_frames(ppasr_stream s) { return s ? s->cache_t : -1; }

size_t ppasr_chunk_workspace_bytes(ppasr_handle h, int T) {
  if (!h || T < h->min_frames()) return 0;
  const size_t Tp = h->front_dims(T).Tp;
  if (h->generic) return (generic_ws_floats(h, 1, T) + (size_t)h->desc.max_len * h->desc.output_size) * sizeof(float);
  // the full-utterance layout for B=1, plus the conv-module input rows and a cache-shift scratch
  // (+ the K-split scratch of the chunk's conv2 launch, reserved for up to its row limit even past it: the size never
  // decreases with T, so one workspace sized for the longest chunk serves every shorter one)
  return (ws_layout(h, 1, T).total + Tp * kD + 64 + (size_t)h->desc.max_len * kD + conv_stage_part_reserve((int)Tp * h->F2)) *
         sizeof(float);
}

ppasr_status ppasr_encode_chunk(ppasr_stream s, const float* feats, int T, int required_cache_size, float* probs,
                                int32_t* frame_argmax, float* frame_maxprob, int* c_out_host, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return ppasr_encode_chunk_mem(s, feats, T, required_cache_size, probs, frame_argmax, frame_maxprob, c_out_host, workspace,
                                workspace_bytes, nullptr, 0, -1, stream);
}

ppasr_status ppasr_encode_chunk_mem(ppasr_stream s, const float* feats, int T, int required_cache_size, float* probs,
                                    int32_t* frame_argmax, float* frame_maxprob, int* c_out_host, void* workspace,
                                    size_t workspace_bytes, ppasr_prob_arena mem_arena, int mem_session, int mem_frames,
                                    void* stream) {
  if (!s || !feats || !workspace) return fail(PPASR_EINVAL, "null argument");
  ppasr_model_s* h = s->m;
  if (T < h->min_frames())
    return fail(PPASR_EINVAL, "chunk shorter than the conv front-end's receptive field (7 frames; conv2d6: 11, conv2d8: 15)");
  const int c = h->front_dims(T).Tp;
  if (workspace_bytes < ppasr_chunk_workspace_bytes(h, T)) return fail(PPASR_ENOSPACE, "workspace too small");
  ChunkPlan p{};
  ppasr_status r = plan_chunk(s, c, required_cache_size, &p);
  if (r != PPASR_OK) return r;
  const MemOut mem{mem_arena, &mem_session, mem_frames < 0 ? nullptr : &mem_frames};
  if (mem_arena) {
    r = mem_check(h, mem, 1, 1, c, "encode_chunk_mem");
    if (r != PPASR_OK) return r;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  const WsLayout wl = ws_layout(h, 1, T);
  float* ws = static_cast<float*>(workspace);
  if (h->generic) {  // the general layer route (capi_generic.hip): same cache bookkeeping, its own layer pieces
    int gframes = c;
    r = is_sq(h) ? generic_sq_chunk(s, p, feats, T, probs, frame_argmax, frame_maxprob, ws, st)
                 : generic_chunk(s, p, feats, T, probs, frame_argmax, frame_maxprob, ws, st, &gframes);
    if (r != PPASR_OK) return r;
    r = finish_chunk(s, p, ws + wl.total, st);
    if (r != PPASR_OK) return r;
    s->offset += gframes;
    if (c_out_host) *c_out_host = gframes;
    return PPASR_OK;
  }
  const StreamWs w = carve_ws(ws, wl, c);
  float* shift_tmp = w.behind;
  int frames = c;
  r = stream_round(h, handle_rows(s, p), w, feats, T, shift_tmp + (size_t)h->desc.max_len * kD, probs, frame_argmax,
                   frame_maxprob, st, &frames, mem);
  if (r != PPASR_OK) return r;
  r = finish_chunk(s, p, shift_tmp, st);
  if (r != PPASR_OK) return r;
  s->offset += frames;
  if (c_out_host) *c_out_host = frames;
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

// Reference-layout views of the caches (what get_encoder_out_chunk returns, conformer/model.py:164-184):
// att_cache [L][h][t][2*dk] (t = ppasr_stream_cache_frames), cnn_cache [L][1][256][lo].
ppasr_status ppasr_stream_export_cache(ppasr_stream s, float* att_cache, float* cnn_cache, void* stream) {
  if (!s) return fail(PPASR_EINVAL, "null stream");
  ppasr_model_s* h = s->m;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int L = h->desc.num_blocks, t = s->cache_t;
  for (int i = 0; i < L; ++i) {
    const int div = layer_factor(h, i);
    if (att_cache && t > 0) {
      // repeat_interleave(cache, 2)[:max_att_len] must cover t frames, or the reference's concat over layers fails
      if (div == 2 && (2 * s->cache_r < t || (is_eff(h) && 2 * s->cache_r != t)))
        return fail(PPASR_EINVAL, "half-rate cache does not match the first layer's cache length (odd cache length)");
      launch_cache_export(s->kc + (size_t)i * s->cap * s->D, s->vc + (size_t)i * s->cap * s->D,
                          att_cache + (size_t)i * (s->D / 64) * t * 128, t, div, st, s->D);
    }
    if (cnn_cache && s->lo > 0)
      launch_cnn_transpose(s->xh_hist + (size_t)i * s->lo * s->D, cnn_cache + (size_t)i * s->D * s->lo, layer_lo(h, i), s->lo, 1, st, s->D);
  }
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

ppasr_status ppasr_stream_import_cache(ppasr_stream s, const float* att_cache, int cache_t, const float* cnn_cache,
                                       int offset, void* stream) {
  if (!s) return fail(PPASR_EINVAL, "null stream");
  if (cache_t < 0 || cache_t > s->cap || offset < 0) return fail(PPASR_EINVAL, "bad cache_t / offset");
  if (cache_t > 0 && !att_cache) return fail(PPASR_EINVAL, "att_cache missing");
  ppasr_model_s* h = s->m;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int L = h->desc.num_blocks;
  for (int i = 0; i < L; ++i) {
    if (cache_t > 0)
      launch_cache_import(att_cache + (size_t)i * (s->D / 64) * cache_t * 128, s->kc + (size_t)i * s->cap * s->D,
                          s->vc + (size_t)i * s->cap * s->D, cache_t, layer_factor(h, i), st, s->D);
    if (cnn_cache && s->lo > 0)
      launch_cnn_transpose(cnn_cache + (size_t)i * s->D * s->lo, s->xh_hist + (size_t)i * s->lo * s->D, layer_lo(h, i), s->lo, 0, st, s->D);
  }
  if (!cnn_cache && s->lo > 0)
    HIP_TRY(hipMemsetAsync(s->xh_hist, 0, (size_t)L * s->lo * s->D * sizeof(float), st));
  s->cache_t = cache_t;
  s->cache_r = ceil_div(cache_t, 2);  // att_cache[i][:, :, ::2]
  s->offset = offset;
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

// =====================================================================================
// Multi-session streaming: a session group holds the streaming state of n_sessions sessions of one model in one
// allocation and advances any listed subset of them with ONE set of launches per chunk round (the rows of all listed
// sessions are stacked: n x c frames -> ceil(n*c/32) row blocks per kernel instead of one).  No reference counterpart:
// PPASR streams one session per call (predict.py:232-337, forward_chunk asserts B = 1); each session here follows exactly
// the single-session arithmetic (required_cache_size < 0: the full history is kept, what PPASRPredictor passes,
// predict.py:306-307).  Each family has its own create call; the launch body of a round:
//   Conformer            ppasr_stream_group_create      fused_group_body: the view of the listed sessions' rows
//   Squeezeformer        ppasr_sq_stream_group_create   (group_rows), then the round a stream handle's chunk runs
//   Efficient-Conformer  ppasr_eff_stream_group_create  (stream_round: front, conformer_ / sq_stream_layers, head)
//   general route        ppasr_gen_stream_group_create  gen_group_body: the same caches at the model's width D;
//                                                       gen_front + gen_layers (capi_generic.hip generic_group_chunk)
//   DeepSpeech2          ppasr_ds2_stream_group_create  ds2_group_body: each session's LSTM / GRU state [L][H] (h, and
//                        c for the LSTM) instead of caches; the wavefront route of ppasr_ds2_encode over the n stacked
//                        windows, states gathered from and scattered back to the slots (capi_ds2.hip ds2_group_round)
// One round, ppasr_encode_chunk_group, is the same for every family: check the arguments and the session list, plan
// every listed session's chunk (plan_chunk_for; DeepSpeech2 carries no cache) -- a refused call leaves every session as it
// was; take the next staging-ring entry and stage the descriptors in it; run the family's body; commit cache_t = T2,
// cache_r = T2_r, offset += frames (finish_chunk with required_cache_size < 0: nothing is dropped) and release the entry
// behind the launches.  A body that fails commits nothing.  Descriptors: {sess, cache_t, pos0, offset} per listed session
// (pos0 = 0 on the general route without relative positions: its one-row zero table); Squeezeformer and
// Efficient-Conformer append their half-rate layers' {sess, used_r, pos0, offset}; DeepSpeech2 stages plain slot indices.
// =====================================================================================
struct ppasr_stream_group_s {
  ppasr_model_s* m;
  int n_sessions, cap, lo;
  int D;               // row width of the caches: 256, or the general route's model width
  GroupFamily family;
  float *kc, *vc;     // [n_sessions][L][cap][D]
  float* xh_hist;     // [n_sessions][L][lo][D] (layer i uses its first kernel_i - 1 rows)
  float* ds2_state;   // DeepSpeech2: h [n_sessions][L][H], then (LSTM) c of the same shape; one allocation
  HistLayer* hist_tab;  // Squeezeformer / Efficient-Conformer: device [L], the layers' pointwise_conv1 (k_pw1_glu_layers)
  StagingRing ring;   // per-call descriptors, room for n_sessions per entry (is_layered: 2 n_sessions)
  std::vector<int> cache_t, cache_r, offset;
};

}  // extern "C"

namespace {

// DeepSpeech2 group: bytes of every session's h (and, LSTM, c) state, [n_sessions][L][H] each
size_t ds2_state_bytes(const ppasr_model_s* h, int n_sessions) {
  const Ds2W& W = h->ds2;
  return (W.gates == 4 ? 2 : 1) * (size_t)n_sessions * W.n_layers * W.H * sizeof(float);
}

ppasr_status group_alloc(ppasr_handle h, int n_sessions, int max_frames, GroupFamily family, ppasr_stream_group* out) {
  auto* g = new ppasr_stream_group_s();  // (value-initialised: every pointer and event null until it exists)
  g->m = h;
  g->n_sessions = n_sessions;
  g->family = family;
  g->cap = (max_frames > 0 && max_frames < h->desc.max_len) ? max_frames : h->desc.max_len;
  g->D = family == GroupFamily::kGeneral ? h->desc.output_size : kD;
  // (the general route without a conv module keeps no history: lo = 0, a one-row allocation as on a stream handle)
  g->lo = (family == GroupFamily::kGeneral && !h->gen.use_cnn) ? 0 : h->desc.cnn_module_kernel - 1;
  const bool layered = is_layered(family);  // (per-layer history table, two descriptor sets)
  // any failure below releases whatever exists so far (ppasr_stream_group_destroy skips what does not)
  auto bail = [g](const char* what, hipError_t e) {
    (void)ppasr_stream_group_destroy(g);
    return fail(PPASR_EHIP, std::string(what) + ": " + hipGetErrorString(e));
  };
  const size_t L = h->desc.num_blocks;
  const bool ds2 = family == GroupFamily::kDeepSpeech2;  // (no caches: the recurrent states)
  const size_t kv = ds2 ? 0 : (size_t)n_sessions * L * g->cap * g->D * sizeof(float);
  const size_t hb = ds2 ? ds2_state_bytes(h, n_sessions) : (size_t)n_sessions * L * std::max(g->lo, 1) * g->D * sizeof(float);
  hipError_t e = hipSuccess;
  if (!ds2) e = hipMalloc(reinterpret_cast<void**>(&g->kc), kv);
  if (e == hipSuccess && !ds2) e = hipMalloc(reinterpret_cast<void**>(&g->vc), kv);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(ds2 ? &g->ds2_state : &g->xh_hist), hb);
  if (e == hipSuccess) e = g->ring.alloc((size_t)(layered ? 2 : 1) * n_sessions * sizeof(SessDesc));
  if (e == hipSuccess && layered) e = hipMalloc(reinterpret_cast<void**>(&g->hist_tab), L * sizeof(HistLayer));
  if (e != hipSuccess) return bail("allocation failed for the session-group caches", e);
  e = hipMemset(ds2 ? g->ds2_state : g->xh_hist, 0, hb);
  if (e != hipSuccess) return bail("clearing the session-group conv histories failed", e);
  if (layered) {
    e = upload_hist_table(h, g->hist_tab);
    if (e != hipSuccess) return bail("uploading the session-group history table failed", e);
  }
  // (as in ppasr_stream_create: the clear and the upload above are null-stream work that a round on the caller's
  // non-blocking stream does not wait for)
  e = hipStreamSynchronize(nullptr);
  if (e != hipSuccess) return bail("waiting for the session-group clears failed", e);
  g->cache_t.assign(n_sessions, 0);
  g->cache_r.assign(n_sessions, 0);
  g->offset.assign(n_sessions, 0);
  *out = g;
  return PPASR_OK;
}

// Squeezeformer / Efficient-Conformer session group: the workspace of n chunks of T frames -- the batched layout for
// B = n (Squeezeformer: its xs holds the pre-reduction rows [n*c][256]), the conv-module input rows [n*c][256] and the GLU'd
// histories [L][n][lo][256] (lo = cnn_module_kernel - 1, the widest layer's)
size_t layered_group_ws_floats(const ppasr_model_s* h, int n, int T) {
  const size_t c = h->front_dims(T).Tp;
  return ws_layout(h, n, T).total + (((size_t)n * c * kD + 63) & ~(size_t)63) +
         (size_t)h->desc.num_blocks * n * (h->desc.cnn_module_kernel - 1) * kD;
}
// Conformer session group: the workspace of n chunks of T frames -- the batched layout for B = n, the conv-module input
// rows [n*c][256] and, for the layer at hand, the listed sessions' gathered and GLU'd histories [n][lo][256] each
size_t conformer_group_ws_floats(const ppasr_model_s* h, int n, int T) {
  const size_t c = ((T - 1) / 2 - 1) / 2;  // (the conv2d front end, the one these groups are built for)
  return ws_layout(h, n, T).total + (size_t)n * c * kD + 64 + (size_t)n * (h->desc.cnn_module_kernel - 1) * kD * 2 + 64;
}

// the rows of a round over the n listed sessions, c frames each: `desc` = the descriptors the round staged (device; the
// half-rate layers' behind the full-rate ones), scratch = the GLU'd-history floats of the family's workspace
StreamRows group_rows(const ppasr_stream_group_s* g, const SessDesc* desc, int n, int c, float* scratch) {
  const long long L = g->m->desc.num_blocks;
  return StreamRows{n, c, ceil_div(c, 2), g->kc, g->vc, g->cap, L * g->cap * kD, g->xh_hist, g->lo, L * g->lo * kD, scratch,
                    g->hist_tab, 0, 0, 0, desc, is_layered(g->family) ? desc + n : nullptr};
}

// ---- launch bodies of a round (ppasr_encode_chunk_group): the launches over the n listed sessions' stacked chunks,
// with the descriptors `desc` the round staged (device) and the workspace ws; *frames = the encoder frames each session
// emitted.  A body that fails returns before the round commits anything. ----
typedef ppasr_status (*GroupBody)(ppasr_stream_group g, const SessDesc* desc, int n, const float* feats, int T, float* probs,
                                  int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st, int* frames,
                                  const MemOut& mem);

// Conformer, Squeezeformer and Efficient-Conformer on the fused 256-wide route: a stream handle's chunk for every listed
// session, rows stacked.  The Efficient-Conformer's plans (plan_chunk_for) double the offset, do not trim the half-rate
// cache and refuse odd cache lengths; its half-rate descriptors carry {sess, cache_r, pos0}, pos0 = 2 offset - cache_t (the
// half-rate layers read every second positional row).
ppasr_status fused_group_body(ppasr_stream_group g, const SessDesc* desc, int n, const float* feats, int T, float* probs,
                              int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st, int* frames,
                                  const MemOut& mem) {
  ppasr_model_s* h = g->m;
  const int c = h->front_dims(T).Tp;
  const StreamWs w = carve_ws(ws, ws_layout(h, n, T), n * c);
  return stream_round(h, group_rows(g, desc, n, c, w.behind), w, feats, T, nullptr, probs, frame_argmax, frame_maxprob, st, frames,
                      mem);
}

// general route: generic_group_chunk over the listed sessions.  pos0 = offset - cache_t picks the relative positional
// rows; abs_pos adds row offset + t.
ppasr_status gen_group_body(ppasr_stream_group g, const SessDesc* desc, int n, const float* feats, int T, float* probs,
                            int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st, int* frames,
                                  const MemOut& mem) {
  *frames = g->m->front_dims(T).Tp;
  return generic_group_chunk(g->m, desc, n, g->kc, g->vc, g->cap, g->xh_hist, g->lo, feats, T, probs, frame_argmax,
                             frame_maxprob, ws, st);
}

// DeepSpeech2: ds2_group_round on the listed sessions' slots (desc holds plain slot indices)
ppasr_status ds2_group_body(ppasr_stream_group g, const SessDesc* desc, int n, const float* feats, int T, float* probs,
                            int32_t* frame_argmax, float* frame_maxprob, float* ws, hipStream_t st, int* frames,
                                  const MemOut& mem) {
  const Ds2W& W = g->m->ds2;
  float* state_h = g->ds2_state;
  float* state_c = W.gates == 4 ? g->ds2_state + (size_t)g->n_sessions * W.n_layers * W.H : nullptr;
  *frames = ((T - 1) / 2 - 1) / 2;
  return ds2_group_round(g->m, reinterpret_cast<const int*>(desc), n, feats, T, state_h, state_c, probs, frame_argmax,
                         frame_maxprob, ws, st);
}

// what a family's groups are built for: the model type (with the refusal of another type, or of a non-streaming handle)
// and the launch body of its rounds; in GroupFamily order
const struct {
  int model_type;
  const char* refusal;
  GroupBody body;
} kGroupKinds[] = {
    {PPASR_MODEL_CONFORMER,
     "session groups are built for streaming (causal) model_type=conformer (Squeezeformer: ppasr_sq_stream_group_create)",
     fused_group_body},
    {PPASR_MODEL_SQUEEZEFORMER, "Squeezeformer session groups are built for streaming (causal) model_type=squeezeformer",
     fused_group_body},
    {PPASR_MODEL_EFFICIENT_CONFORMER,
     "Efficient-Conformer session groups are built for streaming (causal) model_type=efficient_conformer", fused_group_body},
    {PPASR_MODEL_DEEPSPEECH2,
     "DeepSpeech2 session groups are built for streaming (unidirectional) model_type=deepspeech2 "
     "(the reference streams no bidirectional model)",
     ds2_group_body},
    {PPASR_MODEL_CONFORMER, "general-route session groups are built for streaming (causal) model_type=conformer",
     gen_group_body},
};

// the checks every create call shares, then each family's requirements (in the order each create call has made them)
ppasr_status group_create(ppasr_handle h, int n_sessions, int max_frames, GroupFamily family, ppasr_stream_group* out) {
  if (!h || !out || n_sessions < 1) return fail(PPASR_EINVAL, "bad argument");
  const auto& kind = kGroupKinds[(int)family];
  if (h->desc.model_type != kind.model_type || !h->desc.causal) return fail(PPASR_EUNSUPPORTED, kind.refusal);
  if (family == GroupFamily::kDeepSpeech2) {
    if (!h->ds2.wave_tab) return fail(PPASR_EUNSUPPORTED, "DeepSpeech2 session groups run on the wavefront recurrence");
    // (max_frames: no cache grows with the stream -- the state is [L][H] per session whatever its length)
    return group_alloc(h, n_sessions, max_frames, family, out);
  }
  const bool general = family == GroupFamily::kGeneral;
  if (general && !h->generic)
    return fail(PPASR_EUNSUPPORTED, "general-route session groups are built for the general layer route "
                                    "(the fused 256-wide route: ppasr_stream_group_create)");
  if (h->desc.input_layer != 0) return fail(PPASR_EUNSUPPORTED, "session groups are built for the conv2d front end only");
  if (!general && h->generic) return fail(PPASR_EUNSUPPORTED, "session groups are built for the fused 256-wide route");
  if (family == GroupFamily::kSqueezeformer && h->desc.cnn_module_kernel != 31 && h->desc.cnn_module_kernel != 15)
    return fail(PPASR_EUNSUPPORTED, "Squeezeformer session groups: the streaming conv kernels exist for kernel sizes 31 / 15");
  if (family == GroupFamily::kEfficientConformer && __builtin_popcount(eff_stride_mask(h->desc)) > 1)
    return fail(PPASR_EUNSUPPORTED, "Efficient-Conformer session groups are built for at most one stride layer");
  return group_alloc(h, n_sessions, max_frames, family, out);
}

}  // namespace

extern "C" {

ppasr_status ppasr_ds2_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out) {
  return group_create(h, n_sessions, max_frames, GroupFamily::kDeepSpeech2, out);
}
ppasr_status ppasr_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out) {
  return group_create(h, n_sessions, max_frames, GroupFamily::kConformer, out);
}
ppasr_status ppasr_gen_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out) {
  return group_create(h, n_sessions, max_frames, GroupFamily::kGeneral, out);
}
ppasr_status ppasr_sq_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out) {
  return group_create(h, n_sessions, max_frames, GroupFamily::kSqueezeformer, out);
}
ppasr_status ppasr_eff_stream_group_create(ppasr_handle h, int n_sessions, int max_frames, ppasr_stream_group* out) {
  return group_create(h, n_sessions, max_frames, GroupFamily::kEfficientConformer, out);
}

ppasr_status ppasr_stream_group_destroy(ppasr_stream_group g) {
  if (!g) return PPASR_OK;
  g->ring.destroy();
  (void)hipFree(g->kc); (void)hipFree(g->vc); (void)hipFree(g->xh_hist);
  (void)hipFree(g->hist_tab); (void)hipFree(g->ds2_state);
  delete g;
  return PPASR_OK;
}

// session < 0: every session
ppasr_status ppasr_stream_group_reset(ppasr_stream_group g, int session, void* stream) {
  if (!g || session >= g->n_sessions) return fail(PPASR_EINVAL, "bad session");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (g->family == GroupFamily::kDeepSpeech2) {  // zero state (h, c), offset 0
    const Ds2W& W = g->m->ds2;
    const size_t per = (size_t)W.n_layers * W.H, planes = W.gates == 4 ? 2 : 1;
    for (size_t p = 0; p < planes; ++p) {
      float* base = g->ds2_state + p * per * g->n_sessions;
      if (session < 0) HIP_TRY(hipMemsetAsync(base, 0, per * g->n_sessions * sizeof(float), st));
      else HIP_TRY(hipMemsetAsync(base + per * session, 0, per * sizeof(float), st));
    }
    if (session < 0) std::fill(g->offset.begin(), g->offset.end(), 0);
    else g->offset[session] = 0;
    return PPASR_OK;
  }
  const size_t per = (size_t)g->m->desc.num_blocks * g->lo * g->D;
  if (per > 0) {  // (no conv history on a general-route model without a conv module)
    if (session < 0) HIP_TRY(hipMemsetAsync(g->xh_hist, 0, per * g->n_sessions * sizeof(float), st));
    else HIP_TRY(hipMemsetAsync(g->xh_hist + per * session, 0, per * sizeof(float), st));
  }
  if (session < 0) {
    std::fill(g->cache_t.begin(), g->cache_t.end(), 0);
    std::fill(g->cache_r.begin(), g->cache_r.end(), 0);
    std::fill(g->offset.begin(), g->offset.end(), 0);
  } else {
    g->cache_t[session] = 0;
    g->cache_r[session] = 0;
    g->offset[session] = 0;
  }
  return PPASR_OK;
}

int ppasr_stream_group_offset(ppasr_stream_group g, int session) {
  return (g && session >= 0 && session < g->n_sessions) ? g->offset[session] : -1;
}

size_t ppasr_group_chunk_workspace_bytes(ppasr_handle h, int n, int T) {
  if (!h || n < 1 || T < 7) return 0;
  if (h->desc.model_type == PPASR_MODEL_DEEPSPEECH2) return ds2_group_ws_floats(h, n, T) * sizeof(float);
  if (h->generic) return generic_group_ws_floats(h, n, T) * sizeof(float);
  if (is_sq(h) || is_eff(h)) return layered_group_ws_floats(h, n, T) * sizeof(float);
  return conformer_group_ws_floats(h, n, T) * sizeof(float);
}

// One chunk [T frames] for each of the n DISTINCT sessions listed in sessions_host; feats [n][T][F] (device).
// Outputs are indexed by position in the list: probs [n][c][V] (or NULL), frame_argmax / frame_maxprob [n][c].
ppasr_status ppasr_encode_chunk_group(ppasr_stream_group g, const int* sessions_host, int n, const float* feats, int T,
                                      float* probs, int32_t* frame_argmax, float* frame_maxprob, int* c_out_host,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  return ppasr_encode_chunk_group_mem(g, sessions_host, n, feats, T, probs, frame_argmax, frame_maxprob, c_out_host, workspace,
                                      workspace_bytes, nullptr, nullptr, stream);
}

// ppasr_encode_chunk_group, and the round's encoder output behind the listed sessions' frames in the arena `mem_arena`
// (mem_frames_host [n]: rows kept per list position, NULL: all; no arena: the plain round, launch for launch)
ppasr_status ppasr_encode_chunk_group_mem(ppasr_stream_group g, const int* sessions_host, int n, const float* feats, int T,
                                          float* probs, int32_t* frame_argmax, float* frame_maxprob, int* c_out_host,
                                          void* workspace, size_t workspace_bytes, ppasr_prob_arena mem_arena,
                                          const int* mem_frames_host, void* stream) {
  if (!g || !sessions_host || !feats || !workspace || n < 1 || n > g->n_sessions) return fail(PPASR_EINVAL, "bad argument");
  ppasr_model_s* h = g->m;
  if (T < 7) return fail(PPASR_EINVAL, "chunk shorter than the conv front-end's receptive field (7 frames)");
  if (workspace_bytes < ppasr_group_chunk_workspace_bytes(h, n, T)) return fail(PPASR_ENOSPACE, "workspace too small");
  if (!session_list_ok(sessions_host, n, g->n_sessions)) return fail(PPASR_EINVAL, "session index out of range or repeated");
  const bool ds2 = g->family == GroupFamily::kDeepSpeech2, layered = is_layered(g->family);
  const int c = h->front_dims(T).Tp;
  std::vector<ChunkPlan> plans(ds2 ? 0 : n);  // (DeepSpeech2 carries no cache)
  for (size_t b = 0; b < plans.size(); ++b) {
    const int s = sessions_host[b];
    ppasr_status r = plan_chunk_for(h, g->cache_t[s], g->cache_r[s], g->offset[s], g->cap, c, -1, &plans[b]);
    if (r != PPASR_OK) return r;
  }
  const MemOut mem{mem_arena, sessions_host, mem_frames_host};
  if (mem_arena) {
    if (g->family != GroupFamily::kConformer)
      return fail(PPASR_EUNSUPPORTED, "encode_chunk_group_mem: a memory arena is built for Conformer groups on the fused 256-wide "
                                      "route (not DeepSpeech2, general-route, Squeezeformer or Efficient-Conformer groups)");
    ppasr_status r = mem_check(h, mem, n, g->n_sessions, c, "encode_chunk_group_mem");
    if (r != PPASR_OK) return r;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  StagingRing::Entry en;
  HIP_TRY(g->ring.acquire(&en));
  size_t staged = (size_t)n * sizeof(int);
  if (ds2) {
    std::copy(sessions_host, sessions_host + n, reinterpret_cast<int*>(en.host));
  } else {
    const bool zero_pos = g->family == GroupFamily::kGeneral && h->gen.pos != PPASR_OPT_POS_REL;
    SessDesc* desc = reinterpret_cast<SessDesc*>(en.host);
    for (int b = 0; b < n; ++b) {
      const int s = sessions_host[b];
      desc[b] = SessDesc{s, g->cache_t[s], zero_pos ? 0 : plans[b].pos0, g->offset[s]};
      if (layered) desc[n + b] = SessDesc{s, plans[b].used_r, plans[b].pos0, g->offset[s]};
    }
    staged = (size_t)(layered ? 2 : 1) * n * sizeof(SessDesc);
  }
  HIP_TRY(hipMemcpyAsync(en.dev, en.host, staged, hipMemcpyHostToDevice, st));
  int frames = 0;
  ppasr_status r = kGroupKinds[(int)g->family].body(g, reinterpret_cast<const SessDesc*>(en.dev), n, feats, T, probs,
                                                    frame_argmax, frame_maxprob, static_cast<float*>(workspace), st, &frames,
                                                    mem);
  if (r != PPASR_OK) return r;
  for (int b = 0; b < n; ++b) {
    const int s = sessions_host[b];
    if (!ds2) {
      g->cache_t[s] = plans[b].T2;
      g->cache_r[s] = plans[b].T2_r;
    }
    g->offset[s] += frames;
  }
  HIP_TRY(g->ring.release(en, st));
  if (c_out_host) *c_out_host = frames;
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // extern "C"
