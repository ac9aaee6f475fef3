// encode_common.h -- the frame the offline encode walks build around their layer loops: encode_impl (capi.hip),
// squeezeformer_encode (capi_squeezeformer.hip), gen_layers and sq_run (capi_generic.hip).  Included by capi_internal.h
// behind the model struct.  Plain structs and free functions; what differs between the walks is an argument.
#pragma once

// Ragged batches (ppasr_set_skip_padding): rows behind an utterance's valid frames + slack are skipped.  Slack = what
// valid outputs read from the rows behind them.  rc + 4: the right context rc of the non-causal conv module.  A model that
// changes its frame rate (rate_changes: the Efficient-Conformer's stride layer, the Squeezeformer's time reduction and
// recovery) needs more at its ENTRY rate (mul == mul0), where the rows of the reduced rate are made: twice the reduced
// rate's slack (reduced row j reads entry rows 2j - 3 .. 2j + 1; a recovered row t reads reduced row t / 2), plus the
// entry rate's own rc, plus 8 for the stride layer's 2j / 2j + 1 rows and the 3-frame groups of grouped attention.
// `skip` is the walk's own condition (debug taps, input_layer and streaming switch it off differently).
struct RaggedPlan {
  bool skip;
  const int64_t* lens;
  int rc;             // right context of the conv module (0: causal, or no conv module)
  bool rate_changes;
  int mul0;           // pad-mask multiplier of the entry rate (the front end's subsampling)
  int slack(int mul) const { return rate_changes && mul == mul0 ? 2 * (rc + 4) + rc + 8 : rc + 4; }
  PadSkip at(int Tcur, int mul) const {  // for launches over B x Tcur rows whose row t is valid iff mul * t < len
    PadSkip ps;
    if (skip) {
      ps.lens = lens;
      ps.Tp = Tcur;
      ps.mul = mul;
      ps.slack = slack(mul);
    }
    return ps;
  }
  int attn_pad_skip(const PadSkip& ps) const { return skip ? ps.slack + 1 : 0; }  // AttnArgs::pad_skip
};

// Ragged batches on the fused walks: lists of the active row blocks per (frame rate, block size) (rowblock.h PadSkip::tab).
// They live in the CTC head's statistics buffers (`stats`: 2 al64(M) floats, unused until the head), behind conv2's tile
// table (B + 2 ints): first table at round16(B + 2), each table padded to 16 ints, at most four.  A table that does not
// fit is not made and its launches run the padded grid.  (Swept on the host: B = 1 .. 199, T' = 1 .. 139 and 249 / 500 /
// 999, blocks of 16 and 32 rows at the entry rate and at ceil(T' / 2): whenever B + 2 <= al64(M), two tables fit, so the
// test per table never refuses where an all-or-nothing test of two would not.)
struct BlockTables {
  struct Tab { int Ti, R; int* tab; } tabs[4];
  int n = 0, B;
  bool fits, on;  // conv2's tile table fits / lists are made
  size_t off, cap;
  int* base;
  hipStream_t st;
  BlockTables(bool skip, int B_, int M, float* stats, hipStream_t st_)
      : B(B_), off(((size_t)B_ + 2 + 15) / 16 * 16), cap(2 * (((size_t)M + 63) / 64 * 64)), base(reinterpret_cast<int*>(stats)), st(st_) {
    fits = (size_t)B + 2 <= cap / 2;
    on = skip && fits && block_tables_enabled();
  }
  int* tile_tab() const { return fits ? base : nullptr; }  // the active-tile table of the front end's conv2
  PadSkip make(PadSkip p, int Tcur, int R) {  // p with a new list of the active R-row blocks of its B x Tcur rows
    const size_t len = 1 + ((size_t)B * Tcur + R - 1) / R;
    if (!on || n == 4 || off + len > cap) return p;
    int* t = base + off;
    launch_block_table(p, B * Tcur, R, t, st);
    tabs[n++] = Tab{Tcur, R, t};
    off += (len + 15) / 16 * 16;
    p.tab = t;
    return p;
  }
  PadSkip with_table(PadSkip p, int Tcur, int R) {  // ... made on first request
    for (int k = 0; k < n; ++k)
      if (tabs[k].Ti == Tcur && tabs[k].R == R) {
        p.tab = tabs[k].tab;
        return p;
      }
    return make(p, Tcur, R);
  }
};

// debug taps (ppasr_set_debug_taps): copies of the walk's intermediate tensors, in call order, while the buffer has room
struct Taps {
  float* buf;
  size_t cap;
  hipStream_t st;
  size_t off = 0;
  void operator()(const float* src, size_t n_floats) {
    if (buf && off + n_floats <= cap)
      (void)hipMemcpyAsync(buf + off, src, n_floats * sizeof(float), hipMemcpyDeviceToDevice, st);
    off += n_floats;
  }
};

// a walk without kernel classes (ppasr_profile_enable is the Conformer walk's): `spans(cls, fn)` just runs fn
struct NoSpans {
  template <typename Fn>
  void operator()(int, Fn&& fn) const { fn(); }
};

// The 4x / 6x front end of the fused walks (input_layer 0 and 6): conv1 + conv2 -- Conv2dSubsampling4 as one launch with
// conv1's output never leaving the chip (front_fused.hip), or k_conv1 and the quad form of conv2, or k_conv1 and the direct
// form (fp16 x3 mode: conv2 on that route, with its re-packed weight; 5x5 / 3) -- then the input projection into xa.
// ps: the front end's own kernels; ps_embed / embed_slices: the projection's.  spans(0 / 1 / 2, ...): conv1 / conv2 / embed.
template <typename Spans>
inline void front4_fused(const ppasr_model_s* h, const float* feats, int B, int T, const PadSkip& ps, int* tile_tab,
                         bool scale_before_bias, int embed_slices, const PadSkip& ps_embed, float* y1, float* y2, float* xa,
                         hipStream_t st, Spans&& spans) {
  const auto fd = h->front_dims(T);
  const int F = h->desc.input_dim, T1 = fd.T1, F1 = h->F1, Tp = fd.Tp, F2 = h->F2;
  const bool il4 = h->desc.input_layer == 0;
  const f32x4* conv2_h3 = h->gemm_mode == PPASR_GEMM_F16X3 ? h->conv2_w_h3 : nullptr;
  const bool conv12 = il4 && !conv2_h3 && conv12_enabled(h) && conv12_supported(h->front, F, F2);
  if (!conv12) spans(0, [&] { launch_conv1(feats, h->front, y1, B, T, F, T1, F1, st, ps); });
  spans(1, [&] {
    if (conv12) launch_conv12(feats, h->front, y2, B, T, F, Tp, F2, st, ps, tile_tab);
    else if (il4 && !conv2_h3 && conv2_quad_supported(h->front)) launch_conv2_quad(y1, h->front, y2, B, T1, F1, Tp, F2, st, ps, tile_tab);
    else launch_conv2(y1, h->front, y2, B, T1, F1, Tp, F2, st, ps, tile_tab, il4 ? conv2_h3 : nullptr);
  });
  spans(2, [&] {
    launch_embed(y2, h->front, xa, B * Tp, F2 * kD, sqrtf((float)kD), scale_before_bias, st, ps_embed, embed_slices, y1,
                 conv2_h3 ? h->embed_w_h3 : nullptr);
  });
}

// ppasr_set_memory_out: the encoder output [M][D] of an offline encode, from the rows x the head reads (g / b: the after_norm
// the head applies to them, nullptr: none or already applied); ragged batches (ps.lens): 0 behind the valid frames.  One
// small launch of its own beside the head; nothing when the pointer is clear.
inline ppasr_status memory_out(const ppasr_model_s* h, const float* x, const float* g, const float* b, int M, int D,
                               const PadSkip& ps, hipStream_t st) {
  if (!h->memory_out) return PPASR_OK;
  if ((size_t)M * D > h->memory_floats) return fail(PPASR_ENOSPACE, "memory buffer too small (ppasr_set_memory_out)");
  launch_memory_out(x, g, b, h->memory_out, M, D, ps, st);
  return PPASR_OK;
}

// The head of the fused walks over the M = B x ps.Tp rows of x: CTC head (its re-packed weight in the fp16 x3 mode; on an
// under-filled launch the vocabulary tiles over `slices` workgroups per row block, scratch = the conv1 buffer y1) ->
// logits, frame argmax / maxprob (into the workspace when the caller wants none), probabilities in place from the logits
// and the head's row statistics; ragged batches (ps.lens): the outputs behind the valid frames are zeroed.
// spans(7, ...): the head's launch.
template <typename Spans>
inline ppasr_status fused_head_tail(const ppasr_model_s* h, const float* x, float* probs, float* logits, int32_t* frame_argmax,
                                    float* frame_maxprob, float* ws, const WsLayout& wl, int B, int M, int slices,
                                    const PadSkip& ps, hipStream_t st, Spans&& spans) {
  if (ppasr_status ms = memory_out(h, x, h->head.ln_g, h->head.ln_b, M, kD, ps, st)) return ms;
  float* lg = logits ? logits : probs;  // probs are produced in place from the logits tap
  int32_t* fa = frame_argmax ? frame_argmax : reinterpret_cast<int32_t*>(ws + wl.fa);
  float* fp = frame_maxprob ? frame_maxprob : ws + wl.fp;
  spans(7, [&] {
    const bool head_h3 = h->gemm_mode == PPASR_GEMM_F16X3 && h->head_w_h3;
    HeadW hw = h->head;
    if (head_h3) hw.w = h->head_w_h3;
    launch_ctc_head(x, hw, lg, fa, fp, ws + wl.rmax, ws + wl.rsum, M, st, ps, slices, ws + wl.y1, head_h3);
  });
  if (probs) {
    if (logits) HIP_TRY(hipMemcpyAsync(probs, logits, (size_t)M * h->head.V * sizeof(float), hipMemcpyDeviceToDevice, st));
    launch_softmax_from_stats(probs, ws + wl.rmax, ws + wl.rsum, M, h->head.V, st, ps);
  }
  if (ps.lens) launch_zero_pad_rows(probs, logits, fa, fp, ps.lens, B, ps.Tp, ps.mul, h->head.V, st);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

// ---- the Conformer walk's route of one layer (encode_impl) ----
struct LayerRoute {
  int form;        // block form of the layer's stage launches (rbt.h): 32, 16 or kW16
  int S;           // hidden slices per row block (> 1: the split route of under-filled launches, partial sums in y1)
  bool fuse_attn;  // attention + out-projection / GLU as one launch (context rows stay in LDS)
  bool h3, h3s;    // fp16 x3 mode: the fused units / the split route's units on that route (weights: the layer's h3 view)
};
// The row-count half of the fused-attention rule: a layer of `rows` rows may take it.  An under-filled grid is
// latency-bound either way, and the two-kernel route then has 4x the workgroups in its attention half, one per head:
// 2 - 6 % faster end to end up to 128 row blocks, 10 % slower at the bench shape (measured).  The fused kernel reads the
// values in fragment order, which only the fused QKV stage (ffn_qkv_body) writes: a FORCED split of a large batch
// (ppasr_set_ffn_split(2 / 4 / 8), k_ln_qkv) never fuses; ppasr_set_ffn_split(0) always does.
inline bool fuse_rows(const ppasr_model_s* h, int rows) {
  constexpr int fuse_min_blocks = 128;
  return ffn_split_for(h, rows) == 1 && (h->ffn_split == 0 || (rows + kRows - 1) / kRows > fuse_min_blocks);
}
// layer `layer` over B x Ti rows (pad-mask multiplier mul; ragged batches: `skip` with this rate's slack)
inline LayerRoute layer_route(const ppasr_model_s* h, int B, int Ti, int mul, int slack, bool skip, int layer) {
  const int Mi = B * Ti;
  LayerRoute r;
  // under-filled launch, 33 .. 128 row blocks: the 16-row-block kernels (conformer_kernels_t.hip) -- twice the workgroups,
  // each half as long -- with the stand-alone attention between them; up to 32 blocks the split route.  The debug taps
  // take 32-row blocks.
  const int rows = (!h->taps && conv_ffn_16_supported(h->layer_ks[layer], Ti)) ? row_block_for(h, B, Ti, mul, slack, skip) : 32;
  const bool r16 = rows == 16 && h->ffn_split < 0;
  // plain 4 x 64 heads fuse; the debug taps need the context tensor, so they take the two-kernel route
  r.fuse_attn = !r16 && h->layer_group[layer] == 1 && h->desc.attention_heads == 4 && !h->taps && fuse_rows(h, Mi);
  // under-filled grid: FFNs split over S workgroups per row block
  r.S = r16 ? 1 : ffn_split_for(h, Mi);
  // full grid: the same 32-row blocks on 16 waves (k_*_t<kW16>: drop-in for k_ffn_qkv / k_out_glu / k_conv_ffn)
  const bool w16 = rows == kW16 && r.S == 1;
  r.form = r16 ? 16 : w16 ? kW16 : 32;
  // feed-forward GEMMs on the fp16 x3 route (ppasr_set_gemm_mode): the 8-wave 32-row kernels only ...
  r.h3 = h->h3_layers() && !r16 && !w16 && r.S == 1;
  // ... and the split route's units (h3 view for the weights only: the stand-alone attention keeps the fp32 table)
  r.h3s = h->h3_layers() && r.S > 1;
  return r;
}
