// capi_squeezeformer.hip -- weight packing and launch sequence of the Squeezeformer encoder
// (ppasr/model_utils/squeezeformer/{encoder,attention,convolution,positionwise,subsampling,
// time_reduction}.py) behind ppasr_create / ppasr_encode.  The packing goes through the loader every family shares
// (weights.h); what is written here is the Squeezeformer's own: the adaptive-scale vectors, final_proj.
#include "capi_internal.h"

ppasr_status squeezeformer_create(ppasr_model_s* m, Loader& ld) {
  const ppasr_model_desc& dsc = m->desc;
  const int F = dsc.input_dim, d = dsc.output_size, H = dsc.linear_units, V = dsc.vocab_size, KS = dsc.cnn_module_kernel;
  const int F2 = m->F2, L = dsc.num_blocks;
  const float* pe_dev = nullptr;
  LOAD_TRY(ld.pe_table(&pe_dev));
  if (dsc.reduce_idx >= 0 && (dsc.recover_idx <= dsc.reduce_idx || dsc.recover_idx >= L || dsc.reduce_idx == 0))
    return fail(PPASR_EUNSUPPORTED, "squeezeformer: need 0 < reduce_idx < recover_idx < num_blocks (or reduce_idx = -1)");
  // adaptive_scale = False (encoder.py:44): the ada_scale / ada_bias parameters exist in the checkpoint (every module creates
  // them, attention.py:34-37) but are not applied -- fold ones / zeros instead
  const bool no_ada = (dsc.options & PPASR_OPT_SQ_NO_ADAPTIVE_SCALE) != 0;
  const std::vector<float> ones_d(d, 1.f), zeros_d(d, 0.f);
  // a module's adaptive scale / bias [d], which the loader's recipes fold into the module's first dense layer
  const float *as = nullptr, *ab = nullptr;
  auto ada = [&](const std::string& module) -> ppasr_status {
    GETW(s, module + ".ada_scale", d);
    GETW(b, module + ".ada_bias", d);
    as = no_ada ? ones_d.data() : s;
    ab = no_ada ? zeros_d.data() : b;
    return PPASR_OK;
  };
  FrontW& fr = m->front;
  {  // DepthwiseConv2DSubsampling4 (subsampling.py:36-47): two 3x3 / 2 convs; dw_stride = True makes the second one depthwise
    LOAD_TRY(ld.cmvn(F, &fr.cmvn_mean, &fr.cmvn_istd));
    LOAD_TRY(ld.taps("encoder.embed.pw_conv.weight", d, 9, &fr.conv1_w));
    LOAD_TRY(ld.vec("encoder.embed.pw_conv.bias", d, &fr.conv1_b));
    // dw_stride = True (groups = odim): weight [d][1][3][3].  Run as the ordinary conv with a block-diagonal weight -- the
    // off-diagonal products are exact zeros, so the sums are the depthwise conv's; no shipped config sets the option
    bool dw_stride = false;
    const float* c2w = ld.get_either("encoder.embed.dw_conv.weight", (size_t)d * d * 9, (size_t)d * 9, &dw_stride);
    if (!c2w) return ld.emissing();
    const bool quad = d == kD;  // (batched calls: front_fused.hip)
    if (dw_stride)
      LOAD_TRY(ld.conv2(d, 9, [=](int k, int n) { return (k % d) == n ? c2w[(size_t)n * 9 + (k / d)] : 0.f; }, quad,
                        &fr.conv2_w, &fr.conv2_wp));
    else
      LOAD_TRY(ld.conv2(d, 9, Loader::dense_conv(c2w, d, 9), quad, &fr.conv2_w, &fr.conv2_wp));
    LOAD_TRY(ld.vec("encoder.embed.dw_conv.bias", d, &fr.conv2_b));
    LOAD_TRY(ld.embed("encoder.embed.input_proj.0", F2, d, &fr.embed_w, &fr.embed_b));
    LOAD_TRY(ld.norm("encoder.preln", d, &m->preln_g, &m->preln_b));
  }
  m->sq_layers.resize(L);
  for (int i = 0; i < L; ++i) {
    SqLayerW& W = m->sq_layers[i];
    const std::string p = "encoder.encoders." + std::to_string(i) + ".";
    LOAD_TRY(ld.norm(p + "layer_norm1", d, &W.ln1_g, &W.ln1_b));
    LOAD_TRY(ld.norm(p + "layer_norm2", d, &W.ln2_g, &W.ln2_b));
    LOAD_TRY(ld.norm(p + "layer_norm3", d, &W.ln3_g, &W.ln3_b));
    LOAD_TRY(ld.norm(p + "layer_norm4", d, &W.ln4_g, &W.ln4_b));
    LOAD_TRY(ld.conv_module_norm(p + "conv_module.norm", d, &W.ln_cm_g, &W.ln_cm_b, &W.cm_eps));
    LOAD_TRY(ada(p + "ffn1"));
    LOAD_TRY(ld.ffn(p + "ffn1", d, H, as, ab, &W.ff1_w1, &W.ff1_b1, &W.ff1_w2, &W.ff1_b2));
    LOAD_TRY(ada(p + "ffn2"));
    LOAD_TRY(ld.ffn(p + "ffn2", d, H, as, ab, &W.ff2_w1, &W.ff2_b1, &W.ff2_w2, &W.ff2_b2));
    // pos_enc_layer_type != rel_pos (squeezeformer/encoder.py:101-105): conformer's plain MultiHeadedAttention -- no
    // linear_pos, no pos_bias_u / _v, no adaptive scale.  The attention kernels then contract the positional half with a
    // row of zeros (pos_bias = 0, table stride 0), like the Conformer's abs_pos / no_pos layers
    if ((dsc.options & PPASR_OPT_POS_MASK) != PPASR_OPT_POS_REL) {
      LOAD_TRY(ld.qkv_out(p + "self_attn.", d, ones_d.data(), zeros_d.data(), &W.wqkv, &W.bqkv, &W.wo, &W.bo));
      LOAD_TRY(ld.up(zeros_d, &W.pos_u));
      LOAD_TRY(ld.up(zeros_d, &W.pos_v));
      W.ptab = W.pos_u;  // (a row of zeros; read with stride 0)
    } else {
      LOAD_TRY(ada(p + "self_attn"));
      LOAD_TRY(ld.qkv_out(p + "self_attn.", d, as, ab, &W.wqkv, &W.bqkv, &W.wo, &W.bo));
      LOAD_TRY(ld.vec(p + "self_attn.pos_bias_u", d, &W.pos_u));
      LOAD_TRY(ld.vec(p + "self_attn.pos_bias_v", d, &W.pos_v));
      // (linear_pos HAS a bias here, squeezeformer/attention.py:28)
      LOAD_TRY(ld.pos_table(p + "self_attn.", d, true, pe_dev, &W.ptab));
    }
    {
      const std::string cm = p + "conv_module.";
      LOAD_TRY(ada(p + "conv_module"));
      LOAD_TRY(ld.conv_pointwise(cm, d, as, ab, &W.pw1, &W.pw1_b, &W.glu_pad, &W.pw2, &W.pw2_b));
      // the scale / bias and the unfolded pointwise_conv1 as well: a chunk applies the scale in front of its cached inputs
      LOAD_TRY(ld.up(vec_of(as, d), &W.cm_scale));
      LOAD_TRY(ld.up(vec_of(ab, d), &W.cm_bias));
      GETW(p1w, cm + "pointwise_conv1.weight", (size_t)2 * d * d);
      LOAD_TRY(ld.packed(d, 2 * d, [&](int k, int n) { return p1w[(size_t)n * d + k]; }, &W.pw1_raw));
      LOAD_TRY(ld.vec(cm + "pointwise_conv1.bias", 2 * d, &W.pw1_b_raw));
      LOAD_TRY(ld.taps(cm + "depthwise_conv.weight", d, KS, &W.dw_w));
      LOAD_TRY(ld.vec(cm + "depthwise_conv.bias", d, &W.dw_b));
    }
  }
  if (dsc.reduce_idx >= 0) {
    // TimeReductionLayerStream: depthwise kernel 1; TimeReductionLayer1D (non-streaming model): kernel 5
    const std::string tr = "encoder.time_reduction_layer.";
    bool k5 = false;
    const float* rdw = ld.get_either(tr + "dw_conv.weight", d, (size_t)d * 5, &k5);
    if (!rdw) return ld.emissing();
    m->sq_reduce.ks = k5 ? 5 : 1;
    LOAD_TRY(ld.taps(rdw, d, m->sq_reduce.ks, &m->sq_reduce.dw_w));
    LOAD_TRY(ld.vec(tr + "dw_conv.bias", d, &m->sq_reduce.dw_b));
    GETW(rpw, tr + "pw_conv.weight", d * d);
    LOAD_TRY(ld.packed(d, d, [&](int k, int n) { return rpw[(size_t)n * d + k]; }, &m->sq_reduce.pw));
    LOAD_TRY(ld.vec(tr + "pw_conv.bias", d, &m->sq_reduce.pw_b));
    GETW(rw, "encoder.time_recover_layer.weight", d * d);
    LOAD_TRY(ld.packed(d, d, [&](int k, int n) { return rw[(size_t)k * d + n]; }, &m->sq_wrec));
    LOAD_TRY(ld.vec("encoder.time_recover_layer.bias", d, &m->sq_brec));
  }
  {
    // final_proj (output_size != encoder_dim, encoder.py:165-167,234-235): a Linear between the last layer and ctc_lo with
    // nothing in between -- folded into the head at create time, logits = x (W_fp W_ctc) + (b_fp W_ctc + b_ctc), in double
    std::vector<float> cw_f, cb_f;
    const float *cw = nullptr, *cb = nullptr;
    auto fp = ld.sd.find("encoder.final_proj.weight");
    if (fp != ld.sd.end()) {
      const Blob& fb = fp->second;
      if (fb.ndim != 2 || fb.shape[0] != d) return fail(PPASR_EMISSING, "mis-shaped weight: encoder.final_proj.weight");
      const int O = (int)fb.shape[1];
      const float* fw = fb.p;
      GETW(fbias, "encoder.final_proj.bias", O);
      GETW(cw_o, "ctc.ctc_lo.weight", (size_t)O * V);
      GETW(cb_o, "ctc.ctc_lo.bias", V);
      cw_f.resize((size_t)d * V);
      cb_f.resize(V);
      std::vector<double> acc(V);
      for (int k = 0; k < d; ++k) {
        std::fill(acc.begin(), acc.end(), 0.0);
        for (int o = 0; o < O; ++o) {
          const double f = fw[(size_t)k * O + o];
          const float* row = cw_o + (size_t)o * V;
          for (int n = 0; n < V; ++n) acc[n] += f * (double)row[n];
        }
        for (int n = 0; n < V; ++n) cw_f[(size_t)k * V + n] = (float)acc[n];
      }
      for (int n = 0; n < V; ++n) acc[n] = (double)cb_o[n];
      for (int o = 0; o < O; ++o)
        for (int n = 0; n < V; ++n) acc[n] += (double)fbias[o] * (double)cw_o[(size_t)o * V + n];
      for (int n = 0; n < V; ++n) cb_f[n] = (float)acc[n];
      cw = cw_f.data();
      cb = cb_f.data();
      m->sq_final_proj = true;  // (the encoder's own output is then never formed: ppasr_set_memory_out refuses)
    } else {
      GETW(cw_d, "ctc.ctc_lo.weight", (size_t)d * V);
      GETW(cb_d, "ctc.ctc_lo.bias", V);
      cw = cw_d;
      cb = cb_d;
    }
    m->head.ln_g = nullptr;  // no after_norm in Squeezeformer
    m->head.ln_b = nullptr;
    m->head.V = V;
    m->head.n_tiles = (V + 31) / 32;
    LOAD_TRY(ld.head(cw, cb, d, V, 32, &m->head.w, &m->head.b));
    if (m->generic) {  // general route (encoder_dim 512 ..): the head as a plain dense layer over the padded vocabulary
      m->gen_vpad = (V + 255) / 256 * 256;
      LOAD_TRY(ld.head(cw, cb, d, V, 256, &m->gen_head_w, &m->gen_head_b));
    }
  }
  return PPASR_OK;
}

// the conv-module fields of a Squeezeformer layer as the LayerW view k_conv_pre reads
LayerW sq_conv_view(const SqLayerW& W) {
  LayerW v{};
  v.dw_w = W.dw_w; v.dw_b = W.dw_b; v.glu_pad = W.glu_pad;
  v.ln_cm_g = W.ln_cm_g; v.ln_cm_b = W.ln_cm_b; v.cm_eps = W.cm_eps;
  v.pw2 = W.pw2; v.pw2_b = W.pw2_b;
  return v;
}

// SqueezeformerEncoder.forward (squeezeformer/encoder.py:172-236) + ctc softmax
ppasr_status squeezeformer_encode(ppasr_model_s* h, const float* feats, const int64_t* lens, int B, int T, float* probs,
                                  float* logits, int32_t* frame_argmax, float* frame_maxprob, float* ws,
                                  const WsLayout& wl, hipStream_t st) {
  const int Tp = h->front_dims(T).Tp;
  const int Tr = (Tp + 1) / 2;  // Conv1D(k=1, stride 2): ceil(T'/2) frames (time_reduction.py:186,196-199)
  const int M = B * Tp, L = h->desc.num_blocks, H = h->desc.attention_heads;
  const int n_chunks = h->desc.linear_units / 256, KS = h->desc.cnn_module_kernel;
  float *y1 = ws + wl.y1, *y2 = ws + wl.y2, *xa = ws + wl.xa, *xb = ws + wl.xb, *xc = ws + wl.xc;
  float *qkv = ws + wl.qkv, *ctx = ws + wl.ctx, *g = ws + wl.g, *xs = ws + wl.xs;
  Taps tap{h->taps, h->taps_floats, st};
  // ragged batches (ppasr_set_skip_padding, see ppasr_encode; the rule: RaggedPlan -- the rate changes at the time-reduction
  // layer and back at the recovery)
  const bool skip = h->skip_padding && lens && !h->taps;
  const bool causal = h->desc.causal != 0;
  const RaggedPlan ragged{skip, lens, causal ? 0 : (KS - 1) / 2, true, 4};
  const PadSkip psF = ragged.at(Tp, 4), psH = ragged.at(Tr, 8);
  // ragged batch: the active row blocks of the two frame rates as lists (PadSkip::tab), for the layer kernels K_B / K_C --
  // with the beam search of the previous batch on some CUs a padded grid with early exits runs extra rounds (rowblock.h).
  // (one list per rate even where T' = 1 makes the two rates the same rows: make, not with_table)
  const int rowsF = h->taps ? 32 : row_block_for(h, B, Tp, 4, psF.slack, skip);
  const int rowsH = h->taps ? 32 : row_block_for(h, B, Tr, 8, psH.slack, skip);
  BlockTables tables(skip, B, M, ws + wl.rmax, st);
  const PadSkip psF_rb = tables.make(psF, Tp, form_rows(rowsF)), psH_rb = tables.make(psH, Tr, form_rows(rowsH));
  // (the embed GEMM works on 32-row blocks: it takes the full-rate list when that is the 32-row one)
  front4_fused(h, feats, B, T, psF, tables.tile_tab(), /*scale_before_bias=*/true, ffn_split_for(h, M),
               (rowsF != 16 && ffn_split_for(h, M) == 1) ? psF_rb : psF, y1, y2, xa, st, NoSpans{});
  launch_ln_rows(xa, h->preln_g, h->preln_b, M, st, psF);
  tap(xa, (size_t)M * kD);
  float* x = xa;      // current layer input / residual
  float* other = xb;  // ping-pong partner
  bool reduced = false;
  bool have_qkv = false;
  for (int i = 0; i < L; ++i) {
    const SqLayerW& W = h->sq_layers[i];
    if (i == h->desc.reduce_idx) {
      // recover_activations.append(xs) ; time_reduction_layer ; pos_emb[:, ::2]  (encoder.py:210-216)
      HIP_TRY(hipMemcpyAsync(xs, x, (size_t)M * kD * sizeof(float), hipMemcpyDeviceToDevice, st));
      launch_sq_reduce(x, other, qkv, h->sq_reduce, W.wqkv, W.bqkv, lens, B, Tp, Tr, st, psH);
      std::swap(x, other);
      reduced = true;
      have_qkv = true;
    }
    if (i == h->desc.recover_idx && reduced) {
      launch_sq_recover(x, xs, other, qkv, h->sq_wrec, h->sq_brec, W.wqkv, W.bqkv, B, Tp, Tr, st, psF);
      std::swap(x, other);
      reduced = false;
      have_qkv = true;
    }
    const int Ti = reduced ? Tr : Tp;
    const int Mi = B * Ti;
    const int mul = reduced ? 8 : 4;
    const PadSkip& ps = reduced ? psH : psF;
    // under-filled launches up to kSplitRows16Max rows (one utterance, small batches; fp32): the single-unit launches on
    // the Conformer's 16-row kernels through weight views, as a stream handle's chunk does (capi_stream.hip sq_stream_layers)
    const bool views16 = ffn_split_for(h, Mi) > 1 && !(rowsF == 16 && h->ffn_split < 0) && Mi <= kSplitRows16Max &&
                         !h->h3_sq_layers();
    auto qkv_view = [](const SqLayerW& w) {
      LayerW v{};
      v.wqkv = w.wqkv;
      v.bqkv = w.bqkv;
      return v;
    };
    if (!have_qkv) {
      if (views16) launch_ln_qkv(x, qkv, qkv_view(W), Mi, st, ps, nullptr, nullptr, false);
      else launch_sq_qkv(x, qkv, W.wqkv, W.bqkv, Mi, st, ps);
    }
    tap(qkv, (size_t)Mi * 3 * kD);
    AttnArgs a{qkv, 768, qkv + 256, 768, qkv + 512, 768, Ti, Ti, 0, lens, ctx, W.pos_u, W.pos_v, W.ptab, reduced ? 2 : 1, mul, Ti, Ti, 1};
    a.pad_skip = ragged.attn_pad_skip(ps);
    launch_attention(a, B, H, st);
    tap(ctx, (size_t)Mi * kD);
    // under-filled grid (ppasr_set_ffn_split): K_B / K_C cut at their feed-forward modules, partial sums in the conv1 buffer
    // under-filled launch: 16-row blocks (twice the workgroups, each half as long) before the split route
    // ... and full launches: the 32-row blocks on 16 waves (rbt.h kW16)
    const int rows = reduced ? rowsH : rowsF;
    const PadSkip& ps_rb = reduced ? psH_rb : psF_rb;  // (with the list of active blocks of THIS block size)
    const int S = rows == 16 && h->ffn_split < 0 ? 1 : ffn_split_for(h, Mi);  // (an explicit ffn_split mode wins)
    const bool fuse_next = (i + 1 < L) && (i + 1 != h->desc.reduce_idx) && !(i + 1 == h->desc.recover_idx && reduced);
    const SqLayerW* Wn = fuse_next ? &h->sq_layers[i + 1] : nullptr;
    if (S > 1) {
      // (fp16 x3 mode: the two feed-forward modules' slices on that route -- the re-packed weights of the layer's h3 view)
      const bool h3s = h->h3_sq_layers();
      const SqLayerW& Ws = h3s ? h->sq_layers_h3[i] : W;
      // x1 = LN1(x + MHA) in `other` (free until this layer's output)
      if (views16) {
        LayerW vo{};
        vo.wo = W.wo; vo.bo = W.bo; vo.ln_conv_g = W.ln1_g; vo.ln_conv_b = W.ln1_b;
        launch_oproj_ln_16(ctx, x, g, other, vo, Mi, st, ps);  // (the plain sum goes to g, dead until pointwise_conv1 writes it)
      } else {
        launch_sq_oproj(ctx, x, other, W, Mi, st, ps);
      }
      launch_ffn_split(other, nullptr, nullptr, Ws.ff1_w1, W.ff1_b1, Ws.ff1_w2, W.ff1_b2, 1.0f, W.ln2_g, W.ln2_b, y1, xc, Mi,
                       n_chunks, S, st, ps, false, h3s);
      if (views16) {
        LayerW vp{};
        vp.pw1 = W.pw1; vp.pw1_b = W.pw1_b; vp.glu_pad = W.glu_pad;
        launch_pw1_glu_cols_16(xc, g, vp, Mi, st, nullptr, 0, nullptr, nullptr, ps, lens, Ti, mul);
      } else {
        launch_sq_pw1glu(xc, g, nullptr, W, lens, Mi, Ti, mul, st, ps);
      }
      tap(xc, (size_t)Mi * kD);
      tap(g, (size_t)Mi * kD);
      launch_conv_pre(g, nullptr, xc, ctx, sq_conv_view(W), lens, Mi, Ti, KS, mul, st, causal, ps);
      launch_ffn_split(ctx, W.ln3_g, W.ln3_b, Ws.ff2_w1, W.ff2_b1, Ws.ff2_w2, W.ff2_b2, 1.0f, W.ln4_g, W.ln4_b, y1, other, Mi,
                       n_chunks, S, st, ps, /*residual_is_normed=*/true, h3s);
      if (Wn && views16) launch_ln_qkv(other, qkv, qkv_view(*Wn), Mi, st, ps, nullptr, nullptr, false);
      else if (Wn) launch_sq_qkv(other, qkv, Wn->wqkv, Wn->bqkv, Mi, st, ps);
    } else {
      // feed-forward modules on the fp16 x3 route (ppasr_set_gemm_mode): the 8-wave 32-row kernels only
      const bool h3 = h->h3_sq_layers() && rows == 32 && !h->taps && sq_h3_supported(KS, Ti);
      const SqLayerW& Wk = h3 ? h->sq_layers_h3[i] : W;
      launch_sq_mid(ctx, x, xc, g, nullptr, Wk, lens, Mi, Ti, mul, n_chunks, st, ps_rb, rows, h3);
      tap(xc, (size_t)Mi * kD);
      tap(g, (size_t)Mi * kD);
      launch_sq_tail(g, nullptr, xc, other, qkv, Wk, Wn ? Wn->wqkv : nullptr, Wn ? Wn->bqkv : nullptr, lens, Mi, Ti, mul,
                     n_chunks, KS, st, ps_rb, causal, rows, h3);
    }
    std::swap(x, other);
    have_qkv = fuse_next;
    tap(x, (size_t)Mi * kD);
  }
  // (the encoder ends at the full rate after the recovery; without one it stays reduced and M rows = B * Tp is the
  //  caller's contract either way: every row is computed and none zeroed)
  return fused_head_tail(h, x, probs, logits, frame_argmax, frame_maxprob, ws, wl, B, M, ffn_split_for(h, M),
                         reduced ? PadSkip{} : psF, st, NoSpans{});
}
