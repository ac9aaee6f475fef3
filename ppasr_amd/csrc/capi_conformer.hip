// capi_conformer.hip -- weight packing of the Conformer / Efficient-Conformer encoders (fused 256-wide route and the
// general layer route of capi_generic.hip) behind ppasr_create.  Host only: the launch sequence is capi.hip's.
#include "capi_internal.h"

ppasr_status conformer_create(ppasr_model_s* m, Loader& ld) {
  const ppasr_model_desc& desc = m->desc;
  const bool eff = desc.model_type == PPASR_MODEL_EFFICIENT_CONFORMER;
  const int F = desc.input_dim, d = desc.output_size, H = desc.linear_units, V = desc.vocab_size, KS = desc.cnn_module_kernel;
  const int il = desc.input_layer;
  const int F2 = m->F_last();  // feature bins entering the linear layer
  const auto& go = m->gen;
  FrontW& fr = m->front;
  LOAD_TRY(ld.cmvn(F, &fr.cmvn_mean, &fr.cmvn_istd));
  if (il == 1) {  // ---- LinearNoSubsampling (subsampling.py:24-65): out.0 = Linear(idim, odim), out.1 = LayerNorm(eps 1e-12), ReLU ----
    GETW(ew, "encoder.embed.out.0.weight", (size_t)F * d);
    m->lin_kpad = (F + 255) / 256 * 256;  // the feature rows are zero-padded to whole K chunks (k_g_cmvn_pad)
    LOAD_TRY(ld.packed(m->lin_kpad, d, [&](int k, int n) { return k < F ? ew[(size_t)k * d + n] : 0.f; }, &fr.embed_w));
    LOAD_TRY(ld.vec("encoder.embed.out.0.bias", d, &fr.embed_b));
    LOAD_TRY(ld.norm("encoder.embed.out.1", d, &m->lin_ln_g, &m->lin_ln_b));
    fr.conv1_w = fr.conv1_b = fr.conv2_b = nullptr;
    fr.conv2_w = nullptr;
  } else {  // ---- conv front ends ----
    LOAD_TRY(ld.taps("encoder.embed.conv.0.weight", d, 9, &fr.conv1_w));
    LOAD_TRY(ld.vec("encoder.embed.conv.0.bias", d, &fr.conv1_b));
    const int k2 = il == 6 ? 5 : 3;  // Conv2dSubsampling6: Conv2D(odim, odim, 5, 3) (subsampling.py:139-141)
    GETW(c2w, "encoder.embed.conv.2.weight", (size_t)d * d * k2 * k2);
    LOAD_TRY(ld.conv2(d, k2 * k2, Loader::dense_conv(c2w, d, k2 * k2), il == 0 && d == kD, &fr.conv2_w, &fr.conv2_wp));
    LOAD_TRY(ld.vec("encoder.embed.conv.2.bias", d, &fr.conv2_b));
    fr.conv2_k = k2;
    fr.conv2_s = il == 6 ? 3 : 2;
    fr.conv3_w = nullptr;
    fr.conv3_b = nullptr;
    if (il == 8) {  // third Conv2D(odim, odim, 3, 2) (subsampling.py:183-187)
      GETW(c3w, "encoder.embed.conv.4.weight", (size_t)d * d * 9);
      LOAD_TRY(ld.packed(9 * d, d, Loader::dense_conv(c3w, d, 9), &fr.conv3_w));
      LOAD_TRY(ld.vec("encoder.embed.conv.4.bias", d, &fr.conv3_b));
    }
    // Conv2dSubsampling4 names its projection `out` (a Sequential), the 6x / 8x classes `linear` (subsampling.py:142,189)
    LOAD_TRY(ld.embed(il ? "encoder.embed.linear" : "encoder.embed.out.0", F2, d, &fr.embed_w, &fr.embed_b));
  }

  LOAD_TRY(ld.pe_table(&m->pe_dev));
  LOAD_TRY(ld.up(std::vector<float>(d, 0.f), &m->zero_vec));
  if (m->generic) m->gen_x.resize(desc.num_blocks);
  const int max_len = desc.max_len;
  m->layers.resize(desc.num_blocks);
  m->layer_ks.assign(desc.num_blocks, KS);
  m->layer_group.assign(desc.num_blocks, 1);
  for (int i = 0; i < desc.num_blocks; ++i) {
    LayerW& L = m->layers[i];
    // Efficient-Conformer: kernel halves after the stride layer (encoder.py:123-128), grouped attention layers
    const int KSi = eff ? (KS >> eff_strides_before(desc, i)) : KS;  // (cnn_module_kernels: // 2 per stride layer passed)
    const bool grouped = eff && ((desc.group_layer_mask >> i) & 1);
    m->layer_ks[i] = KSi;
    m->layer_group[i] = grouped ? desc.group_size : 1;
    const int pbn = grouped ? desc.group_size * d : d;  // pos_bias_u/v are [h][dk*group_size] on grouped layers
    const std::string p = "encoder.encoders." + std::to_string(i) + ".";
    L = LayerW{};
    // (encoder.py:327-336: norm_ff_macaron exists with the macaron half only, norm_conv / norm_final with the conv module only)
    if (go.macaron) LOAD_TRY(ld.norm(p + "norm_ff_macaron", d, &L.ln_mac_g, &L.ln_mac_b));
    LOAD_TRY(ld.norm(p + "norm_mha", d, &L.ln_mha_g, &L.ln_mha_b));
    if (go.use_cnn) LOAD_TRY(ld.norm(p + "norm_conv", d, &L.ln_conv_g, &L.ln_conv_b));
    LOAD_TRY(ld.norm(p + "norm_ff", d, &L.ln_ff_g, &L.ln_ff_b));
    if (go.use_cnn) LOAD_TRY(ld.norm(p + "norm_final", d, &L.ln_fin_g, &L.ln_fin_b));
    L.cm_eps = 1e-5f;
    if (go.use_cnn) LOAD_TRY(ld.conv_module_norm(p + "conv_module.norm", d, &L.ln_cm_g, &L.ln_cm_b, &L.cm_eps));
    if (go.macaron)
      LOAD_TRY(ld.ffn(p + "feed_forward_macaron", d, H, nullptr, nullptr, &L.ffm_w1, &L.ffm_b1, &L.ffm_w2, &L.ffm_b2));
    LOAD_TRY(ld.ffn(p + "feed_forward", d, H, nullptr, nullptr, &L.ff_w1, &L.ff_b1, &L.ff_w2, &L.ff_b2));
    LOAD_TRY(ld.qkv_out(p + "self_attn.", d, nullptr, nullptr, &L.wqkv, &L.bqkv, &L.wo, &L.bo));
    if (go.pos == PPASR_OPT_POS_REL) {
      LOAD_TRY(ld.vec(p + "self_attn.pos_bias_u", pbn, &L.pos_u));
      LOAD_TRY(ld.vec(p + "self_attn.pos_bias_v", pbn, &L.pos_v));
      // (linear_pos has a bias only in GroupedRelPositionMultiHeadedAttention)
      LOAD_TRY(ld.pos_table(p + "self_attn.", d, grouped, m->pe_dev, &L.ptab));
      if (!grouped && d == kD && desc.attention_heads == 4) {  // plain 4 x 64 heads: the layers k_attn_out_glu can run
        void* dt = nullptr;
        LOAD_TRY(m->alloc((size_t)4 * max_len * sizeof(float), &dt));
        launch_pos_dtab(L.ptab, L.pos_u, L.pos_v, static_cast<float*>(dt), max_len, nullptr);
        HIP_TRY(hipGetLastError());
        L.dtab = static_cast<const float*>(dt);
      }
    } else {  // MultiHeadedAttention (abs_pos / no_pos) has no positional parameters: the attention kernel's positional
              // half contracts with zeros (capi_generic.hip)
      L.pos_u = L.pos_v = L.ptab = m->zero_vec;
    }
    if (go.concat_after) {  // concat_linear = Linear(2 size, size) (encoder.py:341-342)
      GETW(wc, p + "concat_linear.weight", (size_t)2 * d * d);
      LOAD_TRY(ld.packed(2 * d, d, [&](int k, int n) { return wc[(size_t)k * d + n]; }, &m->gen_x[i].wcat));
      LOAD_TRY(ld.vec(p + "concat_linear.bias", d, &m->gen_x[i].bcat));
    }
    if (go.use_cnn) {
      const std::string cm = p + "conv_module.";
      LOAD_TRY(ld.conv_pointwise(cm, d, nullptr, nullptr, &L.pw1, &L.pw1_b, &L.glu_pad, &L.pw2, &L.pw2_b));
      LOAD_TRY(ld.taps(cm + "depthwise_conv.weight", d, KSi, &L.dw_w));
      LOAD_TRY(ld.vec(cm + "depthwise_conv.bias", d, &L.dw_b));
    }
  }
  LOAD_TRY(ld.norm("encoder.after_norm", d, &m->head.ln_g, &m->head.ln_b));
  GETW(cw, "ctc.ctc_lo.weight", (size_t)d * V);
  GETW(cb, "ctc.ctc_lo.bias", V);
  m->head.V = V;
  m->head.n_tiles = (V + 31) / 32;
  LOAD_TRY(ld.head(cw, cb, d, V, 32, &m->head.w, &m->head.b));
  if (m->generic) {  // general route: the head as a plain dense layer, vocabulary padded to whole 256-column blocks
    m->gen_vpad = (V + 255) / 256 * 256;
    LOAD_TRY(ld.head(cw, cb, d, V, 256, &m->gen_head_w, &m->gen_head_b));
  }
  return PPASR_OK;
}
