// capi_rescore.hip -- C-ABI of attention rescoring: the rescorer object (the checkpoint's decoder.* weights through the
// one loader of weights.h) and ppasr_rescore (rescore_kernels.hip).
#include "capi_internal.h"
#include "rescore_kernels.h"
#include "rescorer_handle.h"

namespace {

constexpr size_t al64(size_t n) { return (n + 63) / 64 * 64; }

// workspace offsets in floats
struct RescoreLayout {
  size_t x, qkv, ctx, qc, kv, logp, counts, tile_info, row_info, hyp_row0, total;
  size_t stat, total_loss;  // ppasr_rescorer_loss: the row statistics behind everything ppasr_rescore uses
};
RescoreLayout rescore_layout(const ppasr_rescorer_s* r, const RescoreDims& d) {
  RescoreLayout l;
  const size_t rows = d.rows_cap();
  size_t o = 0;
  auto take = [&](size_t n) {
    const size_t at = o;
    o += al64(n);
    return at;
  };
  l.x = take(rows * kD);
  l.qkv = take(rows * 768);
  l.ctx = take(rows * kD);
  l.qc = take(rows * kD);
  l.kv = take((size_t)d.B * d.Tp * 512 * (r->desc.num_blocks + r->desc.r_num_blocks));
  l.logp = take(rows);
  l.counts = take(64);
  l.tile_info = take(d.tiles_cap());
  l.row_info = take(2 * rows);
  l.hyp_row0 = take((size_t)2 * d.B * d.nbest);
  l.total = o;
  l.stat = take(2 * rows);
  l.total_loss = o;
  return l;
}

RescoreBufs rescore_bufs(float* ws, const RescoreLayout& l) {
  RescoreBufs bf;
  bf.x = ws + l.x;
  bf.qkv = ws + l.qkv;
  bf.ctx = ws + l.ctx;
  bf.qc = ws + l.qc;
  bf.kv = ws + l.kv;
  bf.logp = ws + l.logp;
  bf.tab.counts = reinterpret_cast<int*>(ws + l.counts);
  bf.tab.tile_info = reinterpret_cast<int*>(ws + l.tile_info);
  bf.tab.row_info = reinterpret_cast<int2*>(ws + l.row_info);
  bf.tab.hyp_row0 = reinterpret_cast<int*>(ws + l.hyp_row0);
  return bf;
}

ppasr_status load_side(ppasr_rescorer_s* r, Loader& ld, const std::string& p, int nblk, DecSideW* side,
                       std::vector<std::vector<float>>* kv_w, std::vector<float>* kv_b) {
  const int d = kD, V = r->desc.vocab_size, U = r->desc.linear_units;
  LOAD_TRY(ld.vec(p + ".embed.0.weight", (size_t)V * d, &side->embed));
  LOAD_TRY(ld.norm(p + ".after_norm", d, &side->ang, &side->anb));
  GETW(ow, p + ".output_layer.weight", (size_t)d * V);
  GETW(ob, p + ".output_layer.bias", V);
  LOAD_TRY(ld.head(ow, ob, d, V, 256, &side->wout, &side->bout));
  std::vector<DecLayerW> layers(nblk);
  for (int i = 0; i < nblk; ++i) {
    DecLayerW& lw = layers[i];
    const std::string lp = p + ".decoders." + std::to_string(i);
    LOAD_TRY(ld.norm(lp + ".norm1", d, &lw.n1g, &lw.n1b));
    LOAD_TRY(ld.norm(lp + ".norm2", d, &lw.n2g, &lw.n2b));
    LOAD_TRY(ld.norm(lp + ".norm3", d, &lw.n3g, &lw.n3b));
    LOAD_TRY(ld.qkv_out(lp + ".self_attn.", d, nullptr, nullptr, &lw.wqkv, &lw.bqkv, &lw.wo, &lw.bo));
    GETW(qw, lp + ".src_attn.linear_q.weight", (size_t)d * d);
    GETW(qb, lp + ".src_attn.linear_q.bias", d);
    GETW(ow2, lp + ".src_attn.linear_out.weight", (size_t)d * d);
    GETW(ob2, lp + ".src_attn.linear_out.bias", d);
    LOAD_TRY(ld.linear([=](int k, int n) { return qw[(size_t)k * d + n]; }, qb, d, d, nullptr, nullptr, &lw.wq2, &lw.bq2));
    LOAD_TRY(ld.linear([=](int k, int n) { return ow2[(size_t)k * d + n]; }, ob2, d, d, nullptr, nullptr, &lw.wo2, &lw.bo2));
    LOAD_TRY(ld.ffn(lp + ".feed_forward", d, U, nullptr, nullptr, &lw.w1, &lw.b1, &lw.w2, &lw.b2));
    // the layer's slot of the one key / value matrix: [k | v], each [256][256]
    const char* kvn[2] = {"linear_k", "linear_v"};
    std::vector<float> w((size_t)d * 512);
    for (int j = 0; j < 2; ++j) {
      GETW(wj, lp + ".src_attn." + kvn[j] + ".weight", (size_t)d * d);
      GETW(bj, lp + ".src_attn." + kvn[j] + ".bias", d);
      for (int k = 0; k < d; ++k) std::memcpy(&w[(size_t)k * 512 + j * d], wj + (size_t)k * d, d * sizeof(float));
      kv_b->insert(kv_b->end(), bj, bj + d);
    }
    kv_w->push_back(std::move(w));
  }
  side->nblk = nblk;
  side->layers = nullptr;
  if (nblk > 0) {
    const void* dev = nullptr;
    LOAD_TRY(r->store.upload_bytes(layers.data(), layers.size() * sizeof(DecLayerW), &dev));
    side->layers = static_cast<const DecLayerW*>(dev);
  }
  return PPASR_OK;
}

}  // namespace

extern "C" {

ppasr_status ppasr_rescorer_create(const ppasr_rescorer_desc* desc, const ppasr_weight_blob* blobs, int n_blobs,
                                   ppasr_rescorer* out) {
  if (!desc || !blobs || !out || n_blobs <= 0) return fail(PPASR_EINVAL, "null argument");
  *out = nullptr;
  if (desc->d_model != kD || desc->attention_heads != 4)
    return fail(PPASR_EUNSUPPORTED, "attention decoder: built for d_model 256 with 4 heads of 64");
  if (desc->linear_units < 256 || desc->linear_units % 256 != 0 || desc->linear_units > 4096)
    return fail(PPASR_EUNSUPPORTED, "attention decoder: linear_units must be a multiple of 256 up to 4096");
  if (desc->num_blocks < 1 || desc->num_blocks > 6 || desc->r_num_blocks < 0 || desc->r_num_blocks > 6)
    return fail(PPASR_EUNSUPPORTED, "attention decoder: num_blocks 1..6, r_num_blocks 0..6");
  if (desc->vocab_size < 2) return fail(PPASR_EUNSUPPORTED, "attention decoder: vocab_size >= 2");
  if (desc->max_len < 0) return fail(PPASR_EINVAL, "max_len < 0");
  std::unique_ptr<ppasr_rescorer_s> r(new ppasr_rescorer_s);
  r->desc = *desc;
  const BlobMap sd = blob_map(blobs, n_blobs);
  // the reference's constructor options this decoder is not built for leave their own parameters in the checkpoint
  if (sd.find("decoder.left_decoder.decoders.0.concat_linear1.weight") != sd.end())
    return fail(PPASR_EUNSUPPORTED, "attention decoder: concat_after = True is not built");
  r->store.desc = ppasr_model_desc{};
  r->store.desc.output_size = kD;
  r->store.desc.max_len = desc->max_len;
  Loader ld{&r->store, sd, {}};
  std::vector<std::vector<float>> kv_w;
  std::vector<float> kv_b;
  LOAD_TRY(load_side(r.get(), ld, "decoder.left_decoder", desc->num_blocks, &r->W.side[0], &kv_w, &kv_b));
  LOAD_TRY(load_side(r.get(), ld, "decoder.right_decoder", desc->r_num_blocks, &r->W.side[1], &kv_w, &kv_b));
  const int slots = desc->num_blocks + desc->r_num_blocks;
  LOAD_TRY(ld.packed(kD, 512 * slots, [&](int k, int n) { return kv_w[n / 512][(size_t)k * 512 + (n % 512)]; }, &r->W.wkv));
  LOAD_TRY(ld.up(kv_b, &r->W.bkv));
  LOAD_TRY(ld.pe_table(&r->W.pe));
  r->desc.max_len = r->store.desc.max_len;
  r->W.V = desc->vocab_size;
  r->W.Vp = (desc->vocab_size + 255) / 256 * 256;
  r->W.U = desc->linear_units;
  r->W.n_left = desc->num_blocks;
  HIP_TRY(configure_rescore_kernels());
  *out = r.release();
  return PPASR_OK;
}

ppasr_status ppasr_rescorer_destroy(ppasr_rescorer r) {
  delete r;
  return PPASR_OK;
}

size_t ppasr_rescorer_workspace_bytes(ppasr_rescorer r, int B, int Tp, int nbest, int max_tokens) {
  if (!r || B <= 0 || Tp <= 0 || nbest <= 0 || max_tokens < 0 || max_tokens + 1 > kRescoreMaxRows) return 0;
  return rescore_layout(r, RescoreDims{B, Tp, nbest, max_tokens, 2}).total * sizeof(float);
}

ppasr_status ppasr_rescore(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp, const int32_t* tokens,
                           const int32_t* lens, const double* ctc_scores, int nbest, int max_tokens, double ctc_weight,
                           double reverse_weight, double* att_scores, double* r_att_scores, double* total_scores,
                           int32_t* best, float* token_logp, float* logits_tap, void* workspace, size_t workspace_bytes,
                           void* stream) {
  if (!r) return fail(PPASR_EINVAL, "null rescorer");
  if (!memory || !lens || !ctc_scores || !att_scores || !r_att_scores || !total_scores || !best || !workspace)
    return fail(PPASR_EINVAL, "null argument");
  if (B <= 0 || Tp <= 0 || nbest <= 0 || max_tokens < 0 || (max_tokens > 0 && !tokens)) return fail(PPASR_EINVAL, "bad shape");
  if (!(reverse_weight >= 0.0 && reverse_weight <= 1.0)) return fail(PPASR_EINVAL, "reverse_weight outside [0, 1]");
  if (reverse_weight > 0.0 && r->desc.r_num_blocks == 0)
    return fail(PPASR_EINVAL, "reverse_weight > 0 needs a right decoder (r_num_blocks is 0)");
  if (max_tokens + 1 > r->desc.max_len)
    return fail(PPASR_EUNSUPPORTED, "max_tokens + 1 exceeds the positional table (max_len)");
  if (max_tokens + 1 > kRescoreMaxRows)
    return fail(PPASR_EUNSUPPORTED, "max_tokens + 1 exceeds the 256 rows per hypothesis the kernels are built for");
  if ((size_t)B * nbest > 65535u * 16u || (size_t)B * Tp > (size_t)1 << 24) return fail(PPASR_EUNSUPPORTED, "batch too large");
  if (workspace_bytes < ppasr_rescorer_workspace_bytes(r, B, Tp, nbest, max_tokens))
    return fail(PPASR_ENOSPACE, "workspace too small (ppasr_rescorer_workspace_bytes)");
  const RescoreDims d{B, Tp, nbest, max_tokens, reverse_weight > 0.0 ? 2 : 1};
  const RescoreLayout l = rescore_layout(r, RescoreDims{B, Tp, nbest, max_tokens, 2});
  float* ws = static_cast<float*>(workspace);
  const RescoreBufs bf = rescore_bufs(ws, l);
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIP_TRY(configure_rescore_kernels());  // (a per-device attribute: the call may run on another device than create did)
  if (logits_tap)
    HIP_TRY(hipMemsetAsync(logits_tap, 0, (size_t)B * nbest * 2 * (max_tokens + 1) * r->desc.vocab_size * sizeof(float), st));
  launch_rescore(r->W, d, bf, memory, out_lens, tokens, lens, ctc_scores, ctc_weight, reverse_weight, att_scores, r_att_scores,
                 total_scores, best, token_logp, logits_tap, nullptr, st);
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

size_t ppasr_rescorer_loss_workspace_bytes(ppasr_rescorer r, int B, int Tp, int max_tokens) {
  if (!r || B <= 0 || Tp <= 0 || max_tokens < 0 || max_tokens + 1 > kRescoreMaxRows) return 0;
  return rescore_layout(r, RescoreDims{B, Tp, 1, max_tokens, 2}).total_loss * sizeof(float);
}

ppasr_status ppasr_rescorer_loss(ppasr_rescorer r, const float* memory, const int32_t* out_lens, int B, int Tp,
                                 const int32_t* labels, const int32_t* label_lens, int max_tokens, double lsm_weight,
                                 double reverse_weight, double* att_kl, double* r_att_kl, int32_t* rows, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (!r) return fail(PPASR_EINVAL, "null rescorer");
  if (!memory || !label_lens || !att_kl || !r_att_kl || !rows || !workspace) return fail(PPASR_EINVAL, "null argument");
  if (B <= 0 || Tp <= 0 || max_tokens < 0 || (max_tokens > 0 && !labels)) return fail(PPASR_EINVAL, "bad shape");
  if (!(lsm_weight >= 0.0 && lsm_weight < 1.0)) return fail(PPASR_EINVAL, "lsm_weight outside [0, 1)");
  if (!(reverse_weight >= 0.0 && reverse_weight <= 1.0)) return fail(PPASR_EINVAL, "reverse_weight outside [0, 1]");
  if (reverse_weight > 0.0 && r->desc.r_num_blocks == 0)
    return fail(PPASR_EINVAL, "reverse_weight > 0 needs a right decoder (r_num_blocks is 0)");
  if (max_tokens + 1 > r->desc.max_len)
    return fail(PPASR_EUNSUPPORTED, "max_tokens + 1 exceeds the positional table (max_len)");
  if (max_tokens + 1 > kRescoreMaxRows)
    return fail(PPASR_EUNSUPPORTED, "max_tokens + 1 exceeds the 256 rows per label the kernels are built for");
  if ((size_t)B > 65535u * 16u || (size_t)B * Tp > (size_t)1 << 24) return fail(PPASR_EUNSUPPORTED, "batch too large");
  if (workspace_bytes < ppasr_rescorer_loss_workspace_bytes(r, B, Tp, max_tokens))
    return fail(PPASR_ENOSPACE, "workspace too small (ppasr_rescorer_loss_workspace_bytes)");
  const RescoreDims d{B, Tp, 1, max_tokens, reverse_weight > 0.0 ? 2 : 1};
  const RescoreLayout l = rescore_layout(r, RescoreDims{B, Tp, 1, max_tokens, 2});
  float* ws = static_cast<float*>(workspace);
  const RescoreBufs bf = rescore_bufs(ws, l);
  const RescoreLoss loss{lsm_weight, ws + l.stat, att_kl, r_att_kl, rows};
  HIP_TRY(configure_rescore_kernels());
  launch_rescore(r->W, d, bf, memory, out_lens, labels, label_lens, nullptr, 0.0, reverse_weight, nullptr, nullptr, nullptr,
                 nullptr, nullptr, nullptr, &loss, static_cast<hipStream_t>(stream));
  HIP_TRY(hipGetLastError());
  return PPASR_OK;
}

}  // extern "C"
