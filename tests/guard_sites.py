"""Shared table of the fp16 x3 mode's range-guard sites (a plain module, imported by tests/test_gemm_guard_sites_cpu.py and
tests/test_gemm_guard_sites_gpu.py): every GEMM input the mode splits into fp16 pieces at run time (csrc/h3.h: h3_split4 /
h3_planes_from_tile / unit_std_h3 / ffn_phase_h3), the source lines that split it, the routes that reach it and a RECIPE:
an edit of a small seeded state dict under which ordinary synth_features push that input -- and no other listed one -- past
4 094 = 65 504 / 2^4, next to a CONTROL setting of the same edit that stays inside the range.

A recipe pushes ONE channel through a bias and zeroes that channel in the consumer, so the fp32 and float64 results stay
finite and benign (the pushed value meets a zero weight) and the result does not depend on the setting at all.

What a site's tap sees is the oracle's value of the tensor the kernel splits (oracle `taps`).  Where the library folds a
parameter at create time the kernel's operand is NOT the reference's: the Squeezeformer feed-forward modules get their
adaptive scale and bias folded into w_1 / b_1 (capi_squeezeformer.hip, by the loader's `linear`: csrc/weights.h), so the W1 input the kernels split is the
LayerNorm output in front of the module, and an `ada_bias` edit never reaches it -- the recipe goes through that
LayerNorm's bias."""
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppasr_amd", "csrc")

LIMIT = 65504.0 / 16.0  # 4 094: kH3Max / kH3Sa of csrc/h3.h
W_LIMIT = 65504.0 / 256.0  # 255.875: kH3Max / kH3Sw
PUSH, CONTROL = 6000.0, 3000.0  # >= 1.25 x LIMIT; inside 0.5 x .. 0.9 x LIMIT
CHANNEL = 37  # the pushed channel (head 0, column 37 of its 64); hidden unit of the swish recipes: HIDDEN
HIDDEN = 1301
ENTRY_POINTS = ("h3_split4(", "h3_planes_from_tile(", "unit_std_h3(", "ffn_phase_h3(")
# kernels that split WEIGHTS or the positional table when the mode is switched on (refusal, not the run-time guard)
REPACK_KERNELS = ("k_repack_h3", "k_split_rows_h3")

FUSED, SPLIT, STREAM, GROUP = "fused", "split", "stream", "group"
BATCHED = (FUSED, SPLIT)
ALL = (FUSED, SPLIT, STREAM, GROUP)

# where: (csrc file, line, entry point) of every call that splits this input.
# routes: the routes on which a plain (not grouped-attention) layer reaches the site.
# kernels: per route kind, kernel-name prefixes of which at least one must have been launched ("<": a <.., true> form) on
#          a plain layer that is not layer 0; where the layer decides the kernel, expected_kernels() below says which.
Site = namedtuple("Site", "key what where tap routes kernels edit")

F2 = 19  # feature columns behind the 4x front end at 80 mel bins


def _lay(i):
    return f"encoder.encoders.{i}."


def _set(sd, name, index, value):
    a = np.array(sd[name], np.float32, copy=True)
    a[index] = value
    sd[name] = a


def _conv2_in(sd, i, v):
    _set(sd, "encoder.embed.conv.0.bias", CHANNEL, v)
    _set(sd, "encoder.embed.conv.2.weight", (slice(None), CHANNEL), 0.0)


def _proj_in(sd, i, v):
    _set(sd, "encoder.embed.conv.2.bias", CHANNEL, v)
    _set(sd, "encoder.embed.out.0.weight", slice(CHANNEL * F2, (CHANNEL + 1) * F2), 0.0)


def _w1_in(norm, ffn):
    def edit(sd, i, v):
        _set(sd, _lay(i) + norm + ".bias", CHANNEL, v)
        _set(sd, _lay(i) + ffn + ".w_1.weight", CHANNEL, 0.0)
    return edit


def _w2_in(ffn):
    def edit(sd, i, v):
        _set(sd, _lay(i) + ffn + ".w_1.bias", HIDDEN, v)
        _set(sd, _lay(i) + ffn + ".w_2.weight", HIDDEN, 0.0)
    return edit


def _qkv_in(sd, i, v):
    _set(sd, _lay(i) + "norm_mha.bias", CHANNEL, v)
    for n in ("linear_q", "linear_k", "linear_v"):
        _set(sd, _lay(i) + "self_attn." + n + ".weight", CHANNEL, 0.0)


def _head_col():
    return CHANNEL // 64, CHANNEL % 64


def _k_planes(sd, i, v):
    p = _lay(i) + "self_attn."
    _set(sd, p + "linear_k.bias", CHANNEL, v)
    _set(sd, p + "linear_q.weight", (slice(None), CHANNEL), 0.0)  # q + u of that channel = 0: the scores do not move
    _set(sd, p + "linear_q.bias", CHANNEL, 0.0)
    _set(sd, p + "pos_bias_u", _head_col(), 0.0)


def _q_u(sd, i, v):
    p = _lay(i) + "self_attn."
    _set(sd, p + "pos_bias_u", _head_col(), v)
    _set(sd, p + "linear_k.weight", (slice(None), CHANNEL), 0.0)
    _set(sd, p + "linear_k.bias", CHANNEL, 0.0)


def _q_v(sd, i, v):
    p = _lay(i) + "self_attn."
    _set(sd, p + "pos_bias_v", _head_col(), v)
    _set(sd, p + "linear_pos.weight", (slice(None), CHANNEL), 0.0)  # (no bias on a plain layer's linear_pos)


def _out_in(sd, i, v):
    p = _lay(i) + "self_attn."
    _set(sd, p + "linear_v.bias", CHANNEL, v)  # the context is a convex combination of the values: v + O(1)
    _set(sd, p + "linear_out.weight", CHANNEL, 0.0)


def _pw1_in(sd, i, v):
    _set(sd, _lay(i) + "norm_conv.bias", CHANNEL, v)
    _set(sd, _lay(i) + "conv_module.pointwise_conv1.weight", (slice(None), CHANNEL), 0.0)


def _pw2_in(sd, i, v):
    _set(sd, _lay(i) + "conv_module.norm.bias", CHANNEL, v)  # swish(v + O(1)) = v + O(1)
    _set(sd, _lay(i) + "conv_module.pointwise_conv2.weight", (slice(None), CHANNEL), 0.0)


def _ctc_in(sd, i, v):
    _set(sd, "encoder.after_norm.bias", CHANNEL, v)
    _set(sd, "ctc.ctc_lo.weight", CHANNEL, 0.0)


def _sq_w1_in(norm, ffn):
    # The module's input is also its residual: the LayerNorm behind the module squeezes the other channels of that row
    # (finite, and the same in fp32 and float64).  ada_bias would only move b_1 (folded at create time).
    def edit(sd, i, v):
        _set(sd, _lay(i) + norm + ".bias", CHANNEL, v)
        _set(sd, _lay(i) + ffn + ".w_1.weight", CHANNEL, 0.0)
    return edit


CK, SR, FR, HD, SQ = ("conformer_kernels.hip", "split_route_kernels.hip", "front_kernels.hip", "ctc_head_kernels.hip",
                      "squeezeformer_kernels.hip")
S1 = ("k_ffn_qkv_h3", "k_conv_ffn_h3")  # layer 0's own S1 launch / the NEXT tail of the layer in front
FFN_FIN = {FUSED: ("k_conv_ffn_h3", "k_conv_ffn_stride<"), SPLIT: ("k_ffn_part<",)}

SITES = [
    # ---- front end and head: batched calls only (a chunk's front end and head keep fp32 arithmetic) ----
    Site("conv2_in", "conv2 input (ReLU of conv1)", [(FR, 202, "h3_split4(")], "encoder.embed.conv2_in", BATCHED,
         {FUSED: ("k_conv_stage_h3",), SPLIT: ("k_conv_stage_h3",)}, _conv2_in),
    # (an under-filled launch contracts the projection's K = 4 864 over several workgroups per row block in fp32 --
    #  launch_embed -- so the site exists on full launches only)
    Site("proj_in", "input-projection input (ReLU of conv2)", [(FR, 202, "h3_split4(")], "encoder.embed.proj_in", (FUSED,),
         {FUSED: ("k_embed_h3",)}, _proj_in),
    # ---- Conformer / Efficient-Conformer layers ----
    Site("w1_mac", "W1 input of the macaron FFN", [(CK, 105, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")],
         "{l}feed_forward_macaron.w1_in", ALL, {FUSED: S1, SPLIT: ("k_ffn_part<",)}, _w1_in("norm_ff_macaron", "feed_forward_macaron")),
    Site("w2_mac", "swish hidden values in front of W2 (SwishSideH3), macaron FFN",
         [(CK, 105, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")], "{l}feed_forward_macaron.w2_in", ALL,
         {FUSED: S1, SPLIT: ("k_ffn_part<",)}, _w2_in("feed_forward_macaron")),
    Site("w1_fin", "W1 input of the final FFN",
         [(CK, 1030, "ffn_phase_h3("), (CK, 1198, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")], "{l}feed_forward.w1_in", ALL,
         FFN_FIN, _w1_in("norm_ff", "feed_forward")),
    Site("w2_fin", "swish hidden values in front of W2, final FFN",
         [(CK, 1030, "ffn_phase_h3("), (CK, 1198, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")], "{l}feed_forward.w2_in", ALL,
         FFN_FIN, _w2_in("feed_forward")),
    Site("qkv_in", "Q / K / V input", [(CK, 114, "h3_planes_from_tile("), (SR, 215, "unit_std_h3(")], "{l}self_attn.qkv_in",
         ALL, {FUSED: S1, SPLIT: ("k_ln_qkv<",)}, _qkv_in),
    # (the three attention sites exist with the fused attention only: elsewhere K, q + u and q + v stay fp32)
    Site("k_planes", "K planes written by QkStoreTailH3 for the fused attention", [(CK, 67, "h3_split4(")],
         "{l}self_attn.k", (FUSED,), {FUSED: S1}, _k_planes),
    Site("q_u", "q + pos_bias_u in the score contraction", [(CK, 594, "h3_split4(")], "{l}self_attn.q_u", (FUSED,),
         {FUSED: ("k_attn_out_glu_h3",)}, _q_u),
    Site("q_v", "q + pos_bias_v in the score contraction", [(CK, 598, "h3_split4(")], "{l}self_attn.q_v", (FUSED,),
         {FUSED: ("k_attn_out_glu_h3",)}, _q_v),
    Site("out_in", "linear_out input (attention context)", [(CK, 840, "h3_planes_from_tile("), (CK, 330, "unit_std_h3(")],
         "{l}self_attn.out_in", ALL, {FUSED: ("k_attn_out_glu_h3",), SPLIT: ("k_out_glu<",)}, _out_in),
    # (conformer_kernels.hip:352 is k_out_glu<true> with pointwise_conv1 inside: every launch of the <true> form passes
    #  stop_after_ln today -- launch_out_glu -- so that line is claimed here but reached by no route)
    Site("pw1_in", "pointwise_conv1 input",
         [(CK, 876, "h3_planes_from_tile("), (CK, 396, "unit_std_h3("), (CK, 352, "h3_planes_from_tile(")],
         "{l}conv_module.pw1_in", ALL, {FUSED: ("k_attn_out_glu_h3",), SPLIT: ("k_pw1_glu_cols<",)}, _pw1_in),
    Site("pw2_in", "pointwise_conv2 input",
         [(CK, 1007, "h3_planes_from_tile("), (CK, 1170, "unit_std_h3("), (SR, 61, "unit_std_h3(")], "{l}conv_module.pw2_in", ALL,
         {FUSED: ("k_conv_ffn_h3", "k_conv_ffn_stride<"), SPLIT: ("k_conv_pre<", "k_conv_ffn_stride<")}, _pw2_in),
    Site("ctc_in", "CTC head input", [(HD, 49, "h3_planes_from_tile(")], "ctc.in", BATCHED,
         {FUSED: ("k_ctc_head_h3",), SPLIT: ("k_ctc_head_h3",)}, _ctc_in),
    # ---- Squeezeformer (its own translation unit and counter; the split route's slices count in split_route_kernels.hip) ----
    Site("sq_ffn1_w1", "Squeezeformer ffn1 W1 input", [(SQ, 132, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")], "{l}ffn1.w1_in",
         (FUSED, SPLIT, STREAM), {FUSED: ("k_sq_mid_h3",), SPLIT: ("k_ffn_part<",)}, _sq_w1_in("layer_norm1", "ffn1")),
    Site("sq_ffn1_w2", "Squeezeformer ffn1 swish hidden", [(SQ, 132, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")], "{l}ffn1.w2_in",
         (FUSED, SPLIT, STREAM), {FUSED: ("k_sq_mid_h3",), SPLIT: ("k_ffn_part<",)}, _w2_in("ffn1")),
    Site("sq_ffn2_w1", "Squeezeformer ffn2 W1 input", [(SQ, 236, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")], "{l}ffn2.w1_in",
         (FUSED, SPLIT, STREAM), {FUSED: ("k_sq_tail_h3",), SPLIT: ("k_ffn_part<",)}, _sq_w1_in("layer_norm3", "ffn2")),
    Site("sq_ffn2_w2", "Squeezeformer ffn2 swish hidden", [(SQ, 236, "ffn_phase_h3("), (SR, 96, "ffn_phase_h3(")], "{l}ffn2.w2_in",
         (FUSED, SPLIT, STREAM), {FUSED: ("k_sq_tail_h3",), SPLIT: ("k_ffn_part<",)}, _w2_in("ffn2")),
]
SITE = {s.key: s for s in SITES}
LAYER_SITES = ("w1_mac", "w2_mac", "qkv_in", "out_in", "pw1_in", "pw2_in", "w1_fin", "w2_fin")
ATTN_SITES = ("k_planes", "q_u", "q_v")
S1_SITES = ("w1_mac", "w2_mac", "qkv_in", "k_planes")

# ---- the fixtures: 2 blocks (4 for the Efficient-Conformer: grouped 0, grouped + stride 1, plain 2 and 3), small V ----
V = 97


def base_state_dict(family):
    from ppasr_amd.utils.synth import conformer_state_dict, efficient_conformer_state_dict, squeezeformer_state_dict
    if family == "conformer":
        return conformer_state_dict(vocab_size=V, num_blocks=2, seed=411, perturb_norm=True)
    if family == "efficient":
        return efficient_conformer_state_dict(vocab_size=V, num_blocks=4, seed=412, perturb_norm=True, stride_layer_idx=1,
                                              group_layer_idx=(0, 1))
    return squeezeformer_state_dict(vocab_size=V, num_blocks=2, seed=413, perturb_norm=True)


def encoder_conf(family):
    if family == "conformer":
        return dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15)
    if family == "efficient":
        return dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=4, cnn_module_kernel=15,
                    cnn_module_norm="layer_norm",
                    efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3, stride_kernel=True))
    return dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=2, reduce_idx=None, recover_idx=None,
                feed_forward_expansion_factor=8, cnn_module_kernel=31)


def oracle_kwargs(family):
    if family == "conformer":
        return "conformer", dict(num_blocks=2)
    if family == "efficient":
        return "efficient_conformer", dict(num_blocks=4, stride_layer_idx=1, group_layer_idx=(0, 1))
    return "squeezeformer", dict(num_blocks=2, cnn_module_kernel=31, reduce_idx=None, recover_idx=None)


def _routes(family, site, layer):
    """The routes of `site` at `layer` of the family's fixture, read off capi.hip / encode_common.h / capi_stream.hip (encode_impl and its layer_route;
    conformer_stream_layers / sq_stream_layers, one walk for stream handles and session groups): a grouped-attention
    layer has no fused attention (its out-projection and pointwise_conv1 then keep fp32 on the fused route, and the three
    attention sites do not exist); session groups are exercised on the Conformer."""
    routes = [r for r in SITE[site].routes if r != GROUP or family == "conformer"]
    if family == "efficient" and layer in (0, 1) and site in ("out_in", "pw1_in"):
        routes.remove(FUSED)
    return tuple(routes)


def _recipes():
    out = []
    for s in ("conv2_in", "proj_in", "ctc_in"):
        out.append(("conformer", s, 0))
    out += [("conformer", s, 1) for s in LAYER_SITES + ATTN_SITES]
    out += [("conformer", s, 0) for s in S1_SITES]  # layer 0 runs its S1 in k_ffn_qkv_h3, layer 1 in layer 0's NEXT tail
    out += [("efficient", s, 0) for s in LAYER_SITES]  # a grouped-attention layer
    out += [("efficient", s, 1) for s in ("pw2_in", "w1_fin", "w2_fin")]  # the stride layer's own kernel
    out += [("efficient", s, 2) for s in LAYER_SITES + ATTN_SITES]  # behind the stride layer: halved rows, kernel 7
    out += [("squeezeformer", s, 1) for s in ("sq_ffn1_w1", "sq_ffn1_w2", "sq_ffn2_w1", "sq_ffn2_w2")]
    return out


RECIPES = _recipes()  # (family, site key, layer)
CASES = [(f, s, l, r) for f, s, l in RECIPES for r in _routes(f, s, l)]


def case_id(case):
    return "-".join(str(v) for v in case)


def tap_name(site, layer):
    return SITE[site].tap.format(l=_lay(layer))


def edited(family, site, layer, value):
    """The family's base state dict with the site's recipe at `value` (PUSH / CONTROL)."""
    sd = dict(base_state_dict(family))
    SITE[site].edit(sd, layer, np.float32(value))
    return sd


def listed_taps(family):
    """Every tap name of the family's fixture that belongs to a listed site (what `isolation` is checked over)."""
    n_layers = {"conformer": 2, "efficient": 4, "squeezeformer": 2}[family]
    shared = ("conv2_in", "proj_in", "ctc_in")  # the front end and the head serve every family
    keys = [s.key for s in SITES if s.key in shared or s.key.startswith("sq_") == (family == "squeezeformer")]
    return {tap_name(k, i) for k in keys for i in range(n_layers)}


def batch_features():
    from ppasr_amd.utils.synth import synth_features
    return synth_features(3, 203, lens=[203, 150, 64], seed=414)


def stream_features(n=2):
    from ppasr_amd.utils.synth import synth_features
    x, _ = synth_features(n, 64 * 2 + 67, seed=415)
    return x, [(c, min(c + 67, x.shape[1])) for c in range(0, x.shape[1] - 7 + 1, 64)]  # 3 chunks


# ---- staleness: the source against the table -------------------------------------------------------------------------
_GLOBAL = re.compile(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", re.S)


def _blank_comments(text):
    """`text` with every /* */ and // comment blanked, line breaks and offsets kept"""
    def blank(m):
        return re.sub(r"[^\n]", " ", m.group(0))
    return re.sub(r"/\*.*?\*/|//[^\n]*", blank, text, flags=re.S)


def _kernel_bodies(code):
    """-> [(name, start, end)]: every __global__ kernel of `code` (comments blanked) from its `__global__` to the brace
    that closes its body"""
    out = []
    for m in _GLOBAL.finditer(code):
        i = code.index("{", m.end())
        depth = 0
        for j in range(i, len(code)):
            depth += (code[j] == "{") - (code[j] == "}")
            if depth == 0:
                break
        else:
            raise AssertionError(f"unbalanced braces behind kernel {m.group(1)}")
        out.append((m.group(1), m.start(), j))
    return out


def call_sites():
    """-> [(file, line, entry point)] of every call of an entry point in csrc/*.hip and csrc/*.h outside h3.h and outside
    the BODIES of the weight / table re-pack kernels (a helper written behind such a kernel is not excluded)."""
    found = []
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".h")) or fn == "h3.h":
            continue
        code = _blank_comments(open(os.path.join(CSRC, fn)).read())
        repack = [(a, b) for name, a, b in _kernel_bodies(code) if name in REPACK_KERNELS]
        pos = 0
        for no, line in enumerate(code.split("\n"), 1):
            for ep in ENTRY_POINTS:
                at = line.find(ep)
                if at >= 0 and not any(a <= pos + at <= b for a, b in repack):
                    found.append((fn, no, ep))
            pos += len(line) + 1
    return found


def counter_accessors():
    """-> {accessor name: file} of every translation unit's `unsigned int* NAME() { return h3_ovf_counter(); }`."""
    pat = re.compile(r"unsigned int\*\s+(\w+)\s*\(\s*\)\s*\{\s*return h3_ovf_counter\(\);")
    out = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith(".hip"):
            for m in pat.finditer(open(os.path.join(CSRC, fn)).read()):
                out[m.group(1)] = fn
    return out


def translation_units_with_sites():
    """.hip files that call an entry point or include a header that does (each owns a g_h3_ovf)."""
    return sorted({fn for fn, _, _ in call_sites() if fn.endswith(".hip")})


def guard_ctr_list():
    """The accessors capi.hip snapshots as guard_ctr[i] and the size of the array (kGuardN)."""
    text = open(os.path.join(CSRC, "capi.hip")).read()
    names = re.findall(r"guard_ctr\[(\d+)\]\s*=\s*(\w+)\(\);", text)
    n = int(re.search(r"kGuardN\s*=\s*(\d+)", open(os.path.join(CSRC, "capi_internal.h")).read()).group(1))
    return [name for _, name in sorted(names, key=lambda t: int(t[0]))], n


# ---- GPU side ----------------------------------------------------------------------------------------------------------
def make_model(family, sd):
    if family == "conformer":
        from ppasr_amd.model_utils.conformer.model import ConformerModel as M
    elif family == "efficient":
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
    else:
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
    return M(80, int(sd["ctc.ctc_lo.bias"].shape[0]), streaming=True, encoder_conf=encoder_conf(family), state_dict=sd,
             device="cuda:0")


def make_oracle64(family, sd):
    import numerics as nm
    fam, kw = oracle_kwargs(family)
    return nm.oracle64(fam, sd, **kw)


def set_route(model, route):
    """fused: the 8-wave 32-row kernels whatever the grid; every other route: the handle's defaults (a small batch and a
    chunk then take the split route)"""
    model.set_row_block(32 if route == FUSED else -1)
    model.set_ffn_split(0 if route == FUSED else -1)


def expected_kernels(family, site, layer, kind):
    """The kernels that split `site` at `layer` on route kind FUSED / SPLIT (streams and groups run the SPLIT kind), read
    off capi.hip's layer loop (encode_impl; a layer's route: layer_route in encode_common.h): the Efficient-Conformer's stride layer runs pointwise_conv2 and, where its halved rows are not
    split over slices, its final feed-forward module in k_conv_ffn_stride; on the fused route a layer's S1 (macaron module,
    Q/K/V, K planes) runs in its own k_ffn_qkv_h3 launch at layer 0 and behind the stride layer, which has no NEXT tail, and
    in the NEXT tail of the layer in front (k_conv_ffn_h3) everywhere else."""
    stride = family == "efficient" and layer == 1
    if site in ("pw2_in", "w1_fin", "w2_fin"):
        if kind == FUSED:
            return ("k_conv_ffn_stride<",) if stride else ("k_conv_ffn_h3",)
        if site == "pw2_in":
            return ("k_conv_ffn_stride<",) if stride else ("k_conv_pre<",)
        return ("k_ffn_part<", "k_conv_ffn_stride<") if stride else ("k_ffn_part<",)
    if site in S1_SITES and kind == FUSED:
        own = layer == 0 or (family == "efficient" and layer == 2)
        return ("k_ffn_qkv_h3",) if own else ("k_conv_ffn_h3<",)  # <KS, NX = true>: the form with the NEXT tail
    return SITE[site].kernels[kind]


def launched(kernels, prefixes):
    """one of `prefixes` among the launched kernel names; a prefix ending in "<" stands for the <.., true> form"""
    for p in prefixes:
        for k in kernels:
            if k.startswith(p) and (not p.endswith("<") or k.rstrip().endswith("true>")):
                return True
    return False


# ---- refusal and rescaling fixtures ------------------------------------------------------------------------------------
# (family, parameter, element, re-packed on that family?)  -- capi.hip ppasr_set_gemm_mode: the Conformer families re-pack
# every 256-deep weight of a layer, the front end's conv2 and input projection and the head; a Squeezeformer handle
# re-packs its feed-forward weights (w_1 with the adaptive scale folded in: the element's ada_scale is set to 1), the front
# end and the head -- its attention and conv-module weights keep fp32 arithmetic and take any magnitude.
_L1 = "encoder.encoders.1."
WEIGHTS = [(f, n, e, True) for f in ("conformer", "efficient") for n, e in [
    ("encoder.embed.conv.2.weight", (5, 3, 1, 1)), ("encoder.embed.out.0.weight", (3, 5)),
    (_L1 + "self_attn.linear_q.weight", (3, 5)), (_L1 + "self_attn.linear_k.weight", (3, 5)),
    (_L1 + "self_attn.linear_v.weight", (3, 5)), (_L1 + "self_attn.linear_out.weight", (3, 5)),
    (_L1 + "feed_forward_macaron.w_1.weight", (3, 5)), (_L1 + "feed_forward_macaron.w_2.weight", (3, 5)),
    (_L1 + "feed_forward.w_1.weight", (3, 5)), (_L1 + "feed_forward.w_2.weight", (3, 5)),
    (_L1 + "conv_module.pointwise_conv1.weight", (300, 20, 0)), (_L1 + "conv_module.pointwise_conv2.weight", (7, 11, 0)),
    ("ctc.ctc_lo.weight", (200, 50))]]
# (the elements are chosen per fixture where the fp32 ORACLE stays within a fifth of the budget: tests/test_gemm_guard_sites_cpu.py)
WEIGHTS = [(f, n, (5, 3, 0) if (f, n) == ("efficient", _L1 + "conv_module.pointwise_conv2.weight") else e, r)
           for f, n, e, r in WEIGHTS]
WEIGHTS += [("squeezeformer", n, e, r) for n, e, r in [
    ("encoder.embed.dw_conv.weight", (5, 3, 1, 1), True), ("encoder.embed.input_proj.0.weight", (3, 5), True),
    (_L1 + "ffn1.w_1.weight", (3, 5), True), (_L1 + "ffn1.w_2.weight", (3, 5), True),
    (_L1 + "ffn2.w_1.weight", (3, 5), True), (_L1 + "ffn2.w_2.weight", (3, 5), True), ("ctc.ctc_lo.weight", (200, 50), True),
    (_L1 + "self_attn.linear_q.weight", (3, 5), False), (_L1 + "self_attn.linear_k.weight", (3, 5), False),
    (_L1 + "self_attn.linear_v.weight", (3, 5), False), (_L1 + "self_attn.linear_out.weight", (3, 5), False),
    (_L1 + "conv_module.pointwise_conv1.weight", (300, 20, 0), False), (_L1 + "conv_module.pointwise_conv2.weight", (7, 11, 0), False)]]


def weight_edited(family, name, element, value):
    sd = dict(base_state_dict(family))
    _set(sd, name, element, np.float32(value))
    if family == "squeezeformer" and name.endswith(".w_1.weight"):  # the library re-packs diag(ada_scale) w_1
        _set(sd, name.replace("w_1.weight", "ada_scale"), (0, 0, element[0]), 1.0)
    return sd


def table_scaled(family, layer, factor):
    """linear_pos column CHANNEL of `layer` scaled so that the layer's largest projected-table entry of that column is
    factor x 4 094 (float64; the table is pe[0 .. max_len) @ W (+ b))"""
    sd = dict(base_state_dict(family))
    pe = make_oracle64(family, sd).pe[0].numpy()
    name = _lay(layer) + "self_attn.linear_pos.weight"
    w = np.array(sd[name], np.float64)
    col = pe @ w[:, CHANNEL]
    b = sd.get(_lay(layer) + "self_attn.linear_pos.bias")
    b = 0.0 if b is None else float(b[CHANNEL])
    # |s col + b| max = factor x limit: solved for the entry where |col| is largest (|b| << the target)
    t = int(np.abs(col).argmax())
    s = (np.sign(col[t]) * factor * LIMIT - b) / col[t]
    w[:, CHANNEL] *= s
    sd[name] = w.astype(np.float32)
    got = np.abs(pe @ sd[name][:, CHANNEL].astype(np.float64) + b).max()
    assert abs(got / LIMIT - factor) < 1e-3, got
    return sd


def rescaled(k):
    """norm_ff / norm_ff_macaron gamma and beta x 2^-k, the matching w_1 x 2^k (k < 0: the other way round): exact powers of
    two, the float64 and the fp32 results do not move; the mode's activations move towards the subnormal end (k > 0) or
    towards the guard (k < 0) while its weights move the other way."""
    from ppasr_amd.utils.synth import conformer_state_dict
    sd = dict(conformer_state_dict(vocab_size=97, num_blocks=2, seed=11, perturb_norm=True))
    for i in range(2):
        for norm, ffn in (("norm_ff", "feed_forward"), ("norm_ff_macaron", "feed_forward_macaron")):
            for p in (".weight", ".bias"):
                sd[_lay(i) + norm + p] = (sd[_lay(i) + norm + p] * np.float32(2.0 ** -k)).astype(np.float32)
            sd[_lay(i) + ffn + ".w_1.weight"] = (sd[_lay(i) + ffn + ".w_1.weight"] * np.float32(2.0 ** k)).astype(np.float32)
    return sd
