"""Shared cases of the CTC head tests (a plain module: tests/test_ctc_head_cases_cpu.py, tests/test_ctc_head_vocab_gpu.py).

Small models of every family whose `ctc_lo` can be edited, the column layout of the fused head restated (`owner`), and
the edits that make the head's edges visible: exact ties planted on chosen columns (`plant_tie`, `tie_sets`), a row
that ties as a whole (`uniform_head`) and logits of several hundred nats (`scaled_head`).

The layout, from the header comment of `ctc_head_body` (csrc/ctc_head_kernels.hip): the vocabulary is cut into tiles of
32 columns; workgroup (slice) y of ny and its wave w of 8 walk the tiles w + 8 (y + ny k), k = 0, 1, ...; inside a tile
a lane owns 16 columns, register r of lane half h holding column 8 (r >> 2) + 4 h + (r & 3).  A row's (max, argmax) is
merged in that order: registers and tiles of a lane, the two lane halves, the 8 waves, the ny slices."""
import functools

import numpy as np

from ppasr_amd.utils.synth import (conformer_state_dict, deepspeech2_state_dict, efficient_conformer_state_dict,
                                   squeezeformer_state_dict, synth_features)

FAMILIES = ("conformer", "squeezeformer", "efficient_conformer", "general", "deepspeech2")
WAVES = 8      # waves of a head workgroup
TILE = 32      # vocabulary columns of a tile
MAX_SLICES = 32
# vocabulary sizes of the GPU matrix: on both sides of a tile (32), of a wave's second tile (256), of the row softmax's
# register forms (2048, 5120) and past 256 tiles (8192); 2 is the smallest head
VOCABS = (2, 31, 32, 33, 255, 256, 257, 2048, 2049, 5120, 5121, 8193)
TIE_VOCABS = (257, 4233, 8193)  # tie sets on the unsplit and the split head

# the smallest models the suite builds of each family: one Conformer block (the fused route at width 256, the general
# layer route at width 512 / 8 heads), two Squeezeformer blocks without time reduction, two Efficient-Conformer blocks with
# the stride layer last (the head then sees half the rows the layers started with), one LSTM layer of the smallest rnn_size
_CONF = {
    "conformer": dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=1, cnn_module_kernel=15),
    "general": dict(output_size=512, attention_heads=8, linear_units=2048, num_blocks=1, cnn_module_kernel=15),
    "squeezeformer": dict(encoder_dim=256, output_size=256, attention_heads=4, num_blocks=2, reduce_idx=None, recover_idx=None,
                          feed_forward_expansion_factor=8, cnn_module_kernel=31),
    "efficient_conformer": dict(output_size=256, attention_heads=4, linear_units=2048, num_blocks=2, cnn_module_kernel=15,
                                cnn_module_norm="layer_norm",
                                efficient_conf=dict(stride_layer_idx=[1], stride=[2], group_layer_idx=[0, 1], group_size=3,
                                                    stride_kernel=True)),
    "deepspeech2": dict(num_rnn_layers=1, rnn_size=1024, use_gru=False),
}
_ORACLE_KW = {
    "conformer": dict(num_blocks=1, cnn_module_kernel=15),
    "general": dict(num_blocks=1, cnn_module_kernel=15, attention_heads=8),
    "squeezeformer": dict(num_blocks=2, cnn_module_kernel=31, reduce_idx=None, recover_idx=None),
    "efficient_conformer": dict(num_blocks=2, stride_layer_idx=1, group_layer_idx=(0, 1)),
    "deepspeech2": dict(num_rnn_layers=1, rnn_size=1024, streaming=True, use_gru=False),
}
TIME_REDUCTION = {"conformer": 4, "general": 4, "squeezeformer": 4, "efficient_conformer": 8, "deepspeech2": 4}


def head_key(family):
    return "decoder.ctc_lo" if family == "deepspeech2" else "ctc.ctc_lo"


def head_sd(family, V, seed=7):
    """-> the family's smallest state dict at vocabulary size V (a fresh dict: its `ctc_lo` may be edited)"""
    if family == "conformer":
        return conformer_state_dict(vocab_size=V, num_blocks=1, seed=seed, perturb_norm=True)
    if family == "general":
        return conformer_state_dict(vocab_size=V, num_blocks=1, seed=seed, perturb_norm=True, output_size=512, attention_heads=8)
    if family == "squeezeformer":
        return squeezeformer_state_dict(vocab_size=V, num_blocks=2, seed=seed, perturb_norm=True)
    if family == "efficient_conformer":
        return efficient_conformer_state_dict(vocab_size=V, num_blocks=2, seed=seed, perturb_norm=True, stride_layer_idx=1,
                                              group_layer_idx=(0, 1))
    if family == "deepspeech2":
        return deepspeech2_state_dict(vocab_size=V, num_rnn_layers=1, rnn_size=1024, streaming=True, seed=seed, perturb_norm=True)
    raise ValueError(family)


def oracle_family(family):
    return "conformer" if family == "general" else family


def oracle_kw(family):
    return dict(_ORACLE_KW[family])


def make_model(family, sd):
    """the GPU model of `sd` (imports the model classes late: this module is also read without a GPU)"""
    V = int(np.asarray(sd[head_key(family) + ".bias"]).shape[0])
    if family in ("conformer", "general"):
        from ppasr_amd.model_utils.conformer.model import ConformerModel as M
    elif family == "squeezeformer":
        from ppasr_amd.model_utils.squeezeformer.model import SqueezeformerModel as M
    elif family == "efficient_conformer":
        from ppasr_amd.model_utils.efficient_conformer.model import EfficientConformerModel as M
    else:
        from ppasr_amd.model_utils.deepspeech2.model import DeepSpeech2Model as M
    return M(80, V, streaming=True, encoder_conf=dict(_CONF[family]), state_dict=sd, device="cuda:0")


def inputs(family, B, Tp, seed):
    """features of B utterances that give T' = Tp output frames; the first utterance is full, the others shorter"""
    mul = TIME_REDUCTION[family]
    T = mul * Tp + 3  # ((T - 1) // 2 - 1) // 2 = Tp, or 2 Tp in front of the stride layer
    lens = [T] + [max(mul, T - 9 * mul * (b + 1) // 2) for b in range(B - 1)]
    return synth_features(B, T, lens=lens, seed=seed)


# ---- layout ------------------------------------------------------------------------------------------------------------
def n_tiles(V):
    return (V + TILE - 1) // TILE


def owner(col, V, ny):
    """-> (slice, wave, pass, lane_half, register) of vocabulary column `col` on a fused head of ny slices"""
    assert 0 <= col < V and ny >= 1
    tile = col // TILE
    inside = col % TILE
    return ((tile // WAVES) % ny, tile % WAVES, tile // (WAVES * ny), (inside >> 2) & 1, 4 * (inside >> 3) + (inside & 3))


def column_of(tile, half, reg):
    """the inverse inside a tile: col = 8 (r >> 2) + 4 half + (r & 3)"""
    return tile * TILE + 8 * (reg >> 2) + 4 * half + (reg & 3)


def split_slices(V, rows, forced=8):
    """slices of a split head over `rows` output rows with the feed-forward split forced to `forced`: as many as give
    every wave one tile, at most 32 and at most what fills the chip once, at least the forced split"""
    blocks = (rows + 31) // 32
    return max(forced, min(min((n_tiles(V) + WAVES - 1) // WAVES, MAX_SLICES), 256 // blocks))


# ---- tie sets ----------------------------------------------------------------------------------------------------------
def tie_sets(V, ny):
    """{name: columns} -- every set is planted on a model of its own (`plant_tie`) and must be won by its lowest column.
    The lowest member meets a tied rival at every merge stage that has two non-empty sides at this (V, ny), from both
    directions: rival processed earlier and rival processed later."""
    nt = n_tiles(V)
    last = V - 1
    sets = {}

    def add(name, cols):
        cols = [c for i, c in enumerate(cols) if 0 <= c < V and c not in cols[:i]]
        if len(cols) >= 2:
            sets[name] = cols

    # (a) inside one tile: same register quad, another quad, the other lane half -- in the first tile and in the last whole one
    for tag, base in (("first", 0), ("mid", ((V // TILE) - 1) * TILE if V >= 2 * TILE else -1)):
        if base < 0:
            continue
        add(f"a_{tag}_quad_quad_half", [base + 2, base + 3, base + 10, base + 6])
        add(f"a_{tag}_pair", [base, base + 1])
        # reversal: the lowest member in lane half 1, rivals in lane half 0 (which writes the merged triple)
        add(f"a_{tag}_half1_first", [base + 4, base + 8])
        add(f"a_{tag}_half1_quads", [base + 5, base + 9, base + 17])
    # (b) a later tile of the same wave (the next pass of an unsplit and of this split head) and another wave
    add("b_next_pass_unsplit", [3, 3 + WAVES * TILE])
    add("b_next_pass_split", [3, 3 + WAVES * TILE * ny])
    add("b_next_wave", [9, 9 + TILE])
    add("b_half1_then_later_tile_half0", [4, WAVES * TILE * ny + 8])  # lane half 1 holds the lowest, half 0 meets it late
    # (c) lowest member in tile 7 (wave 7), rival in tile 8 (wave 0's second tile / slice 1): the cross-wave loop starts
    # from wave 0, i.e. from the higher index
    add("c_wave7_vs_wave0_second_tile", [7 * TILE + 5, 8 * TILE + 3])
    add("c_wave7_vs_wave0_three", [7 * TILE + 30, 8 * TILE, 9 * TILE + 1])
    # (d) split head: lowest member in slice 1, rival in slice 0's second pass (tile 8 ny)
    if ny > 1 and nt > WAVES * ny:
        add("d_slice1_vs_slice0_second_pass", [8 * TILE + 7, min(WAVES * ny * TILE + 7, last)])
        add("d_slice0_first_pass_vs_second_pass", [6, min(WAVES * ny * TILE + 7, last)])
    # slices in index order: rival in the last slice that owns a tile
    add("d_slice0_vs_last_tile", [5 * TILE + 1, (nt - 1) * TILE])
    # (e) / (f) the last tile, whose padded columns are -inf: its first column against the last real one and against the
    # wave before it, and tile 0 against both ends of the last tile
    add("e_last_tile_first_vs_last_column", [(nt - 1) * TILE, last])
    add("e_last_tile_vs_previous_wave", [(nt - 2) * TILE + 31, (nt - 1) * TILE, last])
    add("f_tile0_vs_last_tile", [1, (nt - 1) * TILE, last])
    # (g) blank against the last real column
    add("g_blank_vs_last", [0, last])
    return sets


def plant_tie(sd, family, cols, boost):
    """-> a copy of `sd` in which every column of `cols` carries the weight column of min(cols) and the bias
    max(bias) + boost: with boost above the spread of the logits the set is the row maximum of every frame, and its
    members are the same dot product in the same order (bit-identical wherever the columns share a K order)"""
    k = head_key(family)
    sd = dict(sd)
    w = np.array(sd[k + ".weight"], np.float32)
    b = np.array(sd[k + ".bias"], np.float32)
    top = np.float32(b.max() + boost)
    src = w[:, min(cols)].copy()
    for c in cols:
        w[:, c] = src
        b[c] = top
    sd[k + ".weight"], sd[k + ".bias"] = w, b
    return sd


def uniform_head(sd, family):
    """ctc_lo.weight = 0, bias = 0: every frame is a V-way tie"""
    k = head_key(family)
    sd = dict(sd)
    sd[k + ".weight"] = np.zeros_like(np.asarray(sd[k + ".weight"], np.float32))
    sd[k + ".bias"] = np.zeros_like(np.asarray(sd[k + ".bias"], np.float32))
    return sd


def scaled_head(sd, family, factor):
    k = head_key(family)
    sd = dict(sd)
    sd[k + ".weight"] = (np.asarray(sd[k + ".weight"], np.float32) * np.float32(factor)).astype(np.float32)
    return sd


# ---- a numpy model of the head's merge order -----------------------------------------------------------------------------
NONE = 0x7fffffff


def _strict(m2, m, i2, i):
    return m2 > m or (m2 == m and i2 < i)


def _scan_descending(v, cols, tmax, ix):
    for r in range(15, -1, -1):
        if v[r] == tmax:
            ix = cols[r]
    return ix


def _scan_ascending(v, cols, tmax, ix):
    for r in range(16):
        if v[r] == tmax:
            ix = cols[r]
    return ix


RULES = dict(scan=_scan_descending, halves=_strict, waves=_strict, slices=_strict)

# realistic slips, one per copy of "ties go to the lowest index"
MUTATIONS = {
    "waves_le": dict(waves=lambda m2, m, i2, i: m2 >= m),            # `<=` for `<` in the cross-wave merge
    "slices_le": dict(slices=lambda m2, m, i2, i: m2 >= m),          # the same in k_ctc_merge
    "halves_no_index": dict(halves=lambda m2, m, i2, i: m2 > m),     # the `i2 < ix` clause dropped at the lane halves
    "scan_ascending": dict(scan=lambda v, cols, tmax, ix: _scan_ascending(v, cols, tmax, ix)),  # r = 0 .. 15: the last hit stays
    "waves_no_index": dict(waves=lambda m2, m, i2, i: m2 > m),       # (beyond the issue's four: the clause dropped later on)
    "slices_no_index": dict(slices=lambda m2, m, i2, i: m2 > m),
}


def detectable(mutation, V, ny):
    """whether ANY row can show `mutation` at this (V, ny).  A `<=` for `<` shows as soon as its stage merges two sides
    that both hold a real column: two waves from two tiles on, two slices from a ninth tile on a split head.  A dropped
    index clause shows only where the side merged LATER can hold the LOWER column: lane half 1 (columns 4 .. 7) against
    half 0's column 8, and a wave or slice whose second pass (tile 8 ny and up) lies above a later one's first.  The
    in-lane scan needs two columns of one lane.  Below these sizes the stage is correct by construction, whatever its
    rule, and no placement can change that."""
    nt = n_tiles(V)
    if mutation == "scan_ascending":
        return V >= 2
    if mutation == "halves_no_index":
        return V >= 9
    if mutation == "waves_le":
        return nt >= 2
    if mutation == "slices_le":
        return ny > 1 and nt > WAVES
    if mutation == "waves_no_index":
        return nt > WAVES * ny
    if mutation == "slices_no_index":
        return ny > 1 and nt > WAVES * ny
    raise ValueError(mutation)


@functools.lru_cache(maxsize=None)
def _partition(V, ny):
    """{(slice, wave, lane half): {pass: {register: column}}} by `owner`"""
    lanes = {}
    for c in range(V):
        y, w, k, h, r = owner(c, V, ny)
        lanes.setdefault((y, w, h), {}).setdefault(k, {})[r] = c
    return lanes


def head_argmax(row, ny, **rules):
    """argmax of one row of logits the way the fused head finds it (rules: RULES overridden by a mutation): per lane
    over its tiles, the lane halves, the waves in index order, the slices in index order; a lane, wave or slice without
    a column hands on (-inf, NONE)"""
    r = dict(RULES, **rules)
    row = np.asarray(row, np.float32)
    lanes = _partition(row.shape[0], ny)
    ninf = np.float32(-np.inf)
    per_slice = []
    for y in range(ny):
        per_wave = []
        for w in range(WAVES):
            halves = []
            for h in (0, 1):
                mx, ix = ninf, NONE
                passes = lanes.get((y, w, h), {})
                for k in sorted(passes):
                    cols = [passes[k].get(reg, -1) for reg in range(16)]  # (-1: a padded column of the last tile)
                    v = [row[c] if c >= 0 else ninf for c in cols]
                    tmax = max(v)
                    if tmax > mx:
                        ix = r["scan"](v, cols, tmax, ix)
                    mx = max(mx, tmax)
                halves.append((mx, ix))
            (mx, ix), (m2, i2) = halves
            per_wave.append((max(mx, m2), i2 if r["halves"](m2, mx, i2, ix) else ix))
        m, i = per_wave[0]
        for m2, i2 in per_wave[1:]:
            i = i2 if r["waves"](m2, m, i2, i) else i
            m = max(m, m2)
        per_slice.append((m, i))
    m, i = per_slice[0]
    for m2, i2 in per_slice[1:]:
        i = i2 if r["slices"](m2, m, i2, i) else i
        m = max(m, m2)
    return int(i)
