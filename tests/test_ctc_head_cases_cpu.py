"""The cases of tests/head_cases.py can see the bugs they are for (no GPU).

A numpy model of the fused head's merge order (`head_cases.head_argmax`: registers and tiles of a lane, lane halves, waves,
slices, partitioned by `head_cases.owner`) is run on rows that carry a planted tie set.  With the head's own rule every
set is won by its lowest column; with one copy of the rule spoilt (`head_cases.MUTATIONS`) at least one set of every
vocabulary size names another column -- wherever any row could show it at all (`head_cases.detectable`: one tile has
no second wave, eight tiles no second slice, and no placement can change that).

Also here: the fp32 oracle against the float64 oracle on the scaled heads (x8, x32: several hundred nats) stays below
a tenth of F32_BUDGET, so the GPU cases keep the budget unchanged; and columns that share weight column and bias are
one number in both oracles up to the last bits of a CPU matmul's edge columns."""
import numpy as np
import pytest
import torch

import head_cases as hc
import numerics as nm

ALL_V = tuple(sorted(set(hc.VOCABS + hc.TIE_VOCABS)))
SPLIT_ROWS = 33  # rows of the GPU cases' split legs (two row blocks at most: the slice count does not depend on it)


def _slice_counts(V):
    return sorted({1, hc.split_slices(V, SPLIT_ROWS)})


def _row(V, cols, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    row = rng.standard_normal(V).astype(np.float32)
    row[cols] = np.float32(row.max() + 5.0)
    return row


def test_owner_is_a_partition_and_matches_the_walk():
    """every column has one owner; a wave's tiles come in passes of 8 ny; the split of a tile into lane halves and
    registers inverts `column_of`"""
    for V in ALL_V:
        for ny in _slice_counts(V):
            seen = set()
            for c in range(V):
                y, w, k, h, r = hc.owner(c, V, ny)
                assert 0 <= y < ny and 0 <= w < 8 and h in (0, 1) and 0 <= r < 16
                tile = w + 8 * (y + ny * k)  # the tile loop of the head: wave + 8 y, step 8 ny
                assert tile == c // 32 and hc.column_of(tile, h, r) == c
                seen.add((y, w, k, h, r))
            assert len(seen) == V


def test_split_slice_counts():
    """the slice counts the GPU cases rely on: empty slices at V = 2 / 33, one tile per wave from 2049 on, the cap of 32
    with a second pass at 8193"""
    got = {V: hc.split_slices(V, SPLIT_ROWS) for V in ALL_V}
    assert got[2] == got[33] == got[257] == got[2048] == 8
    assert (got[2049], got[4233], got[5120], got[5121], got[8193]) == (9, 17, 20, 21, 32)
    assert hc.n_tiles(8193) > 8 * got[8193] and hc.n_tiles(5121) <= 8 * got[5121]


@pytest.mark.parametrize("V", ALL_V)
def test_tie_sets_catch_every_mutation(V):
    for ny in _slice_counts(V):
        sets = hc.tie_sets(V, ny)
        assert sets, (V, ny)
        rows = {name: _row(V, cols, 31 * V + i) for i, (name, cols) in enumerate(sorted(sets.items()))}
        for name, cols in sets.items():
            assert hc.head_argmax(rows[name], ny) == min(cols) == int(np.argmax(rows[name])), (V, ny, name)
        for mut, rules in hc.MUTATIONS.items():
            caught = [name for name, cols in sets.items() if hc.head_argmax(rows[name], ny, **rules) != min(cols)]
            if hc.detectable(mut, V, ny):
                assert caught, f"V={V} ny={ny}: no tie set distinguishes {mut}"
            else:
                assert not caught, (V, ny, mut, caught)  # (`detectable` says no row can: checked on these)


def test_placements_sit_where_they_claim():
    """the named placements by `owner`: (a) one lane / two lanes of a tile, (b) passes and waves, (c) wave 7 against wave
    0's second tile, (d) slice 1 against slice 0's second pass, (e) - (g) the last tile"""
    V, ny = 8193, hc.split_slices(8193, SPLIT_ROWS)
    s = hc.tie_sets(V, ny)
    own = lambda c, n=ny: hc.owner(c, V, n)
    a = [own(c) for c in s["a_first_quad_quad_half"]]
    assert a[0][:4] == a[1][:4] == a[2][:4] and a[0][4] // 4 == a[1][4] // 4 != a[2][4] // 4 and a[3][3] == 1
    lo, hi = [own(c) for c in s["a_first_half1_first"]]
    assert (lo[3], hi[3]) == (1, 0)
    lo, hi = [own(c, 1) for c in s["b_next_pass_unsplit"]]
    assert lo[:2] == hi[:2] and (lo[2], hi[2]) == (0, 1)
    lo, hi = [own(c) for c in s["d_slice0_first_pass_vs_second_pass"]]
    assert lo[:2] == hi[:2] == (0, 0) and (lo[2], hi[2]) == (0, 1)
    lo, hi = [hc.owner(c, 4233, 2) for c in hc.tie_sets(4233, 2)["b_next_pass_split"]]
    assert lo[:2] == hi[:2] and (lo[2], hi[2]) == (0, 1)
    lo, hi = [own(c, 1) for c in s["c_wave7_vs_wave0_second_tile"]]
    assert (lo[1], lo[2], hi[1], hi[2]) == (7, 0, 0, 1)
    lo, hi = [own(c) for c in s["d_slice1_vs_slice0_second_pass"]]
    assert (lo[0], lo[2], hi[0], hi[2]) == (1, 0, 0, 1)
    assert s["g_blank_vs_last"] == [0, V - 1] and s["e_last_tile_vs_previous_wave"][1] // 32 == hc.n_tiles(V) - 1
    # V = 33: the last tile holds one real column
    assert hc.tie_sets(33, 8)["g_blank_vs_last"] == [0, 32] and hc.owner(32, 33, 8)[:2] == (0, 1)


# ---- the oracles on the edited heads ----------------------------------------------------------------------------------
def _oracles(sd):
    from oracle.conformer_oracle import ConformerOracle
    kw = hc.oracle_kw("conformer")
    return ConformerOracle(sd, dtype=torch.float32, **kw), nm.oracle64("conformer", sd, **kw)


@pytest.mark.parametrize("factor", [1, 8, 32])
def test_scaled_heads_keep_the_budget_margin(factor):
    """fp32 oracle vs float64 oracle, one-block Conformer, V = 257 (measured: x1 max |logit| 28, x8 228, x32 912; errors
    6.7e-7 .. 9.0e-7 throughout -- both metrics are relative to the logit scale)"""
    sd = hc.scaled_head(hc.head_sd("conformer", 257), "conformer", factor)
    x, lens = hc.inputs("conformer", 3, 11, 5)
    o32, o64 = _oracles(sd)
    p32, l32 = o32.get_encoder_out(x, lens, return_logits=True)
    _, l64 = o64.get_encoder_out(x, lens, return_logits=True)
    e_l, e_p = nm.utt_rel(l32, l64), nm.logprob_err(p32, l64)
    print(f"[head] cpu x{factor}: max |logit| {float(l64.abs().max()):.0f} utt_rel {e_l:.2e} logprob_err {e_p:.2e}")
    assert e_l < nm.F32_BUDGET / 10 and e_p < nm.F32_BUDGET / 10, (factor, e_l, e_p)
    assert float(l64.abs().max()) > 30 * factor / 2  # the head really is that large


@pytest.mark.parametrize("V", [300, 8500])
def test_duplicated_columns_are_one_number_in_the_oracles(V):
    """Planted columns in the float64 and the fp32 oracle: bit-equal wherever the CPU's matmul treats the columns alike
    (every set, on the CPUs this was written on), and never more than last bits apart -- some CPUs run the last columns
    of an odd width through another code path (seen: 3.6e-15 at float64 logits of 30).  Where they are bit-equal the
    oracle's own argmax is the set's lowest column; the GPU tests assert against the planted set, not against this."""
    sd0 = hc.head_sd("conformer", V)
    x, lens = hc.inputs("conformer", 2, 9, 6)
    boost = 2 * float(_oracles(sd0)[1].get_encoder_out(x, lens, return_logits=True)[1].abs().max())
    sets = dict(hc.tie_sets(V, 1))
    sets.update(hc.tie_sets(V, hc.split_slices(V, SPLIT_ROWS)))
    apart = []
    for name, cols in sorted(sets.items()):
        for o, eps in zip(_oracles(hc.plant_tie(sd0, "conformer", cols, boost)), (2.0 ** -23, 2.0 ** -52)):
            lg = o.get_encoder_out(x, lens, return_logits=True)[1].numpy()
            assert (lg[..., cols].max(-1) == lg.max(-1)).all(), (V, name)
            off = float(np.abs(lg[..., cols] - lg[..., cols[:1]]).max())
            assert off <= 8 * eps * float(np.abs(lg).max()), (V, name, off)
            if off:
                apart.append((name, off))
            else:
                assert (lg.argmax(-1) == min(cols)).all(), (V, name)
    print(f"[head] cpu V={V}: {len(sets)} tie sets, planted columns not bit-equal in an oracle: {apart or 'none'}")
