"""The guard-site table of tests/guard_sites.py against the float64 oracle and against the source, without a device.

ISOLATION.  Every recipe at its push setting puts its target site at >= 1.25 x 4 094 and every other listed site at
<= 0.5 x 4 094 (float64 oracle, max |x| over all rows of the GEMM input -- the kernels split padded rows as well); at the
control setting the target lies inside 0.5 x .. 0.9 x 4 094.  The factors are conditions, wide enough that fp32 rounding
cannot move a site across 4 094: without them a site that lost its h3_note would pass the GPU matrix because a
downstream site trips instead.  Every pushed checkpoint gives finite fp32 and float64 results, and the fp32 oracle stays
within a tenth of the fp32 budget of the float64 one (the recipes are benign).

STALENESS.  Every call of h3_split4 / h3_planes_from_tile / unit_std_h3 / ffn_phase_h3 in csrc outside h3.h and the
re-pack kernels is claimed by a SITES entry at its file and line, and every translation unit that owns an event counter
is snapshotted by capi.hip's guard_ctr.  A new site or counter fails here until it has a recipe."""
import numpy as np
import pytest
import torch

import guard_sites as gs
import numerics as nm

MEMO = nm.Memo()


def _run(family, sd, dtype):
    fam, kw = gs.oracle_kwargs(family)
    if dtype == torch.float64:
        orc = nm.oracle64(fam, sd, **kw)
    else:
        orc = type(nm.oracle64(fam, sd, **kw))(sd, **kw)
    orc.taps = {}
    x, lens = gs.batch_features()
    _, logits = orc.get_encoder_out(x, lens, return_logits=True)
    xs, wins = gs.stream_features(1)
    att = cnn = None
    off = 0
    chunks = []
    with torch.no_grad():
        for a, b in wins:  # the stream routes see the same sites chunk by chunk
            out, att, cnn = orc.forward_chunk(xs[:, a:b], off, -16, att, cnn)
            chunks.append(orc.ctc_logits(out))
            off += out.shape[1]
    return logits, chunks, orc.taps


@pytest.mark.parametrize("recipe", gs.RECIPES, ids=gs.case_id)
def test_recipe_isolates_its_site(recipe):
    family, site, layer = recipe
    target = gs.tap_name(site, layer)
    listed = gs.listed_taps(family)
    logits64, chunks64, taps = _run(family, gs.edited(family, site, layer, gs.PUSH), torch.float64)
    assert listed <= set(taps), sorted(listed - set(taps))
    others = max(v for k, v in taps.items() if k in listed and k != target)
    print(f"[guard sites] {gs.case_id(recipe)}: push target {taps[target]:.1f} ({taps[target] / gs.LIMIT:.2f} x limit), "
          f"largest other site {others:.1f} ({others / gs.LIMIT:.3f} x)")
    assert taps[target] >= 1.25 * gs.LIMIT, taps[target]
    assert others <= 0.5 * gs.LIMIT, {k: v for k, v in taps.items() if k in listed and k != target and v > 0.5 * gs.LIMIT}
    assert all(torch.isfinite(t).all() for t in [logits64] + chunks64)
    # fp32 arithmetic on the pushed checkpoint: finite, and as close to float64 as on an ordinary one
    logits32, chunks32, _ = _run(family, gs.edited(family, site, layer, gs.PUSH), torch.float32)
    assert all(torch.isfinite(t).all() for t in [logits32] + chunks32)
    e = max([nm.utt_rel(logits32, logits64)] + [nm.utt_rel(a, b) for a, b in zip(chunks32, chunks64)])
    print(f"[guard sites] {gs.case_id(recipe)}: fp32 oracle vs float64 oracle at the push setting {e:.2e}")
    assert e < nm.F32_BUDGET / 10, e
    # control: inside the range, and the same result (the pushed channel meets a zero weight)
    logits_c, chunks_c, taps_c = _run(family, gs.edited(family, site, layer, gs.CONTROL), torch.float64)
    print(f"[guard sites] {gs.case_id(recipe)}: control target {taps_c[target]:.1f} ({taps_c[target] / gs.LIMIT:.2f} x limit)")
    assert 0.5 * gs.LIMIT <= taps_c[target] <= 0.9 * gs.LIMIT, taps_c[target]
    assert max(v for k, v in taps_c.items() if k in listed and k != target) <= 0.5 * gs.LIMIT
    assert torch.isfinite(logits_c).all()


def test_push_and_control_values_come_from_the_header():
    text = open(gs.os.path.join(gs.CSRC, "h3.h")).read()
    assert "kH3Sa = 16.f" in text and "kH3Sw = 256.f" in text and "kH3Max = 65504.f" in text
    assert gs.LIMIT == 4094.0 and gs.W_LIMIT == 255.875
    assert gs.PUSH >= 1.25 * gs.LIMIT and 0.5 * gs.LIMIT <= gs.CONTROL <= 0.9 * gs.LIMIT


def test_every_call_site_is_claimed_by_a_site():
    claimed = {w for s in gs.SITES for w in s.where}
    found = set(gs.call_sites())
    assert found, "no call site found: the grep is broken"
    listing = "\n".join(f"  {f}:{n} {e}" for f, n, e in sorted(found))
    assert found <= claimed, f"call sites without a SITES entry (and a recipe): {sorted(found - claimed)}\nall call sites:\n{listing}"
    assert claimed <= found, f"SITES cites lines that split nothing (moved?): {sorted(claimed - found)}\nall call sites:\n{listing}"
    # every site has a recipe that some case runs
    assert {s for _, s, _ in gs.RECIPES} == set(gs.SITE)


def test_every_counter_is_snapshotted():
    accessors = gs.counter_accessors()
    listed, n = gs.guard_ctr_list()
    assert len(accessors) >= 5 and n == len(listed) == len(set(listed))
    assert set(accessors) == set(listed), (sorted(accessors), listed)
    # a translation unit with a guarded call site but no accessor could not be snapshotted at all
    assert set(gs.translation_units_with_sites()) <= set(accessors.values())


def test_every_case_names_kernels_for_its_route():
    for family, site, layer, route in gs.CASES:
        kind = gs.FUSED if route == gs.FUSED else gs.SPLIT
        assert gs.SITE[site].kernels.get(kind), (site, route)


# ---- the refusal and rescaling fixtures are what the GPU tests take them for --------------------------------------------
def _benign(family, sd, what):
    """float64 run: every listed site inside 0.9 x 4 094 (an accepted checkpoint must not trip the guard), finite, and the
    fp32 oracle within a FIFTH of the fp32 budget: a weight of 255.5 is 4 000 x the initialiser's bound (1 / 16), one product
    then dominates its sum and the cancellation behind it amplifies every fp32 rounding (the oracle's own: 0.6 - 2.8e-6
    against 0.6 - 0.9e-6 on the plain fixtures), so the elements are chosen where fp32 arithmetic itself still leaves the
    kernels a factor of five"""
    l64, c64, taps = _run(family, sd, torch.float64)
    l32, c32, _ = _run(family, sd, torch.float32)
    worst = max(v for k, v in taps.items() if k in gs.listed_taps(family))
    e = max([nm.utt_rel(l32, l64)] + [nm.utt_rel(a, b) for a, b in zip(c32, c64)])
    print(f"[guard sites] {what}: largest site {worst:.1f} ({worst / gs.LIMIT:.2f} x limit), fp32 vs float64 oracle {e:.2e}")
    assert torch.isfinite(l64).all() and torch.isfinite(l32).all()
    assert worst <= 0.9 * gs.LIMIT, worst
    assert e < nm.F32_BUDGET / 5, e
    return l64


@pytest.mark.parametrize("family,name,element,repacked", gs.WEIGHTS, ids=lambda v: str(v).replace("encoder.", "").replace(" ", ""))
def test_boundary_weight_fixtures_are_benign(family, name, element, repacked):
    sign = -1.0 if sum(element) % 2 else 1.0
    _benign(family, gs.weight_edited(family, name, element, sign * 255.5), f"{family} {name} = {sign * 255.5}")


@pytest.mark.parametrize("family,layer", [("conformer", 1), ("efficient", 0), ("efficient", 2), ("squeezeformer", 1)])
def test_boundary_table_fixtures_are_finite(family, layer):
    for factor in (0.9, 1.05):
        l64, _, _ = _run(family, gs.table_scaled(family, layer, factor), torch.float64)
        l32, _, _ = _run(family, gs.table_scaled(family, layer, factor), torch.float32)
        assert torch.isfinite(l64).all() and torch.isfinite(l32).all()


@pytest.mark.parametrize("k", [11, -9])
def test_balanced_rescaling_leaves_float64_alone(k):
    base, _, _ = _run("conformer", gs.rescaled(0), torch.float64)
    sd = gs.rescaled(k)
    got = _benign("conformer", sd, f"rescaled k={k}")
    assert nm.utt_rel(got, base) < 1e-13  # exact powers of two: the same float64 result up to the order of its roundings
    w1 = max(float(np.abs(v).max()) for n, v in sd.items() if n.endswith("w_1.weight"))
    print(f"[guard sites] rescaled k={k}: max |w_1| {w1:.3g}")
    assert w1 < gs.W_LIMIT
