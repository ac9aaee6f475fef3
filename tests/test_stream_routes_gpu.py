"""Which kernels a streaming round launches, pinned per route (tests/golden/stream_routes.json, recorded by
tests/golden/make_stream_routes.py with the library of the commit before the streaming walks were merged).

A stream handle and a session group differ on purpose: consumer-side joins, the Squeezeformer's 16-row weight views, K / V
written straight into the cache and the history moved on the side are handle-only; the Conformer group GLUs its conv
histories per layer, the layered groups and the handles up front.  The oracle tests pass on either route within their
tolerance, so a group that silently took a handle-only route (or a handle that lost one) would go unnoticed; here every
case's second round -- non-empty caches -- must launch exactly the recorded kernels, exactly as often."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_stream_routes", os.path.join(HERE, "golden", "make_stream_routes.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

with open(os.path.join(HERE, "golden", "stream_routes.json")) as _f:
    GOLD = json.load(_f)


def test_the_fixture_holds_every_case():
    assert set(GOLD) == {f"{family}/{case}" for family in mk.FAMILIES for case in mk.CASES}
    assert all(GOLD.values())


@pytest.mark.parametrize("case", list(mk.CASES))
@pytest.mark.parametrize("family", mk.FAMILIES)
def test_a_round_launches_the_recorded_kernels(family, case):
    got = mk.record(family, case)
    want = GOLD[f"{family}/{case}"]
    diff = {k: (want.get(k, 0), got.get(k, 0)) for k in sorted(set(want) | set(got)) if want.get(k, 0) != got.get(k, 0)}
    assert not diff, f"{family}/{case}: kernel -> (recorded, launched) {diff}"
