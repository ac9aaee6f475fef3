"""Which kernels an offline encode launches, pinned per route (tests/golden/encode_routes.json, recorded by
tests/golden/make_encode_routes.py with the library of the commit before the four encode walks came to share one frame:
csrc/encode_common.h).

The walks choose a route per call and per layer -- split or fused feed-forward modules, 32-row, 16-row or 16-wave blocks,
fused or two-kernel attention, NEXT tails, the fp16 x3 views, block tables for ragged batches, three front ends -- from the
batch shape and the handle's settings.  The oracle tests pass on every route within their tolerance, so a call that silently
took a neighbouring route would go unnoticed; here every case must launch exactly the recorded kernels, exactly as often.
(Copies and clears are not kernels: tests/test_buffer_contents_gpu.py covers them.)"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_encode_routes", os.path.join(HERE, "golden", "make_encode_routes.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

with open(os.path.join(HERE, "golden", "encode_routes.json")) as _f:
    GOLD = json.load(_f)


def test_the_fixture_holds_every_case():
    assert set(GOLD) == {f"{name}/{case}" for name, case in mk.cases_of()}
    assert all(GOLD.values())


@pytest.mark.parametrize("name,case", mk.cases_of())
def test_an_encode_launches_the_recorded_kernels(name, case):
    got = mk.record(name, case)
    want = GOLD[f"{name}/{case}"]
    diff = {k: (want.get(k, 0), got.get(k, 0)) for k in sorted(set(want) | set(got)) if want.get(k, 0) != got.get(k, 0)}
    assert not diff, f"{name}/{case}: kernel -> (recorded, launched) {diff}"
