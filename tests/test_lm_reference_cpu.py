"""CPU: the n-gram scorer against an independent walk (tests/lm_cases.py).  The library's host scorer equals a plain
back-off walk over the ARPA file's n-grams on every window of a zoo of models (orders 1 .. 6, tables of 16 slots and up,
.klm renderings) -- exact equality, the sums are reproducible.  The zoo is held to what it is for: every (order, deciding
level), summed back-offs, absent contexts, and -- on the tables the LIBRARY built (ppasr_lm_debug_table) -- every path of
the device probe lm_probe_many: homes in the last slot, the wrap copy, clusters longer than two slots, clusters through the
table's end.  Subtly wrong variants of the factorised form (lm_cases.MUTANTS) must each get a window wrong."""
import ctypes

import numpy as np
import pytest

import lm_cases as L
from ppasr_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _host(lib, spec, tmp_path):
    return L.load(lib, L.write_model(spec, tmp_path), L.vocab_of(spec), host_only=True)


@pytest.mark.parametrize("spec", L.ZOO, ids=lambda s: s.name)
def test_host_scorer_equals_the_reference(lib, tmp_path, spec):
    c = L.case(spec)
    h = _host(lib, spec, tmp_path)
    try:
        assert lib.ppasr_lm_order(h) == spec.order
        assert lib.ppasr_lm_ngram_count(h) == len(c.grams)
        wins = L.handle_windows(lib, h, c)
        if spec.klm is None:
            assert np.array_equal(wins, c.windows)       # the ARPA reader numbers the words as they first appear
        got = L.host_scores(lib, h, wins)
        bad = np.flatnonzero(~L.same(got, c.score))
        assert bad.size == 0, (spec.name, c.windows[bad[0]].tolist(), got[bad[0]], c.score[bad[0]], int(c.level[bad[0]]))
        assert (c.score == L.OOV_SCORE).any() and (c.score > L.OOV_SCORE).any()
    finally:
        lib.ppasr_lm_destroy(h)


def test_the_windows_cover_every_level_of_the_walk():
    """Over the ARPA models of the zoo: every (order, deciding level) occurs; for every order >= 3 a window sums two or
    more back-offs, and a window has an absent context above a present one (the walk consults the contexts of
    order - 1 .. deciding level words; the longer one is not in the model, a shorter one adds its back-off)."""
    levels, two_backoffs, absent_above_present = set(), set(), set()
    for spec in L.ARPA_ZOO:
        c = L.case(spec)
        levels |= {(spec.order, int(n)) for n in np.unique(c.level)}
        for n, used in set(zip(c.level.tolist(), c.used)):
            if len(used) >= 2:
                two_backoffs.add(spec.order)
            if n >= 1 and any(m not in used and any(m2 in used for m2 in range(n, m)) for m in range(n, spec.order)):
                absent_above_present.add(spec.order)
    assert {(o, n) for o in range(1, 7) for n in range(0, o + 1)} <= levels
    assert {3, 4, 5, 6} <= two_backoffs
    assert {3, 4, 5, 6} <= absent_above_present


@pytest.mark.parametrize("spec", L.ZOO, ids=lambda s: s.name)
def test_debug_table_is_the_layout_the_probe_relies_on(lib, tmp_path, spec):
    h = _host(lib, spec, tmp_path)
    try:
        tab = L.table_of(lib, h)
        cap = tab.mask + 1
        assert len(tab.key) == tab.mask + 2 and cap >= 16 and cap & (cap - 1) == 0
        assert (tab.key[-1], tab.prob[-1].tobytes(), tab.backoff[-1].tobytes()) == (
            tab.key[0], tab.prob[0].tobytes(), tab.backoff[0].tobytes())              # the wrap slot
        n = int((tab.key[:cap] != 0).sum())
        assert n == lib.ppasr_lm_ngram_count(h) == len(L.case(spec).grams)
        assert 3 * n <= cap
        assert len(np.unique(tab.key[:cap][tab.key[:cap] != 0])) == n
        assert tab.kenlm_keys == (spec.klm == "probing")
    finally:
        lib.ppasr_lm_destroy(h)
    assert lib.ppasr_lm_debug_table(None, None, 0) == -1


def test_the_zoo_reaches_every_path_of_the_probe(lib, tmp_path):
    """On the library's own tables: the keys the three forms look up for the zoo's windows take every path of
    lm_probe_many -- over the lm_key tables (ARPA, trie binaries) and, separately, over the KenLM-keyed ones."""
    classes = {False: set(), True: set()}
    reached_by = {}
    for spec in L.ZOO:
        c = L.case(spec)
        h = _host(lib, spec, tmp_path)
        try:
            tab = L.table_of(lib, h)
            ctx_keys, pair_keys = L.all_keys(tab, spec.order, L.handle_windows(lib, h, c))
        finally:
            lib.ppasr_lm_destroy(h)
        cl = L.classify(tab, np.concatenate(ctx_keys + pair_keys))
        classes[tab.kenlm_keys] |= cl
        for name, ok in L.probe_requirements(cl).items():
            if ok:
                reached_by.setdefault(name, []).append(spec.name)
    for kenlm_keys in (False, True):
        missing = [name for name, ok in L.probe_requirements(classes[kenlm_keys]).items() if not ok]
        assert not missing, (kenlm_keys, missing)
    # the named cases: the order-5 five-character model (the beam-search rows use it) reaches all of them on its own
    assert set(L.probe_requirements(set()).keys()) == {n for n, by in reached_by.items() if L.WRAP_MODEL.name in by}


def test_restated_factorised_form_equals_the_reference_and_every_mutant_differs(lib, tmp_path):
    """The cases have teeth: the numpy restatement of lm_context_acc + lm_pair_log_cond_prob on the library's table
    equals the reference on every window of every model, and each subtly wrong variant of it gets at least one wrong."""
    caught = {m: [] for m in L.MUTANTS}
    for spec in L.ZOO:
        c = L.case(spec)
        h = _host(lib, spec, tmp_path)
        try:
            tab = L.table_of(lib, h)
            wins = L.handle_windows(lib, h, c)
        finally:
            lib.ppasr_lm_destroy(h)
        got = L.factorised(tab, spec.order, wins)
        bad = np.flatnonzero(~L.same(got, c.score))
        assert bad.size == 0, (spec.name, c.windows[bad[0]].tolist(), got[bad[0]], c.score[bad[0]])
        if spec.n_chars > 5:
            continue                                    # (the mutants are told apart on the small tables)
        for m in L.MUTANTS:
            if not L.same(L.factorised(tab, spec.order, wins, m), c.score).all():
                caught[m].append(spec.name)
    assert all(caught.values()), {m: by for m, by in caught.items() if not by}
    # named cases: the table ends that the seeds were scanned for
    assert "o5c5s0" in caught["wrap_slot_empty"] and "o6c2s57" in caught["no_mask_in_continuation"]
    assert any(n.endswith("-probing") for n in caught["wrap_slot_empty"])       # ... and under KenLM's key chain
    assert {n[:2] for n in caught["one_probe_round"]} == {"o5", "o6"}           # the second round exists from order 5 on


def test_device_score_refuses_a_host_only_handle(lib, tmp_path):
    """ppasr_lm_debug_device_score validates before any HIP call: a host-only handle has no device table"""
    spec = L.ZOO_BY_NAME["o3c2s0"]
    h = _host(lib, spec, tmp_path)
    try:
        wins = (ctypes.c_int32 * 3)(1, 2, 3)
        out = (ctypes.c_double * 1)(7.0)
        assert lib.ppasr_lm_debug_device_score(h, wins, 1, 0, out, None) == _lib.PPASR_EINVAL
        assert b"host-only" in lib.ppasr_last_error()
        assert lib.ppasr_lm_debug_device_score(h, wins, 0, 0, out, None) == _lib.PPASR_EINVAL
        assert lib.ppasr_lm_debug_device_score(None, wins, 1, 0, out, None) == _lib.PPASR_EINVAL
        assert out[0] == 7.0
    finally:
        lib.ppasr_lm_destroy(h)
