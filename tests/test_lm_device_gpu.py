"""GPU: the device n-gram scorer (csrc/lm.h) window by window against the independent walk of tests/lm_cases.py.
ppasr_lm_debug_device_score runs lm_log_cond_prob (form 0) and the factorised form the beam search uses per (hypothesis,
candidate) pair -- lm_context_acc + lm_pair_log_cond_prob reading uni_prob itself (form 1) or handed the unigram (form
2) -- one thread per window.  Every form equals the reference BIT FOR BIT on every window of every zoo model (so the
forms equal each other, which is what lets the search mix them), writes nothing but its outputs, and does not depend on
what the output buffer held.  The zoo's tables reach every path of lm_probe_many (test_lm_reference_cpu.py asserts it)."""
import numpy as np
import pytest
import torch

import lm_cases as L
from ppasr_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64          # doubles before and behind out_dev
FILLS = [-12345.678, float("nan")]


def _score(lib, h, wins_dev, n, form, fill):
    """-> the n outputs; the guard words around them must come back untouched"""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=torch.float64, device="cuda")
    before = buf.cpu().numpy().tobytes()
    _lib.check(lib.ppasr_lm_debug_device_score(h, wins_dev.data_ptr(), n, form, buf.data_ptr() + 8 * GUARD,
                                               torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    out = buf.cpu().numpy()
    guard = 8 * GUARD
    assert out.tobytes()[:guard] == before[:guard] and out.tobytes()[-guard:] == before[-guard:], "guard words written"
    if n == 0:
        assert out.tobytes() == before
    return out[GUARD:GUARD + n]


def _explain(lib, h, c, wins, got, i):
    """a mismatch, localised: the window, the reference's deciding level and back-offs, the probe path of every key"""
    tab = L.table_of(lib, h)
    ctx_keys, pair_keys = L.all_keys(tab, c.spec.order, wins[i:i + 1])
    return dict(model=c.spec.name, window=wins[i].tolist(), arpa_window=c.windows[i].tolist(), got=float(got[i]),
                want=float(c.score[i]), level=int(c.level[i]), backoffs_of=c.used[i],
                context_probes=[L.probe_class(tab, k[0]) for k in ctx_keys],
                candidate_probes=[L.probe_class(tab, k[0]) for k in pair_keys])


def _check_model(tmp_path, spec, kenlm_keys):
    lib = _lib.load()
    c = L.case(spec)
    h = L.load(lib, L.write_model(spec, tmp_path), L.vocab_of(spec), host_only=False)
    try:
        assert lib.ppasr_lm_order(h) == spec.order and L.table_of(lib, h).kenlm_keys == kenlm_keys
        wins = L.handle_windows(lib, h, c)
        wins_dev = torch.from_numpy(wins).cuda()
        n = len(wins)
        want = c.score.tobytes()
        for form in (0, 1, 2):
            for fill in FILLS:
                got = _score(lib, h, wins_dev, n, form, fill)
                if got.tobytes() != want:
                    i = int(np.flatnonzero(~L.same(got, c.score))[0])
                    pytest.fail(f"form {form}, buffer pre-filled with {fill}: {_explain(lib, h, c, wins, got, i)}")
            _score(lib, h, wins_dev, 0, form, FILLS[0])          # n_windows = 0 launches nothing
        # a launch whose last block is partly idle, and a single window
        for m in (1, 257):
            if m <= n:
                assert _score(lib, h, wins_dev, m, 1, FILLS[1]).tobytes() == c.score[:m].tobytes()
    finally:
        lib.ppasr_lm_destroy(h)


@pytest.mark.parametrize("spec", [s for s in L.ZOO if s.klm != "probing"], ids=lambda s: s.name)
def test_device_forms_equal_the_reference(tmp_path, spec):
    """tables keyed by lm_key over the word ids: every ARPA model, and the trie binaries (their own word numbering)"""
    _check_model(tmp_path, spec, kenlm_keys=False)


@pytest.mark.parametrize("spec", [s for s in L.ZOO if s.klm == "probing"], ids=lambda s: s.name)
def test_device_forms_equal_the_reference_kenlm_keys(tmp_path, spec):
    """kenlm_keys = 1: tables taken over from a probing binary, keyed by KenLM's own word-hash chain"""
    _check_model(tmp_path, spec, kenlm_keys=True)


def test_device_score_argument_checks(tmp_path):
    lib = _lib.load()
    spec = L.ZOO_BY_NAME["o3c2s0"]
    c = L.case(spec)
    h = L.load(lib, L.write_model(spec, tmp_path), L.vocab_of(spec), host_only=False)
    try:
        wins_dev = torch.from_numpy(L.handle_windows(lib, h, c)).cuda()
        out = torch.full((len(c.windows),), 3.5, dtype=torch.float64, device="cuda")
        w, o, n = wins_dev.data_ptr(), out.data_ptr(), len(c.windows)
        for args in ((None, w, n, 0, o), (h, None, n, 0, o), (h, w, n, 0, None), (h, w, -1, 0, o), (h, w, n, -1, o),
                     (h, w, n, 3, o)):
            assert lib.ppasr_lm_debug_device_score(*args, None) == _lib.PPASR_EINVAL, args
        torch.cuda.synchronize()
        assert bool((out == 3.5).all())
    finally:
        lib.ppasr_lm_destroy(h)
