"""CPU checks of CTC forced alignment (no GPU needed): the numpy oracle of tests/align_oracle.py against exhaustive
enumeration, its feasibility and tie rules, the new C-ABI symbols, and the refusals of ppasr_ctc_align that come before any
device work (as tests/test_rescore_refusals_cpu.py does for the rescorer)."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import align_oracle as ao
from ppasr_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 3
SHAPES = [(1, 0), (1, 1), (3, 2), (4, 3), (5, 2), (6, 3)]


def _table(T, seed):
    rng = np.random.default_rng(seed)
    z = rng.normal(size=(T, V)) * 2.0
    p = np.exp(z - z.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)).astype(np.float32)


def _token_lists(L):
    """every token sequence of length L over the non-blank symbols {1, 2}: repeats included"""
    return [list(t) for t in itertools.product(range(1, V), repeat=L)]


@pytest.mark.parametrize("T,L", SHAPES)
def test_oracle_optimum_is_the_brute_force_optimum(T, L):
    for seed in range(3):
        p = _table(T, 100 * T + 10 * L + seed)
        for tokens in _token_lists(L):
            bf = ao.brute_force(p, tokens)
            r = ao.align(p, tokens)
            feasible = T >= ao.frames_needed(tokens)
            assert (bf is not None) == feasible, (T, tokens)  # the feasibility rule, against enumeration
            assert (r["status"] == ao.OK) == feasible
            if not feasible:
                assert r["status"] == ao.INFEASIBLE and r["score"] == -np.inf
                assert (r["frame_token"] == -1).all() and (r["begin"] == -1).all() and (r["end"] == -1).all()
                continue
            assert abs(float(r["score"]) - bf) <= 1e-12, (T, tokens, r["score"], bf)
            assert abs(ao.path_score64(p, r["frame_token"], tokens) - bf) <= 1e-12
            r32 = ao.align(p, tokens, dtype=np.float32)  # the same walk in the kernel's precision
            assert abs(float(r32["score"]) - bf) <= ao.tolerance(T, r["abs_log"]) + 1e-30


def test_feasibility_edges():
    p = _table(4, 1)
    assert ao.align(p, [], T=0)["status"] == ao.OK and ao.align(p, [], T=0)["score"] == 0.0
    assert ao.align(p, [1], T=0)["status"] == ao.INFEASIBLE
    assert ao.align(p, [1, 1], T=2)["status"] == ao.INFEASIBLE  # needs a blank between: 3 frames
    assert ao.align(p, [1, 1], T=3)["status"] == ao.OK
    assert (ao.align(p, [1, 1], T=3)["frame_token"] == [0, -1, 1, -1]).all()
    assert ao.align(p, [1, 2], T=2)["status"] == ao.OK
    assert ao.align(p, [0], T=4)["status"] == ao.BAD_INPUT   # the blank as a token
    assert ao.align(p, [V], T=4)["status"] == ao.BAD_INPUT
    assert ao.align(p, [-1], T=4)["status"] == ao.BAD_INPUT
    r = ao.align(p, [], T=3)  # no tokens: all blanks
    assert r["status"] == ao.OK and (r["frame_token"] == -1).all()
    assert abs(float(r["score"]) - float(ao.emissions(p[:3])[:, 0].sum())) <= 1e-12


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("T,tokens", [(6, [1, 2, 3]), (7, [1, 1, 2]), (9, [2, 2, 2, 1]), (5, [3]), (4, []), (3, [1, 1])])
def test_tie_rule_on_a_uniform_table_gives_the_left_packed_path(T, tokens, dtype):
    p = np.full((T, 4), 0.25, np.float32)
    r = ao.align(p, tokens, dtype=dtype)
    want = ao.left_packed(tokens, T)
    assert (r["frame_token"] == want).all(), (r["frame_token"], want)
    for l in range(len(tokens)):
        at = np.nonzero(want == l)[0]
        assert r["begin"][l] == at[0] and r["end"][l] == at[-1] + 1 and r["peak"][l] == at[0]
        assert r["conf"][l] == np.float32(0.25)
    if len(tokens):  # trailing blanks: the path ends in the final blank state whenever it can
        assert r["states"][-1] == 2 * len(tokens) or T == ao.frames_needed(tokens)


def test_path_score64_rejects_what_is_not_an_alignment():
    p = _table(5, 3)
    ok = np.array([0, -1, 1, -1, -1], np.int32)
    assert np.isfinite(ao.path_score64(p, ok, [1, 1]))
    for bad, tokens, T in [([0, 1, -1, -1, -1], [1, 1], 5),   # a repeat without a blank between
                           ([1, 0, -1, -1, -1], [1, 2], 5),   # not monotone
                           ([0, -1, -1, -1, -1], [1, 2], 5),  # a token missing
                           ([-1, 1, -1, -1, -1], [1, 2], 5),  # does not start at token 0
                           ([0, 1, -1, -1, 1], [1, 2], 4),    # a token past frame_lens
                           ([0, 2, -1, -1, -1], [1, 2], 5)]:  # index out of range
        with pytest.raises(AssertionError):
            ao.path_score64(p, np.asarray(bad, np.int32), tokens, T)


def test_new_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "ppasr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    lib = _lib.load()
    for name in ("ppasr_ctc_align", "ppasr_ctc_align_workspace_bytes"):
        assert re.search(r"PPASR_API [a-z_ ]+\b%s\s*\(" % name, code), name
        assert name in exported and hasattr(lib, name)


def test_workspace_bytes():
    lib = _lib.load()
    f = lib.ppasr_ctc_align_workspace_bytes
    assert f(0, 10, 10) == 0 and f(1, -1, 10) == 0 and f(1, 10, -1) == 0 and f(1, 10, 256) == 0
    assert f(1, 0, 0) > 0
    # the emission table [B, Tp, >= 1 + max_tokens] f32 and 128 bytes of back-pointers per frame fit
    for B, Tp, mt in [(1, 1, 0), (5, 257, 255), (32, 250, 50)]:
        assert f(B, Tp, mt) >= B * Tp * (4 * (1 + mt) + 128)
    assert f(2, 100, 40) > f(1, 100, 40) and f(1, 200, 40) > f(1, 100, 40) and f(1, 100, 80) > f(1, 100, 40)


def _call(lib, probs=1, frame_lens=None, B=1, Tp=4, V=5, blank=0, tokens=1, n_tokens=1, max_tokens=3, frame_token=1,
          score=1, status=1, workspace=1, workspace_bytes=1 << 20):
    """Pointers: 1 = some non-NULL address (16-byte aligned; never dereferenced: every case here is refused first)."""
    a = lambda x: None if x is None else 4096 * x
    rc = lib.ppasr_ctc_align(a(probs), a(frame_lens), B, Tp, V, blank, a(tokens), a(n_tokens), max_tokens, a(frame_token),
                             None, None, None, None, a(score), a(status), a(workspace), workspace_bytes, None)
    return rc, lib.ppasr_last_error()


@pytest.mark.parametrize("kw,word", [
    (dict(probs=None), b"null"), (dict(tokens=None), b"null"), (dict(n_tokens=None), b"null"),
    (dict(frame_token=None), b"null"), (dict(score=None), b"null"), (dict(status=None), b"null"),
    (dict(workspace=None), b"null"),
    (dict(B=0), b"shape"), (dict(B=-1), b"shape"), (dict(Tp=-1), b"shape"), (dict(V=1), b"shape"), (dict(max_tokens=-1), b"shape"),
    (dict(blank=-1), b"blank"), (dict(blank=5), b"blank"),
    (dict(workspace_bytes=0), b"workspace"), (dict(workspace_bytes=255), b"workspace"),
])
def test_einval_refusals_come_before_any_device_work(kw, word):
    rc, msg = _call(_lib.load(), **kw)
    assert rc == _lib.PPASR_EINVAL, (kw, msg)
    assert word in msg, msg


def test_workspace_one_byte_short_is_refused():
    lib = _lib.load()
    need = lib.ppasr_ctc_align_workspace_bytes(1, 4, 3)
    rc, msg = _call(lib, workspace_bytes=need - 1)
    assert rc == _lib.PPASR_EINVAL and b"workspace" in msg


@pytest.mark.parametrize("mt", [256, 1000])
def test_more_than_255_tokens_is_unsupported(mt):
    rc, msg = _call(_lib.load(), max_tokens=mt)
    assert rc == _lib.PPASR_EUNSUPPORTED, msg
    assert b"255" in msg


def test_python_wrapper_refuses_before_the_device():
    import torch
    from ppasr_amd.decoders import ctc_alignment as ca
    vocab = ["<blank>", "a", "b", "<space>", "<unk>"]
    assert ca.text_to_ids("ab a<unk>", vocab) == [1, 2, 3, 1, 4]
    with pytest.raises(ValueError, match="not in the vocabulary"):
        ca.text_to_ids("abz", vocab)
    p = np.full((3, 5), 0.2, np.float32)
    with pytest.raises(ValueError, match="'z'"):
        ca.forced_align(p, "az", vocab)
    with pytest.raises(ValueError, match=r"T = 3 frames, 5 needed"):
        ca.forced_align(p, "aaa", vocab)
    with pytest.raises(ValueError, match="blank"):
        ca.forced_align(p, [0], vocab)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.PPASRHipError):  # no device: no fallback
            ca.forced_align(p, "ab", vocab)
