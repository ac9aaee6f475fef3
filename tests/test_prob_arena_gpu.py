"""The probability arena (ppasr_prob_arena_*, csrc/ctc_align.hip) and the alignment that reads it (ppasr_ctc_align_arena).

Definition of correct: what ``read`` returns is, word for word, what was appended; and every output of the alignment over
the arena is byte-identical to ``ppasr_ctc_align`` on the dense tables of the same sessions (same emissions, same chain),
so nothing here has a tolerance.  The dense call itself is held to the float64 oracle by test_align_gpu.py.

Shapes: page_frames P in {4, 16}; session lengths one below, at and one above a page, two pages and a frame, and 257
(17 pages of 16, the back-pointer walk's fifth block); token counts 0, 1, 5, 64 (a full gather stride) and 255 (the full
wave); V = 5 and the shipped 4233 for the copies (a row of 4233 floats is not a multiple of 16 bytes)."""
import ctypes

import numpy as np
import pytest
import torch

import poison
import numerics as nm
import test_align_gpu as tag
from ppasr_amd import _lib
from ppasr_amd.decoders import ctc_alignment as ca

pytestmark = pytest.mark.gpu
MEMO = nm.Memo()
V = 50
OUT_NAMES = tag.OUT_NAMES
SPECIALS = np.asarray([0x00000000, 0x00000001, 0x00800000, 0x3F800000, 0x7FC12345, 0xFFC00001, 0x7F812345], np.uint32)
# 0.0, the smallest denormal, FLT_MIN, 1.0, a quiet NaN with a payload, a negative NaN, a signalling NaN pattern


def bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32)


def fill_interleaved(arena, tables, c=16, order=None):
    """Append every session's table in rounds of c frames, all unfinished sessions per round (ragged through `frames`), so
    that the pages of one session are not contiguous in the slab."""
    done = [0] * len(tables)
    rnd = 0
    while any(done[s] < len(tables[s]) for s in range(len(tables))):
        live = [s for s in range(len(tables)) if done[s] < len(tables[s])]
        if order is not None:
            live = sorted(live, key=lambda s: order[(s + rnd) % len(order)])
        chunk = np.full((len(live), c, tables[0].shape[1]), np.nan, np.float32)  # rows behind frames[k] are never copied
        frames = []
        for k, s in enumerate(live):
            f = min(c, len(tables[s]) - done[s])
            chunk[k, :f] = tables[s][done[s]:done[s] + f]
            done[s] += f
            frames.append(f)
        arena.append(live, chunk, frames)
        rnd += 1


def dense_call(tables, sessions, token_lists, blank=0, max_tokens=None, n_tokens=None):
    """ppasr_ctc_align on the dense tables of the listed sessions: Tp = the longest, NaN behind every session's end"""
    Tp = max(len(tables[s]) for s in sessions)
    probs = np.full((len(sessions), Tp, tables[sessions[0]].shape[1]), np.nan, np.float32)
    for k, s in enumerate(sessions):
        probs[k, :len(tables[s])] = tables[s]
    return tag.run(probs, token_lists, [len(tables[s]) for s in sessions], blank, max_tokens, n_tokens)


def arena_call(arena, sessions, token_lists, blank=0, max_tokens=None, n_tokens=None):
    tk, nt = tag.pack_tokens(token_lists, max_tokens)
    out = arena.align_ids(sessions, tk, nt if n_tokens is None else np.asarray(n_tokens, np.int32), blank)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_same(got, ref, label):
    for k in OUT_NAMES:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (label, k)
        assert got[k].tobytes() == ref[k].tobytes(), (label, k, got[k], ref[k])


# ---- round trip ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [4, 16])
@pytest.mark.parametrize("V_", [5, 4233])
def test_read_returns_the_words_that_were_appended(V_, P):
    rng = np.random.default_rng(100 * P + V_)
    arena = ca.ProbArena(3, V_, page_frames=P, n_pages=40)
    # (c, sessions, frames or None): changing subsets, so that a session's pages lie apart in the slab
    rounds = [(16, [0, 1, 2], None), (5, [2, 0], None), (1, [1], None), (16, [1], None), (5, [0, 1, 2], [5, 3, 0]),
              (1, [2, 0], None), (16, [2], [16]), (5, [1, 0], [0, 5]), (1, [0, 1, 2], None)]
    kept = [[] for _ in range(3)]
    for c, sessions, frames in rounds:
        words = rng.integers(0, 2 ** 32, size=(len(sessions), c, V_), dtype=np.uint64).astype(np.uint32)
        words[:, 0, :5] = SPECIALS[:5]
        words[:, -1, -5:] = SPECIALS[2:7]
        arena.append(sessions, torch.from_numpy(words.view(np.float32)), frames)
        for k, s in enumerate(sessions):
            kept[s].append(words[k, :c if frames is None else frames[k]])
    torch.cuda.synchronize()
    used = 0
    for s in range(3):
        want = np.concatenate(kept[s])
        assert arena.frames(s) == len(want)
        assert np.array_equal(bits(arena.read(s)), want), s
        used += -(-len(want) // P)
    assert arena.free_pages() == 40 - used
    arena.reset(1)
    assert arena.frames(1) == 0 and tuple(arena.read(1).shape) == (0, V_)
    assert np.array_equal(bits(arena.read(2)), np.concatenate(kept[2]))  # the neighbours keep their tables


# ---- alignment equality --------------------------------------------------------------------------------------------------
L_LIST = [0, 1, 5, 64, 255]
GROUPS = [[5], [0, 1], [4, 3, 2], [0, 2, 4, 5], [1, 2, 3, 4, 5]]  # 1 to 5 sessions of different T in one call


def equality_setup(P):
    def make():
        rng = np.random.default_rng(200 + P)
        Ts = [1, P - 1, P, P + 1, 2 * P + 1, 257]
        tables = [tag.softmax_table(rng, T, V) for T in Ts]
        for t in tables:  # zeros, denormals, FLT_MIN and ones among the emissions
            t[::3, 1:5] = SPECIALS[:4].view(np.float32)
        return Ts, tables
    return MEMO.get(("equality", P), make)


@pytest.mark.parametrize("P", [4, 16])
def test_alignment_equals_the_dense_call(P):
    Ts, tables = equality_setup(P)
    arena = ca.ProbArena(len(Ts), V, page_frames=P, n_pages=sum(-(-T // P) for T in Ts))
    fill_interleaved(arena, tables, c=16, order=[3, 0, 5, 1, 4, 2])
    assert arena.free_pages() == 0
    rng = np.random.default_rng(300 + P)
    seen = set()
    for sessions in GROUPS:
        for rep in range(len(L_LIST)):
            toks = []
            for k, s in enumerate(sessions):
                admitted = [L for L in L_LIST if L <= Ts[s]]
                L = admitted[(k + rep) % len(admitted)]
                toks.append(tag.random_tokens(rng, L, Ts[s], V, repeats=Ts[s] > L))
                seen.add((Ts[s], L))
            got = arena_call(arena, sessions, toks)
            ref = dense_call(tables, sessions, toks)
            assert (ref["status"] == 0).all()
            assert_same(got, ref, (P, sessions, [len(t) for t in toks]))
    assert {(257, L) for L in L_LIST} <= seen and {(T, 1) for T in Ts} <= seen


@pytest.mark.parametrize("P", [4, 16])
def test_infeasible_and_bad_input_are_reproduced_beside_good_neighbours(P):
    Ts, tables = equality_setup(P)
    arena = ca.ProbArena(len(Ts), V, page_frames=P, n_pages=sum(-(-T // P) for T in Ts) + 2)
    fill_interleaved(arena, tables, c=5)
    rng = np.random.default_rng(400 + P)
    sessions = [4, 1, 5, 2, 3]
    toks = [tag.random_tokens(rng, 5, Ts[4], V),
            list(range(1, P + 1)),                # P tokens in P - 1 frames: status 1
            tag.random_tokens(rng, 64, 257, V),
            [3, V, 4],                            # an id outside the table: status 2
            [7, 0, 9]]                            # the blank as a token: status 2
    got = arena_call(arena, sessions, toks)
    ref = dense_call(tables, sessions, toks)
    assert ref["status"].tolist() == [0, 1, 0, 2, 2]
    assert_same(got, ref, P)
    # n_tokens outside [0, max_tokens] is status 2 as well
    nt = [len(t) for t in toks]
    nt[0], nt[2] = 65, -1
    got = arena_call(arena, sessions, toks, n_tokens=nt)
    ref = dense_call(tables, sessions, toks, n_tokens=nt)
    assert ref["status"].tolist() == [2, 1, 2, 2, 2]
    assert_same(got, ref, (P, "n_tokens"))


# ---- page reuse ----------------------------------------------------------------------------------------------------------
def test_a_reused_page_is_never_read_behind_its_new_owners_last_frame():
    P = 4
    rng = np.random.default_rng(5)
    arena = ca.ProbArena(2, V, page_frames=P, n_pages=3)
    arena.append([0], np.full((1, 3 * P, V), np.nan, np.float32))
    assert arena.free_pages() == 0 and arena.frames(0) == 3 * P
    arena.reset(0)
    assert arena.free_pages() == 3 and arena.frames(0) == 0
    table = tag.softmax_table(rng, P - 1, V)
    arena.append([1], table[None])
    assert arena.free_pages() == 2 and arena.frames(1) == P - 1
    assert np.array_equal(bits(arena.read(1)), table.view(np.uint32))
    tables = [None, table]
    for toks in ([[4, 9]], [[4, 4]], [[]], [[1, 2, 3]]):
        assert_same(arena_call(arena, [1], toks), dense_call(tables, [1], toks), toks)
    # the other two pages go to session 0 again; session 1 is untouched
    t0 = tag.softmax_table(rng, 2 * P, V)
    arena.append([0], t0[None])
    assert arena.free_pages() == 0
    tables[0] = t0
    toks = [[5, 6, 6], [2]]
    assert_same(arena_call(arena, [0, 1], toks), dense_call(tables, [0, 1], toks), "both")


# ---- exhaustion ----------------------------------------------------------------------------------------------------------
def test_an_append_that_does_not_fit_changes_nothing():
    P = 4
    rng = np.random.default_rng(6)
    arena = ca.ProbArena(2, V, page_frames=P, n_pages=4)
    t0 = tag.softmax_table(rng, 12, V)
    t1 = tag.softmax_table(rng, 4, V)
    arena.append([0], t0[None, :9])  # three pages
    assert arena.free_pages() == 1
    more = tag.softmax_table(rng, 5, V)
    with pytest.raises(_lib.PPASRHipError) as e:  # five frames need two pages
        arena.append([1], more[None])
    assert e.value.status == _lib.PPASR_ENOSPACE
    assert (arena.frames(0), arena.frames(1), arena.free_pages()) == (9, 0, 1)
    # all or nothing: the first entry alone would fit (its three frames fill the session's last page)
    chunk = np.zeros((2, 5, V), np.float32)
    chunk[0, :3] = t0[9:]
    chunk[1] = more
    with pytest.raises(_lib.PPASRHipError) as e:
        arena.append([0, 1], chunk, [3, 5])
    assert e.value.status == _lib.PPASR_ENOSPACE
    assert (arena.frames(0), arena.frames(1), arena.free_pages()) == (9, 0, 1)
    chunk[1, :4] = t1
    arena.append([0, 1], chunk, [3, 4])  # one page less: fits
    assert (arena.frames(0), arena.frames(1), arena.free_pages()) == (12, 4, 0)
    with pytest.raises(_lib.PPASRHipError) as e:
        arena.append([1], more[None, :1])
    assert e.value.status == _lib.PPASR_ENOSPACE
    tables = [t0, t1]
    for s in range(2):
        assert np.array_equal(bits(arena.read(s)), tables[s].view(np.uint32))
    toks = [tag.random_tokens(rng, 5, 12, V), tag.random_tokens(rng, 3, 4, V)]
    assert_same(arena_call(arena, [0, 1], toks), dense_call(tables, [0, 1], toks), "after ENOSPACE")


# ---- workspace contents --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", poison.PATTERNS)
def test_no_result_depends_on_workspace_contents(pattern, monkeypatch):
    Ts, tables = equality_setup(16)
    rng = np.random.default_rng(7)
    calls = [([0, 2, 4, 5], [tag.random_tokens(rng, L, Ts[s], V) for s, L in ((0, 1), (2, 5), (4, 0), (5, 64))]),
             ([3, 1], [tag.random_tokens(rng, L, Ts[s], V) for s, L in ((3, 5), (1, 1))])]
    other = ([5], [tag.random_tokens(rng, 255, 257, V)])

    def go(s):
        if s.pattern == "zero":
            ca.scratch._ws.clear()
        arena = ca.ProbArena(len(Ts), V, page_frames=16, n_pages=40)
        fill_interleaved(arena, tables)
        if s.stale:
            arena.align_ids(other[0], *tag.pack_tokens(other[1]))
        outs = {}
        for i, (sessions, toks) in enumerate(calls):
            s.scratch(ca.scratch)
            out = arena.align_ids(sessions, *tag.pack_tokens(toks))
            s.observe(ca.scratch, f"call {i}")
            torch.cuda.synchronize()
            outs.update({f"{i}/{k}": out[k] for k in OUT_NAMES})
        return outs, ca.scratch

    poison.check("ctc_align_arena", go, pattern, monkeypatch, MEMO)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_are_statuses_and_leave_the_arena_usable():
    lib = _lib.load()
    P = 4
    rng = np.random.default_rng(8)
    arena = ca.ProbArena(3, V, page_frames=P, n_pages=8)
    tables = [tag.softmax_table(rng, T, V) for T in (6, 3, 9)]
    fill_interleaved(arena, tables, c=5)
    dev = arena._device
    stream = torch.cuda.current_stream(dev).cuda_stream
    chunk = torch.zeros(2, 4, V, device=dev)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    h = arena._h

    def append(sessions=ints(0, 1), n=2, probs=chunk.data_ptr(), c=4, frames=None, a=h):
        return lib.ppasr_prob_arena_append(a, sessions, n, probs, c, frames, stream)

    EINVAL = _lib.PPASR_EINVAL
    assert append(sessions=ints(0, 3)) == EINVAL          # outside the arena
    assert append(sessions=ints(-1, 0)) == EINVAL
    assert append(sessions=ints(1, 1)) == EINVAL          # twice in one call
    assert append(c=-1) == EINVAL
    assert append(n=0) == EINVAL
    assert append(frames=ints(4, 5)) == EINVAL            # outside [0, c]
    assert append(frames=ints(-1, 2)) == EINVAL
    assert append(sessions=None) == EINVAL
    assert append(probs=None) == EINVAL
    assert append(a=None) == EINVAL
    assert lib.ppasr_prob_arena_reset(h, 3) == EINVAL
    assert lib.ppasr_prob_arena_read(h, 3, chunk.data_ptr(), stream) == EINVAL
    assert lib.ppasr_prob_arena_read(h, 0, None, stream) == EINVAL
    assert lib.ppasr_prob_arena_frames(h, 3) == -1 and lib.ppasr_prob_arena_frames(h, -1) == -1
    assert lib.ppasr_prob_arena_free_pages(None) == -1

    toks = [[4, 9, 9], [2], [7, 7, 1, 3]]
    tk, nt = (torch.as_tensor(x).to(dev) for x in tag.pack_tokens(toks))
    mt = tk.shape[1]
    ft = torch.empty(3, 9, dtype=torch.int32, device=dev)
    score = torch.empty(3, dtype=torch.float32, device=dev)
    status = torch.empty(3, dtype=torch.int32, device=dev)
    need = lib.ppasr_ctc_align_arena_workspace_bytes(3, 9, mt)
    assert need == lib.ppasr_ctc_align_workspace_bytes(3, 9, mt) > 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device=dev)

    def align(sessions=ints(0, 1, 2), n=3, blank=0, tokens=tk.data_ptr(), n_tokens=nt.data_ptr(), max_tokens=mt,
              frame_token=ft.data_ptr(), score_=score.data_ptr(), status_=status.data_ptr(), workspace=ws.data_ptr(),
              bytes_=need, a=h):
        return lib.ppasr_ctc_align_arena(a, sessions, n, blank, tokens, n_tokens, max_tokens, frame_token, None, None, None,
                                         None, score_, status_, workspace, bytes_, stream)

    assert align(sessions=ints(0, 1, 3)) == EINVAL
    assert align(sessions=ints(0, 1, 1)) == EINVAL
    assert align(n=0) == EINVAL
    assert align(blank=V) == EINVAL and align(blank=-1) == EINVAL
    assert align(max_tokens=-1) == EINVAL
    for kw in ("sessions", "tokens", "n_tokens", "frame_token", "score_", "status_", "workspace", "a"):
        assert align(**{kw: None}) == EINVAL, kw
    assert align(workspace=ws.data_ptr() + 4) == EINVAL   # not 16-byte aligned
    assert align(max_tokens=256) == _lib.PPASR_EUNSUPPORTED
    assert align(bytes_=need - 1) == _lib.PPASR_ENOSPACE
    assert lib.ppasr_last_error()

    # nothing above changed a session, and the arena still works
    assert [arena.frames(s) for s in range(3)] == [6, 3, 9] and arena.free_pages() == 8 - (2 + 1 + 3)
    assert align() == _lib.PPASR_OK  # begin .. conf may be NULL, as in ppasr_ctc_align
    torch.cuda.synchronize()
    ref = dense_call(tables, [0, 1, 2], toks)
    assert ft.cpu().numpy().tobytes() == ref["frame_token"].tobytes()
    assert score.cpu().numpy().tobytes() == ref["score"].tobytes() and (status.cpu().numpy() == ref["status"]).all()
    assert_same(arena_call(arena, [2, 0, 1], [toks[2], toks[0], toks[1]]), dense_call(tables, [2, 0, 1], [toks[2], toks[0], toks[1]]),
                "after refusals")
    # the wrapper's own argument checks
    for bad in ([0, 0], [3], []):
        with pytest.raises(ValueError):
            arena.append(bad, np.zeros((len(bad), 1, V), np.float32))
    with pytest.raises(ValueError):
        arena.append([0], np.zeros((1, 1, V + 1), np.float32))
    with pytest.raises(ValueError):
        arena.align([0], [[0]])                      # the blank as a token
    with pytest.raises(ValueError):
        arena.align([1], [[1, 2, 3, 4]])             # four tokens in three frames
    with pytest.raises(_lib.PPASRHipError) as e:
        arena.align([2], [[1] * 256])
    assert e.value.status == _lib.PPASR_EUNSUPPORTED
    spans = arena.align([0, 2], [toks[0], toks[2]])
    for k, s in enumerate((0, 2)):
        assert spans[k] == ca.align_one(torch.as_tensor(tables[s]).to(dev), toks[s])
