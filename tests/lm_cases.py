"""Cases and the reference of the n-gram scorer (csrc/lm.h), shared by tests/test_lm_reference_cpu.py,
tests/test_lm_device_gpu.py and the zoo rows of tests/test_ctc_beam_lm_gpu.py.

* `ref_walk`: Scorer::get_log_cond_prob as a plain back-off walk over the dictionary of the ARPA file's n-grams
  (lm_util.read_arpa), float32 sums and one double division.  It never calls the library.
* the model zoo (`ZOO`, `case`, `write_model`): synthetic ARPA models of orders 1 .. 6 whose tables are SMALL (16 .. 1024 slots), so that
  keys whose home is the last slot and clusters that run through the table's end occur, two models over ~300 characters,
  and .klm renderings; with the windows every model is scored on and the reference's answers.
* a restatement of the probe and of the factorised form (lm_probe_many, lm_context_acc, lm_pair_log_cond_prob) in numpy
  that runs on the table the LIBRARY built (ppasr_lm_debug_table) -- only the key function is restated, the layout is
  the real one -- with `classify` (which probe paths a key takes) and `MUTANTS` (subtly wrong variants of the
  factorised form that the windows must tell apart from the reference)."""
import ctypes
import itertools
import os
from collections import namedtuple

import numpy as np

from klm_writer import write_klm
from lm_util import read_arpa, write_synthetic_arpa

OOV_SCORE = -1000.0                      # kLmOovScore
LOG10E = np.float32(0.4342944819)        # kLmLog10E
MAX_WINDOWS = 20000
PAR = 3                                  # kLmPar

# ---------------------------------------------------------------------------------------------------------------------
# the reference


def gram_dict(lm):
    """read_arpa's arrays -> {n-gram (tuple of ARPA word ids, oldest first): (float32 log10 prob, float32 log10 back-off)}"""
    return {tuple(int(w) for w in lm["gram_w"][i, :lm["gram_n"][i]]): (lm["prob"][i], lm["backoff"][i])
            for i in range(len(lm["gram_n"]))}


def ref_walk(grams, order, win):
    """-> (score, deciding level, context levels whose back-off was added).  Level 0: the OOV score (a word of the window
    is 0, or the last word has no unigram)."""
    if any(w == 0 for w in win):
        return OOV_SCORE, 0, ()
    acc = np.float32(0.0)
    used = []
    for n in range(order, 0, -1):
        g = grams.get(tuple(win[order - n:]))
        if g is not None:
            return float(np.float32(acc + g[0])) / float(LOG10E), n, tuple(used)
        c = grams.get(tuple(win[order - n:order - 1])) if n > 1 else None
        if c is not None:
            acc = np.float32(acc + c[1])
            used.append(n - 1)
    return OOV_SCORE, 0, tuple(used)


# ---------------------------------------------------------------------------------------------------------------------
# the zoo

Spec = namedtuple("Spec", "name order n_chars seed n_sent sent_len klm")


def _spec(order, n_chars, seed, n_sent, sent_len, klm=None):
    name = f"o{order}c{n_chars}s{seed}" + (f"-{klm}" if klm else "")
    return Spec(name, order, n_chars, seed, n_sent, sent_len, klm)


# (order, characters) -> (seed, n_sent, sent_len).  The seeds were chosen by scanning on the CPU until the tables the
# LIBRARY builds from these models reach every class of probe_requirements() and every mutant of MUTANTS is told apart
# (tests/test_lm_reference_cpu.py asserts both).
SMALL = {
    (1, 1): (0, 3, 9), (1, 2): (0, 3, 9), (1, 3): (0, 3, 9), (1, 5): (0, 3, 9),
    (2, 1): (0, 3, 9), (2, 2): (0, 3, 9), (2, 3): (0, 3, 9), (2, 5): (0, 3, 9),
    (3, 1): (0, 3, 9), (3, 2): (0, 3, 9), (3, 3): (0, 3, 9), (3, 5): (0, 3, 9),
    (4, 1): (0, 3, 9), (4, 2): (0, 3, 9), (4, 3): (0, 3, 9), (4, 5): (0, 3, 9),
    (5, 1): (0, 3, 9), (5, 2): (0, 3, 9), (5, 3): (0, 3, 9), (5, 5): (0, 3, 9),
    (6, 1): (0, 3, 9), (6, 2): (57, 6, 10), (6, 3): (0, 3, 9), (6, 5): (0, 3, 9),
}
# the .klm renderings: a five-character model of every order 2 .. 6, as `probing` (KenLM's own key chain on the device)
# and `trie`.  Seed 24: the probing tables of orders 5 and 6 reach every required probe class on their own.
KLM = {2: (0, 3, 9), 3: (0, 3, 9), 4: (0, 3, 9), 5: (24, 3, 9), 6: (24, 3, 9)}

ZOO = ([_spec(o, c, *SMALL[(o, c)]) for (o, c) in sorted(SMALL)]
       + [_spec(3, 300, 3, 120, 12), _spec(6, 300, 6, 120, 12)]
       + [_spec(o, 5, *KLM[o], klm=t) for o in sorted(KLM) for t in ("probing", "trie")])
ZOO_BY_NAME = {s.name: s for s in ZOO}
WRAP_MODEL = ZOO_BY_NAME["o5c5s0"]       # order 5, five characters: its table has an occupied last slot and a wrapping cluster
ARPA_ZOO = [s for s in ZOO if s.klm is None]
KLM_ZOO = [s for s in ZOO if s.klm is not None]


def chars_of(spec):
    return [chr(0x4E00 + i) for i in range(spec.n_chars)]


def vocab_of(spec):
    """acoustic vocabulary: every character of the model and three the model does not know"""
    return ["<blank>", "<unk>"] + chars_of(spec) + [chr(0x5000 + i) for i in range(3)] + ["<eos>"]


Case = namedtuple("Case", "spec lm grams n_words windows score level used")
_cases = {}


def _windows(spec, lm, grams):
    """[N][order] ARPA word ids (0 = OOV).  Every window over {known words, <s>, </s>, OOV} when there are at most
    MAX_WINDOWS of them; else every n-gram of the model right-aligned and extended to the left with <s>, with its own
    leading words, and with a word that makes the extension absent, plus a seeded random fill.  Always: <s>-padded starts
    of every length, </s> last, OOV in every position, and candidates at and above n_words."""
    order, bos, eos = spec.order, lm["bos"], lm["eos"]
    n_words = len(lm["words"])
    known = sorted(lm["words"][c] for c in chars_of(spec))
    rng = np.random.Generator(np.random.PCG64(1000 + spec.seed + 7 * order + spec.n_chars))
    pick = lambda k: [int(x) for x in rng.choice(known, size=k)]
    always = []
    for k in range(order + 1):                         # k leading <s>
        for _ in range(3):
            always.append([bos] * k + pick(order - k))
    for k in range(order):
        always.append([bos] * k + pick(order - k - 1) + [eos])
    for i in range(order):                             # OOV in position i
        w = pick(order)
        w[i] = 0
        always.append(w)
        w = [bos] * order
        w[i] = 0
        always.append(w)
    for k in range(order):                             # a candidate the unigram table does not hold
        for cand in (n_words, n_words + 3):
            always.append([bos] * k + pick(order - k - 1) + [cand])
    symbols = [0, bos, eos] + known
    if len(symbols) ** order <= MAX_WINDOWS:
        body = [list(w) for w in itertools.product(symbols, repeat=order)]
    else:
        body = []
        for g in sorted(grams):
            n = len(g)
            if n == order:
                body.append(list(g))
                continue
            body.append([bos] * (order - n) + list(g))
            body.append(list((g * order)[:order - n]) + list(g))
            absent = [x for x in known + [eos] if (x,) + g not in grams]
            if absent:
                x = absent[int(rng.integers(len(absent)))]
                body.append([bos] * (order - n - 1) + [x] + list(g))
        body = body[:MAX_WINDOWS - len(always)]
        n_fill = MAX_WINDOWS - len(always) - len(body)
        if n_fill > 0:
            fill = rng.choice(known, size=(n_fill, order))
            for i in range(0, n_fill, 7):
                fill[i, :int(rng.integers(1, order))] = bos
            fill[::11, -1] = eos
            fill[5::13, int(rng.integers(order))] = 0
            body += fill.tolist()
    return np.array(always + body, np.int32)


def case(spec):
    """windows and the reference's answers for the model of `spec` (its .klm renderings share them); computed once"""
    key = spec._replace(name="", klm=None)
    if key not in _cases:
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            arpa = write_synthetic_arpa(os.path.join(d, "lm.arpa"), chars_of(spec), order=spec.order, n_sent=spec.n_sent,
                                        sent_len=spec.sent_len, seed=spec.seed)
            lm = read_arpa(arpa, vocab_of(spec))
        assert lm["order"] == spec.order
        grams = gram_dict(lm)
        wins = _windows(spec, lm, grams)
        score = np.empty(len(wins))
        level = np.empty(len(wins), np.int8)
        used = []
        for i, w in enumerate(wins.tolist()):
            score[i], level[i], u = ref_walk(grams, spec.order, w)
            used.append(u)
        for a in (wins, score, level):
            a.setflags(write=False)
        _cases[key] = (lm, grams, wins, score, level, tuple(used))
    lm, grams, wins, score, level, used = _cases[key]
    return Case(spec, lm, grams, len(lm["words"]), wins, score, level, used)


def write_model(spec, directory):
    """writes the model file of `spec` (ARPA, or the .klm rendering of that ARPA file) into `directory` -> its path"""
    arpa = write_synthetic_arpa(os.path.join(str(directory), spec.name.split("-")[0] + ".arpa"), chars_of(spec),
                                order=spec.order, n_sent=spec.n_sent, sent_len=spec.sent_len, seed=spec.seed)
    if spec.klm is None:
        return arpa
    return write_klm(arpa, os.path.join(str(directory), spec.name + ".klm"), model_type=spec.klm)


# ---------------------------------------------------------------------------------------------------------------------
# the library's side


def load(lib, path, vocab, host_only):
    from ppasr_amd import _lib
    words = (ctypes.c_char_p * len(vocab))(*[w.encode("utf-8") for w in vocab])
    h = ctypes.c_void_p()
    create = lib.ppasr_lm_debug_load_host if host_only else lib.ppasr_lm_create
    _lib.check(create(str(path).encode(), words, len(vocab), ctypes.byref(h)))
    return h


def handle_windows(lib, h, c):
    """the windows of case `c` in the word indices of handle `h` (a .klm numbers its words differently), through
    ppasr_lm_word_index / ppasr_lm_bos / ppasr_lm_eos; indices >= n_words stay as they are"""
    vocab = vocab_of(c.spec)
    ids = np.arange(int(c.windows.max()) + 1, dtype=np.int32)
    ids[:c.n_words] = 0
    for t, s in enumerate(vocab):
        if s in c.lm["words"] and s != "<unk>":
            ids[c.lm["words"][s]] = lib.ppasr_lm_word_index(h, t)
    ids[c.lm["bos"]] = lib.ppasr_lm_bos(h)
    ids[c.lm["eos"]] = lib.ppasr_lm_eos(h)
    return np.ascontiguousarray(ids[c.windows])


def host_scores(lib, h, wins):
    out = np.empty(len(wins))
    for i in range(len(wins)):
        out[i] = lib.ppasr_lm_debug_host_score(h, wins[i].ctypes.data_as(ctypes.c_void_p))
    return out


Table = namedtuple("Table", "key prob backoff mask kenlm_keys")
_slot_dtype = np.dtype([("key", "<u8"), ("prob", "<f4"), ("backoff", "<f4")])


def table_of(lib, h):
    """the library's own table (mask + 2 slots: the last one is the copy of slot 0)"""
    n = lib.ppasr_lm_debug_table(h, None, 0)
    assert n >= 17
    raw = np.zeros(n, _slot_dtype)
    assert lib.ppasr_lm_debug_table(h, raw.ctypes.data_as(ctypes.c_void_p), n) == n
    assert lib.ppasr_lm_debug_table(h, raw.ctypes.data_as(ctypes.c_void_p), n - 1) == -1
    kenlm = lib.ppasr_lm_format(h) in (b"klm-probing", b"klm-rest-probing")
    return Table(raw["key"].copy(), raw["prob"].copy(), raw["backoff"].copy(), n - 2, kenlm)


# ---------------------------------------------------------------------------------------------------------------------
# the key function of lm.h, restated over uint64 arrays (the only part of the table's addressing that is restated)

_U = np.uint64


def _mix(h, v):
    h = h ^ (v + _U(0x9e3779b97f4a7c15) + (h << _U(6)) + (h >> _U(2)))
    h = h * _U(0xff51afd7ed558ccd)
    return h ^ (h >> _U(33))


def suffix_keys(kenlm_keys, cols):
    """cols: word-index arrays, NEWEST first -> [key of the n-gram made of the newest n words, n = 1 .. len(cols)]"""
    keys = []
    with np.errstate(over="ignore"):
        h = None
        for n, col in enumerate(cols, 1):
            w = col.astype(np.uint32).astype(_U)
            if kenlm_keys:
                h = w if n == 1 else (h * _U(8978948897894561157)) ^ ((w + _U(1)) * _U(17894857484156487943))
                k = _mix(np.full_like(h, _U(0x2545f4914f6cdd1d ^ n)), h)
            else:
                h = _mix(np.full_like(w, _U(0xcbf29ce484222325)), w) if n == 1 else _mix(h, w)
                k = _mix(h ^ _U(0x9ae16a3b2f90404f), np.full_like(h, _U(n)))
            keys.append(k | _U(1))
    return keys


# ---------------------------------------------------------------------------------------------------------------------
# lm_probe_many, restated on the library's table

Probe = namedtuple("Probe", "found prob backoff dist home_last wraps")


def probe(tab, keys, want=None, mutant=None):
    """Both slots home, home + 1 are read first (home + 1 of the last slot is the wrap copy), a longer cluster continues
    from (home + 2) & mask.  dist: slots past the home slot at which the walk ended (hit, or the empty slot)."""
    K = tab.key
    if mutant == "wrap_slot_empty":
        K = K.copy()
        K[-1] = 0
    mask = np.int64(tab.mask)
    keys = np.asarray(keys, _U)
    want = np.ones(len(keys), bool) if want is None else want
    home = ((keys >> _U(17)).astype(np.int64)) & mask
    idx = np.full(len(keys), -1, np.int64)
    dist = np.zeros(len(keys), np.int64)
    s0, s1 = K[home], K[home + 1]
    hit0 = want & (s0 == keys)
    go1 = want & ~hit0 & (s0 != 0)
    hit1 = go1 & (s1 == keys)
    go2 = go1 & ~hit1 & (s1 != 0)
    idx[hit0] = home[hit0]
    idx[hit1] = home[hit1] + 1
    dist[go1] = 1
    if mutant != "two_slots_only":
        no_mask = mutant == "no_mask_in_continuation"
        slot = home + 2 if no_mask else (home + 2) & mask
        active = go2
        d = 2
        while active.any():
            k = np.where(slot < len(K), K[np.minimum(slot, len(K) - 1)], _U(0))   # (past the array: an empty slot)
            dist[active] = d
            hit = active & (k == keys)
            idx[hit] = slot[hit]
            active = active & ~hit & (k != 0)
            slot = slot + 1 if no_mask else (slot + 1) & mask
            d += 1
    found = idx >= 0
    at = np.maximum(idx, 0)
    return Probe(found, np.where(found, tab.prob[at], np.float32(0)), np.where(found, tab.backoff[at], np.float32(0)),
                 dist, home == mask, home + dist > mask)


def classify(tab, keys):
    """-> set of (hit, min(dist, 2), home is the last slot, the walk passes from the last slot to slot 0)"""
    p = probe(tab, np.unique(keys))
    return set(zip(p.found.tolist(), np.minimum(p.dist, 2).tolist(), p.home_last.tolist(), p.wraps.tolist()))


def probe_class(tab, key):
    p = probe(tab, np.array([key], _U))
    return dict(hit=bool(p.found[0]), dist=int(p.dist[0]), home_last=bool(p.home_last[0]), wraps=bool(p.wraps[0]))


# what the zoo must reach: a hit and a miss whose home is the last slot and that consult slot 0 through the wrap copy; a
# hit at distance >= 2; a miss after >= 2; a walk that passes the table's end at distance >= 2.
def probe_requirements(classes):
    return {
        "hit, home = last slot, slot 0 through the wrap copy": any(h and d >= 1 and hl for h, d, hl, w in classes),
        "miss, home = last slot, slot 0 through the wrap copy": any(not h and d >= 1 and hl for h, d, hl, w in classes),
        "hit at distance >= 2": any(h and d >= 2 for h, d, hl, w in classes),
        "miss after >= 2 slots": any(not h and d >= 2 for h, d, hl, w in classes),
        "walk passes the last slot at distance >= 2": any(d >= 2 and w for h, d, hl, w in classes),
    }


# ---------------------------------------------------------------------------------------------------------------------
# lm_context_acc + lm_pair_log_cond_prob, restated (vectorised over the windows), and its mutants

MUTANTS = ["wrap_slot_empty",            # the slot behind the table is not a copy of slot 0
           "two_slots_only",             # a cluster longer than two slots is not walked
           "no_mask_in_continuation",    # ... or walked without `& mask`
           "one_probe_round",            # orders 5 and 6: the second round of kLmPar probes is dropped (both functions)
           "acc_one_level_off",          # the pair takes acc[n - 1] for the n-gram that decides
           "absent_context_backoff",     # an absent context m-gram contributes the back-off of the (m - 1)-gram
           "no_nan_check"]               # a candidate without a unigram is not sent to the OOV score


def all_keys(tab, order, wins):
    """every key the three forms look up for these windows: [context m-grams, m = 1 .. order - 1], [n-grams ending in the
    candidate, n = 1 .. order]"""
    cols = [wins[:, order - 1 - i].astype(np.int64) for i in range(order)]     # newest first
    return suffix_keys(tab.kenlm_keys, cols[1:]), suffix_keys(tab.kenlm_keys, cols)


def factorised(tab, order, wins, mutant=None):
    """[N] doubles: the factorised form on the windows `wins` ([N][order], the handle's word indices)"""
    N = len(wins)
    ctx_keys, pair_keys = all_keys(tab, order, wins)
    word = wins[:, order - 1]
    oov = (wins[:, :order - 1] == 0).any(axis=1)
    bo = np.zeros((order + 1, N), np.float32)
    has = np.zeros((order + 1, N), bool)
    for r0 in range(1, order, PAR):
        if mutant == "one_probe_round" and r0 > 1:
            break
        for m in range(r0, min(r0 + PAR, order)):
            p = probe(tab, ctx_keys[m - 1], ~oov, mutant)
            bo[m], has[m] = p.backoff, p.found
    if mutant == "absent_context_backoff":
        for m in range(2, order):
            bo[m] = np.where(has[m], bo[m], bo[m - 1])
            has[m] = True
    acc = np.zeros((order + 1, N), np.float32)
    a = np.zeros(N, np.float32)
    for n in range(order, 0, -1):
        acc[n] = a
        if n >= 2:
            a = np.where(has[n - 1], a + bo[n - 1], a)
    out = np.full(N, np.nan)
    done = oov | (word == 0)
    out[done] = OOV_SCORE
    for r in range((order - 1 + PAR - 1) // PAR):
        if mutant == "one_probe_round" and r > 0:
            break
        for n in range(order - PAR * r, max(order - PAR * r - PAR, 1), -1):
            p = probe(tab, pair_keys[n - 1], ~done, mutant)
            hit = p.found & ~done
            lvl = acc[n - 1] if mutant == "acc_one_level_off" else acc[n]
            out[hit] = ((lvl + p.prob)[hit]).astype(np.float64) / np.float64(LOG10E)
            done |= hit
    u = probe(tab, pair_keys[0])                       # uni_prob[word]: the unigram's entry, NaN when there is none
    uni = np.where(u.found, u.prob, np.float32("nan"))
    rest = ~done
    val = (acc[1] + uni).astype(np.float64) / np.float64(LOG10E)
    if mutant != "no_nan_check":
        val = np.where(np.isnan(uni), OOV_SCORE, val)
    out[rest] = val[rest]
    return out


def same(a, b):
    """elementwise: the same double (a NaN equals nothing, itself included)"""
    return np.asarray(a) == np.asarray(b)
