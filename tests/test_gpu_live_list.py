"""The live worklist (kernels/bounds_pass.inc): the bounds pass bounds halves with an N on sixteen buckets where eight passed, and
hands the exact kernel only the worklist entries for which some k of some half still has a pass bit (or that have a whole-read
segment).  An entry it drops is DEAD: trew_hip_debug_counters counts them, trew_hip_debug_live_list returns what is left.

What is asserted everywhere: the tables equal the oracle's whatever was dropped, and nothing the oracle accepts is dropped.  The
second is a condition, not a rate: a read one of whose halves the oracle's class counts accept at some k (MAX / COUNT >= LOW) must
be in the live list.

TREW_FLAG_DEBUG_NO_LIVE_LIST switches both steps off (the parent's behaviour: eight buckets, the prefilter's worklist)."""
import functools
import random
from collections import Counter

import numpy as np
import pytest

import oracle as O
import trew_amd as T
from helpers import mutate, periodic
from test_gpu_parity import _table_diff
from trew_amd import capi

pytestmark = pytest.mark.gpu

DEFAULT, NOLIVE, NOGROUP, SMALL = 0, T.FLAG_DEBUG_NO_LIVE_LIST, T.FLAG_DEBUG_NO_GROUP, T.FLAG_DEBUG_SMALL_BOUNDS
PS = (5, 32, 0.5, 0.8)
SMALL_CAP = 64  # entries of the hand-over buffer with TREW_FLAG_DEBUG_SMALL_BOUNDS (include/trew_hip.h)
TELO = "TTAGGG"


def _halves(n):
    return (0, n // 2), (n - (n + 1) // 2, (n + 1) // 2)


def _acgt(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _single_n(rnd, n=150):
    """a random read with one N, 30..45 bases into one of its halves: the few windows left at the large k pass eight buckets by chance"""
    s = list(_acgt(rnd, n))
    start, _ = _halves(n)[rnd.randrange(2)]
    s[start + rnd.randint(30, 45)] = "N"
    return "".join(s)


def _run(reads, flags, passes=1, ps=PS):
    """(worklist, live list, dead entries, tables) of every pass of the uniform batch on slot 0 of one context"""
    mn, mx, low, high = ps
    n = len(reads[0])
    assert all(len(r) == n for r in reads)
    words, _, _ = capi.pack_reads(reads)
    out = []
    with T.TrewHip(mode=T.MODE_SHORT, min_mer=mn, max_mer=mx, low=low, high=high, max_batch_reads=max(len(reads) + 8, 256),
                   max_batch_words=max(len(words) + 64, 1 << 19), flags=flags) as t:
        b = capi.Batch(words.ctypes.data, len(words), None, None, n, 3 * ((n + 31) // 32), len(reads), 0, n)
        for _ in range(passes):
            t.reset_tables()
            t.submit(b, 0)
            t.wait(0)
            dead = t.debug_counters()["dead_entries"]
            out.append((t.debug_worklist(0).copy(), t.debug_live_list(0).copy(), dead, t.collect()))
    return out


def _want(reads, ps=PS):
    mn, mx, low, high = ps
    return O.run_short(O.OracleParams(min_mer=mn, max_mer=mx, low=low, high=high), reads)


def _accepted(reads, ps=PS):
    """indices of the reads of which the oracle accepts some k in some half (the per-read call of test_filter_is_sound)"""
    mn, mx, low, high = ps
    p = O.OracleParams(min_mer=mn, max_mer=mx, low=low, high=high)
    out = set()
    for i, r in enumerate(reads):
        n = len(r)
        if 4 * mn > n:
            continue
        for start, ln in _halves(n):
            st = O.segment_stats(p, r[start:start + ln], mn, min(n // 4, mx))
            if any(cnt and m / cnt >= low for cnt, m, _ in st.values()):
                out.add(i)
                break
    return out


def _check_lists(wl, live, dead, label=""):
    """the live list is contained in the worklist as a multiset, and what is missing is what was counted dead"""
    cw, cl = Counter(int(x) for x in wl), Counter(int(x) for x in live)
    assert not (cl - cw), (label, "live entries that the worklist does not hold", sorted((cl - cw))[:5])
    assert len(live) + dead == len(wl), (label, len(live), dead, len(wl))


# ---- the input of the first three cases: N false positives among the bench generator's telomeric and junction reads ----

@functools.lru_cache(maxsize=None)
def _n_case():
    rnd = random.Random(4100)
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 80000, 150)
    telo, junction = [], []
    for s, e in zip(st, nd):
        r = buf[s:e + 1]
        hits = r.count(b"TTAGGG") + r.count(b"CCCTAA")
        if hits >= 16 and len(telo) < 500:  # 25 units in a telomeric read, 12 in a junction read, 1 % substitutions
            telo.append(r)
        elif 6 <= hits <= 13 and len(junction) < 250:
            junction.append(r)
    assert len(telo) == 500 and len(junction) == 250, (len(telo), len(junction))
    reads = [_single_n(rnd).encode() for _ in range(20000)] + telo + junction
    rnd.shuffle(reads)
    return tuple(reads), _want(reads)


@functools.lru_cache(maxsize=None)
def _n_case_default():
    reads, _ = _n_case()
    return _run(list(reads), DEFAULT, passes=3)


def test_n_false_positives():
    reads, want = _n_case()
    wl, live, dead, tables = _n_case_default()[0]
    print("flagged %d, live %d, dead %d of %d reads" % (len(wl), len(live), dead, len(reads)))
    assert tables == want, _table_diff(tables, want)
    for f in (NOLIVE, NOGROUP):
        wl_f, live_f, dead_f, tables_f = _run(list(reads), f)[0]
        assert tables_f == want, (f, _table_diff(tables_f, want))
        assert np.array_equal(np.sort(wl_f), np.sort(wl)), ("worklist", f)
        assert dead_f == 0 and np.array_equal(live_f, wl_f), f  # nothing is dropped: the exact kernel walks the worklist itself
    assert dead > 0
    _check_lists(wl, live, dead)


def test_soundness():
    reads, _ = _n_case()
    wl, live, dead, _ = _n_case_default()[0]
    accepted = _accepted(reads)
    assert len(accepted) >= 700  # the telomeric and the junction reads
    missing = accepted - set(int(x) for x in live)
    print("the oracle accepts %d reads, %d live, %d missing" % (len(accepted), len(live), len(missing)))
    assert not missing, sorted(missing)[:10]


def test_stability():
    """three passes on one slot: both counter blocks, the live list written three times"""
    _, want = _n_case()
    runs = _n_case_default()
    for wl, live, dead, tables in runs:
        assert tables == want
        assert np.array_equal(np.sort(live), np.sort(runs[0][1]))
        assert dead == runs[0][2]
        _check_lists(wl, live, dead)


# ---- the tail: worklist entries beyond the hand-over buffer follow the live ones unchanged ----

def test_tail():
    rnd = random.Random(4200)
    reads = [_single_n(rnd) for _ in range(3000)] + [mutate(periodic(TELO, 150, i % 6), rnd, p_sub=0.01) for i in range(300)]
    rnd.shuffle(reads)
    reads = [r.encode() for r in reads]
    want = _want(reads)
    wl, live, dead, tables = _run(reads, SMALL)[0]
    print("flagged %d, live %d, dead %d" % (len(wl), len(live), dead))
    assert 300 <= len(wl) <= 1500
    assert tables == want, _table_diff(tables, want)
    _check_lists(wl, live, dead, "small")
    assert dead <= SMALL_CAP
    tail = wl[SMALL_CAP:]
    assert np.array_equal(live[len(live) - len(tail):], tail)  # unchanged, and in the worklist's order
    assert not (Counter(int(x) for x in tail) - Counter(int(x) for x in live))


# ---- a read with a whole-read segment is never dead ----

@pytest.mark.parametrize("n", [120, 151])
def test_never_dead(n):
    rnd = random.Random(4300 + n)
    reads = [_single_n(rnd, n) for _ in range(6000)] + [mutate(periodic(TELO, n, i % 6), rnd, p_sub=0.01) for i in range(100)]
    reads = [r.encode() for r in reads]
    wl, live, dead, tables = _run(reads, DEFAULT)[0]
    print("%d bases: flagged %d, live %d, dead %d" % (n, len(wl), len(live), dead))
    want = _want(reads)
    assert tables == want, _table_diff(tables, want)
    _check_lists(wl, live, dead)
    assert len(wl) > 100
    if n < 4 * PS[1]:  # 120 bases at 5 32: the whole-read segment is valid (k = 31, 32 ... n / 2)
        assert dead == 0 and np.array_equal(np.sort(live), np.sort(wl))


# ---- empty ends ----

def test_nothing_flagged():
    rnd = random.Random(4400)
    reads = [_acgt(rnd, 150).encode() for _ in range(64)]
    wl, live, dead, tables = _run(reads, DEFAULT)[0]
    assert len(wl) == 0 and len(live) == 0 and dead == 0
    assert all(len(tb) == 0 for tb in tables.values())


def _plane_codes():
    """(lo, hi) plane bit of every base, read off the packed words of a four-base read (triples of lo, hi and N words)"""
    words, _, _ = capi.pack_reads([b"ACGT"])
    return {c: ((int(words[0]) >> i) & 1, (int(words[1]) >> i) & 1) for i, c in enumerate("ACGT")}


def _no_pass_on_16(half, codes, mn, mx, low):
    """The bound of the bounds pass, restated on the CPU: at every k, the largest of the sixteen buckets (the parities of the lo
    bits, the hi bits, the bases with both and the cyclically adjacent equal bases of a window) stays under LOW * COUNT."""
    L = len(half)
    lo = np.array([codes.get(c, (0, 0))[0] for c in half]), np.array([codes.get(c, (0, 0))[1] for c in half])
    code = lo[0] + 2 * lo[1]
    isn = np.array([c not in codes for c in half], dtype=np.int64)
    pre = lambda x: np.concatenate([[0], np.cumsum(x)])
    S1, S2, S3, SN = pre(lo[0]), pre(lo[1]), pre(lo[0] & lo[1]), pre(isn)
    SD = pre((code[:-1] == code[1:]).astype(np.int64))
    for k in range(mn, min(mx, L) + 1):
        i = np.arange(L - k + 1)
        ok = (SN[i + k] - SN[i]) == 0
        if not ok.any():
            continue
        f4 = (SD[i + k - 1] - SD[i] + (code[i] == code[i + k - 1])) & 1
        b = ((S1[i + k] - S1[i]) & 1) | (((S2[i + k] - S2[i]) & 1) << 1) | (((S3[i + k] - S3[i]) & 1) << 2) | (f4 << 3)
        if np.bincount(b[ok], minlength=16).max() >= low * ok.sum():
            return False
    return True


def test_everything_dead():
    """256 random reads with one N, chosen on the CPU so that a flagged one is dead: no k of either half reaches LOW on sixteen
    buckets (the bound restated above), and the oracle's class counts accept nothing.  The exact kernel gets an empty list."""
    rnd = random.Random(4500)
    codes = _plane_codes()
    mn, mx, low, _ = PS
    reads = []
    while len(reads) < 256:
        r = _single_n(rnd)
        if all(_no_pass_on_16(r[s:s + ln], codes, mn, mx, low) for s, ln in _halves(len(r))):
            reads.append(r.encode())
    assert not _accepted(reads)
    wl, live, dead, tables = _run(reads, DEFAULT)[0]
    print("flagged %d, dead %d" % (len(wl), dead))
    assert len(live) == 0 and dead == len(wl)
    assert all(len(tb) == 0 for tb in tables.values())


def test_one_telomeric_read():
    reads = [periodic(TELO, 150, 2).encode()]
    wl, live, dead, tables = _run(reads, DEFAULT)[0]
    assert list(wl) == [0] and list(live) == [0] and dead == 0
    assert tables == _want(reads)


# ---- off the N path the stored words are the parent's ----

def test_words_without_n_are_unchanged():
    """A batch without an N: the group pass decides from the stored words (default) what it decides from the words its own rows
    pack by the 8-bucket rule (TREW_FLAG_DEBUG_SMALL_BOUNDS: every entry beyond the 64th), from the parent's stored words
    (TREW_FLAG_DEBUG_NO_LIVE_LIST) and what a wave per segment decides without any (TREW_FLAG_DEBUG_NO_GROUP): equal tables."""
    rnd = random.Random(4600)
    reads = [mutate(periodic(TELO, 150, i % 6), rnd, p_sub=0.02 * (i % 4)) for i in range(300)]
    reads += [(periodic(_acgt(rnd, rnd.choice([2, 3, 5, 7, 11])), 75, 0) + _acgt(rnd, 75)) for _ in range(300)]
    reads += [_acgt(rnd, 150) for _ in range(400)]
    rnd.shuffle(reads)
    reads = [r.encode() for r in reads]
    assert not any(b"N" in r for r in reads)
    want = _want(reads)
    got = {f: _run(reads, f)[0] for f in (DEFAULT, SMALL, NOLIVE, NOGROUP)}
    for f, (wl, live, dead, tables) in got.items():
        assert tables == want, (f, _table_diff(tables, want))
        assert np.array_equal(np.sort(wl), np.sort(got[DEFAULT][0])), f
        _check_lists(wl, live, dead, f)
    assert len(got[DEFAULT][0]) > 4 * SMALL_CAP
