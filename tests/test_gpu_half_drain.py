"""The prefilter's two drains of what its uniform fast path sets aside (kernels/prefilter.inc, 3-word kernel).  The fast loop
gives a verdict per HALF; a unit of which exactly one half has to be judged (an N in it, or a 4-bucket pass) goes to the half
list and filter_deferred_half judges that half alone, a unit with two or more goes to the whole-unit list and
filter_deferred_uni.  Dropping the other half's drain loop must change no verdict: the worklist is the same multiset as the
general path's (TREW_FLAG_DEBUG_NO_UNI_DRAIN), no unit appears twice, every read the oracle records is present, the tables
equal the oracle's, and trew_hip_debug_counters shows both drains at work (out[8] half-items, out[9] whole units).

Reads of 190 bases (halves of 95) leave the joint fast loop through its geometry check (5..32 has k with more than 72 windows),
so every set-aside unit is a whole unit there: that case asserts half_drain == 0 and unit_drain > 0.

A batch of 2 400 units is ten blocks of one round each, so it takes only the end-of-input drains; the tiled batch
(test_half_drain_block_fulls) gives every block several rounds, so that both lists reach a block-full in mid-stream."""
import functools
import random
from collections import Counter

import numpy as np
import pytest

import oracle as O
import trew_amd as T
from trew_amd import capi
from helpers import mutate, periodic

FLAGS = (0, T.FLAG_DEBUG_NO_UNI_DRAIN)
TELO = "TTAGGG"
N_UNITS = 2400  # not a multiple of the block's 256
CATEGORIES = ("n_left", "n_right", "n_first", "n_last", "n_left_end", "n_right_start", "n_both", "n_other_telo", "n_self_telo",
              "n_rejected", "junction", "telomeric", "near_miss", "random")
MUST_FLAG = ("n_other_telo", "n_self_telo", "junction", "telomeric")  # the oracle records (nearly) all of these


def _halves(n):
    """(start, length) of the two halves of a short read of n bases, as get_segment (trew_common.hpp) splits it: slots 0, 1."""
    return (0, n // 2), (n - (n + 1) // 2, (n + 1) // 2)


def _acgt(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _put_n(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "N"
    return "".join(s)


def _telo(rnd, n):
    return periodic(TELO, n, rnd.randint(0, 5))


def _read(rnd, cat, n):
    (ls, ll), (rs, rl) = _halves(n)
    left, right = range(ls, ls + ll), range(rs, rs + rl)
    base = _telo(rnd, n) if rnd.random() < 0.5 else _acgt(rnd, n)  # the N-position categories: telomeric and random reads
    if cat == "n_left":
        return _put_n(base, [rnd.choice(left)])
    if cat == "n_right":
        return _put_n(base, [rnd.choice(right)])
    if cat == "n_first":
        return _put_n(base, [0])
    if cat == "n_last":
        return _put_n(base, [n - 1])
    if cat == "n_left_end":
        return _put_n(base, [ls + ll - 1])
    if cat == "n_right_start":
        return _put_n(base, [rs])
    if cat == "n_both":
        return _put_n(base, [rnd.choice(left), rnd.choice(right)])
    if cat in ("n_other_telo", "n_self_telo", "junction"):
        telo_left = rnd.random() < 0.5
        s = (_telo(rnd, ll) + _acgt(rnd, n - ll)) if telo_left else (_acgt(rnd, n - rl) + _telo(rnd, rl))
        if cat == "junction":
            return s
        n_in_left = telo_left == (cat == "n_self_telo")
        return _put_n(s, [rnd.choice(left if n_in_left else right)])
    if cat == "n_rejected":
        return _put_n(_acgt(rnd, n), [rnd.randrange(n)])
    if cat == "telomeric":
        return mutate(_telo(rnd, n), rnd, p_sub=rnd.choice([0, 0.01, 0.03]))
    if cat == "near_miss":
        unit = _acgt(rnd, rnd.choice([1, 2, 3, 5, 6, 7, 11, 16, 24, 31]))
        return (mutate(periodic(unit, n, rnd.randint(0, 7)), rnd, p_sub=rnd.choice([0.05, 0.1, 0.15, 0.2, 0.3])) + _acgt(rnd, n))[:n]
    return _acgt(rnd, n)


def _n_halves(read, n):
    """which halves of the read hold an N: (left, right)"""
    (ls, ll), (rs, rl) = _halves(n)
    return "N" in read[ls:ls + ll], "N" in read[rs:rs + rl]


@functools.lru_cache(maxsize=None)
def short_case(n, count=N_UNITS):
    """(reads, category of each, indices the oracle records, the oracle's tables) -- computed once per read length"""
    rnd = random.Random(7300 + n)
    cats = [CATEGORIES[i % len(CATEGORIES)] for i in range(count)]
    reads = [_read(rnd, c, n) for c in cats]
    p = O.OracleParams()
    passing = frozenset(i for i, r in enumerate(reads) if any(len(tb) for tb in O.run_short(p, [r.encode()]).values()))
    # "n_rejected" is the reads of that construction the oracle does reject
    cats = [("random_n_recorded" if (c == "n_rejected" and i in passing) else c) for i, c in enumerate(cats)]
    return [r.encode() for r in reads], cats, passing, O.run_short(p, [r.encode() for r in reads])


@functools.lru_cache(maxsize=None)
def pair_case(n=150, count=N_UNITS):
    """Pairs: mate 1 from the short categories; mate 2 random without an N (so that one half of the four is the usual case), or,
    for a third of the pairs, another constructed read (two to four halves)."""
    rnd = random.Random(7777)
    cats = [CATEGORIES[i % len(CATEGORIES)] for i in range(count)]
    r1 = [_read(rnd, c, n).encode() for c in cats]
    r2 = [(_read(rnd, rnd.choice(CATEGORIES), n) if i % 3 == 2 else _acgt(rnd, n)).encode() for i in range(count)]
    p = O.OracleParams()
    passing = frozenset(i for i in range(count) if any(len(tb) for tb in O.run_pair(p, [r1[i]], [r2[i]]).values()))
    return r1, r2, cats, passing, O.run_pair(p, r1, r2)


def check_non_vacuous(cats, passing):
    """enough of everything, stated on the CPU from the reads' construction and the oracle"""
    assert len(passing) >= 200
    per = Counter(cats)
    for c in CATEGORIES:
        assert per[c] >= 50, (c, per[c])
    for c in MUST_FLAG:
        assert sum(1 for i, x in enumerate(cats) if x == c and i in passing) >= 50, c


def _run(mode, words, n_reads, n, flags, tables=True):
    stride = 3 * ((n + 31) // 32)
    with T.TrewHip(mode=mode, max_batch_reads=n_reads + 8, max_batch_words=max(len(words) + 64, 1 << 20), flags=flags) as t:
        t.reset_tables()  # the drains' counters are kept per device
        b = capi.Batch(words.ctypes.data, len(words), None, None, n, stride, n_reads, 0, 0)  # uniform batch: the fast path
        t.submit(b, 0)
        t.wait(0)
        wl = t.debug_worklist(0).copy()
        return wl, (t.collect() if tables else None), t.debug_counters()


def _check(got, passing, want):
    for f in FLAGS:
        wl, tables, _ = got[f]
        cnt = Counter(int(x) for x in wl)
        assert max(cnt.values()) == 1, ("a unit twice in the worklist", f)
        missing = passing - set(cnt)
        assert not missing, ("a unit with a passing (segment, k) was dropped by the prefilter", f, sorted(missing)[:5])
        assert tables == want, f
    assert np.array_equal(np.sort(got[0][0]), np.sort(got[T.FLAG_DEBUG_NO_UNI_DRAIN][0]))
    ref = got[T.FLAG_DEBUG_NO_UNI_DRAIN][2]
    assert ref["half_drain"] == 0 and ref["unit_drain"] == 0, ref  # the reference is the general path


@pytest.mark.gpu
@pytest.mark.parametrize("n", [128, 150, 151, 190])
def test_half_drain_short(n):
    reads, cats, passing, want = short_case(n)
    check_non_vacuous(cats, passing)
    words, _, _ = capi.pack_reads(reads)
    got = {f: _run(T.MODE_SHORT, words, len(reads), n, f) for f in FLAGS}
    _check(got, passing, want)
    c = got[0][2]
    nh = [_n_halves(r.decode(), n) for r in reads]
    both = sum(1 for a, b in nh if a and b)
    assert both >= 50
    assert c["half_drain"] + c["unit_drain"] >= sum(1 for a, b in nh if a or b), c  # every read with an N is drained once
    assert c["half_drain"] + c["unit_drain"] <= len(reads), c
    assert c["unit_drain"] >= both, c  # an N in both halves: a whole unit
    if n == 190:  # no joint fast loop at this length: no per-half verdicts, whole units only
        assert c["half_drain"] == 0, c
    else:
        assert c["half_drain"] > 0, c
        assert c["half_drain"] <= len(reads) - both, c


@pytest.mark.gpu
def test_half_drain_pairs():
    n = 150
    r1, r2, cats, passing, want = pair_case(n)
    check_non_vacuous(cats, passing)
    inter = [r for ab in zip(r1, r2) for r in ab]
    words, _, _ = capi.pack_reads(inter)
    got = {f: _run(T.MODE_PAIR, words, len(inter), n, f) for f in FLAGS}
    _check(got, passing, want)
    c = got[0][2]
    assert c["half_drain"] > 0 and c["unit_drain"] > 0, c
    assert c["half_drain"] + c["unit_drain"] <= len(r1), c


@pytest.mark.gpu
def test_half_drain_end_of_input_only():
    """70 reads: one block, one round, nothing but the end-of-input drains of both lists."""
    n = 150
    reads, cats, passing, _ = short_case(n)
    reads, passing = reads[:70], {i for i in passing if i < 70}
    assert len(passing) >= 10
    want = O.run_short(O.OracleParams(), reads)
    words, _, _ = capi.pack_reads(reads)
    got = {f: _run(T.MODE_SHORT, words, len(reads), n, f) for f in FLAGS}
    _check(got, passing, want)
    c = got[0][2]
    assert c["half_drain"] > 0 and c["unit_drain"] > 0, c
    assert c["half_drain"] + c["unit_drain"] <= 70, c


@pytest.mark.gpu
def test_half_drain_block_fulls():
    """The 2 400 reads of the 150-bp case a thousand times over: every persistent block takes several rounds, so both lists
    reach a block-full in mid-stream.  The verdict of a read does not depend on its neighbours: the worklist is the small
    batch's, tiled."""
    n, times = 150, 1000
    reads, _, _, _ = short_case(n)
    words, _, _ = capi.pack_reads(reads)
    stride = 3 * ((n + 31) // 32)
    body = words[: len(reads) * stride]
    small, _, _ = _run(T.MODE_SHORT, words, len(reads), n, 0, tables=False)
    big, _, c = _run(T.MODE_SHORT, np.ascontiguousarray(np.tile(body, times)), times * len(reads), n, 0, tables=False)
    want = (np.sort(small).astype(np.int64)[None, :] + len(reads) * np.arange(times, dtype=np.int64)[:, None]).ravel()
    assert np.array_equal(np.sort(big).astype(np.int64), want)
    assert c["half_drain"] > 0 and c["unit_drain"] > 0, c


@pytest.mark.gpu
def test_half_drain_repeated_passes_are_identical():
    """20 passes over a 300 k-read device-generated batch give the same worklist (a regression check on the barrier windows
    around the two list lengths, not a detector)."""
    n, L = 300_000, 150
    stride = 3 * ((L + 31) // 32)
    with T.TrewHip(mode=T.MODE_SHORT, max_batch_reads=n, max_batch_words=16, table_log2_slots=20) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        first = None
        for _ in range(20):
            t.submit(t.device_uniform_batch(d, n, L))
            t.wait()
            wl = np.sort(t.debug_worklist(0))
            if first is None:
                first = wl
                assert len(first) > 1000
            assert np.array_equal(wl, first)
        t.free(d)
