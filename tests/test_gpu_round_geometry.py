"""The prefilter's batch geometry (FilterGeom, trew_common.hpp): filter_kernel no longer derives the segment geometry of a batch
of equal-length reads in every round, it reads a block the host fills once per read length, behind the threshold table.  What can
go wrong is a block that is wrong at an edge, or stale; none of it may change a verdict.

Edges -- every read length at which the block changes kind, 2 400 reads each (the random, telomeric and junction reads with N
sites of tests/test_gpu_read_setup.py), with default flags, TREW_FLAG_DEBUG_NO_JOINT and TREW_FLAG_DEBUG_NO_UNI_DRAIN: the three
sorted worklists are equal, every read the oracle accepts is flagged, the tables equal the oracle's.

    single-end, 5..32   127, 128, 129   the joint loop's lower edge
                        150, 151        equal halves, and a right half one base longer
                        153, 154        its upper edge
                        190             no joint loop, the whole-unit drain alone
                        120             a whole-read segment exists: the 5-word kernel, no joint loop, no uniform drain
    single-end, 9..32   159, 160        both halves from one load of the read against a load per half
    paired, 5..32       2 x 150, 2 x 151

Staleness -- a slot keeps its block until the read length changes: 150, 151, 128, 150 on one slot, then a longer sequence over two
slots, then a ragged batch (which has no block) between two uniform ones; every submit must give the worklist and the tables of a
fresh context handed that batch alone.  And one batch tiled so that every persistent block takes many rounds on one block:
nothing a round leaves behind may reach the next (compared with the TREW_FLAG_DEBUG_NO_JOINT run of the same batch)."""
import functools
import random

import numpy as np
import pytest

import oracle as O
import trew_amd as T
from trew_amd import capi

import test_gpu_read_setup as RS

FLAGS = RS.FLAGS
SHORT_LENGTHS = (127, 128, 129, 150, 151, 153, 154, 190, 120)


def _counters_fit(n, got, joint, uni_drain):
    """the path the block chose is the one the table above names"""
    c = got[0][2]
    if joint:
        assert c["half_drain"] > 0 and c["unit_drain"] > 0, (n, c)
    else:
        assert c["half_drain"] == 0, (n, c)  # only the joint loop fills the half list
        assert (c["unit_drain"] > 0) == uni_drain, (n, c)
    assert got[T.FLAG_DEBUG_NO_JOINT][2]["half_drain"] == 0
    ref = got[T.FLAG_DEBUG_NO_UNI_DRAIN][2]
    assert ref["half_drain"] == 0 and ref["unit_drain"] == 0, ref


@pytest.mark.gpu
@pytest.mark.parametrize("n", SHORT_LENGTHS)
def test_block_at_every_edge_short(n):
    reads, passing, want = RS.short_case(n)
    RS._non_vacuous(reads, passing, n)
    words, _, _ = capi.pack_reads(reads)
    got = {f: RS._run(T.MODE_SHORT, words, len(reads), n, f) for f in FLAGS}
    RS._check(got, passing, want)
    _counters_fit(n, got, joint=128 <= n <= 153, uni_drain=n >= 128)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [159, 160])
def test_block_one_load_against_two_loads(n):
    reads, passing, want, must = RS.edge_case(n)
    words, _, _ = capi.pack_reads(reads)
    got = {f: RS._run(T.MODE_SHORT, words, len(reads), n, f, **RS.EDGE_PARAMS) for f in FLAGS}
    RS._check(got, passing, want)
    for f in FLAGS:
        assert not must - set(int(x) for x in got[f][0]), f
    _counters_fit(n, got, joint=True, uni_drain=True)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 151])
def test_block_pairs(n):
    r1, r2, passing, want = RS.pair_case(n)
    inter = [r for ab in zip(r1, r2) for r in ab]
    words, _, _ = capi.pack_reads(inter)
    got = {f: RS._run(T.MODE_PAIR, words, len(inter), n, f) for f in FLAGS}
    RS._check(got, passing, want)
    c = got[0][2]
    assert c["unit_drain"] > 0, c
    if n == 151:
        # the second mate's right half comes first and is the longer one, so the joint loop leaves that mate to the per-segment
        # loops and no unit can go to the half list
        assert c["half_drain"] == 0, c


@functools.lru_cache(maxsize=None)
def single_half_pairs(n):
    """Pairs of which exactly ONE of the four halves has to be judged by a drain -- it holds an N, or it is telomeric -- and clean
    pairs between them: with 2 x 150 these are the units of the half list, and the slot handed to the drain is the block's
    slot_p / slot_q of that pair of halves (the second mate has its right half in the first slot)."""
    rnd = random.Random(7700 + n)
    h = RS._right_start(n)
    spans = ((0, 0, n // 2), (0, h, n), (1, h, n), (1, 0, n // 2))  # (mate, first base, end) of slots 0..3
    r1, r2 = [], []
    for i in range(RS.N_UNITS):
        mates = [RS._acgt(rnd, n), RS._acgt(rnd, n)]
        mate, a, b = spans[i % 4]
        how = (i // 4) % 3
        if how == 0:  # an N, walking through the half, its first and last base included
            pos = a + (i // 12) % (b - a)
            mates[mate] = RS._plant(mates[mate], (pos,))
        elif how == 1:  # the half telomeric, the rest of the read random
            t = RS.periodic(RS.TELO[(i // 12) % 2], b - a, (i // 24) % 6)
            mates[mate] = mates[mate][:a] + t + mates[mate][b:]
        r1.append(mates[0].encode())
        r2.append(mates[1].encode())
    p = O.OracleParams()
    passing = frozenset(i for i in range(len(r1)) if any(len(tb) for tb in O.run_pair(p, [r1[i]], [r2[i]]).values()))
    return r1, r2, passing, O.run_pair(p, r1, r2)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 151])
def test_block_pairs_one_half_to_judge(n):
    r1, r2, passing, want = single_half_pairs(n)
    # the oracle accepts the pairs whose telomeric half is a left one (slots 0 and 3); the prefilter has to flag the others as
    # well: every window of a telomeric half at k = 6 is of one class, so its largest bucket is COUNT
    assert len(passing) >= 400 and all(sum(1 for i in passing if i % 4 == slot) >= 150 for slot in (0, 3))
    telomeric = frozenset(i for i in range(len(r1)) if (i // 4) % 3 == 1)
    inter = [r for ab in zip(r1, r2) for r in ab]
    words, _, _ = capi.pack_reads(inter)
    got = {f: RS._run(T.MODE_PAIR, words, len(inter), n, f) for f in FLAGS}
    RS._check(got, passing, want)
    for f in FLAGS:
        missing = telomeric - set(int(x) for x in got[f][0])
        assert not missing, ("a pair with one telomeric half was dropped", f, sorted(missing)[:5], [i % 4 for i in sorted(missing)[:5]])
    c = got[0][2]
    if n == 150:  # all four halves went through the joint loop: two units in three have one half to judge
        assert c["half_drain"] >= RS.N_UNITS // 2, c
    else:
        assert c["half_drain"] == 0 and c["unit_drain"] > 0, c


# ---- staleness ----
def _uniform_batch(n):
    reads, _, want = RS.short_case(n)
    words, _, _ = capi.pack_reads(reads)
    return words, len(reads), want


def _fresh_worklist(n, _cache={}):
    if n not in _cache:
        words, count, _ = _uniform_batch(n)
        _cache[n] = np.sort(RS._run(T.MODE_SHORT, words, count, n, 0, tables=False)[0])
    return _cache[n]


def _submit_uniform(t, n, slot):
    words, count, want = _uniform_batch(n)
    stride = 3 * ((n + 31) // 32)
    t.reset_tables()
    t.submit(capi.Batch(words.ctypes.data, len(words), None, None, n, stride, count, 0, 0), slot)
    t.wait(slot)
    assert np.array_equal(np.sort(t.debug_worklist(slot)), _fresh_worklist(n)), ("worklist", n, slot)
    assert t.collect() == want, ("tables", n, slot)


def _context():
    return T.TrewHip(mode=T.MODE_SHORT, n_slots=2, max_batch_reads=RS.N_UNITS + 8, max_batch_words=1 << 20)


@pytest.mark.gpu
def test_block_follows_the_read_length_on_one_slot():
    with _context() as t:
        for n in (150, 151, 128, 150):
            _submit_uniform(t, n, 0)


@pytest.mark.gpu
def test_block_follows_the_read_length_on_two_slots():
    """slot 0 sees 150, 128, 151, 150 and slot 1 sees 151, 150, 128, 128: each slot has a block of its own"""
    with _context() as t:
        for i, n in enumerate((150, 151, 128, 150, 151, 128, 150, 128)):
            _submit_uniform(t, n, i % 2)


@pytest.mark.gpu
def test_ragged_batch_between_uniform_ones():
    """a ragged batch has no threshold table and no block (the general path); the slot's block of before must still serve after"""
    mixed = [r for n in (150, 128, 151, 190, 120) for r in RS.short_case(n)[0][:300]]
    want = O.run_short(O.OracleParams(), mixed)
    with _context() as t:
        _submit_uniform(t, 150, 0)
        t.reset_tables()
        t.submit_reads(mixed, 0)
        t.wait(0)
        assert t.collect() == want
        _submit_uniform(t, 150, 0)
        _submit_uniform(t, 151, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 151])
def test_many_rounds_on_one_block(n):
    """The 2 400 reads a thousand times over: every persistent block takes several rounds, and both lists reach block-fulls in
    mid-stream.  The worklist, as a multiset, is that of the run without the joint loop."""
    times = 1000
    words, count, _ = _uniform_batch(n)
    body = np.ascontiguousarray(np.tile(words[: count * 3 * ((n + 31) // 32)], times))
    big, _, c = RS._run(T.MODE_SHORT, body, times * count, n, 0, tables=False)
    ref, _, _ = RS._run(T.MODE_SHORT, body, times * count, n, T.FLAG_DEBUG_NO_JOINT, tables=False)
    assert np.array_equal(np.sort(big), np.sort(ref))
    assert len(big) == times * len(_fresh_worklist(n))
    assert c["half_drain"] > 0 and c["unit_drain"] > 0, c
