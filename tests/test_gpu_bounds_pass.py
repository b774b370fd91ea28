"""The bounds pass (kernels/bounds_pass.inc): the packed bounds of the flagged short reads, computed a lane per half between the
prefilter and the exact kernel, and read back by the rows of the group pass (run_short_group) instead of being bounded there.

Every case runs one batch four ways and wants bit-equal tables from all of them:

  default    the bounds pass covers every flagged read of these small batches;
  small      TREW_FLAG_DEBUG_SMALL_BOUNDS: it covers 64 worklist entries, later ones are bounded in row layout -- both in one batch;
  nogroup    TREW_FLAG_DEBUG_NO_GROUP: no group pass, no bounds pass, a wave per segment;
  oracle     the CPU oracle.

The worklist of the three GPU runs must be the same.  The prefilter appends in the order its waves and blocks get there (on an
MI355X even the four waves of one block come in either order from run to run), so "the same" is stated on the sorted worklist,
with no unit twice.

A word about the k ranges.  MIN_MER >= 3 (trew_hip_init) and 64-bit words end at MAX_MER = 32, so the widest range the stored
bounds ever see has 30 indices: 3..32.  A range with exactly 32 indices needs MAX_MER > 32, i.e. 128-bit words, which keep the row
layout by design; 5..36 is run all the same: it pins that such a context queues no bounds pass and computes what it did."""
import functools
import random

import numpy as np
import pytest

import edge_cases as E
import oracle as O
import trew_amd as T
from helpers import mutate, periodic
from test_gpu_half_drain import short_case
from test_gpu_parity import _table_diff
from trew_amd import capi

pytestmark = pytest.mark.gpu

DEFAULT, SMALL, NOGROUP = 0, T.FLAG_DEBUG_SMALL_BOUNDS, T.FLAG_DEBUG_NO_GROUP
GPU_RUNS = (DEFAULT, SMALL, NOGROUP)
PS_DEFAULT = (5, 32, 0.5, 0.8)
TELO = "TTAGGG"
SMALL_CAP = 64  # entries of the hand-over buffer with TREW_FLAG_DEBUG_SMALL_BOUNDS (include/trew_hip.h)


def _acgt(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _halves(n):
    return (0, n // 2), (n - (n + 1) // 2, (n + 1) // 2)


def _put(s, positions, c="N"):
    s = list(s)
    for p in positions:
        s[p] = c
    return "".join(s)


def _context(ps, flags, max_reads=4096):
    mn, mx, low, high = ps
    return T.TrewHip(mode=T.MODE_SHORT, min_mer=mn, max_mer=mx, low=low, high=high, max_batch_reads=max_reads, max_batch_words=1 << 19,
                     flags=flags)


def _batch(t, reads, uniform):
    words, offs, lens = capi.pack_reads(reads)
    if not uniform:
        return t.host_batch(words, offs, lens)
    n = len(reads[0])
    assert all(len(r) == n for r in reads)
    stride = 3 * ((n + 31) // 32)
    b = capi.Batch(words.ctypes.data, len(words), None, None, n, stride, len(reads), 0, n)
    b._keep = (words,)
    return b


def _gpu(reads, ps, flags, uniform, passes=1):
    """(worklist, tables) of every pass of the batch on slot 0 of one context"""
    out = []
    with _context(ps, flags, max(len(reads) + 8, 256)) as t:
        b = _batch(t, reads, uniform)
        for _ in range(passes):
            t.reset_tables()
            t.submit(b, 0)
            t.wait(0)
            out.append((t.debug_worklist(0).copy(), t.collect()))
    return out


def _want(ps, reads):
    mn, mx, low, high = ps
    return O.run_short(O.OracleParams(min_mer=mn, max_mer=mx, low=low, high=high), reads)


def _four_ways(reads, ps, uniform, want=None, passes=1):
    """The comparison of one case; returns the default run's worklist."""
    want = _want(ps, reads) if want is None else want
    got = {f: _gpu(reads, ps, f, uniform, passes) for f in GPU_RUNS}
    first = got[DEFAULT][0][0]
    assert len(set(int(x) for x in first)) == len(first), "a unit twice in the worklist"
    for f in GPU_RUNS:
        for wl, tables in got[f]:
            assert np.array_equal(np.sort(wl), np.sort(first)), ("worklist", f)
            assert tables == want, ("flags %d" % f, _table_diff(tables, want))
    return first


# ---- flagged-read counts: lane fill of the bounds pass, pairing of the group pass, an odd read left without a partner ----

@functools.lru_cache(maxsize=None)
def _count_case(count, n=150):
    """`count` telomeric reads (distinct: phase and a few substitutions) among 64 random ones, which the prefilter does not flag"""
    rnd = random.Random(9100 + count)
    telo = [mutate(periodic(TELO, n, i % 6), rnd, p_sub=0.01 if i % 3 else 0.0) for i in range(count)]
    rand = [_acgt(rnd, n) for _ in range(64)]
    reads = rand[:32] + telo + rand[32:]
    return tuple(r.encode() for r in reads)


@pytest.mark.parametrize("count", [0, 1, 2, 31, 32, 33, 65])
def test_flagged_counts(count):
    """With the small buffer, 65 flagged reads leave the last one both without a partner and without stored bounds."""
    reads = list(_count_case(count))
    wl = _four_ways(reads, PS_DEFAULT, uniform=True)
    print("flagged %d of %d reads, %d wanted" % (len(wl), len(reads), count))
    assert len(wl) == count
    assert count <= SMALL_CAP or len(wl) > SMALL_CAP  # (65: an entry beyond the small buffer)


# ---- read lengths: halves of 64 (never three words), 75, 75 + 76 in one wave, 95 (91 windows at k = 5) ----

@pytest.mark.parametrize("n", [128, 150, 151, 190])
def test_lengths(n):
    """The 2 400 reads of test_gpu_half_drain.py at this length (telomeric, junction, near misses, one N at every edge of a half,
    an N in both halves): more than 64 are flagged, so the small buffer splits the worklist."""
    reads, cats, passing, want = short_case(n)
    wl = _four_ways(list(reads), PS_DEFAULT, uniform=True, want=want)
    assert len(wl) > 4 * SMALL_CAP and len(passing) >= 200


# ---- N: has_n, the more-than-four-N hand-back, N at the first and the last base of a half, in both halves ----

@functools.lru_cache(maxsize=None)
def _n_case():
    rnd = random.Random(9200)
    reads = []
    for n in (150, 151):
        (ls, ll), (rs, rl) = _halves(n)
        spots = {"first_left": [ls], "last_left": [ls + ll - 1], "first_right": [rs], "last_right": [rs + rl - 1],
                 "both_edges": [ls, ls + ll - 1, rs, rs + rl - 1]}
        for rep in range(6):
            base = mutate(periodic(TELO, n, rep), rnd, p_sub=0.01 * (rep % 2))
            for pos in spots.values():
                reads.append(_put(base, pos))
            for how_many in (1, 4, 5):
                left = rnd.sample(range(ls, ls + ll), how_many)
                right = rnd.sample(range(rs, rs + rl), how_many)
                reads += [_put(base, left), _put(base, right), _put(base, left + right)]
                reads.append(_put(base, list(range(ls + 20, ls + 20 + how_many))))  # adjacent N: one gap of windows
    return tuple(r.encode() for r in reads)


@pytest.mark.parametrize("uniform", [False], ids=["ragged"])
def test_n_in_halves(uniform):
    reads = list(_n_case())
    wl = _four_ways(reads, PS_DEFAULT, uniform)
    assert len(wl) > SMALL_CAP  # most of them are flagged: reads on either side of the small buffer


# ---- a ragged batch: the four lengths in one wave of the bounds pass, with reads too short for halves ----

@functools.lru_cache(maxsize=None)
def _ragged_case(mn):
    rnd = random.Random(9300 + mn)
    reads = []
    # No length in 96..127: with MAX_MER = 32 such a read has a whole-read segment of more than 95 bases, and the batch would go to
    # the 5-word kernels, which have no bounds pass (test_ragged_lengths_and_k_ranges asserts the geometry).
    lengths = [128, 150, 151, 190, 4 * mn - 1, 2 * mn, 4 * mn, 2 * mn - 1, 95, 64]
    for i in range(360):
        n = lengths[i % len(lengths)] if i % 11 else rnd.choice([rnd.randint(1, 95), rnd.randint(128, 190)])
        kind = i % 5
        if kind == 0:
            s = _acgt(rnd, n)
        elif kind == 1:
            s = periodic(TELO, n, rnd.randint(0, 5))
        elif kind == 2:
            unit = _acgt(rnd, rnd.randint(1, 12))
            s = mutate(periodic(unit, n, rnd.randint(0, 3)), rnd, p_sub=0.03)
        elif kind == 3:
            s = mutate(periodic(TELO, n), rnd, p_sub=0.02, p_n=0.02)
        else:
            h = n // 2
            s = periodic(TELO, h) + _acgt(rnd, n - h)
        reads.append(s)
    return tuple(r.encode() for r in reads)


# k ranges: the defaults; a narrow one (bound words above MAX_MER are empty); the widest 64-bit words allow (30 indices); 32 indices
# (128-bit words: no bounds pass, see the module's docstring)
K_RANGES = [(5, 32, 0.5, 0.8), (10, 20, 0.5, 0.8), (3, 32, 0.5, 0.8), (5, 36, 0.5, 0.8)]


@pytest.mark.parametrize("ps", K_RANGES, ids=lambda ps: "%d-%d" % ps[:2])
def test_ragged_lengths_and_k_ranges(ps):
    reads = list(_ragged_case(ps[0]))
    longest = max(ln for r in reads for _, _, _, ln, _, _ in E.segments(E.SHORT, len(r), len(r), ps[0], ps[1]))
    assert longest == 95 or ps[1] > 32  # the 3-word kernels: halves of 190-base reads, and no longer whole-read segment
    assert sum(1 for r in reads if len(r) < 4 * ps[0]) >= 20  # reads without halves among them
    wl = _four_ways(reads, ps, uniform=False)
    assert len(wl) > SMALL_CAP


@pytest.mark.parametrize("ps", K_RANGES[:3], ids=lambda ps: "%d-%d" % ps[:2])
def test_uniform_k_ranges(ps):
    """The same ranges on a uniform batch of 151-base reads (halves of 75 and 76)."""
    reads, _, _, want = short_case(151)
    reads = list(reads[:700])
    wl = _four_ways(reads, ps, uniform=True, want=want if ps == PS_DEFAULT and len(reads) == 2400 else None)
    assert len(wl) > SMALL_CAP


# ---- reads on the pass/fail edge, for LOW and for HIGH ----

def _records_high(p, read):
    return any(len(tb) for name, tb in O.run_short(p, [read]).items() if name.endswith("_high"))


@functools.lru_cache(maxsize=None)
def _high_edge_pairs(ps, n, chains=60):
    """edge_cases.chain with 'the oracle records something for HIGH_BASELINE' as the property that one substitution ends"""
    rnd = random.Random("bounds-pass-high|%r|%d" % (ps, n))
    p = E.params(ps)
    out = []
    for _ in range(chains):
        start, pos = E._start(rnd, E.SHORT, ps, n, n, 150)
        read = start[0].encode()
        if not _records_high(p, read):
            continue
        rnd.shuffle(pos)
        for i in pos:
            other = rnd.choice([c for c in b"ACGTN" if c != read[i]])
            nxt = read[:i] + bytes([other]) + read[i + 1:]
            if not _records_high(p, nxt):
                out.append((read, nxt))
                break
            read = nxt
    return tuple(out)


@pytest.mark.parametrize("ps", [E.PARAM_SETS[0], E.PARAM_SETS[3]], ids=["0.5-0.8", "0.667-0.9"])
@pytest.mark.parametrize("n", [150, 151])
def test_edge_reads(ps, n):
    low_pairs = E.edge_pairs(E.SHORT, ps, n)
    high_pairs = _high_edge_pairs(ps, n)
    assert len(low_pairs) >= 30 and len(high_pairs) >= 20, (len(low_pairs), len(high_pairs))
    reads = [a[0] for a, _ in low_pairs] + [b[0] for _, b in low_pairs] + [a for a, _ in high_pairs] + [b for _, b in high_pairs]
    wl = _four_ways(reads, ps, uniform=True)
    assert len(wl) > SMALL_CAP


# ---- three passes on one slot: both counter blocks, the buffer written three times ----

def test_three_passes_on_one_slot():
    reads, _, _, want = short_case(150)
    _four_ways(list(reads), PS_DEFAULT, uniform=True, want=want, passes=3)
