"""The set-up of a read in the prefilter's joint loop (kernels/prefilter.inc, 3-word kernel): the read is loaded once
(load_read5), one prefix parity per plane serves both halves (halves_prefix_read5), and the has-N test of each half reads the
raw N words against masks for [0, L) and [start_B, start_B + len_B).  None of it may change a verdict.

Read lengths inside the joint loop at 5..32 (128, 129, 150, 151, 152, 153 single-end, 2 x 150 and 2 x 151 paired) and just outside
it (127, 154, which keep the per-segment loops).  Reads are 2 400 per case -- ten blocks of one round each, which the end-of-input
drains handle -- random, telomeric (all six phases, both strands) and junction reads (both orientations), with one N planted at
each word border of the read, around the right half's start, at the last base, and a second N in the other half.

Every case runs with default flags, with TREW_FLAG_DEBUG_NO_JOINT and with TREW_FLAG_DEBUG_NO_UNI_DRAIN: the sorted worklists
of the three runs are equal, every read the oracle accepts is flagged, and the collected tables equal the oracle's.

Reads of 159 and 160 bases at 9..32 (test_read_setup_at_the_five_word_edge) reach the joint loop outside 5..32: 159 is the
longest read the one load takes, and at 160 bit L of the right half's prefix parity would be bit 160 of the read's, which five
words do not hold, so that length keeps a prefix parity per half.

The last four tests pin the drain of whole units (filter_deferred_uni) on the reads that fill it: telomeric reads alone, the
same among reads with an N in each half, both tiled until the list reaches block-fulls in mid-stream, and hand-built reads whose
halves each pass four buckets at some k and eight at none, which sit among telomeric reads and must come out unflagged."""
import functools
import os
import random

import numpy as np
import pytest

import oracle as O
import trew_amd as T
from trew_amd import capi
from helpers import periodic

FLAGS = (0, T.FLAG_DEBUG_NO_JOINT, T.FLAG_DEBUG_NO_UNI_DRAIN)
N_UNITS = 2400  # not a multiple of the block's 256
TELO = ("TTAGGG", "CCCTAA")  # both strands
JOINT_LENGTHS = (128, 129, 150, 151, 152, 153)  # halves of 64 .. 77
OUTSIDE_LENGTHS = (127, 154)                    # 5..32 has a k with fewer than 33 / more than 72 windows: no joint loop
BASES = ("random", "telomeric", "junction")


def _right_start(n):
    return n - (n + 1) // 2


def _acgt(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _base_read(rnd, kind, i, n):
    """i picks phase, strand and orientation in turn, so that 2 400 reads hold every combination many times"""
    unit, phase = TELO[(i // 6) % 2], i % 6
    if kind == "telomeric":
        return periodic(unit, n, phase)
    if kind == "junction":
        h = n // 2
        if (i // 12) % 2:
            return periodic(unit, h, phase) + _acgt(rnd, n - h)
        return _acgt(rnd, h) + periodic(unit, n - h, phase)
    return _acgt(rnd, n)


def n_sites(n):
    """where an N is planted: None = no N; a tuple = the positions"""
    h = _right_start(n)
    single = sorted({p for p in (0, 31, 32, 63, 64, 95, 96, 127, 128, h - 1, h, h + 1, n - 1) if 0 <= p < n})
    sites = [None] + [(p,) for p in single]
    # a second N in the other half
    sites += [(p, n - 1 - p) for p in (0, 31, 32, 63, h - 1) if p < h and n - 1 - p >= h] + [(h - 1, h), (0, n - 1)]
    return sites


def _plant(s, pos):
    s = list(s)
    for p in pos or ():
        s[p] = "N"
    return "".join(s)


def make_reads(n, seed, count=N_UNITS):
    rnd = random.Random(seed)
    sites = n_sites(n)
    reads = []
    for i in range(count):
        m = i // len(BASES)  # every kind of read meets every site, and every site every phase, strand and orientation
        reads.append(_plant(_base_read(rnd, BASES[i % len(BASES)], m // len(sites), n), sites[m % len(sites)]).encode())
    return reads


@functools.lru_cache(maxsize=None)
def short_case(n):
    """(reads, indices the oracle accepts, the oracle's tables): computed once per length and left unchanged"""
    reads = make_reads(n, 9100 + n)
    p = O.OracleParams()
    passing = frozenset(i for i, r in enumerate(reads) if any(len(tb) for tb in O.run_short(p, [r]).values()))
    return reads, passing, O.run_short(p, reads)


@functools.lru_cache(maxsize=None)
def pair_case(n):
    r1 = make_reads(n, 9500 + n)
    r2 = make_reads(n, 9700 + n)
    r2 = r2[7:] + r2[:7]  # mate 2 out of step with mate 1: every combination of kinds and N sites over the four halves
    p = O.OracleParams()
    passing = frozenset(i for i in range(len(r1)) if any(len(tb) for tb in O.run_pair(p, [r1[i]], [r2[i]]).values()))
    return r1, r2, passing, O.run_pair(p, r1, r2)


def _run(mode, words, n_reads, n, flags, tables=True, **params):
    stride = 3 * ((n + 31) // 32)
    with T.TrewHip(mode=mode, max_batch_reads=n_reads + 8, max_batch_words=max(len(words) + 64, 1 << 20), flags=flags, **params) as t:
        t.reset_tables()  # the drains' counters are kept per device
        b = capi.Batch(words.ctypes.data, len(words), None, None, n, stride, n_reads, 0, 0)  # uniform batch: the fast path
        t.submit(b, 0)
        t.wait(0)
        wl = t.debug_worklist(0).copy()
        return wl, (t.collect() if tables else None), t.debug_counters()


def _check(got, passing, want):
    lists = {f: np.sort(got[f][0]) for f in FLAGS}
    for f in FLAGS:
        wl = lists[f]
        assert len(wl) == len(np.unique(wl)), ("a unit twice in the worklist", f)
        missing = passing - set(int(x) for x in wl)
        assert not missing, ("a unit the oracle accepts was dropped by the prefilter", f, sorted(missing)[:5])
        assert got[f][1] == want, f
    for f in FLAGS[1:]:
        assert np.array_equal(lists[0], lists[f]), f


def _non_vacuous(reads, passing, n):
    h = _right_start(n)
    assert len(passing) >= 200
    assert sum(1 for r in reads if b"N" in r[:n // 2] and b"N" in r[h:]) >= 50  # whole units because of Ns
    assert sum(1 for r in reads if b"N" not in r) >= 50
    for p in (0, h - 1, h, n - 1):
        assert sum(1 for r in reads if r[p:p + 1] == b"N") >= 50, p


@pytest.mark.gpu
@pytest.mark.parametrize("n", JOINT_LENGTHS + OUTSIDE_LENGTHS)
def test_read_setup_short(n):
    reads, passing, want = short_case(n)
    _non_vacuous(reads, passing, n)
    words, _, _ = capi.pack_reads(reads)
    got = {f: _run(T.MODE_SHORT, words, len(reads), n, f) for f in FLAGS}
    _check(got, passing, want)
    c = got[0][2]
    if n in JOINT_LENGTHS:  # the joint loop ran: it is what fills the half list
        assert c["half_drain"] > 0 and c["unit_drain"] > 0, c
    else:
        assert c["half_drain"] == 0, c
    assert got[T.FLAG_DEBUG_NO_JOINT][2]["half_drain"] == 0
    ref = got[T.FLAG_DEBUG_NO_UNI_DRAIN][2]
    assert ref["half_drain"] == 0 and ref["unit_drain"] == 0, ref


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 151])
def test_read_setup_pairs(n):
    """2 x 151: the first mate's halves (75 and 76) take the joint loop, the second mate's (its right half comes first) do not."""
    r1, r2, passing, want = pair_case(n)
    _non_vacuous(r1, passing, n)
    inter = [r for ab in zip(r1, r2) for r in ab]
    words, _, _ = capi.pack_reads(inter)
    got = {f: _run(T.MODE_PAIR, words, len(inter), n, f) for f in FLAGS}
    _check(got, passing, want)
    c = got[0][2]
    assert c["unit_drain"] > 0, c


def _telomeric_only(n, count):
    return [periodic(TELO[(i // 6) % 2], n, i % 6).encode() for i in range(count)]


def _n_in_each_half(n, count, seed):
    rnd = random.Random(seed)
    h = _right_start(n)
    return [_plant(_acgt(rnd, n), (rnd.randrange(0, n // 2), rnd.randrange(h, n))).encode() for _ in range(count)]


@pytest.mark.gpu
def test_telomeric_batch_is_all_whole_units():
    """Telomeric reads without an N: both halves pass four buckets, so every read is a whole unit, and every one is flagged."""
    n = 150
    reads = _telomeric_only(n, N_UNITS)
    words, _, _ = capi.pack_reads(reads)
    wl, _, c = _run(T.MODE_SHORT, words, len(reads), n, 0, tables=False)
    assert c["unit_drain"] == len(reads) and c["half_drain"] == 0, c
    assert np.array_equal(np.sort(wl), np.arange(len(reads)))


@pytest.mark.gpu
def test_telomeric_batch_interleaved_with_n_units():
    """The same reads interleaved with reads that carry an N in each half: all of them whole units; the telomeric ones are
    flagged, and the others exactly where the general path flags them."""
    n = 150
    telo, withn = _telomeric_only(n, N_UNITS // 2), _n_in_each_half(n, N_UNITS // 2, 4242)
    reads = [r for ab in zip(telo, withn) for r in ab]
    words, _, _ = capi.pack_reads(reads)
    wl, _, c = _run(T.MODE_SHORT, words, len(reads), n, 0, tables=False)
    ref, _, _ = _run(T.MODE_SHORT, words, len(reads), n, T.FLAG_DEBUG_NO_UNI_DRAIN, tables=False)
    assert c["unit_drain"] == len(reads) and c["half_drain"] == 0, c
    assert np.array_equal(np.sort(wl), np.sort(ref))
    assert set(range(0, len(reads), 2)) <= set(int(x) for x in wl)


@pytest.mark.gpu
def test_whole_units_reach_block_fulls():
    """Telomeric reads, reads with an N in each half and random reads, a few hundred times over: every persistent block takes
    several rounds and the whole-unit list reaches a block-full in mid-stream with both kinds in it.  The verdict of a read does
    not depend on its neighbours: the worklist is the small batch's, tiled."""
    n, times = 150, 400
    rnd = random.Random(77)
    telo, withn = _telomeric_only(n, 800), _n_in_each_half(n, 800, 4343)
    reads = [r for abc in zip(telo, withn, (_acgt(rnd, n).encode() for _ in range(800))) for r in abc]
    words, _, _ = capi.pack_reads(reads)
    stride = 3 * ((n + 31) // 32)
    body = words[: len(reads) * stride]
    small, _, _ = _run(T.MODE_SHORT, words, len(reads), n, 0, tables=False)
    big, _, c = _run(T.MODE_SHORT, np.ascontiguousarray(np.tile(body, times)), times * len(reads), n, 0, tables=False)
    want = (np.sort(small).astype(np.int64)[None, :] + len(reads) * np.arange(times, dtype=np.int64)[:, None]).ravel()
    assert np.array_equal(np.sort(big).astype(np.int64), want)
    assert c["unit_drain"] >= 1600 * times, c


# ---- double near misses: both halves pass four buckets at some k and eight at none ----
# Such a read joins the telomeric ones in the list of whole units without an N and is never flagged there, so its wave runs
# the drain's k loop to the end.  Built by hand: copies of a random unit of 17..32 bases (twice that is past MAX_MER), in some of
# which an A and a T of the unit are a G and a C.  With T, G, C, A = 0, 1, 2, 3 as (hi, lo) that leaves the lo plane periodic
# and the number of hi bits of a window that holds both bases unchanged, so nearly all windows of that length share their two
# plane parities, while the parity of the As splits them.  The two tests are restated below on the bases themselves.
CODE = {"T": 0, "G": 1, "C": 2, "A": 3}


def bucket_verdicts(seg, kmin=5, kmax=32):
    """(some k passes the 4-bucket test, some k passes the 8-bucket test) of an N-free segment at LOW = 0.5: a test passes when
    twice its largest bucket reaches COUNT.  At 75 bases every k from 12 on has at most 64 windows, so the fast loop looks at
    all of them as this does; below that it looks at the first 64 against a threshold lowered by the rest, which passes
    whenever this does."""
    n = len(seg)
    planes = ([CODE[c] & 1 for c in seg], [CODE[c] >> 1 for c in seg], [int(c == "A") for c in seg])
    pre = []
    for v in planes:
        acc = [0]
        for x in v:
            acc.append(acc[-1] ^ x)
        pre.append(acc)
    pass4 = pass8 = False
    for k in range(kmin, kmax + 1):
        count = n - k + 1
        b4, b8 = {}, {}
        for i in range(count):
            key = tuple(p[i] ^ p[i + k] for p in pre)
            b4[key[:2]] = b4.get(key[:2], 0) + 1
            b8[key] = b8.get(key, 0) + 1
        pass4 = pass4 or 2 * max(b4.values()) >= count
        pass8 = pass8 or 2 * max(b8.values()) >= count
    return pass4, pass8


def _near_miss_half(rnd, n):
    while True:
        k = rnd.randint(17, 32)
        unit = [rnd.choice("ACGT") for _ in range(k)]
        ia, it = [i for i, c in enumerate(unit) if c == "A"], [i for i, c in enumerate(unit) if c == "T"]
        if not ia or not it:
            continue
        swaps = [(rnd.choice(ia), rnd.choice(it)) for _ in range(rnd.randint(1, 2))]
        out = []
        while len(out) < n + k:
            copy = list(unit)
            for p, q in swaps:
                if rnd.random() < 0.5:
                    copy[p], copy[q] = "G", "C"
            out += copy
        phase = rnd.randrange(k)
        seg = "".join(out[phase:phase + n])
        if bucket_verdicts(seg) == (True, False):
            return seg


@functools.lru_cache(maxsize=None)
def double_near_misses(n=150, count=60):
    """reads of two such halves that the oracle does not accept"""
    rnd = random.Random(31337)
    p = O.OracleParams()
    assert (p.min_mer, p.max_mer, n // 4) == (5, 32, 37) and p.low == 0.5  # what bucket_verdicts restates
    reads = []
    while len(reads) < count:
        r = (_near_miss_half(rnd, n // 2) + _near_miss_half(rnd, n // 2)).encode()
        if not any(len(tb) for tb in O.run_short(p, [r]).values()):
            reads.append(r)
    return reads


@pytest.mark.gpu
def test_double_near_misses_stay_unflagged_among_telomeric_reads():
    n = 150
    misses = double_near_misses(n)
    assert len(misses) >= 50
    reads = _telomeric_only(n, N_UNITS)
    where = [17 + 37 * i for i in range(len(misses))]  # spread over the waves: every one of them shares its wave with telomeric reads
    assert where[-1] < len(reads)
    for at, r in zip(where, misses):
        reads[at] = r
    words, _, _ = capi.pack_reads(reads)
    wl, _, c = _run(T.MODE_SHORT, words, len(reads), n, 0, tables=False)
    ref, _, _ = _run(T.MODE_SHORT, words, len(reads), n, T.FLAG_DEBUG_NO_UNI_DRAIN, tables=False)
    assert c["unit_drain"] == len(reads) and c["half_drain"] == 0, c  # both halves of every read passed four buckets
    assert np.array_equal(np.sort(wl), np.sort(ref))
    assert np.array_equal(np.sort(wl), np.array(sorted(set(range(len(reads))) - set(where)), dtype=wl.dtype))


# ---- the edge of the five words: 159 and 160 bases at 9..32 ----
# tests/golden/read_setup_tight_halves.txt: 64 halves of 80 bases that sit ON the threshold.  Each is a random unit of 17..32
# bases repeated, with 8..20 % of the bases replaced, kept when (k from 9 to 32, the tests restated as in bucket_verdicts)
#   - every k that passes four buckets is at least 17 (at most 64 windows: the container range of the joint loop), passes
#     with the smallest largest bucket that can (2 m4 - COUNT is 0 or 1) and has its LAST window in that bucket, and
#   - some such k passes eight buckets as well, so the read has to be flagged.
# One window of such a half in another bucket and the half is not set aside: the last window is the one whose parity needs
# bit L of the half's prefix parity.  About one candidate in 200 qualifies, hence a fixture; the properties are checked below.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_setup_tight_halves.txt")
EDGE_PARAMS = dict(min_mer=9, max_mer=32)


def _k_stats(seg, kmin, kmax):
    """(k, COUNT, largest of four buckets, largest of eight, the last window is in the largest of four) per k"""
    n = len(seg)
    planes = ([CODE[c] & 1 for c in seg], [CODE[c] >> 1 for c in seg], [int(c == "A") for c in seg])
    pre = []
    for v in planes:
        acc = [0]
        for x in v:
            acc.append(acc[-1] ^ x)
        pre.append(acc)
    out = []
    for k in range(kmin, kmax + 1):
        count = n - k + 1
        b4, b8 = {}, {}
        for i in range(count):
            key = tuple(p[i] ^ p[i + k] for p in pre)
            b4[key[:2]] = b4.get(key[:2], 0) + 1
            b8[key] = b8.get(key, 0) + 1
        m4 = max(b4.values())
        out.append((k, count, m4, max(b8.values()), b4[key[:2]] == m4))
    return out


def _odd_parities(read):
    """the read with its first base chosen so that the numbers of lo bits and of hi bits of the whole read are both odd: bit
    n of the read's prefix parities is then 1 in both planes"""
    lo = sum(CODE[c] & 1 for c in read[1:]) & 1
    hi = sum(CODE[c] >> 1 for c in read[1:]) & 1
    first = {v: c for c, v in CODE.items()}[(1 - lo) | ((1 - hi) << 1)]
    return first + read[1:]


@functools.lru_cache(maxsize=None)
def edge_case(n):
    """(reads, indices the oracle accepts, the oracle's tables, indices the 8-bucket bound of a half keeps: those must be flagged)"""
    tight = open(GOLDEN).read().split()
    assert len(tight) >= 60 and all(len(h) == 80 and set(h) <= set("ACGT") for h in tight)
    for h in tight:  # the fixture is what the comment above says
        passes = [x for x in _k_stats(h, 9, 32) if 2 * x[2] >= x[1]]
        assert passes and all(k >= 17 and 2 * m4 - c <= 1 and last for k, c, m4, _, last in passes)
        assert any(2 * m8 >= c for _, c, _, m8, _ in passes)
    rnd = random.Random(1590 + n)
    reads = [r.decode() for r in make_reads(n, 9900 + n)]
    h = _right_start(n)
    where = [11 + 18 * i for i in range(2 * len(tight))]
    assert where[-1] < len(reads)
    for i, at in enumerate(where):
        half = tight[i // 2]
        if i % 2 == 0 or n % 2:  # as the right half (80 bases at both lengths); total parities odd
            reads[at] = _odd_parities(_acgt(rnd, h) + half)
        else:  # as the left half of a 160-base read
            reads[at] = half + _acgt(rnd, n - len(half))
    assert all(len(r) == n for r in reads)
    (ls, ll), (rs, rl) = (0, n // 2), (h, n - h)
    must = frozenset(at for at in where
                     if any(2 * m8 >= c for seg in (reads[at][ls:ls + ll], reads[at][rs:rs + rl]) for _, c, _, m8, _ in _k_stats(seg, 9, min(32, n // 4))))
    assert len(must) >= 100
    assert sum(1 for at in where if sum(CODE[c] & 1 for c in reads[at]) % 2 and sum(CODE[c] >> 1 for c in reads[at]) % 2) >= 60
    reads = [r.encode() for r in reads]
    p = O.OracleParams(**EDGE_PARAMS)
    passing = frozenset(i for i, r in enumerate(reads) if any(len(tb) for tb in O.run_short(p, [r]).values()))
    return reads, passing, O.run_short(p, reads), must


@pytest.mark.gpu
@pytest.mark.parametrize("n", [159, 160])
def test_read_setup_at_the_five_word_edge(n):
    reads, passing, want, must = edge_case(n)
    _non_vacuous(reads, passing, n)
    words, _, _ = capi.pack_reads(reads)
    got = {f: _run(T.MODE_SHORT, words, len(reads), n, f, **EDGE_PARAMS) for f in FLAGS}
    _check(got, passing, want)
    for f in FLAGS:
        missing = must - set(int(x) for x in got[f][0])
        assert not missing, ("a read with a half on the threshold was dropped", f, sorted(missing)[:5])
    c = got[0][2]
    assert c["half_drain"] > 0 and c["unit_drain"] > 0, c  # the joint loop ran at this geometry
    assert got[T.FLAG_DEBUG_NO_JOINT][2]["half_drain"] == 0
