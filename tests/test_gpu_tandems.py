"""De novo repeats under indels, every tract of a read, on the GPU (trew_hip_tandems through ctypes).  Every record of every
batch is compared, integer for integer, with trew_tandems_host (itself checked against tests/tandem_ref.py in
test_tandems_cpu.py), and with tandem_ref where the reads are few or short."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import period_ref as P
import refine_ref as R
import tandem_ref as T
from period_cases import fuzz_reads, junk, noisy, rep
from refine_cases import TEL, UNITS
from repeat_cases import SAT, stack_reads
from tandem_cases import HAND, STRONG_FIRST, WEAK, WEAK_FIRST, extent_read, piece_bound_reads, piece_hi_reads, two_tract_set
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 20  # a log that holds every tract of every batch here
KS = (1, 2, 3, 6, 16, 31, 32)


def rec(x):
    return tuple(int(v) for v in x)


def same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in T.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at record %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_tandems(reads_or_packed, *args, mode=capi.MODE_LONG, max_records=BIG):
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16)) as t:
        t.tandems(t.host_batch(words, offsets, lengths), *args, max_records=max_records)
        return t.tandems_results()


def check(reads, *args, ref=()):
    """GPU == host, records, counts and number; the reads whose indices are in `ref` against the reference as well"""
    packed = capi.pack_reads(reads)
    want, want_counts, found = capi.tandems_host(packed, *args)
    got, counts, n = gpu_tandems(packed, *args)
    assert n == found == len(want)
    assert (counts == want_counts).all(), np.flatnonzero(counts != want_counts)[:5]
    same(got, want)
    ref = list(ref)
    if ref:
        sub, sub_counts = T.tandems([reads[i] for i in ref], *args)
        assert (want_counts[ref] == sub_counts).all()
        at = np.concatenate([[0], np.cumsum(want_counts.astype(np.int64))])
        mine = np.concatenate([want[at[i]:at[i + 1]] for i in ref])
        mine["read"] = sub["read"]
        same(mine, sub)
    return want, want_counts


# ---- shapes and sizes
def test_hand_worked_vectors():
    got, counts, n = gpu_tandems([r.encode() for r, _ in HAND])
    assert counts.tolist() == [len(w) for _, w in HAND] and n == sum(len(w) for _, w in HAND)
    assert [rec(x)[1:] for x in got] == [w for _, ws in HAND for w in ws]


@pytest.mark.parametrize("k", KS)
def test_unit_lengths_and_read_lengths(k):
    """perfect, shifted, noisy and random reads of every listed length, and two tracts of the unit around a spacer, for the
    unit length k"""
    rnd = random.Random(k)
    unit = UNITS[k]
    short, long_ = [], []
    for n in (0, 1, k, 2 * k, 31, 32, 33, 2047, 2048, 2049):
        into = short if n <= 64 else long_
        into.append(rep(unit, n))
        into.append(rep(unit, n, rnd.randrange(k)))
        into.append(noisy(rnd, unit, n, 0.03, 0.06, 0.004))
        into.append(junk(rnd, n, "ACGTN" if n % 2 else "ACGT"))
        into.append(rep(unit, n) + junk(rnd, 35) + rep(SAT if k != 5 else TEL, 40 + n // 8))
    for args in ((1, 32, 3, 1), (1, 32, 1, 24), (1, 32, 64, 1)):
        check(short, *args, ref=range(len(short)))
    want, counts = check(long_, 1, 32, 3, 24, ref=(0, 4))
    assert (counts[:2] == 1).all() and (want["period"][:2] == k).all() and counts[4] == 2
    check(long_, 1, 32, 1, 1)
    check(long_, k, k, 64, 1)


# ---- the bounds of a piece
@pytest.mark.parametrize("k", KS)
def test_piece_bounds_at_word_edges_and_the_64_word_seam(k):
    reads, wanted = piece_bound_reads(k)
    want, counts = check(reads, 1, 32, 3, 24, ref=range(len(reads)))
    assert (counts == 2).all()
    for i, (lo, at_start) in enumerate(wanted):
        mine = want[want["read"] == i]
        top, child = mine[mine["depth"] == 0][0], mine[mine["depth"] == 1][0]
        assert int(top["period"]) == 5 and int(top["end"]) == lo  # the child piece is [lo, n)
        assert int(child["scored_period"]) % k == 0
        if at_start:  # the tract, its longest run and its seed window at the piece's first base
            assert int(child["start"]) == lo and reads[i][lo - 5] == "N"
        else:  # and at its last
            assert int(child["end"]) == len(reads[i]) and int(child["start"]) > lo
    assert {lo & 31 for lo, _ in wanted} == {31, 0, 1} and {lo for lo, _ in wanted} >= {2047, 2048, 2049}
    check(reads, k, k, 64, 8)
    check(reads, 1, 32, 1, 30)


@pytest.mark.parametrize("k", KS)
def test_piece_ends_at_word_edges_and_the_64_word_seam(k):
    """the mirror: the piece ends at hi, the start of the depth-0 tract, and the child's tract ends at the piece's last base"""
    reads, wanted = piece_hi_reads(k)
    want, counts = check(reads, 1, 32, 3, 24, ref=range(len(reads)))
    for i, (lo, hi, shape) in enumerate(wanted):
        mine = want[want["read"] == i]
        top = mine[mine["depth"] == 0][0]
        assert int(top["period"]) == 5 and int(top["start"]) == hi and reads[i][hi + 4] == "N"  # the piece in front ends at hi
        (child,) = [x for x in mine if int(x["end"]) == hi]  # the tract, its longest run and its seed window at the piece's last base
        assert int(child["scored_period"]) % k == 0
        if shape == "end":  # the piece is [0, hi)
            assert len(mine) == 2 and int(child["depth"]) == 1 and int(child["start"]) > 0
        else:  # the piece is [lo, hi), between two tracts, and the child's tract fills it
            assert len(mine) == 3 and int(child["depth"]) == 2 and int(child["start"]) == lo and int(mine[0]["end"]) == lo
    assert {hi & 31 for _, hi, _ in wanted} == {31, 0, 1} and {hi for _, hi, _ in wanted} >= {255, 256, 257, 2047, 2048, 2049}
    check(reads, k, k, 64, 8)
    check(reads, 1, 32, 1, 30)


def test_children_lie_around_the_refined_tract():
    """the refined extent is wider than the periods tract: were the children formed from the periods tract, the copies between
    the two ends would give a third record"""
    read = extent_read()
    per, x = P.period_read(read), R.refine_read(read)
    assert x[T.END] > per[T.P_END] + 24 and P.period_read(read[per[T.P_END]:x[T.END]]) != P.ZERO
    rnd = random.Random(1)
    reads = [junk(rnd, o) + read for o in range(0, 64, 3)]  # the ends of both tracts at many bits of a word
    want, counts = check(reads, 1, 32, 3, 24, ref=range(0, len(reads), 5))
    assert (counts == 2).all() and want["depth"].tolist() == [0, 1] * len(reads)
    assert (want["end"][0::2] - want["start"][0::2] == x[T.END] - x[T.START]).all()


def test_weak_pieces_give_no_record_and_split_at_the_periods_tract():
    rnd = random.Random(2)
    reads = [WEAK, WEAK_FIRST, STRONG_FIRST] + [junk(rnd, o) + WEAK_FIRST for o in (1, 30, 31, 32, 33)] + [WEAK + junk(rnd, 28) + WEAK]
    want, counts = check(reads, 1, 32, 3, 24, ref=range(len(reads)))
    assert counts.tolist()[:3] == [0, 1, 1] and counts[-1] == 0
    assert want["depth"].tolist()[:2] == [1, 0]  # below a weak piece: depth 1 without a depth-0 record
    for i in range(3, 8):  # with a lead the weak piece starts at other bits; what it gives is the reference's business
        mine = want[want["read"] == i]
        assert len(mine) >= 1 and int(mine[-1]["period"]) == 6 and int(mine[-1]["depth"]) >= 1
    check(reads, 1, 32, 3, 23, ref=range(len(reads)))  # at 23 the weak read is a tract


# ---- the stack
def test_stack_chains_tree_and_64_tracts_in_one_wave():
    """many short tracts: the longer child on the right (the longest tract first), on the left (last) and on either side"""
    reads = stack_reads()
    want, counts = check(reads, 1, 32, 3, 24, ref=range(3))
    assert counts.tolist() == [6, 6, 6, 64]
    depth = [int(want[want["read"] == r]["depth"].max()) for r in range(4)]
    assert depth[:3] == [5, 5, 2] and depth[3] >= 4
    check(reads * 3, 1, 32, 64, 8)


# ---- the log
def test_log_overflow_exact_numbers_and_repeated_calls():
    rnd = random.Random(4096)
    one = junk(rnd, 120) + noisy(rnd, TEL, 200, 0.02, 0.04) + junk(rnd, 90) + rep(SAT, 150) + junk(rnd, 77)
    want1, counts1, found1 = capi.tandems_host([one])
    assert found1 == 2
    n = 2048
    packed = capi.pack_reads([one] * n)
    want = np.repeat(want1.reshape(1, 2), n, axis=0).reshape(-1).copy()
    want["read"] = np.repeat(np.arange(n), 2)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=n) as t:
        b = t.host_batch(*packed)
        for cap in (1, n, 2 * n - 1, 2 * n, 2 * n + 1, BIG, 2 * n - 1, 2 * n):  # below, at and above the need, and back
            t.tandems(b, max_records=cap)
            got, counts, found = t.tandems_results()
            assert found == 2 * n and (counts == 2).all()  # exact also on overflow
            if cap < 2 * n:
                assert len(got) == 0  # nothing is copied from an overflowed log
            else:
                same(got, want)
        # a caller's buffer smaller than the log: the first records of the sorted order, the numbers exact
        t.tandems(b, max_records=2 * n)
        num = C.c_uint64(0)
        five = np.zeros(5, dtype=capi.TANDEM_DTYPE)
        cnt = np.zeros(n, dtype=np.uint32)
        assert t.lib.trew_hip_tandems_results(t.ctx, 0, five.ctypes.data, 5, C.byref(num), cnt.ctypes.data, None) == 0
        assert num.value == 2 * n and (cnt == 2).all()
        same(five, want[:5])
        assert t.lib.trew_hip_tandems_results(t.ctx, 0, None, 0, None, None, None) != 0
        assert t.lib.trew_hip_tandems_results(t.ctx, 0, None, 5, C.byref(num), None, None) != 0
        with pytest.raises(capi.TrewHipError, match="max_records must be at least 1"):
            t.tandems(b, max_records=0)


def test_convenience_entry_point_retries():
    import trew_amd

    reads = fuzz_reads(2, 300, 500)
    want, want_counts, found = capi.tandems_host(reads, 1, 32, 3, 8)
    assert found > 50  # the first log overflows
    got, counts = trew_amd.tandems(reads, 1, 32, 3, 8, max_records=50)
    same(got, want)
    assert (counts == want_counts).all()
    got, counts = trew_amd.tandems(reads)
    same(got, capi.tandems_host(reads)[0])


# ---- long reads
def test_long_read_with_two_noisy_tracts():
    rnd = random.Random(70000)
    parts = [junk(rnd, 21_000), noisy(rnd, SAT, 900, 0.03, 0.06), junk(rnd, 30_000), noisy(rnd, TEL, 600, 0.03, 0.06)]
    read = "".join(parts) + junk(rnd, 70_000 - sum(len(p) for p in parts))
    assert len(read) == 70_000
    want, counts = check([read], 1, 32, 3, 40)
    big = want[want["end"] - want["start"] >= 500]
    assert big["period"].tolist() == [5, 6] and big["depth"].tolist() == [0, 1]
    assert 21_000 <= int(big[0]["start"]) <= 21_020 and int(big[0]["end"]) >= 21_880  # both tracts whole
    assert 51_900 <= int(big[1]["start"]) <= 51_920 and int(big[1]["end"]) >= 52_480


def test_two_tract_set_against_the_reference():
    fs = two_tract_set()
    reads = [r for r, _ in fs]
    want, counts = check(reads, 1, 32, 3, 24, ref=range(len(reads)))
    assert (counts >= 2).sum() >= 27
    check(reads, 1, 32, 1, 24)
    check(reads, 2, 12, 64, 10)


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_ragged_reads_and_parameters(seed):
    reads = fuzz_reads(seed, 200, 500)
    for min_score in (24, 8):
        for penalty in (1, 64):
            for lo, hi in ((1, 32), (5, 7)):
                check(reads, lo, hi, penalty, min_score)
    check(reads, 1, 1, 3, 8)
    check(reads, 32, 32, 3, 8)
    want, counts = check(reads, 1, 32, 3, 8, ref=range(0, 200, 13))
    assert (counts >= 2).sum() >= 20 and int(want["depth"].max()) >= 2


# ---- depth 0 is refine
def test_depth_zero_equals_refine_on_the_gpu():
    reads = fuzz_reads(99, n=1500, max_len=400) + [WEAK.encode(), WEAK_FIRST.encode()]
    packed = capi.pack_reads(reads)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        t.refine(b)
        ref = t.refine_results()
        t.tandems(b, max_records=BIG)
        got, counts, found = t.tandems_results()
        t.periods(b)
        per = t.periods_results()
    strong = ref["score"] >= 24
    assert 150 <= strong.sum() <= 1400 and ((ref["period"] > 0) & ~strong).sum() >= 2  # weak reads are among them
    zero = got[got["depth"] == 0]
    assert (zero["read"] == np.flatnonzero(strong)).all()
    for f in R.FIELDS:
        assert (zero[f] == ref[f][zero["read"]]).all(), f
    assert (counts[per["period"] == 0] == 0).all()  # no periods record, no tract
    assert (got["score"] >= 24).all()
    same(got, capi.tandems_host(packed)[0])


# ---- batch shapes and contexts
@pytest.fixture(scope="module")
def uniform150():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 4000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.tandems_host(reads, 1, 32, 3, 8)
    assert (want[0]["period"] == 6).sum() >= 30 and want[2] > (want[1] > 0).sum()  # some reads have two tracts
    return reads, want


@pytest.mark.parametrize("shape", ["host_ragged", "offsets_lengths_words", "words_offsets_lengths", "host_uniform", "device_uniform"])
def test_batch_shapes(uniform150, shape):
    n, L = 4000, 150
    reads, (want, want_counts, found) = uniform150
    words, offsets, lengths = (np.ascontiguousarray(a, dtype=np.uint32) for a in capi.pack_reads(reads))
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 20) as t:
        d = None
        if shape == "host_ragged":
            b = t.host_batch(words, offsets, lengths)
        elif shape == "offsets_lengths_words":
            b = t.host_batch(words, offsets, lengths, contiguous=True)
        elif shape == "words_offsets_lengths":
            buf = np.concatenate([words, offsets, lengths])
            base = buf.ctypes.data
            b = capi.Batch(base, len(words), base + 4 * len(words), base + 4 * (len(words) + n), 0, 0, n, 0, 0)
            b._keep = (buf,)
        elif shape == "host_uniform":
            b = capi.Batch(words.ctypes.data, len(words), None, None, L, stride, n, 0, 0)
            b._keep = (words,)
        else:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(20250218, 0, n, L, d)
            b = t.device_uniform_batch(d, n, L)
        for _ in range(2):  # a repeated call gives the same
            t.tandems(b, 1, 32, 3, 8, max_records=BIG)
            got, counts, num = t.tandems_results()
            same(got, want)
            assert (counts == want_counts).all() and num == found
        if d is not None:
            t.free(d)


@pytest.mark.parametrize("max_length", ["known", "unknown"])
def test_device_resident_ragged(max_length):
    n = 60
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    want, want_counts, found = capi.tandems_host([buf[s:e + 1] for s, e in zip(st, nd)])
    assert (want["period"] == 6).sum() >= 2
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        if max_length == "unknown":
            b.max_length = 0
        t.tandems(b, max_records=BIG)
        got, counts, num, ms = t.tandems_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, want)
    assert (counts == want_counts).all() and num == found


def test_pair_mode_context_two_slots_and_errors():
    a, b = fuzz_reads(41, n=250), fuzz_reads(42, n=151)  # an odd number of reads is refused in pair mode
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_tandems"):
            t.tandems_results()
        t.refine(ba)  # neither a refine call nor a repeats call is a tandems call: the buffers are separate
        t.refine_results()
        t.repeats(ba)
        t.repeats_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_tandems"):
            t.tandems_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.tandems(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:150]))
        t.tandems(ba, 1, 32, 3, 8, max_records=BIG, slot=0)  # the mates are two reads; the two slots overlap
        t.tandems(bb, 2, 12, 7, 5, max_records=BIG, slot=1)
        got1, got0 = t.tandems_results(1), t.tandems_results(0)
        for got, want in ((got1, capi.tandems_host(b[:150], 2, 12, 7, 5)), (got0, capi.tandems_host(a, 1, 32, 3, 8))):
            same(got[0], want[0])
            assert (got[1] == want[1]).all() and got[2] == want[2] > 100
        for lo, hi in ((0, 5), (3, 2), (1, 33)):
            with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
                t.tandems(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.tandems(ba, penalty=penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.tandems(ba, min_score=0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.tandems(ba, slot=3)


# ---- independence
def test_independent_of_scan_and_the_other_measures():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = capi.tandems_host(a, 1, 32, 3, 12), capi.tandems_host(b, 2, 12, 5, 12)
    LOG = 1 << 16

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    def fetch(t, slot=0):
        return ((t.annotate_results(slot), t.tracts_results(slot)) + t.intervals_results(slot) + t.variants_results(slot) + (t.periods_results(slot),) +
                t.chain_results(slot) + t.repeats_results(slot) + t.satellites_results(slot) + (t.align_results(slot), t.refine_results(slot)))

    with fresh() as t:  # without any tandems call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.annotate(ba, motifs)
        t.tracts(ba, motifs, 3)
        t.intervals(ba, motifs, 6, 12, LOG)
        t.variants(ba, motifs)
        t.periods(ba)
        t.chain(ba, motifs, 8 * LOG)
        t.repeats(ba, max_records=LOG)
        t.satellites(ba, 1, 64, max_records=LOG)
        t.align(ba, motifs, 3)
        t.refine(ba)
        alone = fetch(t)
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # tandems calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.tandems(ba, 1, 32, 3, 12, max_records=LOG, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.tandems(bb, 2, 12, 5, 12, max_records=LOG, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.intervals(ba, motifs, 6, 12, LOG, slot=0)
        t.variants(ba, motifs, slot=0)
        t.periods(ba, slot=0)
        t.chain(ba, motifs, 8 * LOG, slot=0)
        t.repeats(ba, max_records=LOG, slot=0)
        t.satellites(ba, 1, 64, max_records=LOG, slot=0)
        t.align(ba, motifs, 3, slot=0)
        t.refine(ba, slot=0)
        t.submit(bb, slot=1)
        got_1 = t.tandems_results(1)
        got_0 = t.tandems_results(0)
        got = fetch(t)
        tables = t.collect()
    for g, w in ((got_0, want_a), (got_1, want_b)):
        same(g[0], w[0])
        assert (g[1] == w[1]).all() and g[2] == w[2] > 0
    assert len(got) == len(alone)
    for x, y in zip(got, alone):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- the `trew tandems` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


def two_noisy_tract_reads(n=30, seed=8):
    """generator long reads, cut to at most 3 kb, with two planted tracts of 0.3 - 0.9 kb of two of four units that carry
    substitutions and indels: one inside the read, one as its tail"""
    rnd = random.Random(seed)
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    units = [TEL, "CCCTAA", SAT, UNITS[17]]
    out = []
    for i, (s, e) in enumerate(zip(st, nd)):
        body = buf[s:e + 1].decode()[:rnd.randint(400, 3000)]
        at = rnd.randint(0, len(body))
        mid = noisy(rnd, units[i % 4], rnd.randint(300, 900), 0.03, 0.06, 0.002)
        out.append((body[:at] + mid + body[at:] + noisy(rnd, units[(i + 1) % 4], rnd.randint(300, 900), 0.03, 0.06, 0.002)).encode())
    return out


def test_cli_generator_long_reads_with_two_noisy_tracts(tmp_path):
    reads = two_noisy_tract_reads()
    path = str(tmp_path / "two.fastq")
    write_fastq(path, reads)
    # rows formatted from the reference itself for the first reads, from the host definition (equal to it) for all
    host3, counts, found = capi.tandems_host(reads)
    first = host3[host3["read"] < 2]
    same(first, T.tandems(reads[:2])[0])
    rows, summary = T.cli_lines(path, reads, host3, 3)
    assert found > len(reads) and (counts >= 2).sum() >= len(reads) - 3 and len(summary) - 2 >= 4  # the planted tracts are found
    out, err = run_cli("tandems", path, "-t", "2", "--stats")
    assert out == rows + summary
    # more tracts than reads: the first log of the one batch overflowed and the batch was resubmitted once
    assert "%d tracts, 1 batch(es) resubmitted with a larger log" % found in err
    assert run_cli("tandems", path, "-t", "5")[0] == rows + summary
    rows7, summary7 = T.cli_lines(path, reads, capi.tandems_host(reads, 5, 12, 7, 60)[0], 7)
    assert 10 <= len(rows7) - 2 < len(rows) - 2  # the units of 17 are out of the range, and P = 7 leaves the noisier tracts below 60
    assert run_cli("tandems", path, "--min_period", "5", "--max_period", "12", "--penalty", "7", "--min_score", "60", "-t", "3")[0] == rows7 + summary7
    # two files: the summary is over both
    got, _ = run_cli("tandems", path, path)
    assert got.count(">" + os.path.realpath(path)) == 2
    twice = np.concatenate([host3, host3])
    twice["read"][len(host3):] += len(reads)
    assert got[got.index(">Summary"):] == T.cli_lines(path, reads + reads, twice, 3)[1]
    # the depth-0 rows are the rows of `trew refine`, without the depth column
    ref, _ = run_cli("refine", path)
    zero = [",".join(x.split(",")[:2] + x.split(",")[3:]) for x in out[2:out.index(">Summary")] if x.split(",")[2] == "0"]
    assert ref[2:ref.index(">Summary")] == zero
