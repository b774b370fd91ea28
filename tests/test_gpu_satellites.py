"""De novo repeats with periods up to 256 on the GPU (trew_hip_satellites through ctypes).  Every record of every batch is
compared, integer for integer, with trew_satellites_host (itself checked against tests/satellite_ref.py in
test_satellites_cpu.py), and with the reference where the reads are few.  A test that pins one k runs at min_period =
max_period = k or a range of three; the full range 1 .. 256 belongs to the mixed-read and fuzz tests."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import period_ref as R
import satellite_ref as SR
from period_cases import TEL, fuzz_reads, junk, noisy, rep
from repeat_cases import SAT
from satellite_cases import (FUZZ_N, FUZZ_SEEDS, boundary_reads, end_reads, eq_edge_reads, long_span_read, majority_reads, monomer, n_phase_read,
                             root_vectors, sat_fuzz_reads, three_kinds, tie_read, wide_edge_reads, wide_stack_reads)
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 18  # a log that holds every tract of every batch here


def same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in SR.FIELDS if len(got) else ():
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))
        assert len(bad) == 0, "%s differs at record %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_satellites(reads_or_packed, *args, mode=capi.MODE_LONG, max_records=BIG):
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16)) as t:
        t.satellites(t.host_batch(words, offsets, lengths), *args, max_records=max_records)
        return t.satellites_results()


def check(reads, *args, ref=()):
    """GPU == host, records, counts and number; the reads whose indices are in `ref` against the brute-force reference as well"""
    packed = capi.pack_reads(reads)
    want, want_counts, found = capi.satellites_host(packed, *args)
    got, counts, n = gpu_satellites(packed, *args)
    assert n == found == len(want)
    assert (counts == want_counts).all(), np.flatnonzero(counts != want_counts)[:5]
    same(got, want)
    if len(ref):
        sub, sub_counts = SR.satellites([reads[i] for i in ref], *args)
        assert (want_counts[list(ref)] == sub_counts).all()
        at = np.concatenate([[0], np.cumsum(want_counts.astype(np.int64))])
        mine = np.concatenate([want[at[i]:at[i + 1]] for i in ref])
        mine["read"] = sub["read"]
        same(mine, sub)
    return want, want_counts


# ---- the eq word
@pytest.mark.parametrize("k", [33, 63, 64, 65, 96, 127, 128, 129, 171, 255, 256])
def test_eq_word_at_word_and_iteration_boundaries(k):
    reads, wanted = eq_edge_reads(k)
    assert len(reads) >= 40 and max(len(r) for r in reads) > 32 * 128 + 2 * k
    want, counts = check(reads, k, k, 3, 24, ref=range(0, len(reads), 11))
    assert (counts >= 1).all()
    hit = sum(any(int(x[side]) == at for x in want[want["read"] == i]) for i, (at, side) in enumerate(wanted))
    print("k = %d: tracts whose start or end lies where it was asked for: %d of %d" % (k, hit, len(wanted)))
    assert hit >= 0.9 * len(wanted)  # chance matches in the background move a few ends by a base
    check(reads, max(k - 1, 1), min(k + 1, 256), 64, 8)
    # the partner word is the read's last word, or does not exist
    reads = end_reads(k)
    want, counts = check(reads, k, k, 3, 1, ref=range(0, len(reads), 7))
    assert (counts >= 1).all()
    assert sum(int(want[want["read"] == i]["end"].max()) == len(r) for i, r in enumerate(reads)) >= 15  # tracts that end with the read


def test_bits_past_the_read_end_do_not_matter():
    rnd = random.Random(6)
    reads = [noisy(rnd, monomer(k), n, 0.02) + junk(rnd, m) for k in (33, 64, 171, 256) for n in (2 * k + 1, 2 * k + 31, 3 * k) for m in (0, 3, 41)]
    words, offsets, lengths = capi.pack_reads(reads)
    want, want_counts, found = capi.satellites_host((words, offsets, lengths), 1, 256, 3, 12)
    dirty = np.array(words, dtype=np.uint32)
    for o, n in zip(offsets.tolist(), lengths.tolist()):
        if n % 32:
            last = o + 3 * (n // 32)
            hi = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
            dirty[last + 2] |= hi                                      # nmask set past the end, which the format allows
            dirty[last] |= np.uint32(rnd.getrandbits(32)) & hi         # and anything in the planes there
            dirty[last + 1] |= np.uint32(rnd.getrandbits(32)) & hi
    assert (dirty != words).any() and found >= len(reads)
    same(capi.satellites_host((dirty, offsets, lengths), 1, 256, 3, 12)[0], want)
    got, counts, n = gpu_satellites((dirty, offsets, lengths), 1, 256, 3, 12)
    same(got, want)
    assert (counts == want_counts).all() and n == found


# ---- pieces
@pytest.mark.parametrize("k", [33, 64, 171])
def test_piece_edges_at_every_bit(k):
    reads, equal = wide_edge_reads(k)
    assert len(reads) == 3 * len({0, 1, k - 1, k, 40}) * 2 * 64
    want, counts = check(reads, k, k, 3, 20, ref=range(0, len(reads), 197))
    assert (counts >= 1).all() and (counts >= 2).sum() >= 300
    # the children's lo (the end of a tract in front) and hi (the start of a tract behind) take every bit of a word
    child = want[want["depth"] > 0]
    assert len(set((child["start"] & 31).tolist())) == 32 and len(set((child["end"] & 31).tolist())) == 32
    first = want[np.concatenate([[True], want["read"][1:] != want["read"][:-1]])]
    assert len(set((first["end"] & 31).tolist())) == 32
    # penalty 64, one unit twice with 0 < g < k substituted bases between: a substituted base costs two mismatches, 128, and the
    # shorter tract scores 2 k (3 k bases), so the gap is not bridged and there are two records where 128 g > 3 k
    want, counts = check(reads, k, k, 64, 20, ref=range(5, len(reads), 393))
    two = [i for i, e in enumerate(equal) if e and 0 < e[0] < k and 128 * e[0] > 3 * k]
    assert (counts[two] == 2).all() and len(two) > 0
    check(reads, k - 1, k + 1, 1, 8)


def test_left_deep_and_right_deep_chains_with_wide_units():
    reads = wide_stack_reads()
    want, counts = check(reads, 1, 256, 3, 24, ref=range(2))
    assert counts.tolist() == [6, 6, 6]
    assert [int(want[want["read"] == r]["depth"].max()) for r in range(3)] == [5, 5, 2]
    check(reads * 3, 30, 180, 64, 8)


# ---- the consensus
@pytest.mark.parametrize("k", [171, 256])
def test_consensus_every_majority_a_tie_and_a_phase_of_n(k):
    reads = majority_reads(k) + [tie_read(k)[0], n_phase_read(k)]
    for penalty in (3, 1):
        want, counts = check(reads, k, k, penalty, 24, ref=range(len(reads)))
    assert (counts >= 1).all()  # at penalty 1 the tie read scores
    units = [SR.unit_codes(x["unit"], k) for x in want[:4]]
    assert want["period"][:4].tolist() == [k] * 4 and all(units[r] == [(c + r) % 4 for c in units[0]] for r in range(1, 4))
    assert len(set(units[0])) == 4


def test_consensus_span_longer_than_an_iteration():
    read = long_span_read()
    assert len(read) > 2048 + 400
    want, counts = check([read, read[7:], read[:2300]], 171, 171, 3, 24, ref=range(3))
    assert want["period"].tolist() == [171] * 3 and (want["end"].astype(np.int64) - want["start"] > 2048).all()


def test_bins_left_by_a_wide_user_are_clean_for_the_next():
    """4096 reads alternating a k = 256 tract and a k = 6 tract: a grid-stride wave meets the bins its last user left"""
    rnd = random.Random(4096)
    pair = [junk(rnd, 20) + rep(monomer(256), 256 * 2 + 40) + junk(rnd, 20), junk(rnd, 30) + rep(TEL, 90) + junk(rnd, 30)]
    want2, counts2, found2 = capi.satellites_host(pair, 1, 256, 3, 24)
    assert found2 == 2 and want2["period"].tolist() == [256, 6] and counts2.tolist() == [1, 1]
    n = 4096
    want = np.tile(want2, n // 2)
    want["read"] = np.arange(n)
    got, counts, found = gpu_satellites(pair * (n // 2), 1, 256, 3, 24)
    assert found == n and (counts == 1).all()
    same(got, want)


def test_primitive_roots_and_unit_word_boundaries():
    for read, K, d in root_vectors():
        want, counts = check([read, junk(random.Random(K), 60) + read], K, K, 3, 24, ref=range(1))
        assert want["period"].tolist() == [d, d] and want["scored_period"].tolist() == [K, K]
    want, counts = check([monomer(19) * 27], 171, 171, 3, 24, ref=range(1))
    assert want["period"].tolist() == [19]
    for read, d in boundary_reads():
        want, counts = check([read], d, d, 3, 24, ref=range(1))
        words = want["unit"][0].tolist()
        assert want["period"].tolist() == [d] and capi.satellite_unit_text(words, d) == read[:d]
        assert words[(d - 1) >> 4] >> (2 * ((d - 1) & 15) + 2) == 0 and not any(words[((d - 1) >> 4) + 1:])
    # all of them in one batch over the whole range: every wave packs units of different widths one after the other
    reads = [x[0] for x in boundary_reads()] + [x[0] for x in root_vectors()]
    check(reads * 8, 1, 256, 3, 24)


# ---- mixed reads and extremes
def test_mixed_reads_equal_repeats_on_the_gpu_up_to_32():
    reads = fuzz_reads(99, n=2000, max_len=400)
    packed = capi.pack_reads(reads)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        t.repeats(b, 1, 32, 3, 24, max_records=BIG)
        rp, rc, rn = t.repeats_results()
        t.satellites(b, 1, 32, 3, 24, max_records=BIG)
        got, counts, found = t.satellites_results()
        t.periods(b)
        per = t.periods_results()
    assert found == rn > 200 and (counts == rc).all()
    for f in SR.SCALARS:
        assert (got[f] == rp[f]).all(), f
    for a, b in zip(got, rp):
        assert capi.satellite_unit_text(a["unit"], a["period"]) == R.unit_text(b["unit"], int(a["period"]))
    zero = got[got["depth"] == 0]  # the depth-0 record is the periods record
    assert (zero["read"] == np.flatnonzero(per["period"] > 0)).all()
    for f in R.FIELDS[:-1]:
        assert (zero[f] == per[f][zero["read"]]).all(), f
    same(got, capi.satellites_host(packed, 1, 32, 3, 24)[0])


def test_long_read_with_three_planted_tracts_one_of_them_wide():
    rnd = random.Random(200000)
    # exact tracts: at P = 64 one substituted base costs 128 and would cut a tract in two
    parts = [junk(rnd, 60_000), rep(SAT, 900), junk(rnd, 70_000), rep(monomer(171), 171 * 12), junk(rnd, 60_000), rep(TEL, 1200)]
    read = "".join(parts) + junk(rnd, 200_000 - sum(len(p) for p in parts))
    assert len(read) == 200_000
    want, counts = check([read], 1, 256, 64, 24)
    assert counts.tolist() == [3] and want["period"].tolist() == [5, 171, 6] and want["depth"].tolist() == [1, 0, 1]
    assert [int(x["end"]) - int(x["start"]) >= n for x, n in zip(want, (900, 171 * 12, 1200))] == [True] * 3


@pytest.mark.parametrize("sub", [0, 0.02, 0.05])
def test_three_kinds_of_tract_in_one_read(sub):
    rnd = random.Random(int(sub * 100) + 7)
    reads = [three_kinds(rnd, sub) for _ in range(8)]
    want, counts = check(reads, 1, 256, 3, 24, ref=range(1))
    assert counts[0] == 3 and want["period"][:3].tolist() == [5, 171, 6]


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(seed):
    reads = sat_fuzz_reads(seed, FUZZ_N)
    for min_score in (24, 8):
        for penalty in (1, 3, 64):
            for lo, hi in ((1, 256), (33, 256), (171, 171), (200, 256), (1, 32)):
                check(reads, lo, hi, penalty, min_score)
    want, counts = check(reads, 1, 256, 3, 8, ref=range(0, FUZZ_N, 13))
    assert (counts >= 3).sum() >= 30 and int(want["depth"].max()) >= 3


# ---- the log
def test_log_overflow_exact_numbers_and_repeated_calls():
    rnd = random.Random(4097)
    one = junk(rnd, 120) + rep(monomer(68), 200) + junk(rnd, 90) + rep(SAT, 150) + junk(rnd, 77)
    want1, counts1, found1 = capi.satellites_host([one])
    assert found1 == 2 and sorted(want1["period"].tolist()) == [5, 68]
    n = 1024
    packed = capi.pack_reads([one] * n)
    want = np.tile(want1, n)
    want["read"] = np.repeat(np.arange(n), 2)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=n) as t:
        b = t.host_batch(*packed)
        for cap in (1, n, 2 * n - 1, 2 * n, 2 * n + 1, BIG, 2 * n - 1, 2 * n):  # below, at and above the need, and back
            t.satellites(b, max_records=cap)
            got, counts, found = t.satellites_results()
            assert found == 2 * n and (counts == 2).all()  # exact also on overflow
            if cap < 2 * n:
                assert len(got) == 0  # nothing is copied from an overflowed log
            else:
                same(got, want)
        # a caller's buffer smaller than the log: the first records of the sorted order
        t.satellites(b, max_records=2 * n)
        num = C.c_uint64(0)
        five = np.zeros(5, dtype=capi.SATELLITE_DTYPE)
        assert t.lib.trew_hip_satellites_results(t.ctx, 0, five.ctypes.data, 5, C.byref(num), None, None) == 0
        assert num.value == 2 * n
        same(five, want[:5])
        assert t.lib.trew_hip_satellites_results(t.ctx, 0, None, 0, None, None, None) != 0
        assert t.lib.trew_hip_satellites_results(t.ctx, 0, None, 5, C.byref(num), None, None) != 0
        with pytest.raises(capi.TrewHipError, match="max_records must be at least 1"):
            t.satellites(b, max_records=0)


def test_convenience_entry_point_retries():
    import trew_amd

    reads = sat_fuzz_reads(FUZZ_SEEDS[0], FUZZ_N)
    want, want_counts, found = capi.satellites_host(reads, 1, 256, 3, 8)
    assert found > len(reads)  # the first log, one record per read, overflows
    got, counts = trew_amd.satellites(reads, 1, 256, 3, 8)
    same(got, want)
    assert (counts == want_counts).all()
    got, counts = trew_amd.satellites(reads)
    same(got, capi.satellites_host(reads)[0])


# ---- batch shapes and contexts
@pytest.fixture(scope="module")
def uniform150():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 4000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.satellites_host(reads, 1, 149, 3, 8)
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
        t.satellites(b, 1, 149, 3, 8, max_records=BIG)
        got, counts, num = t.satellites_results()
        if d is not None:
            t.free(d)
    same(got, want)
    assert (counts == want_counts).all() and num == found


@pytest.mark.parametrize("max_length", ["known", "unknown"])
def test_device_resident_ragged(max_length):
    n = 60
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    want, want_counts, found = capi.satellites_host([buf[s:e + 1] for s, e in zip(st, nd)], 1, 64)
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        if max_length == "unknown":
            b.max_length = 0
        t.satellites(b, 1, 64, max_records=BIG)
        got, counts, num, ms = t.satellites_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0 and found > 0
    same(got, want)
    assert (counts == want_counts).all() and num == found


def test_pair_mode_context_two_slots_and_errors():
    a, b = sat_fuzz_reads(41, 100), sat_fuzz_reads(42, 61)  # an odd number of reads is refused in pair mode
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_satellites"):
            t.satellites_results()
        t.repeats(ba)  # a repeats call is no satellites call: the buffers are separate
        t.repeats_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_satellites"):
            t.satellites_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.satellites(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:60]))
        t.satellites(ba, 1, 256, 3, 8, max_records=BIG, slot=0)  # the mates are two reads; the two slots overlap
        t.satellites(bb, 20, 200, 7, 5, max_records=BIG, slot=1)
        got1, got0 = t.satellites_results(1), t.satellites_results(0)
        for got, want in ((got1, capi.satellites_host(b[:60], 20, 200, 7, 5)), (got0, capi.satellites_host(a, 1, 256, 3, 8))):
            same(got[0], want[0])
            assert (got[1] == want[1]).all() and got[2] == want[2] > 60
        for lo, hi in ((0, 5), (3, 2), (1, 257)):
            with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 256"):
                t.satellites(ba, lo, hi)
        with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
            t.repeats(ba, 1, 33)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.satellites(ba, penalty=penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.satellites(ba, min_score=0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.satellites(ba, slot=3)


# ---- independence
def test_independent_of_scan_and_the_other_measures():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 12000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:7000], reads[7000:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = capi.satellites_host(a, 1, 149, 3, 12), capi.satellites_host(b, 20, 70, 5, 12)
    LOG = 1 << 16

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    def others(t, ba, slot=0):
        t.annotate(ba, motifs, slot=slot)
        t.tracts(ba, motifs, 3, slot=slot)
        t.intervals(ba, motifs, 6, 12, LOG, slot=slot)
        t.variants(ba, motifs, slot=slot)
        t.periods(ba, slot=slot)
        t.chain(ba, motifs, 8 * LOG, slot=slot)
        t.repeats(ba, max_records=LOG, slot=slot)

    def fetch(t, slot=0):
        return ((t.annotate_results(slot), t.tracts_results(slot)) + t.intervals_results(slot) + t.variants_results(slot) + (t.periods_results(slot),) +
                t.chain_results(slot) + t.repeats_results(slot))

    with fresh() as t:  # without any satellites call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        others(t, ba)
        alone = fetch(t)
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # satellites calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.satellites(ba, 1, 149, 3, 12, max_records=LOG, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.satellites(bb, 20, 70, 5, 12, max_records=LOG, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.intervals(ba, motifs, 6, 12, LOG, slot=0)
        t.variants(ba, motifs, slot=0)
        t.periods(ba, slot=0)
        t.chain(ba, motifs, 8 * LOG, slot=0)
        t.repeats(ba, max_records=LOG, slot=0)
        t.submit(bb, slot=1)
        got_s1 = t.satellites_results(1)
        got_s0 = t.satellites_results(0)
        got = fetch(t)
        tables = t.collect()
    for g, w in ((got_s0, want_a), (got_s1, want_b)):
        same(g[0], w[0])
        assert (g[1] == w[1]).all() and g[2] == w[2] > 0
    assert len(got) == len(alone)
    for x, y in zip(got, alone):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- the `trew satellites` subcommand, end to end
def write_fastq(path, reads):
    with open(path, "wb") as f:
        f.write(b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads)))


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


def split_sections(lines):
    at = lines.index(">Summary")
    return lines[:at], lines[at:]


def test_cli_generated_file_with_planted_tracts(tmp_path):
    rnd = random.Random(17)
    reads = []
    for i in range(40):
        units = [TEL, "CCCTAA", monomer(68), monomer(171), SAT, None, R.revcomp(monomer(171))]
        body = junk(rnd, rnd.randint(50, 300))
        for j in range(i % 4):
            unit = units[(i + j) % 7]
            if unit is None:
                body += junk(rnd, 20)
            elif len(unit) < 33:
                body += noisy(rnd, unit, rnd.randint(70, 160), 0.02)
            else:  # exact, so that every tract of a wide unit has the unit itself, rotated, as its consensus
                body += noisy(rnd, unit, 3 * len(unit) + rnd.randint(0, 90))
            body += junk(rnd, rnd.randint(160, 250))
        reads.append(body.encode())
    reads.append(three_kinds(rnd).encode())
    path = str(tmp_path / "planted.fastq")
    write_fastq(path, reads)
    for args in ((1, 256, 3, 24), (40, 200, 5, 40)):
        recs, counts = SR.satellites(reads, *args)
        rows, summary = SR.cli_lines(os.path.realpath(path), reads, recs)
        out, err = run_cli("satellites", path, "--min_period", str(args[0]), "--max_period", str(args[1]), "--penalty", str(args[2]), "--min_score",
                           str(args[3]), "-t", "2", "--stats")
        got_rows, got_summary = split_sections(out)
        assert got_rows == rows  # sorted by read, then start
        assert got_summary == summary
        if args[0] == 1:
            assert len(rows) - 2 > len(reads) and (counts >= 3).sum() >= 5 and len(summary) - 2 >= 4
            # more tracts than reads: the first log of the one batch overflowed and the batch was resubmitted once
            assert "%d tracts, 1 batch(es) resubmitted with a larger log" % len(recs) in err
            # the 171-mer and its reverse complement fall into one summary row
            assert sum(1 for x in summary[2:] if x.startswith("171,")) == 1
    # the defaults are the whole range; two files: the summary is over both
    out, _ = run_cli("satellites", path, path)
    assert out.count(">" + os.path.realpath(path)) == 2
    recs = SR.satellites(reads)[0]
    twice = np.concatenate([recs, recs])
    twice["read"][len(recs):] += len(reads)
    assert split_sections(out)[1] == SR.cli_lines(os.path.realpath(path), reads + reads, twice)[1]
    # at periods of at most 32 the rows are those of `trew repeats`
    sat, _ = run_cli("satellites", path, "--max_period", "32")
    rep_, _ = run_cli("repeats", path)
    assert sat == rep_
