"""De novo repeat period and unit per read on the GPU (trew_hip_periods through ctypes).  Every read of every batch is
compared, integer for integer, with trew_periods_host (itself checked against tests/period_ref.py in test_periods_cpu.py),
and with period_ref where the reads are few or short."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import period_ref as R
from conftest import GOLDEN, read_fastq
from period_cases import KAT32, TEL, UNITS, fuzz_reads, junk, noisy, rep, tie_reads
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at read %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_periods(reads_or_packed, *args, mode=capi.MODE_LONG):
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16)) as t:
        t.periods(t.host_batch(words, offsets, lengths), *args)
        return t.periods_results()


def check(reads, *args, ref=0):
    """GPU == host on every read; the first `ref` reads against the brute-force reference as well"""
    packed = capi.pack_reads(reads)
    want = capi.periods_host(packed, *args)
    same(gpu_periods(packed, *args), want)
    if ref:
        same(want[:ref], R.periods(reads[:ref], *args))
    return want


# ---- word and iteration boundaries
def boundary_reads(k, seed):
    """a perfect tract of about 5 k bases whose start (first set) or end (second set) falls on bit 30, 31, 0 or 1 around the
    start of word 1, 2, 63, 64, 126 and 128, in random background; the longest read has about 4200 bases"""
    rnd = random.Random(seed)
    unit, tract = UNITS[k], max(5 * k, 24)
    reads = []
    for w in (1, 2, 63, 64, 126, 128):
        for d in (-2, -1, 0, 1):
            at = 32 * w + d
            reads.append(junk(rnd, at) + rep(unit, tract, rnd.randrange(k)) + junk(rnd, 40))       # the start at `at`
            if at >= tract:
                reads.append(junk(rnd, at - tract) + rep(unit, tract, rnd.randrange(k)) + junk(rnd, 40))  # the end at `at`
    return reads


@pytest.mark.parametrize("k", [1, 2, 3, 6, 31, 32])
def test_word_and_iteration_boundaries(k):
    reads = boundary_reads(k, k)
    assert 4100 <= max(len(r) for r in reads) <= 4400
    for penalty in (1, 3, 64):
        check(reads, 1, 32, penalty, 1, ref=4 if penalty == 3 else 0)
    want = check(reads, k, k, 3, 1)
    assert (want["score"] >= max(5 * k, 24) - k).all()  # the tract is found, whatever chance adds to it


def test_k32_partners_in_the_next_iteration():
    """k = 32, eq positions in the last word of an iteration (word 63), their partner bases in the next iteration's first"""
    rnd = random.Random(32)
    reads = [junk(rnd, at) + rep(UNITS[32], ln) + junk(rnd, tail) for at in (2016, 2017, 2040, 2047, 2048) for ln in (64, 65, 96) for tail in (0, 1, 50)]
    want = check(reads, 32, 32, 3, 1, ref=3)
    assert (want["score"] >= 32).all()
    check(reads, 1, 32, 64, 1)


# ---- read ends
def test_tract_that_ends_at_the_read_end_and_small_reads():
    rnd = random.Random(5)
    reads = []
    for k, unit in UNITS.items():
        for n in (0, 1, 2, k, k + 1, 31, 32, 33, 63, 64, 65):
            reads.append(rep(unit, n))
            reads.append(junk(rnd, n))
        for n in (100, 2048, 2049, 2048 + k, 2080):
            reads.append(junk(rnd, n - min(n, 6 * k + 3)) + rep(unit, min(n, 6 * k + 3)))  # the tract ends exactly at n
    reads += ["N" * 70, "N" * 2100, ""]
    for args in ((1, 32, 3, 1), (1, 32, 1, 24), (1, 1, 3, 1), (32, 32, 3, 1), (6, 6, 64, 1)):
        check(reads, *args, ref=len(reads) if args == (1, 32, 3, 1) else 0)


def test_bits_past_the_read_end_do_not_matter():
    rnd = random.Random(6)
    reads = [noisy(rnd, rnd.choice(list(UNITS.values())), n, 0.03) for n in (1, 5, 31, 33, 40, 63, 65, 70, 100, 2047, 2050, 2079) for _ in range(3)]
    words, offsets, lengths = capi.pack_reads(reads)
    want = capi.periods_host((words, offsets, lengths), 1, 32, 3, 1)
    dirty = np.array(words, dtype=np.uint32)
    for o, n in zip(offsets.tolist(), lengths.tolist()):
        if n % 32:
            last = o + 3 * (n // 32)
            hi = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
            dirty[last + 2] |= hi                                      # nmask set past the end, which the format allows
            dirty[last] |= np.uint32(rnd.getrandbits(32)) & hi         # and anything in the planes there
            dirty[last + 1] |= np.uint32(rnd.getrandbits(32)) & hi
    assert (dirty != words).any()
    same(capi.periods_host((dirty, offsets, lengths), 1, 32, 3, 1), want)
    same(gpu_periods((dirty, offsets, lengths), 1, 32, 3, 1), want)


# ---- ties
@pytest.mark.parametrize("gap,lead", [(40, 33), (70, 61), (2100, 33), (4200, 2040)])
def test_tie_vectors(gap, lead):
    """the competing tracts in neighbouring words, and in different iterations"""
    ab, ba, twice = tie_reads(gap, lead)
    want = check([ab, ba, twice], 1, 32, 3, 10, ref=3)
    assert want["scored_period"].tolist() == [2, 2, 6] and want["score"].tolist() == [18, 18, 42]
    assert int(want["start"][2]) == lead  # the earlier of the two identical tracts


# ---- consensus
@pytest.mark.parametrize("k", [6, 32])
def test_every_phase_and_base_majority(k):
    rnd = random.Random(k)
    reads = []
    for j in range(k):
        for c in "ACGT":
            unit = UNITS[k][:j] + c + UNITS[k][j + 1:]
            copies = [unit] * 12
            for i in rnd.sample(range(2, 10), 2):  # a minority of two other bases at that phase
                copies[i] = unit[:j] + rnd.choice([x for x in "ACGT" if x != c]) + unit[j + 1:]
            reads.append(junk(rnd, rnd.randrange(70)) + "".join(copies) + junk(rnd, 20))
    want = check(reads, 1, 32, 1, 24, ref=8)
    assert (want["scored_period"] % k == 0).sum() >= len(reads) // 2 and (want["support"] < want["end"] - want["start"]).sum() >= len(reads) // 2


def test_consensus_tie_long_span_and_reductions():
    rnd = random.Random(8)
    tie = "GAT" + "TTAGGG" * 4 + "TTACGG" * 4 + "TTA"  # phase 3 of the unit: four G and four C in the span; the smaller code (G) wins
    long_span = junk(rnd, 500) + noisy(rnd, TEL, 3000, 0.02) + junk(rnd, 300)
    reads = [tie, long_span, TEL * 40, "A" * 200, "ACGT" * 60, junk(rnd, 1000) + "AC" * 400]
    want = check(reads, 1, 32, 1, 10, ref=len(reads))
    x = R.period_read(tie, 1, 32, 1, 10)
    cnt = [[0] * 4 for _ in range(6)]
    for p in range(x[3], x[4]):
        cnt[(p - x[3]) % 6][R.CODE[tie[p]]] += 1
    assert any(sorted(c)[-1] == sorted(c)[-2] > 0 for c in cnt)  # the tie is there
    assert int(want["end"][1]) - int(want["start"][1]) > 2048 + 64 and want["period"][1] == 6
    got = check(reads, 7, 32, 3, 10, ref=len(reads))
    assert (got["scored_period"][2], got["period"][2]) == (12, 6)  # 12 -> 6
    got = check(reads, 32, 32, 3, 10, ref=len(reads))
    assert (got["scored_period"][3], got["period"][3], got["unit"][3]) == (32, 1, 3)  # 32 -> 1
    assert (got["scored_period"][4], got["period"][4]) == (32, 4)


# ---- a long read
def test_long_read_with_a_tract_at_its_far_end():
    rnd = random.Random(200000)
    read = "".join(rnd.choices("ACGT", k=200_000 - 3000)) + noisy(rnd, TEL, 3000, 0.01)
    want = check([read], 1, 32, 64, 24)
    assert want["period"][0] == 6 and want["start"][0] >= 197_000
    want = check([read], 1, 32, 3, 24)
    assert want["period"][0] == 6 and want["end"][0] - want["start"][0] >= 2900


# ---- repeatability
def test_many_copies_repeated_calls_and_mixed_order():
    rnd = random.Random(4096)
    one = junk(rnd, 300) + noisy(rnd, TEL, 500, 0.05, 0.01) + junk(rnd, 77)
    want1 = capi.periods_host([one])
    assert want1["period"][0] == 6
    got = gpu_periods([one] * 4096)
    same(got, np.repeat(want1, 4096))
    reads = fuzz_reads(99, n=2000, max_len=400)
    rnd.shuffle(reads)
    packed = capi.pack_reads(reads)
    want = capi.periods_host(packed)
    assert 200 <= (want["period"] > 0).sum() <= 1800
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        for _ in range(3):
            t.periods(b)
            same(t.periods_results(), want)


# ---- fuzz
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(seed):
    rnd = random.Random(seed)
    reads = fuzz_reads(1000 + seed)
    for penalty in (1, 3, 64):
        for min_score in (1, 24):
            lo = rnd.randint(1, 32)
            hi = rnd.randint(lo, 32)
            check(reads, lo, hi, penalty, min_score)
    want = check(reads, 1, 32, 3, 24, ref=60)
    assert (want["period"] > 0).sum() >= 100


# ---- batch shapes and contexts
@pytest.fixture(scope="module")
def uniform150():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 4000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.periods_host(reads)
    assert (want["period"] == 6).sum() >= 30
    return reads, want


@pytest.mark.parametrize("shape", ["host_ragged", "offsets_lengths_words", "words_offsets_lengths", "host_uniform", "device_uniform"])
def test_batch_shapes(uniform150, shape):
    n, L = 4000, 150
    reads, want = uniform150
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
        t.periods(b)
        got = t.periods_results()
        if d is not None:
            t.free(d)
    same(got, want)


@pytest.mark.parametrize("max_length", ["known", "unknown"])
def test_device_resident_ragged(max_length):
    n = 200
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    want = capi.periods_host([buf[s:e + 1] for s, e in zip(st, nd)])
    assert (want["period"] == 6).sum() >= 5
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        if max_length == "unknown":
            b.max_length = 0
        t.periods(b)
        got, ms = t.periods_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, want)


def test_pair_mode_context_two_slots_and_errors():
    a, b = fuzz_reads(41, n=250), fuzz_reads(42, n=151)  # an odd number of reads is refused in pair mode
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_periods"):
            t.periods_results()
        t.tracts(ba, [TEL], 3)  # a tracts call is no periods call: the buffers are separate
        t.tracts_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_periods"):
            t.periods_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.periods(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:150]))
        t.periods(ba, 1, 32, 3, 24, slot=0)  # the mates are two reads
        t.periods(bb, 2, 12, 7, 5, slot=1)
        same(t.periods_results(1), capi.periods_host(b[:150], 2, 12, 7, 5))
        same(t.periods_results(0), capi.periods_host(a))
        for lo, hi in ((0, 5), (3, 2), (1, 33)):
            with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
                t.periods(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.periods(ba, penalty=penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.periods(ba, min_score=0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.periods(ba, slot=3)
        # results larger than the caller's buffer: the count is reported, cap records are copied
        t.periods(ba)
        n = C.c_uint64(0)
        three = np.zeros(3, dtype=capi.PERIOD_DTYPE)
        assert t.lib.trew_hip_periods_results(t.ctx, 0, three.ctypes.data, 3, C.byref(n), None) == 0
        assert n.value == 250
        same(three, capi.periods_host(a[:3]))


def test_convenience_entry_point():
    import trew_amd

    reads = fuzz_reads(77, n=120)
    same(trew_amd.periods(reads), capi.periods_host(reads))
    same(trew_amd.periods(reads, 3, 8, penalty=5, min_score=9), capi.periods_host(reads, 3, 8, 5, 9))


# ---- independence
def test_independent_of_scan_and_the_other_measures():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 12000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:7000], reads[7000:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = capi.periods_host(a), capi.periods_host(b, 2, 12, 5, 12)
    BIG = 1 << 16

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    with fresh() as t:  # without any periods call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.annotate(ba, motifs)
        alone_a = t.annotate_results()
        t.tracts(ba, motifs, 3)
        alone_t = t.tracts_results()
        t.intervals(ba, motifs, 6, 12, BIG)
        alone_i = t.intervals_results()
        t.variants(ba, motifs)
        alone_v = t.variants_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # everything interleaved on slot 0, periods and a scan on slot 1; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.periods(ba, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.periods(bb, 2, 12, 5, 12, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.variants(ba, motifs, slot=0)
        t.intervals(ba, motifs, 6, 12, BIG, slot=0)
        t.submit(bb, slot=1)
        got_p1 = t.periods_results(1)
        got_p0 = t.periods_results(0)
        got_a = t.annotate_results(0)
        got_t = t.tracts_results(0)
        got_i = t.intervals_results(0)
        got_v = t.variants_results(0)
        tables = t.collect()
    same(got_p0, want_a)
    same(got_p1, want_b)
    # the four motif measures are unchanged by the periods calls around them (each is checked against its own reference in
    # its own test file; here against its host definition)
    packed_a = capi.pack_reads(a)
    assert (got_a == alone_a).all() and (alone_a == capi.annotate_host(packed_a, motifs)).all()
    assert (got_t == alone_t).all() and (alone_t == capi.tracts_host(packed_a, motifs, 3)).all()
    assert (got_i[0] == alone_i[0]).all() and (got_i[1] == alone_i[1]).all() and got_i[2] == alone_i[2] > 0
    assert all((x == y).all() for x, y in zip(got_v, alone_v)) and (alone_v[0] == capi.variants_host(packed_a, motifs)[0]).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- cross-check with the scan
def test_period_agrees_with_the_scan_on_pure_repeats():
    """TREW_MODE_SEGMENT on the four known-answer motifs x 20 and on a dozen random primitive motifs of 5 .. 32 bases repeated
    to 150 bases: k_high of the scan is the period, and the scan's class word and the unit are rotations of each other."""
    rnd = random.Random(12)
    motifs = []
    while len(motifs) < 12:
        m = junk(rnd, rnd.randint(5, 32))
        if R.primitive(R.codes(m).tolist()) == len(m) and len(set(m)) >= 3:
            motifs.append(m)
    segs = [(m * 20).encode() for m in KAT32] + [rep(m, 150).encode() for m in motifs]
    want = capi.periods_host(segs)
    with capi.TrewHip(mode=capi.MODE_SEGMENT, min_mer=5, max_mer=32, max_batch_reads=64, max_batch_words=1 << 16) as t:
        b = t.submit_reads(segs)
        t.wait()
        kh, _, sh, _ = t.segment_results(len(segs))
        t.periods(b)
        got = t.periods_results()
    same(got, want)
    for i, m in enumerate(KAT32 + motifs):
        k = len(m)
        assert int(kh[i]) == int(got["period"][i]) == k, (m, int(kh[i]), got[i])
        assert O.rot_seq(sh[i], k) == O.rot_seq(int(got["unit"][i]), k)


# ---- the `trew periods` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def split_sections(lines):
    at = lines.index(">Summary")
    return lines[:at], lines[at:]


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_cli_golden_long(suffix):
    path = os.path.join(GOLDEN, "test_long.fastq" + suffix)
    reads = read_fastq(os.path.join(GOLDEN, "test_long.fastq"))
    rows, summary = R.cli_lines(os.path.realpath(path), reads, R.periods(reads))
    got_rows, got_summary = split_sections(run_cli("periods", path, "-t", "3"))
    assert got_rows[:2] == rows[:2] and sorted(got_rows[2:]) == sorted(rows[2:])
    assert got_summary == summary


def test_cli_generated_file_with_planted_tracts(tmp_path):
    rnd = random.Random(17)
    reads = []
    for i in range(60):
        unit = [TEL, "CCCTAA", "AAT", "TG", KAT32[2], None][i % 6]
        body = junk(rnd, rnd.randint(50, 900))
        reads.append((body if unit is None else body + noisy(rnd, unit, rnd.randint(60, 700), 0.03) + junk(rnd, rnd.randint(0, 80))).encode())
    path = str(tmp_path / "planted.fastq")
    write_fastq(path, reads)
    for args in ((1, 32, 3, 24), (2, 12, 5, 40)):
        recs = R.periods(reads, *args)
        rows, summary = R.cli_lines(os.path.realpath(path), reads, recs)
        assert len(rows) - 2 >= 40 and len(summary) - 2 >= 3
        got_rows, got_summary = split_sections(run_cli("periods", path, "--min_period", str(args[0]), "--max_period", str(args[1]), "--penalty", str(args[2]),
                                                       "--min_score", str(args[3]), "-t", "2"))
        assert got_rows[:2] == rows[:2] and sorted(got_rows[2:]) == sorted(rows[2:])
        assert got_summary == summary
    # two files: the summary is over both
    got = run_cli("periods", path, path)
    assert got.count(">" + os.path.realpath(path)) == 2
    both = R.cli_lines(os.path.realpath(path), reads + reads, np.concatenate([R.periods(reads)] * 2))[1]
    assert split_sections(got)[1] == both
