"""De novo repeats, every tract of a read, on the GPU (trew_hip_repeats through ctypes).  Every record of every batch is
compared, integer for integer, with trew_repeats_host (itself checked against tests/repeat_ref.py in test_repeats_cpu.py), and
with repeat_ref where the reads are few or short."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import period_ref as R
import repeat_ref as RR
from period_cases import TEL, UNITS, fuzz_reads, junk, noisy, rep
from repeat_cases import SAT, edge_reads, k32_seam_reads, seam_reads, stack_reads, two_satellites
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 20  # a log that holds every tract of every batch here


def same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in RR.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at record %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_repeats(reads_or_packed, *args, mode=capi.MODE_LONG, max_records=BIG):
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16)) as t:
        t.repeats(t.host_batch(words, offsets, lengths), *args, max_records=max_records)
        return t.repeats_results()


def check(reads, *args, ref=()):
    """GPU == host, records, counts and number; the reads whose indices are in `ref` against the brute-force reference as well"""
    packed = capi.pack_reads(reads)
    want, want_counts, found = capi.repeats_host(packed, *args)
    got, counts, n = gpu_repeats(packed, *args)
    assert n == found == len(want)
    assert (counts == want_counts).all(), np.flatnonzero(counts != want_counts)[:5]
    same(got, want)
    if len(ref):
        sub, sub_counts = RR.repeats([reads[i] for i in ref], *args)
        assert (want_counts[list(ref)] == sub_counts).all()
        at = np.concatenate([[0], np.cumsum(want_counts.astype(np.int64))])
        mine = np.concatenate([want[at[i]:at[i + 1]] for i in ref])
        mine["read"] = sub["read"]
        same(mine, sub)
    return want, want_counts


# ---- piece edges at every bit
@pytest.mark.parametrize("k", [1, 2, 3, 6, 31, 32])
def test_piece_edges_at_every_bit(k):
    reads, equal = edge_reads(k)
    assert len(reads) == 3 * len({0, 1, k - 1, k, 40}) * 2 * 64
    want, counts = check(reads, 1, 32, 3, 20, ref=range(0, len(reads), 97))
    assert (counts >= 1).all() and (counts >= 2).sum() >= 300
    # the children's lo (the end of a tract in front) and hi (the start of a tract behind) take every bit of a word
    child = want[want["depth"] > 0]
    assert len(set((child["start"] & 31).tolist())) == 32 and len(set((child["end"] & 31).tolist())) == 32
    first = want[np.concatenate([[True], want["read"][1:] != want["read"][:-1]])]
    assert len(set((first["end"] & 31).tolist())) == 32
    # penalty 64: no segment bridges the gap; with equal units and 0 < g < k the reference says two records (test_repeats_cpu.py)
    want, counts = check(reads, 1, 32, 64, 20, ref=range(5, len(reads), 193))
    two = [i for i, e in enumerate(equal) if e and 0 < e[0] < k]
    assert (counts[two] == 2).all() and (len(two) > 0) == (k >= 2)
    check(reads, k, k, 1, 8)


# ---- iteration seams relative to the piece
@pytest.mark.parametrize("k", [2, 6, 32])
def test_iteration_seams_relative_to_the_piece(k):
    reads, wanted = seam_reads(k)
    assert 4400 <= max(len(r) for r in reads) <= 5200
    want, counts = check(reads, 1, 32, 3, 24, ref=range(0, len(reads), 41))
    assert (counts >= 2).all()
    hit = 0
    for i, (lo, at, side) in enumerate(wanted):
        mine = want[want["read"] == i]
        parent_end = int(mine[mine["depth"] == 0]["end"][0])  # the 400-base tract, whose end is the child's lo
        child = [x for x in mine if x["depth"] > 0 and int(x["scored_period"]) % k == 0 and int(x[side]) == at]
        hit += parent_end == lo and len(child) == 1 and int(child[0]["end"]) - parent_end > 2048 - 64
    print("reads whose child tract has its %s where it was asked for: %d of %d" % ("start or end", hit, len(wanted)))
    assert hit >= 0.9 * len(wanted)  # chance matches in the background move a few ends by a base
    check(reads, k, k, 64, 8)


def test_k32_partners_in_the_next_iteration_of_a_piece():
    reads = k32_seam_reads()
    want, counts = check(reads, 1, 32, 3, 24, ref=range(0, len(reads), 13))
    assert (counts >= 2).all()
    assert ((want["scored_period"] == 32) & (want["depth"] > 0)).sum() >= len(reads) - 2
    check(reads, 32, 32, 3, 1)


# ---- the stack
def test_stack_chains_tree_and_64_tracts_in_one_wave():
    reads = stack_reads()
    want, counts = check(reads, 1, 32, 3, 24, ref=range(4))
    assert counts.tolist() == [6, 6, 6, 64]
    depth = [int(want[want["read"] == r]["depth"].max()) for r in range(4)]
    assert depth[:3] == [5, 5, 2] and depth[3] >= 4
    check(reads * 5, 1, 32, 64, 8)


# ---- the log
def test_log_overflow_exact_numbers_and_repeated_calls():
    rnd = random.Random(4096)
    one = junk(rnd, 120) + rep(TEL, 200) + junk(rnd, 90) + rep(SAT, 150) + junk(rnd, 77)
    want1, counts1, found1 = capi.repeats_host([one])
    assert found1 == 2
    n = 4096
    packed = capi.pack_reads([one] * n)
    want = np.repeat(want1.reshape(1, 2), n, axis=0).reshape(-1).copy()
    want["read"] = np.repeat(np.arange(n), 2)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=n) as t:
        b = t.host_batch(*packed)
        for cap in (1, n, 2 * n - 1, 2 * n, 2 * n + 1, BIG, 2 * n - 1, 2 * n):  # below, at and above the need, and back
            t.repeats(b, max_records=cap)
            got, counts, found = t.repeats_results()
            assert found == 2 * n and (counts == 2).all()  # exact also on overflow
            if cap < 2 * n:
                assert len(got) == 0  # nothing is copied from an overflowed log
            else:
                same(got, want)
        # a caller's buffer smaller than the log: the first records of the sorted order
        t.repeats(b, max_records=2 * n)
        num = C.c_uint64(0)
        five = np.zeros(5, dtype=capi.REPEAT_DTYPE)
        assert t.lib.trew_hip_repeats_results(t.ctx, 0, five.ctypes.data, 5, C.byref(num), None, None) == 0
        assert num.value == 2 * n
        same(five, want[:5])
        assert t.lib.trew_hip_repeats_results(t.ctx, 0, None, 0, None, None, None) != 0
        assert t.lib.trew_hip_repeats_results(t.ctx, 0, None, 5, C.byref(num), None, None) != 0
        with pytest.raises(capi.TrewHipError, match="max_records must be at least 1"):
            t.repeats(b, max_records=0)


def test_convenience_entry_point_retries():
    import trew_amd

    reads = fuzz_reads(2, 400, 700)
    want, want_counts, found = capi.repeats_host(reads, 1, 32, 3, 8)
    assert found > len(reads)  # the first log, one record per read, overflows
    got, counts = trew_amd.repeats(reads, 1, 32, 3, 8)
    same(got, want)
    assert (counts == want_counts).all()
    got, counts = trew_amd.repeats(reads)
    same(got, capi.repeats_host(reads)[0])


# ---- read ends
def test_degenerate_and_small_reads():
    rnd = random.Random(5)
    reads = []
    for k, unit in UNITS.items():
        for n in (0, 1, 2, k, k + 1, 31, 32, 33, 63, 64, 65):
            reads.append(rep(unit, n))
            reads.append(junk(rnd, n))
        for n in (100, 2048, 2049, 2048 + k, 2080):
            reads.append(junk(rnd, n - min(n, 6 * k + 3)) + rep(unit, min(n, 6 * k + 3)))  # the tract ends exactly at n
            reads.append(rep(unit, min(n, 6 * k + 3)) + junk(rnd, n - min(n, 6 * k + 3)))  # and starts at 0
    reads += ["N" * 70, "N" * 2100, "", rep(TEL, 60) + "N" * 40 + rep(SAT, 60)]
    for args in ((1, 32, 3, 1), (1, 32, 1, 24), (1, 1, 3, 1), (32, 32, 3, 1), (6, 6, 64, 1), (1, 32, 3, 8)):
        check(reads, *args, ref=range(0, len(reads), 3) if args == (1, 32, 3, 8) else ())


def test_bits_past_the_read_end_do_not_matter():
    rnd = random.Random(6)
    reads = [noisy(rnd, rnd.choice(list(UNITS.values())), n, 0.03) + junk(rnd, m) for n in (1, 5, 31, 33, 40, 63, 65, 70, 100, 2047, 2050, 2079)
             for m in (0, 3, 41)]
    words, offsets, lengths = capi.pack_reads(reads)
    want, want_counts, found = capi.repeats_host((words, offsets, lengths), 1, 32, 3, 4)
    dirty = np.array(words, dtype=np.uint32)
    for o, n in zip(offsets.tolist(), lengths.tolist()):
        if n % 32:
            last = o + 3 * (n // 32)
            hi = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
            dirty[last + 2] |= hi                                      # nmask set past the end, which the format allows
            dirty[last] |= np.uint32(rnd.getrandbits(32)) & hi         # and anything in the planes there
            dirty[last + 1] |= np.uint32(rnd.getrandbits(32)) & hi
    assert (dirty != words).any() and found > len(reads)
    same(capi.repeats_host((dirty, offsets, lengths), 1, 32, 3, 4)[0], want)
    got, counts, n = gpu_repeats((dirty, offsets, lengths), 1, 32, 3, 4)
    same(got, want)
    assert (counts == want_counts).all() and n == found


# ---- a long read
def test_long_read_with_three_planted_tracts():
    rnd = random.Random(200000)
    # exact tracts: at P = 64 one substituted base costs 128 and would cut a tract in two
    parts = [junk(rnd, 60_000), rep(SAT, 900), junk(rnd, 70_000), rep(TEL, 3000), junk(rnd, 65_000), rep("AC", 400)]
    read = "".join(parts) + junk(rnd, 200_000 - sum(len(p) for p in parts))
    assert len(read) == 200_000
    want, counts = check([read], 1, 32, 64, 24)
    assert counts.tolist() == [3] and want["period"].tolist() == [5, 6, 2] and want["depth"].tolist() == [1, 0, 1]
    assert [int(x["end"]) - int(x["start"]) >= n for x, n in zip(want, (900, 3000, 400))] == [True] * 3


# ---- fuzz
@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz(seed):
    reads = fuzz_reads(seed, 400, 700)
    for min_score in (24, 8):
        for penalty in (1, 3, 64):
            for lo, hi in ((1, 32), (1, 1), (32, 32), (5, 7), (2, 31)):
                check(reads, lo, hi, penalty, min_score)
    want, counts = check(reads, 1, 32, 3, 8, ref=range(0, 400, 9))
    assert (counts >= 3).sum() >= 30 and int(want["depth"].max()) >= 3


# ---- depth 0 is periods
def test_depth_zero_equals_periods_on_mixed_reads():
    reads = fuzz_reads(99, n=2000, max_len=400)
    packed = capi.pack_reads(reads)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        t.periods(b)
        per = t.periods_results()
        t.repeats(b, max_records=BIG)
        got, counts, found = t.repeats_results()
    assert 200 <= (per["period"] > 0).sum() <= 1800
    zero = got[got["depth"] == 0]
    assert (zero["read"] == np.flatnonzero(per["period"] > 0)).all() and ((counts > 0) == (per["period"] > 0)).all()
    for f in R.FIELDS:
        assert (zero[f] == per[f][zero["read"]]).all(), f
    same(got, capi.repeats_host(packed)[0])


# ---- batch shapes and contexts
@pytest.fixture(scope="module")
def uniform150():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 4000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.repeats_host(reads, 1, 32, 3, 8)
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
        t.repeats(b, 1, 32, 3, 8, max_records=BIG)
        got, counts, num = t.repeats_results()
        if d is not None:
            t.free(d)
    same(got, want)
    assert (counts == want_counts).all() and num == found


@pytest.mark.parametrize("max_length", ["known", "unknown"])
def test_device_resident_ragged(max_length):
    n = 200
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    want, want_counts, found = capi.repeats_host([buf[s:e + 1] for s, e in zip(st, nd)])
    assert (want["period"] == 6).sum() >= 5
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        if max_length == "unknown":
            b.max_length = 0
        t.repeats(b, max_records=BIG)
        got, counts, num, ms = t.repeats_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, want)
    assert (counts == want_counts).all() and num == found


def test_pair_mode_context_two_slots_and_errors():
    a, b = fuzz_reads(41, n=250), fuzz_reads(42, n=151)  # an odd number of reads is refused in pair mode
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_repeats"):
            t.repeats_results()
        t.periods(ba)  # a periods call is no repeats call: the buffers are separate
        t.periods_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_repeats"):
            t.repeats_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.repeats(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:150]))
        t.repeats(ba, 1, 32, 3, 8, max_records=BIG, slot=0)  # the mates are two reads; the two slots overlap
        t.repeats(bb, 2, 12, 7, 5, max_records=BIG, slot=1)
        got1, got0 = t.repeats_results(1), t.repeats_results(0)
        for got, want in ((got1, capi.repeats_host(b[:150], 2, 12, 7, 5)), (got0, capi.repeats_host(a, 1, 32, 3, 8))):
            same(got[0], want[0])
            assert (got[1] == want[1]).all() and got[2] == want[2] > 150
        for lo, hi in ((0, 5), (3, 2), (1, 33)):
            with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
                t.repeats(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.repeats(ba, penalty=penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.repeats(ba, min_score=0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.repeats(ba, slot=3)


# ---- independence
def test_independent_of_scan_and_the_other_measures():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 12000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:7000], reads[7000:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = capi.repeats_host(a, 1, 32, 3, 12), capi.repeats_host(b, 2, 12, 5, 12)
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

    def fetch(t, slot=0):
        return (t.annotate_results(slot), t.tracts_results(slot)) + t.intervals_results(slot) + t.variants_results(slot) + (t.periods_results(slot),) + t.chain_results(slot)

    with fresh() as t:  # without any repeats call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        others(t, ba)
        alone = fetch(t)
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # repeats calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.repeats(ba, 1, 32, 3, 12, max_records=LOG, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.repeats(bb, 2, 12, 5, 12, max_records=LOG, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.intervals(ba, motifs, 6, 12, LOG, slot=0)
        t.variants(ba, motifs, slot=0)
        t.periods(ba, slot=0)
        t.chain(ba, motifs, 8 * LOG, slot=0)
        t.submit(bb, slot=1)
        got_r1 = t.repeats_results(1)
        got_r0 = t.repeats_results(0)
        got = fetch(t)
        tables = t.collect()
    for g, w in ((got_r0, want_a), (got_r1, want_b)):
        same(g[0], w[0])
        assert (g[1] == w[1]).all() and g[2] == w[2] > 0
    assert len(got) == len(alone)
    for x, y in zip(got, alone):
        assert (np.asarray(x) == np.asarray(y)).all()
    same_p = capi.periods_host(a)
    assert all((got[-5][f] == same_p[f]).all() for f in R.FIELDS)
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- the `trew repeats` subcommand, end to end
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
    for i in range(60):
        units = [TEL, "CCCTAA", "AAT", "TG", SAT, None]
        body = junk(rnd, rnd.randint(50, 400))
        for j in range(i % 4):  # tracts shorter than what the background between them costs: no period bridges two of them
            unit = units[(i + j) % 6]
            body += (junk(rnd, 20) if unit is None else noisy(rnd, unit, rnd.randint(70, 160), 0.02)) + junk(rnd, rnd.randint(160, 250))
        reads.append(body.encode())
    reads.append(two_satellites(rnd, 0.02).encode())
    path = str(tmp_path / "planted.fastq")
    write_fastq(path, reads)
    for args in ((1, 32, 3, 24), (2, 12, 5, 40)):
        recs, counts = RR.repeats(reads, *args)
        rows, summary = RR.cli_lines(os.path.realpath(path), reads, recs)
        assert len(rows) - 2 > len(reads) and (counts >= 3).sum() >= 5 and len(summary) - 2 >= 4
        out, err = run_cli("repeats", path, "--min_period", str(args[0]), "--max_period", str(args[1]), "--penalty", str(args[2]), "--min_score", str(args[3]),
                           "-t", "2", "--stats")
        got_rows, got_summary = split_sections(out)
        assert got_rows == rows  # sorted by read, then start
        assert got_summary == summary
        # more tracts than reads: the first log of the one batch overflowed and the batch was resubmitted once
        assert "%d tracts, 1 batch(es) resubmitted with a larger log" % len(recs) in err
    # two files: the summary is over both
    out, _ = run_cli("repeats", path, path)
    assert out.count(">" + os.path.realpath(path)) == 2
    recs = RR.repeats(reads)[0]
    twice = np.concatenate([recs, recs])
    twice["read"][len(recs):] += len(reads)
    assert split_sections(out)[1] == RR.cli_lines(os.path.realpath(path), reads + reads, twice)[1]
    # `trew periods` is the depth-0 rows without the depth column
    per, _ = run_cli("periods", path)
    zero = [",".join(x.split(",")[:2] + x.split(",")[3:]) for x in split_sections(out)[0][2:2 + len(recs)] if x.split(",")[2] == "0"]
    assert split_sections(per)[0][2:] == zero
