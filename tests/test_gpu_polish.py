"""De novo repeats under indels for periods up to 256 on the GPU (trew_hip_polish through ctypes).  Every read of every batch
is compared, integer for integer, with trew_polish_host (itself checked against tests/polish_ref.py in test_polish_cpu.py)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import period_ref as P
import polish_cases as PC
import polish_ref as R
import refine_cases
import satellite_ref as SR
from period_cases import fuzz_reads, junk, noisy, rep
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ_LONG = os.path.join(ROOT, "tests", "golden", "test_long.fastq")


def rec(x):
    return R.as_tuple(x)


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at read %d: got %s, want %s" % (f, bad[0][0], got[bad[0][0]], want[bad[0][0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18, flags=0):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16, flags=flags)


def gpu_polish(reads_or_packed, *args, mode=capi.MODE_LONG):
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16)) as t:
        t.polish(t.host_batch(words, offsets, lengths), *args)
        return t.polish_results()


def check(reads, *args):
    """GPU == the host definition on every read"""
    want = capi.polish_host(reads, *args)
    same(gpu_polish(reads, *args), want)
    return want


# ---- layouts, unit lengths and read lengths
def shape_reads(k, seed):
    """perfect, shifted, noisy and random reads of every listed length for a planted unit of k bases"""
    rnd = random.Random(seed)
    unit = PC.unit_of(k, 31) if k > 2 else "A" if k == 1 else "TG"
    reads = []
    for n in (0, 1, k, k + 1, 2 * k - 1, 2 * k, 2 * k + 1, 4 * k + 37) + ((2047, 2048, 2049) if k in (2, 33, 65, 171, 256) else ()):
        reads += [rep(unit, n), rep(unit, n, rnd.randrange(k)), noisy(rnd, unit, n, 0.03, 0.02, 0.004), junk(rnd, n, "ACGTN" if n % 2 else "ACGT")]
    return reads


@pytest.mark.parametrize("max_period", [32, 64, 65, 128, 129, 256])
def test_layout_edges_unit_lengths_and_read_lengths(max_period):
    """every Q at both ends of its range; every planted k up to max_period, so small units on wide layouts too (a last live
    lane with fewer than Q live slots, dead lanes above it)"""
    reads = []
    for k in PC.GPU_KS:
        if k <= max_period:
            reads += shape_reads(k, 100 * max_period + k)
    for args in ((1, max_period, 3, 1), (1, max_period, 2, 24), (1, max_period, 64, 1)):
        want = check(reads, *args)
    assert (want["period"] > 0).sum() >= len(reads) // 3
    lo = max(1, max_period - 40)
    check(reads, lo, max_period, 3, 5)


def test_small_units_on_the_widest_layout():
    """k = 6 and k = 33 under max_period 256 (Q = 4): long noisy arrays, so all three passes run with most lanes dead"""
    rnd = random.Random(633)
    reads = [junk(rnd, rnd.randint(0, 50)) + noisy(rnd, u, rnd.randint(300, 1500), 0.04, 0.03, 0.002) + junk(rnd, rnd.randint(0, 50))
             for u in ("TTAGGG", PC.unit_of(33, 1)) for _ in range(40)]
    want = check(reads, 1, 256, 3, 24)
    assert (want["changed"] > 0).sum() >= 3 and ((want["period"] == 6) | (want["period"] == 33)).sum() >= 60
    check(reads, 1, 256, 2, 24)


# ---- the seed: seams of the longest run, equal runs, N, a root that is a proper divisor
@pytest.mark.parametrize("k", [33, 64, 171])
def test_longest_run_at_word_lane_and_iteration_seams(k):
    """The longest run starts (first set) or ends (second set) at bit 31, bit 0 and bit 1 of a word -- a word is a lane -- and at
    the 64-word seam; then one base is removed and one is added right there.  The eq word is the wide one."""
    unit = PC.unit_of(k, 21)
    length = 70 + 3 * k
    reads = []
    for seam in (31, 32, 33, 64, 2047, 2048, 2049):
        pair = [PC.runs_read(unit, seam, length)] + ([PC.runs_read(unit, seam - length, length)] if seam > length else [])
        reads += pair
        for base in pair:
            reads.append(PC.with_deletion(base, seam))
            reads.append(PC.with_insertion(base, seam, "C"))
    rnd = random.Random(k)
    reads += [PC.run_at(unit, lead, 90 + k, 40, rnd) for lead in (31, 32, 33, 2047, 2048, 2049)]
    want = check(reads, 1, 256, 3, 24)
    assert (want["period"] == k).sum() >= len(reads) - 4
    check(reads, k, k, 2, 1)


def test_two_and_three_runs_of_equal_length_the_first_wins():
    reads = []
    for k in (33, 64, 171):
        unit = PC.unit_of(k, 21)
        length = 100 + k
        reads += [PC.runs_read(unit, start, length, 2) for start in (40, 2048 - length, 2048 - length - k - 1, 2049, 4096 - length)]
        reads.append(PC.runs_read(unit, 33, length, 3))
    check(reads, 1, 256, 3, 24)


def test_seed_and_vote_edges():
    """an N in the seed window at phase 80 (another lane's consensus phase supplies it; the builder asserts where it lies), a seed whose root is a proper
    divisor, the seed-kept case, tied counts (two variants of a unit in turn: the seed's base or the smallest code), a phase
    without votes (an N there in every copy), and arrays whose first and last phases carry the errors"""
    u40, u100, u171 = PC.unit_of(40, 41), PC.unit_of(100, 41), PC.unit_of(171, 41)
    reads = [PC.n_in_seed_window(), PC.SEED_KEPT, PC.n_in_seed_window(lead=90, tail=70)]
    for u in (u40, u100, u171):
        k = len(u)
        for at in (0, 1, k // 2, k - 2, k - 1):
            v = PC.replaced(u, at)
            reads.append((u + v) * 4)                      # tied counts at phase `at`
            o = [PC.replaced(u, (at + 5 + 9 * i) % k) for i in range(5)]
            reads.append(o[0] + o[1] + v + v + o[2] + o[3] + o[4])  # the seed is v (the longest run), the vote changes phase `at` back to u's base
            reads.append((u[:at] + "N" + u[at + 1:]) * 5)  # a phase without votes
    want = check(reads, 1, 256, 3, 10)
    assert rec(want[1])[:4] == (33, 33, 33, 0) and rec(want[0])[:3] == (100, 100, 100)
    assert (want["changed"] > 0).sum() >= 3
    same(gpu_polish([PC.divisor_read()], 34, 256, 3, 24), capi.polish_host([PC.divisor_read()], 34, 256, 3, 24))
    assert rec(capi.polish_host([PC.divisor_read()], 34, 256, 3, 24)[0])[:4] == (17, 17, 34, 0)


@pytest.mark.parametrize("max_period,q,read,one_lane,two_lanes", PC.TIE_READS, ids=["%d-q%d-%d" % (t[0], t[1], len(t[2])) for t in PC.TIE_READS])
def test_tied_votes_where_the_smallest_phase_decides_the_record(max_period, q, read, one_lane, two_lanes):
    """a voting row whose largest V lies in several phases -- in two slots of one lane, in two lanes -- where the record differs
    when another of them gets the vote (asserted with the reference in test_polish_cpu.py), on the layout of `max_period`"""
    want = check([read, read[3:], read], 1, max_period, 3, 24)
    assert 64 * q >= max_period > 32 * q and want["period"][0] == want["period"][2] > 32 and want["support"][0] > 0


# ---- the alignment: runs of deleted and inserted bases across the wrap and across lane seams
@pytest.mark.parametrize("k", [40, 100, 171, 256])
def test_runs_of_deleted_and_inserted_bases_at_the_wrap_and_at_lane_seams(k):
    unit = PC.unit_of(k, 51)
    q = PC.q_of(k)
    reads = []
    for phase in sorted({0, 1, q - 1, q, 2 * q - 1, 2 * q, 17 * q - 1, 17 * q, k - 2, k - 1}):
        for d in (1, 2, 3, 5):
            # three copies in front and one and a bit behind: two equal halves around the run would repeat at a period of their own
            head, p = "ACGTAC" + rep(unit, 3 * k + phase % k), phase % k
            reads.append(head + rep(unit, k + 17, (p + d) % k) + "TTGCA")
            reads.append(head + "GATCA"[:d] + rep(unit, k + 17, p) + "TTGCA")
    want = check(reads, 1, 256, 3, 24)
    assert (want["period"] == k).sum() >= len(reads) - 8
    cols = capi.refine_columns(want, 3)
    assert (cols["deletions"] > 0).sum() >= len(reads) // 4 and (cols["insertions"] > 0).sum() >= len(reads) // 4
    check(reads, 1, 256, 2, 24)


def test_one_error_at_every_7th_position_of_a_68_base_unit():
    reads = [r for _, _, r in PC.one_error_reads()]
    want = check(reads, 1, 256, 3, 24)
    assert (want["period"] == 68).all()


# ---- the fuzz sets and the consequences on the GPU
def test_equals_trew_hip_refine_at_max_period_32_on_refines_fuzz_set():
    reads = [r for _, r in refine_cases.fuzz_set()] + [r for r, _, _ in refine_cases.HAND]
    packed = capi.pack_reads(reads)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        for penalty in (1, 3, 64):
            t.polish(b, 1, 32, penalty, 24)
            t.refine(b, 1, 32, penalty, 24)
            got, ref = t.polish_results(), t.refine_results()
            for f in R.U32_FIELDS:
                assert (got[f] == ref[f]).all(), f
            for g, x in zip(got, ref):
                assert SR.unit_text(g["unit"], g["period"]) == P.unit_text(x["unit"], int(x["period"]))
                assert SR.unit_text(g["seed_unit"], g["seed_period"]) == P.unit_text(x["seed_unit"], int(x["seed_period"]))
            same(got, capi.polish_host(packed, 1, 32, penalty, 24))


@pytest.fixture(scope="module")
def fuzz():
    reads = [r for _, r, _, _ in PC.fuzz_set()]
    return reads, capi.polish_host(reads)


def test_fuzz_set(fuzz):
    reads, want = fuzz
    same(gpu_polish(reads), want)
    assert (want["changed"] > 0).sum() >= 5 and (want["period"] > 32).sum() >= 36
    short = [r for _, r, _, _ in PC.short_set()]
    for max_period in (64, 128, 256):
        check(short, 1, max_period, 3, 24)


def test_alignments_equal_trew_hip_monomers_on_the_gpu(fuzz):
    """seed_score, and with changed = 0 the whole of A2 = A1, equal the forward fields of trew_hip_monomers with the unit S;
    with changed > 0 the fields of A2 equal those with the unit U"""
    reads, _ = fuzz
    packed = capi.pack_reads(reads)
    checked = 0
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        t.polish(b)
        got = t.polish_results()
        for field, length, pick in (("seed_unit", "seed_period", lambda i: True), ("unit", "period", lambda i: got["changed"][i] > 0)):
            idx = [i for i in range(len(reads)) if got[length][i] >= 3 and pick(i)]
            for at in range(0, len(idx), 8):
                part = idx[at:at + 8]
                t.monomers(b, [SR.unit_text(got[field][i], got[length][i]) for i in part], 3)
                a = t.monomers_results()
                for m, i in enumerate(part):
                    five = tuple(int(a[n][i, m]) for n in ("score_fwd", "start_fwd", "end_fwd", "consumed_fwd", "matches_fwd"))
                    if field == "seed_unit":
                        assert five[0] == int(got["seed_score"][i])
                    if field == "unit" or got["changed"][i] == 0:
                        assert five == rec(got[i])[4:9]
                        checked += 1
    assert checked >= 36


# ---- long reads
def test_long_perfect_repeat_and_long_noisy_read():
    rnd = random.Random(70000)
    u171, u256 = PC.unit_of(171, 61), PC.unit_of(256, 61)
    perfect = rep(u171, 70_000, 2)
    noisy_read = junk(rnd, 1500) + noisy(rnd, u256, 100_000 - 2500, 0.02, 0.004, 0.001) + junk(rnd, 1000)
    want = check([perfect], 1, 256, 3, 24)
    assert rec(want[0])[:9] == (171, 171, 171, 0, 70_000, 0, 70_000, 70_000, 70_000)
    want = check([noisy_read], 1, 256, 64, 24)
    assert want["scored_period"][0] in (255, 256) and want["score"][0] >= 24


# ---- repeatability and persistence
def test_many_copies_and_repeated_calls():
    rnd = random.Random(4096)
    one = junk(rnd, 300) + noisy(rnd, PC.unit_of(100, 71), 900, 0.04, 0.02) + junk(rnd, 77)
    want1 = capi.polish_host([one])
    assert want1["period"][0] > 32 and want1["score"][0] >= 500
    same(gpu_polish([one] * 512), np.repeat(want1, 512))
    reads = fuzz_reads(99, n=400, max_len=400)
    packed = capi.pack_reads(reads)
    want = capi.polish_host(packed)
    assert 40 <= (want["period"] > 0).sum() <= 360
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        for _ in range(3):
            t.polish(b)
            same(t.polish_results(), want)


@pytest.mark.parametrize("max_period", [64, 128, 256])
def test_waves_go_well_past_their_first_read(max_period):
    """TREW_FLAG_DEBUG_ONE_CU: 32 waves for a few thousand short reads, about a hundred reads a wave"""
    rnd = random.Random(max_period)
    units = [PC.unit_of(k, 8) for k in (5, 33, 40, 64, 65, 100) if k <= max_period]
    reads = [junk(rnd, rnd.randint(0, 20), "ACGTN") + noisy(rnd, rnd.choice(units), rnd.randint(0, 260), 0.03, 0.03, 0.01) for _ in range(3000)]
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads), flags=capi.FLAG_DEBUG_ONE_CU) as t:
        assert t.debug_measure_grid(len(reads)) == 8
        t.polish(t.host_batch(words, offsets, lengths), 1, max_period, 3, 12)
        got = t.polish_results()
    want = capi.polish_host(reads, 1, max_period, 3, 12)
    same(got, want)
    assert (want["period"] > 0).sum() >= 1000 and (want["period"] == 0).sum() >= 100


# ---- batch shapes and contexts
@pytest.fixture(scope="module")
def uniform150():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 4000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.polish_host(reads, 1, 100, 3, 24)
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
        t.polish(b, 1, 100, 3, 24)
        got = t.polish_results()
        if d is not None:
            t.free(d)
    same(got, want)


@pytest.mark.parametrize("max_length", ["known", "unknown"])
def test_device_resident_ragged(max_length):
    n = 24
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    want = capi.polish_host([buf[s:e + 1] for s, e in zip(st, nd)])
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        if max_length == "unknown":
            b.max_length = 0
        t.polish(b)
        got, ms = t.polish_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, want)


def test_pair_mode_context_two_slots_and_errors():
    a, b = fuzz_reads(41, n=250), fuzz_reads(42, n=151)  # an odd number of reads is refused in pair mode
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_polish"):
            t.polish_results()
        t.refine(ba)  # a refine call is no polish call: the buffers are separate
        t.refine_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_polish"):
            t.polish_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.polish(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:150]))
        t.polish(ba, 1, 256, 3, 24, slot=0)  # the mates are two reads; the two slots overlap
        t.polish(bb, 2, 70, 7, 5, slot=1)
        same(t.polish_results(1), capi.polish_host(b[:150], 2, 70, 7, 5))
        same(t.polish_results(0), capi.polish_host(a))
        for lo, hi in ((0, 5), (3, 2), (1, 257)):
            with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 256"):
                t.polish(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.polish(ba, penalty=penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.polish(ba, min_score=0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.polish(ba, slot=3)
        # results larger than the caller's buffer: the count is reported, cap records are copied
        t.polish(ba)
        n = C.c_uint64(0)
        three = np.zeros(3, dtype=capi.POLISH_DTYPE)
        assert t.lib.trew_hip_polish_results(t.ctx, 0, three.ctypes.data, 3, C.byref(n), None) == 0
        assert n.value == 250
        same(three, capi.polish_host(a[:3]))
        assert t.lib.trew_hip_polish_results(t.ctx, 0, None, 0, C.byref(n), None) == 0 and n.value == 250
        # no reads: no records, no kernel
        t.polish(t.host_batch(*capi.pack_reads([])))
        assert t.polish_results().shape == (0,)


def test_convenience_entry_point():
    import trew_amd

    reads = fuzz_reads(77, n=120)
    same(trew_amd.polish(reads), capi.polish_host(reads))
    same(trew_amd.polish(reads, 3, 80, penalty=5, min_score=9), capi.polish_host(reads, 3, 80, 5, 9))


# ---- independence
def test_independent_of_scan_and_the_other_measures():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 5000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3000], reads[3000:]
    units = [PC.unit_of(100, 9), PC.unit_of(36, 9)]
    want_a, want_b = capi.polish_host(a), capi.polish_host(b, 2, 70, 5, 12)
    LOG = 1 << 16

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    def fetch(t, slot=0):
        return (t.refine_results(slot),) + t.satellites_results(slot) + (t.monomers_results(slot),)

    with fresh() as t:  # without any polish call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.refine(ba)
        t.satellites(ba, 1, 256, max_records=LOG)
        t.monomers(ba, units, 3)
        alone = fetch(t)
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # polish calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.polish(ba, slot=0)
        t.refine(ba, slot=0)
        t.polish(bb, 2, 70, 5, 12, slot=1)
        t.satellites(ba, 1, 256, max_records=LOG, slot=0)
        t.monomers(ba, units, 3, slot=0)
        t.submit(bb, slot=1)
        got_1 = t.polish_results(1)
        got_0 = t.polish_results(0)
        got = fetch(t)
        tables = t.collect()
    same(got_0, want_a)
    same(got_1, want_b)
    assert len(got) == len(alone)
    for x, y in zip(got, alone):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- the `trew polish` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def planted_array_reads(n=24, seed=8):
    """generator long reads, cut to at most 3 kb, with a planted array of 0.5 - 3 kb of one of four units that carries
    substitutions and indels"""
    rnd = random.Random(seed)
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    units = ["TTAGGG", PC.unit_of(48, 3), PC.unit_of(100, 3), PC.unit_of(171, 3)]
    out = []
    for i, (s, e) in enumerate(zip(st, nd)):
        body = buf[s:e + 1].decode()[:rnd.randint(300, 3000)]
        out.append((body + noisy(rnd, units[i % 4], rnd.randint(500, 3000), 0.02, 0.01, 0.002)).encode())
    return out


def test_cli_generator_long_reads_with_planted_arrays(tmp_path):
    reads = planted_array_reads()
    path = str(tmp_path / "arrays.fastq")
    write_fastq(path, reads)
    host3 = capi.polish_host(reads)
    rows, summary = R.cli_lines(path, reads, host3, 3)
    assert len(rows) - 2 >= len(reads) - 2 and len(summary) - 2 >= 4  # the planted arrays are found
    assert run_cli("polish", path, "-t", "2") == rows + summary
    assert run_cli("polish", path, "-t", "5") == rows + summary
    rows, summary = R.cli_lines(path, reads, capi.polish_host(reads, 40, 120, 2, 60), 2, min_score=60)
    assert 5 <= len(rows) - 2
    assert run_cli("polish", path, "--min_period", "40", "--max_period", "120", "--penalty", "2", "--min_score", "60", "-t", "3") == rows + summary
    got = run_cli("polish", path, path)
    assert got.count(">" + os.path.realpath(path)) == 2
    both = R.cli_lines(path, reads + reads, np.concatenate([host3] * 2), 3)[1]
    assert got[got.index(">Summary"):] == both


def test_cli_equals_trew_refine_at_max_period_32_on_the_golden_long_reads():
    ours, theirs = run_cli("polish", FQ_LONG, "--max_period", "32"), run_cli("refine", FQ_LONG)
    assert ours == theirs and ours[0].startswith(">") and len(ours) > 4
    ours, theirs = run_cli("polish", FQ_LONG, "--max_period", "32", "--penalty", "5", "--min_score", "40"), run_cli("refine", FQ_LONG, "--penalty", "5", "--min_score", "40")
    assert ours == theirs
