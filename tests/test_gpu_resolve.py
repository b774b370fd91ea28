"""Refine's unit with the period chosen by alignment on the GPU (trew_hip_resolve through ctypes).  Every read of every batch
is compared, word for word, with trew_resolve_host (itself checked against tests/resolve_ref.py in test_resolve_cpu.py), and
with resolve_ref directly where the reads are few or short."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import period_ref as P
import refine_ref as R
import resolve_ref as V
from period_cases import fuzz_reads, junk, noisy, rep
from refine_cases import fuzz_set
from resolve_cases import (ARGS, FLANK, GPU_KS, HAND, N_IN_SEED, ROTATED_SEED, SCORE_TIE, SEED_KEPT, SHORT_REPAIRED, T10, TEL, UNITS, mixed_reads, seeds_of,
                           shape_reads)
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
CS = (1, 2, 3, 4)


def rec(x):
    return tuple(int(v) for v in x)


def same(got, want, fields=V.FIELDS):
    assert got.shape == want.shape
    for f in fields:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at read %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18, flags=0):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16, flags=flags)


def gpu_resolve(reads_or_packed, *args, mode=capi.MODE_LONG, flags=0):
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16), flags=flags) as t:
        t.resolve(t.host_batch(words, offsets, lengths), *args)
        return t.resolve_results()


def check(reads, *args, ref=False):
    """GPU == host definition on every read (ref: also host definition == reference)"""
    got = gpu_resolve(reads, *args)
    want = capi.resolve_host(reads, *args)
    if ref:
        same(want, V.resolve(reads, *args))
    same(got, want)
    return want


@pytest.fixture(scope="module")
def fuzz():
    """(reads, {C: the host definition's records}) of the committed fuzz set, computed once"""
    reads = [r for _, r in fuzz_set()]
    return reads, {c: capi.resolve_host(reads, *ARGS, c) for c in CS}


# ---- shapes and sizes
def test_hand_worked_vectors():
    for args, c in sorted({(a, c) for _, a, c, _ in HAND}):
        rows = [(r, w) for r, a, cc, w in HAND if (a, cc) == (args, c)]
        got = gpu_resolve([r.encode() for r, _ in rows], *args, c)
        assert [rec(g) for g in got] == [w for _, w in rows]


@pytest.mark.parametrize("k", GPU_KS)
def test_unit_lengths_and_read_lengths(k):
    """perfect, one-deletion, one-insertion and noisy reads of every listed length, for the unit length k and every C"""
    short, long_ = shape_reads(k, random.Random(k))
    for c in CS:
        check(short, 1, 32, 3, 1, c, ref=c == 3)
        want = check(long_, *ARGS, c)
        assert (want["period"][:3] == k).all() and want["rank"][0] == 0 and want["candidates"][0] == min(c, 32 // k)
    check(short, 1, 32, 1, 24, 4)
    check(short, 1, 32, 64, 1, 2)
    check(long_, 1, 32, 1, 1, 4)
    check(long_, k, min(2 * k, 32), 64, 1, 3)


# ---- the cases that fail without the candidate loop
def test_winning_rank_one_and_two_on_the_fuzz_set(fuzz):
    reads, want = fuzz
    for c in CS:
        same(gpu_resolve(reads, *ARGS, c), want[c])
    later = [i for i in range(len(reads)) if want[3]["rank"][i] > 0]
    assert {int(want[3]["rank"][i]) for i in later} == {1, 2} and len(later) >= 8
    picked = [reads[i] for i in later]
    by_ref = V.resolve(picked)  # the reference itself for the reads that were repaired
    same(want[3][later], by_ref)
    same(gpu_resolve(picked), by_ref)
    assert (by_ref["score"] > by_ref["first_score"]).all()


def test_shortest_repaired_read():
    want = V.resolve_read(SHORT_REPAIRED)
    assert want[15] == 1 and want[4] > want[17]
    got = gpu_resolve([SHORT_REPAIRED, T10, SHORT_REPAIRED])
    assert rec(got[0]) == rec(got[2]) == want and got["rank"][1] == 0
    assert rec(gpu_resolve([SHORT_REPAIRED], *ARGS, 1)[0])[:14] == R.refine_read(SHORT_REPAIRED)


# ---- ties, the skipped duplicate seed and the rotated seed
def test_ties_and_seeds():
    perfect = ["A" * 40, T10, FLANK + T10 + FLANK, rep(UNITS[16], 100), rep(UNITS[3], 64, 1)]
    for read in perfect:  # the final scores of a unit and of its multiples tie; the multiples' seeds are the unit: skipped
        assert len({tuple(s) for s in seeds_of(read, 3)}) == 1
    s = seeds_of(ROTATED_SEED)
    assert len(s) == 2 and s[0] != s[1] and sorted(s[0]) == sorted(s[1])  # a rotation: aligned, not skipped
    reads = perfect + [SCORE_TIE, ROTATED_SEED, SEED_KEPT, N_IN_SEED, perfect[1] + ROTATED_SEED, ROTATED_SEED + "N" * 40 + SCORE_TIE]
    for c in CS:
        want = check(reads, *ARGS, c, ref=True)
        assert (want["rank"][:len(perfect)] == 0).all()
        check(reads, 1, 32, 3, 10, c, ref=True)
    want = capi.resolve_host(reads)
    assert rec(want[5])[14:] == (3, 1, 3, 33) and (want["candidates"][:3] == 3).all()


# ---- agreement with refine and align on the GPU
def test_candidates_one_is_trew_hip_refine_and_the_winner_is_trew_hip_align(fuzz):
    reads, _ = fuzz
    packed = capi.pack_reads(reads)
    checked = 0
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        t.refine(b)
        refined = t.refine_results()
        t.resolve(b, *ARGS, 1)
        same(V.refined(t.resolve_results()), refined.astype(R.DTYPE), R.FIELDS)
        t.resolve(b)
        got = t.resolve_results()
        assert (got["first_period"] == refined["period"]).all() and (got["first_score"] == refined["score"]).all()
        first = got["rank"] == 0
        same(V.refined(got[first]), refined[first].astype(R.DTYPE), R.FIELDS)
        idx = [i for i in range(len(reads)) if got["seed_period"][i] >= 3 and (got["changed"][i] == 0 or got["period"][i] >= 3)]
        for at in range(0, len(idx), 8):
            part = idx[at:at + 8]
            t.align(b, [P.unit_text(got["unit"][i], int(got["period"][i])) for i in part], 3)
            a = t.align_results()
            for m, i in enumerate(part):
                assert rec(a[i, m])[:5] == rec(got[i])[4:9]
                checked += 1
    assert checked >= 80


# ---- long reads
def test_long_perfect_repeat_and_long_noisy_read():
    rnd = random.Random(20000)
    perfect = rep(TEL, 70_000, 2)
    noisy_read = junk(rnd, 700) + noisy(rnd, UNITS[17], 20_000 - 1200, 0.03, 0.06, 0.001) + junk(rnd, 500)
    want = check([perfect, noisy_read])
    assert rec(want[0])[:9] == (6, 6, 6, 0, 70_000, 0, 70_000, 70_000, 70_000) and rec(want[0])[14:] == (3, 0, 6, 70_000)
    assert want["candidates"][1] == 3 and want["end"][1] - want["start"][1] >= 15_000


# ---- repeatability, many reads a wave
def test_many_reads_per_wave_with_different_candidate_counts():
    """one CU's grid: 32 waves take a few thousand reads, many each, with 0 .. 4 candidates one after the other -- the bins and
    the best-so-far words do not leak from read to read"""
    reads = mixed_reads(7, 3000) + [SHORT_REPAIRED, "", SCORE_TIE, "A"] * 8
    packed = capi.pack_reads(reads)
    want = capi.resolve_host(packed, *ARGS, 4)
    assert sorted(set(want["candidates"].tolist())) == [0, 1, 2, 3, 4] and (want["rank"] > 0).sum() >= 40
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads), flags=capi.FLAG_DEBUG_ONE_CU) as t:
        assert t.debug_measure_grid(len(reads)) == 8
        b = t.host_batch(*packed)
        for _ in range(2):  # repeated calls
            t.resolve(b, *ARGS, 4)
            same(t.resolve_results(), want)
        t.resolve(b, 2, 20, 2, 12, 2)
        same(t.resolve_results(), capi.resolve_host(packed, 2, 20, 2, 12, 2))
    same(gpu_resolve(packed, *ARGS, 4), want)


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_ragged_reads_and_parameters(seed):
    rnd = random.Random(seed)
    reads = fuzz_reads(3000 + seed, n=300)
    for penalty in (1, 3, 64):
        lo = rnd.randint(1, 32)
        check(reads, lo, rnd.randint(lo, 32), penalty, rnd.choice((1, 24)), rnd.choice(CS))
    want = check(reads[:40], *ARGS, 3, ref=True)
    assert (want["period"] > 0).sum() >= 10


# ---- batch shapes and contexts
@pytest.fixture(scope="module")
def uniform150():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 4000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.resolve_host(reads)
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
        t.resolve(b)
        got = t.resolve_results()
        if d is not None:
            t.free(d)
    same(got, want)


@pytest.mark.parametrize("max_length", ["known", "unknown"])
def test_device_resident_ragged(max_length):
    n = 40
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    want = capi.resolve_host([buf[s:e + 1] for s, e in zip(st, nd)])
    assert (want["period"] == 6).sum() >= 1
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        if max_length == "unknown":
            b.max_length = 0
        t.resolve(b)
        got, ms = t.resolve_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, want)


def test_pair_mode_context_two_slots_and_errors():
    a, b = fuzz_reads(41, n=250), fuzz_reads(42, n=151)  # an odd number of reads is refused in pair mode
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_resolve"):
            t.resolve_results()
        t.refine(ba)  # a refine call is no resolve call: the buffers are separate
        t.refine_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_resolve"):
            t.resolve_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.resolve(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:150]))
        t.resolve(ba, 1, 32, 3, 24, 3, slot=0)  # the mates are two reads; the two slots overlap
        t.resolve(bb, 2, 12, 7, 5, 4, slot=1)
        same(t.resolve_results(1), capi.resolve_host(b[:150], 2, 12, 7, 5, 4))
        same(t.resolve_results(0), capi.resolve_host(a))
        for lo, hi in ((0, 5), (3, 2), (1, 33)):
            with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
                t.resolve(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.resolve(ba, penalty=penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.resolve(ba, min_score=0)
        for c in (0, 5):
            with pytest.raises(capi.TrewHipError, match="resolve: 1 <= candidates <= 4 is required"):
                t.resolve(ba, candidates=c)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.resolve(ba, slot=3)
        same(t.resolve_results(0), capi.resolve_host(a))  # a refused call leaves the last results in place
        # results larger than the caller's buffer: the count is reported, cap records are copied
        n = C.c_uint64(0)
        three = np.zeros(3, dtype=capi.RESOLVE_DTYPE)
        assert t.lib.trew_hip_resolve_results(t.ctx, 0, three.ctypes.data, 3, C.byref(n), None) == 0
        assert n.value == 250
        same(three, capi.resolve_host(a[:3]))
        assert t.lib.trew_hip_resolve_results(t.ctx, 0, None, 0, C.byref(n), None) == 0 and n.value == 250


def test_convenience_entry_point():
    import trew_amd

    reads = fuzz_reads(77, n=120)
    same(trew_amd.resolve(reads), capi.resolve_host(reads))
    same(trew_amd.resolve(reads, 3, 8, penalty=5, min_score=9, candidates=2), capi.resolve_host(reads, 3, 8, 5, 9, 2))


# ---- independence
def test_scan_and_refine_unchanged_by_resolve_calls_in_between():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]
    want_a, want_b = capi.resolve_host(a), capi.resolve_host(b, 2, 12, 5, 12, 4)

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    with fresh() as t:  # without any resolve call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.refine(ba)
        t.periods(ba)
        alone = (t.refine_results(), t.periods_results())
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # resolve calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.resolve(ba, slot=0)
        t.refine(ba, slot=0)
        t.resolve(bb, 2, 12, 5, 12, 4, slot=1)
        t.periods(ba, slot=0)
        t.submit(bb, slot=1)
        got_1 = t.resolve_results(1)
        got_0 = t.resolve_results(0)
        got = (t.refine_results(0), t.periods_results(0))
        tables = t.collect()
    same(got_0, want_a)
    same(got_1, want_b)
    for x, y in zip(got, alone):
        assert (np.asarray(x) == np.asarray(y)).all()
    same(got[0], capi.refine_host(a), R.FIELDS)
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- the `trew resolve` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_cli_small_generated_file(tmp_path):
    reads = [r.encode() for r in mixed_reads(19, 120) + [SHORT_REPAIRED, SCORE_TIE, T10, ""]]
    path = str(tmp_path / "mixed.fastq")
    write_fastq(path, reads)
    host3 = capi.resolve_host(reads)
    same(host3[-4:], V.resolve([r.decode() for r in reads[-4:]]))  # rows formatted from the reference itself for the last reads
    rows, summary = V.cli_lines(path, reads, host3, 3)
    assert len(rows) - 2 >= 60 and sum(int(line.rsplit(",", 1)[1]) for line in summary[2:]) >= 3  # some reads are repaired
    assert run_cli("resolve", path, "-t", "2") == rows + summary
    assert run_cli("resolve", path, "--candidates", "3", "-t", "4") == rows + summary
    one = V.cli_lines(path, reads, capi.resolve_host(reads, *ARGS, 1), 3)
    assert run_cli("resolve", path, "--candidates", "1") == one[0] + one[1] and all(line.endswith(",0") for line in one[1][2:])
    rows, summary = V.cli_lines(path, reads, capi.resolve_host(reads, 5, 12, 7, 30, 4), 7, min_score=30)
    assert run_cli("resolve", path, "--min_period", "5", "--max_period", "12", "--penalty", "7", "--min_score", "30", "--candidates", "4") == rows + summary
    got = run_cli("resolve", path, path)  # two files: the summary is over both
    assert got.count(">" + os.path.realpath(path)) == 2
    assert got[got.index(">Summary"):] == V.cli_lines(path, reads + reads, np.concatenate([host3] * 2), 3)[1]
