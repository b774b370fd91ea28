"""Units in place with no motif given on the GPU (trew_hip_decompose through ctypes) against the reference of decompose_ref.py,
or, where that is too slow, against trew_decompose_host (which tests/test_decompose_cpu.py checks against the reference).  Every
item of every read of every batch is compared, field for field, and with the items the counts and the records."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import decompose_ref as D
import oracle as O
import period_ref as P
from align_cases import revcomp, with_deletion
from decompose_cases import END_TIE, GPU_KS, ROW_BLOCK, UNITS, block_reads, rotation_reads, shape_reads, small_set
from period_cases import junk, noisy, rep
from refine_cases import TEL, fuzz_set
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 22  # rows (128 MB of workspace): no test batch claims more


def same(got, want):
    """(items, counts, records) of the device against those of a reference"""
    gi, gc, gr = got[:3]
    wi, wc, wr = want[:3]
    assert gr.shape == wr.shape and gc.shape == wc.shape
    for f in wr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert len(bad) == 0, "record %s differs at read %d: got %s, want %s" % (f, bad[0], gr[bad[0]], wr[bad[0]])
    bad = np.flatnonzero(gc != wc)
    assert len(bad) == 0, "counts differ at read %d: got %d, want %d" % (bad[0], gc[bad[0]], wc[bad[0]])
    assert len(gi) == len(wi)
    bad = np.flatnonzero(gi != wi)
    assert len(bad) == 0, "item %d differs: got %s, want %s" % (bad[0], gi[bad[0]], wi[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu(reads, penalty=3, min_score=24, min_period=1, max_period=32, mode=capi.MODE_SHORT, max_items=1 << 20, max_rows=BIG):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.decompose(t.host_batch(words, offsets, lengths), min_period, max_period, penalty, min_score, max_items, max_rows)
        out = t.decompose_results()
    assert out[3] <= max_items and out[4] <= max_rows and out[3] == len(out[0]) == out[1].sum()
    return out


def host(reads, penalty=3, min_score=24, min_period=1, max_period=32):
    return capi.decompose_host(reads, min_period, max_period, penalty, min_score)


def tup(it):
    return tuple(int(v) for v in it)[3:11]


@pytest.fixture(scope="module")
def fuzz():
    """(refine's fuzz set, the host definition at P = 3), computed once"""
    reads = [r for _, r in fuzz_set()]
    return reads, host(reads)


def test_hand_worked_vectors_and_the_end_phase_tie():
    reads = ["A" * 40, "TG" * 30, "GT" * 30, "ACGT" + "A" * 20 + "C" + "A" * 20 + "GT", "AATT" * 12, "CCCTAA" * 10, TEL * 2 + "TTAGG" + "N" + TEL * 8,
             "", "ACGTTGCATGCA", "AAAC" * 5 + "AAAG" * 5 + "AACG" * 5]
    got = gpu(reads)
    same(got, D.decompose(reads))
    assert [tup(it) for it in got[0] if it["read"] == 2] == [(0, 1, 1, 1, 1, 0, 0, 0), (1, 58, 29, 0, 58, 0, 0, 0), (59, 1, 1, 0, 1, 0, 0, 0)]
    assert (got[1][-3:] == 0).all() and (got[2]["reserved"][-3:] == 0).all() and 0 < got[2]["score"][-1] < 24
    read, penalty, min_score, phases = END_TIE
    want = D.decompose([read, read[3:] + "ACGT"], 1, 32, penalty, min_score)
    assert want[1][0] >= 3
    same(gpu([read, read[3:] + "ACGT"], penalty, min_score), want)
    same(host([read], penalty, min_score), D.decompose([read], 1, 32, penalty, min_score))


@pytest.mark.parametrize("k", GPU_KS)
def test_unit_and_read_lengths(k):
    """k x n in {0, 1, k, 2k - 1, 2k, 31, 32, 33, 2047, 2048, 2049} as perfect, shifted, noisy and random reads, and an indel at
    bits 31 and 0 of a word and at the 64-word seam"""
    reads = shape_reads(UNITS[k], k)
    for penalty, min_score in ((1, 5), (3, 24), (64, 3)):
        want = host(reads, penalty, min_score)
        assert (want[1] > 0).sum() >= 25
        same(gpu(reads, penalty, min_score), want)
    # the yardstick itself against the reference, on the short reads (the long ones: tests/test_decompose_cpu.py's fuzz set)
    pick = [r for r in reads if len(r) <= 33]
    same(host(pick, 3, 5), D.decompose(pick, 1, 32, 3, 5))


@pytest.mark.parametrize("k", [2, 6, 17, 32])
def test_every_rotation_offset(k):
    """a perfect repeat begun at each of its k rotations: refine cuts the unit where the read begins, so every anchor 0 .. k - 1
    occurs; M is the same for all, and the first item's phase follows the rotation"""
    reads = rotation_reads(UNITS[k], 20)
    got = gpu(reads)
    same(got, host(reads))
    assert sorted(int(a) for a in got[2]["reserved"]) == list(range(k))
    assert len({capi.decompose_anchor(r) for r in got[2]}) == 1
    first = [int(got[0][got[0]["read"] == q][0]["phase"]) for q in range(k)]
    assert first == [(first[0] + q) % k for q in range(k)]
    same(got, D.decompose(reads))


def test_tracts_around_the_row_block():
    """ROW_BLOCK = 64 rows is what the walk fetches at a time, counted down from the tract's end: tracts of 64 q - 1, 64 q and
    64 q + 1 bases (the last block lacks a row, is full, holds one row), at several places in the read"""
    assert ROW_BLOCK == 64
    for unit in (TEL, UNITS[17], UNITS[2]):
        reads = block_reads(unit)
        want = host(reads, 3, 20)
        lens = {int(r["end"]) - int(r["start"]) for r in want[2]}
        for q in (1, 2, 3):
            assert {64 * q - 1, 64 * q, 64 * q + 1} <= lens
        same(gpu(reads, 3, 20), want)
        same(want, D.decompose(reads, 1, 32, 3, 20))


@pytest.mark.parametrize("k", GPU_KS)
def test_runs_of_deleted_bases(k):
    """d deleted unit bases in a row for every d < k, at P = 1 and 3"""
    unit = UNITS[k]
    base = rep(unit, 40 * k)
    reads = [with_deletion(base, 20 * k + 1, d) for d in range(1, k)] + [base]
    for penalty in (1, 3):
        want = host(reads, penalty)
        assert (want[1] > 0).all()
        same(gpu(reads, penalty), want)
    if 3 <= k <= 6:
        want = D.decompose(reads[:5], penalty=1)
        assert int(want[0][want[0]["read"] == 0]["deletions"].sum()) == 1
        same(host(reads[:5], 1), want)


def test_long_reads():
    """a perfect repeat of 70 000 bases from phase 2: an end piece, one run of 11 666 copies; a 200 000-base noisy read"""
    rnd = random.Random(4)
    perfect = rep(TEL, 70_000, 2)
    got = gpu([perfect], mode=capi.MODE_LONG)
    assert [tup(it) for it in got[0]] == [(0, 4, 1, 2, 4, 0, 0, 0), (4, 69_996, 11_666, 0, 69_996, 0, 0, 0)]
    same(got, host([perfect]))
    noisy_read = (junk(rnd, 3000) + noisy(rnd, TEL, 200_000, 0.01, 0.02) + junk(rnd, 500))[:200_000]
    want = host([noisy_read])
    assert want[3] > 5000 and int(want[2]["end"][0]) - int(want[2]["start"][0]) > 190_000
    same(gpu([noisy_read], mode=capi.MODE_LONG), want)


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_fuzz_sets(fuzz, penalty):
    reads = fuzz[0]
    same(gpu(reads, penalty), fuzz[1] if penalty == 3 else host(reads, penalty))
    small = [r for _, r in small_set()]
    same(gpu(small, penalty), host(small, penalty))


def test_cross_checks_against_trace_and_refine_on_the_gpu(fuzz):
    """the records are trew_hip_refine's in every field but reserved; for k >= 3 the items are the forward-strand items of
    trew_hip_trace with the motif M: the new kernel against the merged ones, on the same device"""
    reads = fuzz[0]
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        t.decompose(b, 1, 32, 3, 24, 1 << 20, BIG)
        items, counts, recs, _, _ = t.decompose_results()
        t.refine(b, 1, 32, 3, 24)
        refined = t.refine_results()
        for f in refined.dtype.names:
            if f != "reserved":
                assert (refined[f] == recs[f]).all(), f
        assert (refined["reserved"] == 0).all() and (recs["reserved"] > 0).sum() > 40
        checked = 0
        for lo in range(0, len(reads), 8):  # eight motifs a trace call: a read against the M of its own, picked out of the batch's
            idx = [i for i in range(lo, min(lo + 8, len(reads))) if counts[i] > 0 and int(recs["period"][i]) >= 3]
            if not idx:
                continue
            motifs = [P.unit_text(capi.decompose_anchor(recs[i]), int(recs["period"][i])) for i in idx]
            sub = [reads[i] for i in idx]
            t.trace(t.host_batch(*capi.pack_reads(sub)), motifs, 3, 24, 1 << 20, BIG)
            tr = t.trace_results()
            for q, i in enumerate(idx):
                theirs = tr[0][(tr[0]["read"] == q) & (tr[0]["motif"] == q) & (tr[0]["strand"] == 0)]
                mine = items[items["read"] == i]
                assert [tup(it) for it in theirs] == [tup(it) for it in mine]
                a = tr[2][q, q]
                assert (int(a["score_fwd"]), int(a["start_fwd"]), int(a["end_fwd"]), int(a["consumed_fwd"]), int(a["matches_fwd"])) == tuple(
                    int(recs[f][i]) for f in ("score", "start", "end", "consumed", "matches"))
                checked += 1
        assert checked >= 80


def test_a_reads_items_do_not_depend_on_the_batch(fuzz):
    reads, want = fuzz
    for r in (0, 17, 50, 92):
        alone = gpu([reads[r]])
        mine = want[0][want[0]["read"] == r].copy()
        mine["read"] = 0
        assert (alone[0] == mine).all() and alone[2][0] == want[2][r]
    # min_score above every score: no items, no rows
    none = gpu(reads, 3, 5000)
    assert none[3] == 0 and none[4] == 0 and none[1].sum() == 0 and (none[2]["reserved"] == 0).all()


def test_overflow_of_the_log_and_of_the_workspace(fuzz):
    """max_items = 1 and max_rows = 1: nothing is copied, the numbers are exact, and the retry with them succeeds; either one
    alone overflows in the same way, also one short of enough"""
    reads = fuzz[0][:30]
    want = host(reads)
    full = gpu(reads)
    same(full, want)
    n_items, n_rows = full[3], full[4]
    assert n_items > 50 and n_rows > 500 and n_rows == int((want[2]["end"] - want[2]["start"])[want[1] > 0].sum())
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        for max_items, max_rows in ((1, 1), (1, BIG), (1 << 20, 1), (n_items - 1, n_rows), (n_items, n_rows - 1)):
            t.decompose(b, 1, 32, 3, 24, max_items, max_rows)
            got = t.decompose_results()
            assert len(got[0]) == 0 and (got[3], got[4]) == (n_items, n_rows)
            assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
            # the raw call: a buffer is left untouched
            buf = np.full(4, 7, dtype=capi.TRACE_DTYPE)
            ni, nr = C.c_uint64(0), C.c_uint64(0)
            assert t.lib.trew_hip_decompose_results(t.ctx, 0, buf.ctypes.data, 4, C.byref(ni), C.byref(nr), None, None, None) == 0
            assert (ni.value, nr.value) == (n_items, n_rows) and (buf["read"] == 7).all()
            t.decompose(b, 1, 32, 3, 24, got[3], got[4])  # the retry: exactly what was reported
            same(t.decompose_results(), want)
        # cap below the number of items: the first ones of the sorted order
        buf = np.zeros(5, dtype=capi.TRACE_DTYPE)
        ni, nr = C.c_uint64(0), C.c_uint64(0)
        assert t.lib.trew_hip_decompose_results(t.ctx, 0, buf.ctypes.data, 5, C.byref(ni), C.byref(nr), None, None, None) == 0
        assert ni.value == n_items and (buf == want[0][:5]).all()
    # the refused workspace on the tracts around the row block: the walk fills every block by computing the rows again
    for unit in (TEL, UNITS[17], UNITS[2]):
        reads = block_reads(unit)
        want = host(reads, 3, 20)
        n_rows = int((want[2]["end"].astype(np.int64) - want[2]["start"])[want[1] > 0].sum())  # the definition's: a traced read's tract
        assert (want[1] > 0).sum() >= 9 and n_rows > 1
        words, offsets, lengths = capi.pack_reads(reads)
        with ctx(words=len(words) + 64, reads=len(reads)) as t:
            b = t.host_batch(words, offsets, lengths)
            t.decompose(b, 1, 32, 3, 20, 1 << 20, 1)
            got = t.decompose_results()
            assert len(got[0]) == 0 and (got[3], got[4]) == (want[3], n_rows)
            assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
            t.decompose(b, 1, 32, 3, 20, got[3], got[4])
            same(t.decompose_results(), want)


def long_reads(n):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def noisy_tail_reads(n=40, seed=8):
    """generator long reads, cut to at most 6 kb, with a planted (TTAGGG)n tail (or, reverse-complemented, head) of 0.3 - 2 kb
    that carries substitutions and indels"""
    rnd = random.Random(seed)
    out = []
    for i, r in enumerate(long_reads(n)):
        body = r.decode()[:rnd.randint(500, 6000)]
        s = body + noisy(rnd, TEL, rnd.randint(300, 2000), 0.03, 0.06, 0.002)
        out.append((revcomp(s.upper().replace("R", "N")) if i % 4 == 3 else s).encode())
    return out


@pytest.fixture(scope="module")
def tails():
    reads = noisy_tail_reads()
    want = host(reads)
    assert (want[1] >= 10).sum() >= len(reads) // 2  # the planted tails are found and cut into units
    return reads, want


def test_generator_long_reads_every_batch_shape(tails):
    reads, want = tails
    same(gpu(reads, mode=capi.MODE_LONG), want)
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=64) as t:
        t.decompose(t.host_batch(words, offsets, lengths, contiguous=True), 1, 32, 3, 24, 1 << 20, BIG)
        same(t.decompose_results(), want)
    # device-resident generator reads, the longest read unknown
    full = long_reads(60)
    with ctx(mode=capi.MODE_LONG, reads=64, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, 60)
        b.max_length = 0
        t.decompose(b, 1, 32, 3, 24, 1 << 20, BIG)
        got = t.decompose_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert got[5] > 0
    want = host(full)
    assert want[3] > 0
    same(got, want)


def test_uniform_short_reads():
    n, L = 4000, 150
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = host(reads)
    assert (want[1] > 0).sum() >= 20
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.decompose(t.device_uniform_batch(d, n, L), 1, 32, 3, 24, 1 << 20, BIG)
        got = t.decompose_results()
        t.free(d)
    same(got, want)
    words, offsets, lengths = capi.pack_reads(reads)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    with ctx() as t:
        b = capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0)
        t.decompose(b, 1, 32, 3, 24, 1 << 20, BIG)
        same(t.decompose_results(), want)


def test_pair_mode_two_slots_repeated_calls_and_errors():
    rnd = random.Random(6)
    a = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, TEL, rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(100)]
    b = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, "CCCTA", rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(61)]
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_decompose"):
            t.decompose_results()
        t.refine(ba)  # a refine call is no decompose call: the buffers are separate
        t.refine_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_decompose"):
            t.decompose_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.decompose(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:60]))
        t.decompose(ba, 1, 32, 3, 24, 1 << 16, 1 << 18, slot=0)  # the mates are two reads; the two slots overlap
        t.decompose(bb, 2, 9, 7, 10, 1 << 16, 1 << 18, slot=1)
        got1, got0 = t.decompose_results(1), t.decompose_results(0)
        same(got1, host(b[:60], 7, 10, 2, 9))
        same(got0, host(a))
        assert got0[3] > 100 and got1[3] > 50
        # repeated calls on one slot: fewer reads, another penalty; the last call is what results returns
        t.decompose(bb, 1, 32, 1, 24, 1 << 16, 1 << 18, slot=0)
        t.decompose(ba, 1, 16, 2, 30, 1 << 16, 1 << 18, slot=0)
        same(t.decompose_results(0), host(a, 2, 30, 1, 16))
        same(t.decompose_results(0), host(a, 2, 30, 1, 16))  # fetching twice changes nothing
        for lo, hi in ((0, 32), (1, 33), (7, 6)):
            with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
                t.decompose(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.decompose(ba, 1, 32, penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.decompose(ba, 1, 32, 3, 0)
        with pytest.raises(capi.TrewHipError, match="max_items must be at least 1"):
            t.decompose(ba, 1, 32, 3, 24, 0, 10)
        with pytest.raises(capi.TrewHipError, match="max_rows must be at least 1"):
            t.decompose(ba, 1, 32, 3, 24, 10, 0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.decompose(ba, slot=3)
        ni = C.c_uint64(0)
        assert t.lib.trew_hip_decompose_results(t.ctx, 0, None, 0, C.byref(ni), None, None, None, None) != 0
        assert b"n_items and n_rows must not be null" in t.lib.trew_hip_last_error(t.ctx)
        assert t.lib.trew_hip_decompose_results(t.ctx, 0, None, 3, C.byref(ni), C.byref(ni), None, None, None) != 0
        assert b"items must not be null" in t.lib.trew_hip_last_error(t.ctx)
        # no reads: no items, no rows, no kernel
        t.decompose(t.host_batch(*capi.pack_reads([])))
        got = t.decompose_results()
        assert len(got[0]) == 0 and got[1].shape == (0,) and got[2].shape == (0,) and got[3:] == (0, 0)


def test_scan_refine_and_trace_unchanged_by_decompose_calls_in_between():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]
    want_a, want_b = host(a), host(b, 5, 30)

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    with fresh() as t:  # without any decompose call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.refine(ba)
        alone = t.refine_results()
        t.trace(ba, [TEL], 3, 24, 1 << 18, 1 << 20)
        alone_trace = t.trace_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # decompose calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.decompose(ba, 1, 32, 3, 24, 1 << 18, 1 << 20, slot=0)
        t.refine(ba, slot=0)
        t.trace(ba, [TEL], 3, 24, 1 << 18, 1 << 20, slot=0)
        t.decompose(bb, 1, 32, 5, 30, 1 << 18, 1 << 20, slot=1)
        t.submit(bb, slot=1)
        got_1 = t.decompose_results(1)
        got_0 = t.decompose_results(0)
        got = t.refine_results(0)
        got_trace = t.trace_results(0)
        tables = t.collect()
    same(got_0, want_a)
    same(got_1, want_b)
    assert (got == alone).all()
    same(got_trace, alone_trace)
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_convenience_entry_point_retries_inside(fuzz):
    import trew_amd

    reads = fuzz[0][:24]
    want = host(reads)
    same(trew_amd.decompose(reads), want)  # the defaults: periods 1 .. 32, penalty 3, min_score 24
    same(trew_amd.decompose(reads, max_items=1, max_rows=1), want)
    same(trew_amd.decompose(reads, penalty=7, min_score=40), host(reads, 7, 40))


# ---- the `trew decompose` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args, env=None):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


def test_cli_planted_noisy_tails(tmp_path, tails):
    reads, host3 = tails
    path = str(tmp_path / "tails.fastq")
    write_fastq(path, reads)
    # rows formatted from the reference itself for the shortest reads, from the host definition (equal to it) for all
    few = sorted(reads, key=len)[:4]
    same(host(few), D.decompose(few))
    rows, tail = D.cli_lines(path, reads, host3, 3)
    assert len(rows) - 2 >= len(reads) - 2 and len(tail) >= 3
    assert any(" =" in ln and any(c in ln.split(",")[-1] for c in "ACGT") and any(c in ln.split(",")[-1] for c in "acgt") for ln in rows)
    assert {ln.split(",")[-4] for ln in rows[2:]} == {"+", "-"}  # the reverse-complemented reads are cut at the other strand's rotation
    assert run_cli("decompose", path, "-t", "2")[0] == rows + tail
    assert run_cli("decompose", path, "-t", "5")[0] == rows + tail
    irows, itail = D.cli_lines(path, reads, host3, 3, per_item=True)
    assert itail == tail and run_cli("decompose", path, "-t", "3", "--items")[0] == irows + itail
    other = host(reads, 7, 60, 3, 12)
    rows2, tail2 = D.cli_lines(path, reads, other, 7, min_score=60)
    assert 5 <= len(rows2) - 2 <= 30
    assert run_cli("decompose", path, "--penalty", "7", "--min_score", "60", "--min_period", "3", "--max_period", "12", "-t", "3")[0] == rows2 + tail2
    # the file is one batch, whose items outnumber the log's first size (sixteen per read): it is resubmitted once with the exact
    # numbers, which --stats counts
    assert host3[3] > 16 * len(reads)
    out, err = run_cli("decompose", path, "-t", "2", "--stats")
    assert out == rows + tail
    assert "%d items, 1 batch(es) resubmitted with a larger log" % host3[3] in err
