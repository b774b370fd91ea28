"""Units in place under indels on the GPU (trew_hip_trace through ctypes) against the reference of trace_ref.py, or, where that
is too slow, against trew_trace_host (which tests/test_trace_cpu.py checks against the reference).  Every item of every read
of every batch is compared, field for field, and with the items the counts and the alignment records."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import trace_ref as T
from align_cases import GPU_KS, TEL, UNITS, fuzz_sets, revcomp, with_deletion
from period_cases import junk, noisy, rep
from trace_cases import HAND, ROW_BLOCK, block_reads, shape_reads, two_strand_reads
from trew_amd import capi

pytestmark = pytest.mark.gpu
assert tuple(capi.TRACE_DTYPE.names) == T.ITEM_FIELDS  # the reference and the record name their fields alike, in the same order
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 22  # rows (256 MB of workspace): no test batch claims more


def same(got, want):
    """(items, counts, records) of the device against those of a reference"""
    gi, gc, gr = got[:3]
    wi, wc, wr = want[:3]
    assert gr.shape == wr.shape and gc.shape == wc.shape
    for f in wr.dtype.names:
        bad = np.argwhere(gr[f] != wr[f])
        assert len(bad) == 0, "record %s differs at (read, motif) %s: got %s, want %s" % (f, bad[0].tolist(), gr[tuple(bad[0])], wr[tuple(bad[0])])
    bad = np.argwhere(gc != wc)
    assert len(bad) == 0, "counts differ at (read, motif, strand) %s: got %d, want %d" % (bad[0].tolist(), gc[tuple(bad[0])], wc[tuple(bad[0])])
    assert len(gi) == len(wi)
    bad = np.flatnonzero(gi != wi)
    assert len(bad) == 0, "item %d differs: got %s, want %s" % (bad[0], gi[bad[0]], wi[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_trace(reads, motifs, penalty=3, min_score=24, mode=capi.MODE_SHORT, max_items=1 << 20, max_rows=BIG):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.trace(t.host_batch(words, offsets, lengths), motifs, penalty, min_score, max_items, max_rows)
        out = t.trace_results()
    assert out[3] <= max_items and out[4] <= max_rows and out[3] == len(out[0]) == out[1].sum()
    return out


def host(reads, motifs, penalty=3, min_score=24):
    return capi.trace_host(reads, motifs, penalty, min_score)


def test_hand_worked_vectors():
    for read, motif, penalty, min_score, strand, items in HAND:
        got, counts, records, n_items, n_rows = gpu_trace([read.encode()], [motif], penalty, min_score)
        mine = [tuple(int(x) for x in it)[3:11] for it in got if it["strand"] == strand]
        assert mine == items and counts[0, 0, strand] == len(items)
        same((got, counts, records), T.trace([read], [motif], penalty, min_score))


def test_end_phase_tie():
    """(AAT)x10 against AATAAT: the phases 2 and 5 hold equal cells in the end row, the smaller one wins"""
    got = gpu_trace(["AAT" * 10, "ACGT" + "AAT" * 30 + "C"], ["AATAAT"], 3, 24)
    assert [tuple(int(x) for x in it)[3:11] for it in got[0] if it["read"] == 0 and it["strand"] == 0] == [
        (0, 3, 1, 3, 3, 0, 0, 0), (3, 24, 4, 0, 24, 0, 0, 0), (27, 3, 1, 0, 3, 0, 0, 0)]
    same(got, T.trace(["AAT" * 10, "ACGT" + "AAT" * 30 + "C"], ["AATAAT"], 3, 24))


@pytest.mark.parametrize("k", GPU_KS)
def test_motif_and_read_lengths(k):
    unit = UNITS[k]
    reads = shape_reads(unit, k)
    for penalty, min_score in ((1, 5), (3, 24), (64, 3)):
        want = host(reads, [unit], penalty, min_score)
        assert want[3] >= 40
        same(gpu_trace(reads, [unit], penalty, min_score), want)
    # the yardstick itself against the reference, on the short reads and on the two longest kinds
    pick = [r for r in reads if len(r) <= 33] + reads[-18:-12]
    same(host(pick, [unit], 3, 5), T.trace(pick, [unit], 3, 5))


def test_tracts_around_the_row_block():
    """ROW_BLOCK = 64 rows is what the walk fetches at a time, counted down from the tract's end: tracts of 64 q - 1, 64 q and
    64 q + 1 bases (the last block lacks a row, is full, holds one row), at several places in the read and on both strands"""
    assert ROW_BLOCK == 64
    for unit in (TEL, UNITS[17]):
        reads = block_reads(unit)
        want = T.trace(reads, [unit], 3, 24)
        lens = sorted({int(r["end_fwd"]) - int(r["start_fwd"]) for r in want[2][:, 0]} | {int(r["end_rev"]) - int(r["start_rev"]) for r in want[2][:, 0]})
        for q in (1, 2, 3):
            assert {64 * q - 1, 64 * q, 64 * q + 1} <= set(lens)
        same(gpu_trace(reads, [unit], 3, 24), want)
        same(host(reads, [unit], 3, 24), want)


@pytest.mark.parametrize("k", GPU_KS)
def test_runs_of_deleted_bases(k):
    """d deleted motif bases in a row for every d < k, at P = 1 (where d < 2 (k - d) of them are d deletions, in one copy or
    across the seam of two) and 3"""
    unit = UNITS[k]
    base = rep(unit, 40 * k)
    reads = [with_deletion(base, 20 * k + 1, d) for d in range(1, k)]
    want = T.trace(reads, [unit], 1, 24)
    for d in range(1, k):
        if 3 * d < 2 * k:
            mine = want[0][(want[0]["read"] == d - 1) & (want[0]["strand"] == 0)]
            assert int(mine["deletions"].sum()) == d and int(mine["insertions"].sum()) == 0 and 3 <= len(mine) <= 4
    same(gpu_trace(reads, [unit], 1, 24), want)
    same(gpu_trace(reads, [unit], 3, 24), host(reads, [unit], 3, 24))


def test_long_reads():
    """a perfect repeat of 70 000 bases from phase 2: an end piece, one run of 11 666 copies and no more than one end piece; a
    200 000-base noisy read"""
    rnd = random.Random(4)
    perfect = rep(TEL, 70_000, 2)
    got = gpu_trace([perfect], [TEL], 3, 24, mode=capi.MODE_LONG)
    fwd = [tuple(int(x) for x in it)[3:11] for it in got[0] if it["strand"] == 0]
    assert fwd == [(0, 4, 1, 2, 4, 0, 0, 0), (4, 69_996, 11_666, 0, 69_996, 0, 0, 0)]
    same(got, host([perfect], [TEL], 3, 24))
    noisy_read = (junk(rnd, 3000) + noisy(rnd, TEL, 200_000, 0.01, 0.02) + junk(rnd, 500))[:200_000]
    want = host([noisy_read], [TEL], 3, 24)
    assert want[3] > 5000 and int(want[2]["end_fwd"][0, 0]) - int(want[2]["start_fwd"][0, 0]) > 190_000
    same(gpu_trace([noisy_read], [TEL], 3, 24, mode=capi.MODE_LONG), want)


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_fuzz_sets(penalty):
    for unit, reads in fuzz_sets():
        same(gpu_trace(reads, [unit], penalty, 24), host(reads, [unit], penalty, 24))


def test_eight_motifs_at_once():
    rnd = random.Random(2025)
    motifs = [UNITS[k] for k in GPU_KS]
    reads = []
    for i in range(48):
        unit = motifs[i % 8] if i % 3 else revcomp(motifs[i % 8])
        reads.append(junk(rnd, rnd.randint(0, 100), "ACGTACGTACGTN") + noisy(rnd, unit, rnd.randint(100, 500), 0.03, 0.06, 0.003) + junk(rnd, rnd.randint(0, 100)))
    for penalty in (1, 3):
        want = host(reads, motifs, penalty, 24)
        assert all(want[1][:, mi].sum() > 0 for mi in range(8))
        same(gpu_trace(reads, motifs, penalty, 24), want)
    few = sorted(reads, key=len)[:3]
    same(host(few, motifs, 3, 24), T.trace(few, motifs, 3, 24))


def test_both_strands_one_strand_and_none():
    reads = two_strand_reads()
    want = T.trace(reads, [TEL], 3, 24)
    both = (want[1][:, 0, 0] > 0) & (want[1][:, 0, 1] > 0)
    one = (want[1][:, 0, 0] > 0) ^ (want[1][:, 0, 1] > 0)
    assert both.sum() >= 4 and one.sum() >= 2
    for r in np.flatnonzero(both):  # different ranges: the rows of the two strands share the workspace rows of their overlap only
        rec = want[2][r, 0]
        assert (int(rec["start_fwd"]), int(rec["end_fwd"])) != (int(rec["start_rev"]), int(rec["end_rev"]))
    got = gpu_trace(reads, [TEL], 3, 24)
    same(got, want)
    assert 0 < got[4] <= sum(len(r) for r in reads)
    # a key's items do not depend on the rest of the batch
    for r in (0, 2, 5):
        alone = gpu_trace([reads[r]], [TEL], 3, 24)
        mine = got[0][got[0]["read"] == r].copy()
        mine["read"] = 0
        assert (alone[0] == mine).all()
    # min_score above every score: no items, no rows, the records as ever
    top = int(max(want[2]["score_fwd"].max(), want[2]["score_rev"].max()))
    none = gpu_trace(reads, [TEL], 3, top + 1)
    assert none[3] == 0 and none[4] == 0 and len(none[0]) == 0 and none[1].sum() == 0
    for f in want[2].dtype.names:
        assert (none[2][f] == want[2][f]).all()
    exactly = gpu_trace(reads, [TEL], 3, top)
    assert exactly[3] > 0 and (exactly[1] > 0).sum() == 1


def test_overflow_of_the_log_and_of_the_workspace():
    """max_items = 1 and max_rows = 1: nothing is copied, the numbers are exact, and the retry with them succeeds; either one
    alone overflows in the same way"""
    reads = [r for _, rs in fuzz_sets()[3:9] for r in rs] + two_strand_reads(3, 6)
    motifs = [TEL, fuzz_sets()[3][0]]
    want = host(reads, motifs, 3, 24)
    full = gpu_trace(reads, motifs, 3, 24)
    same(full, want)
    n_items, n_rows = full[3], full[4]
    assert n_items > 50 and n_rows > 500
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        for max_items, max_rows in ((1, 1), (1, BIG), (1 << 20, 1), (n_items - 1, n_rows), (n_items, n_rows - 1)):
            t.trace(b, motifs, 3, 24, max_items, max_rows)
            got = t.trace_results()
            assert len(got[0]) == 0 and (got[3], got[4]) == (n_items, n_rows)
            assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
            # the raw call: a buffer is left untouched
            buf = np.full(4, 7, dtype=capi.TRACE_DTYPE)
            ni, nr = C.c_uint64(0), C.c_uint64(0)
            assert t.lib.trew_hip_trace_results(t.ctx, 0, buf.ctypes.data, 4, C.byref(ni), C.byref(nr), None, None, None) == 0
            assert (ni.value, nr.value) == (n_items, n_rows) and (buf["read"] == 7).all()
            t.trace(b, motifs, 3, 24, got[3], got[4])  # the retry: exactly what was reported
            same(t.trace_results(), want)
        # cap below the number of items: the first ones of the sorted order
        buf = np.zeros(5, dtype=capi.TRACE_DTYPE)
        ni, nr = C.c_uint64(0), C.c_uint64(0)
        assert t.lib.trew_hip_trace_results(t.ctx, 0, buf.ctypes.data, 5, C.byref(ni), C.byref(nr), None, None, None) == 0
        assert ni.value == n_items and (buf == want[0][:5]).all()
    # the refused workspace on the tracts around the row block: the walk fills every block by computing the rows again
    for unit in (TEL, UNITS[17]):
        reads = block_reads(unit)
        want = host(reads, [unit], 3, 24)
        a = want[2].astype([(f, "<i8") for f in capi.ALIGN_DTYPE.names])
        fwd, rev = a["score_fwd"] >= 24, a["score_rev"] >= 24
        lo = np.minimum(np.where(fwd, a["start_fwd"], 1 << 40), np.where(rev, a["start_rev"], 1 << 40))
        hi = np.maximum(np.where(fwd, a["end_fwd"], 0), np.where(rev, a["end_rev"], 0))
        n_rows = int((hi - lo)[fwd | rev].sum())  # the definition's: from the first start to the last end of the traced strands
        assert (want[1][:, 0, 0] > 0).any() and (want[1][:, 0, 1] > 0).any() and n_rows > 1
        words, offsets, lengths = capi.pack_reads(reads)
        with ctx(words=len(words) + 64, reads=len(reads)) as t:
            b = t.host_batch(words, offsets, lengths)
            t.trace(b, [unit], 3, 24, 1 << 20, 1)
            got = t.trace_results()
            assert len(got[0]) == 0 and (got[3], got[4]) == (want[3], n_rows)
            assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
            t.trace(b, [unit], 3, 24, got[3], got[4])
            same(t.trace_results(), want)


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
    want = host(reads, [TEL], 3, 24)
    assert ((want[1][:, 0, 0] >= 10) | (want[1][:, 0, 1] >= 10)).sum() >= len(reads) // 2  # the planted tails are found and cut into units
    return reads, want


def test_generator_long_reads_every_batch_shape(tails):
    reads, want = tails
    same(gpu_trace(reads, [TEL], 3, 24, mode=capi.MODE_LONG), want)
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=64) as t:
        t.trace(t.host_batch(words, offsets, lengths, contiguous=True), [TEL], 3, 24, 1 << 20, BIG)
        same(t.trace_results(), want)
    # device-resident generator reads, the longest read unknown
    full = long_reads(60)
    with ctx(mode=capi.MODE_LONG, reads=64, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, 60)
        b.max_length = 0
        t.trace(b, [TEL], 3, 24, 1 << 20, BIG)
        got = t.trace_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert got[5] > 0
    want = host(full, [TEL], 3, 24)
    assert want[3] > 0
    same(got, want)


def test_uniform_short_reads():
    n, L = 4000, 150
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = host(reads, [TEL], 3, 24)
    assert (want[1][:, 0, 0] > 0).sum() >= 10 and (want[1][:, 0, 1] > 0).sum() >= 10
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.trace(t.device_uniform_batch(d, n, L), [TEL], 3, 24, 1 << 20, BIG)
        got = t.trace_results()
        t.free(d)
    same(got, want)
    words, offsets, lengths = capi.pack_reads(reads)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    with ctx() as t:
        b = capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0)
        t.trace(b, [TEL], 3, 24, 1 << 20, BIG)
        same(t.trace_results(), want)


def test_pair_mode_two_slots_repeated_calls_and_errors():
    rnd = random.Random(6)
    a = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, TEL, rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(100)]
    b = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, "CCCTA", rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(61)]
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_trace"):
            t.trace_results()
        t.align(ba, [TEL], 3)  # an align call is no trace call: the buffers are separate
        t.align_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_trace"):
            t.trace_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.trace(t.host_batch(*capi.pack_reads(b)), [TEL])
        bb = t.host_batch(*capi.pack_reads(b[:60]))
        t.trace(ba, [TEL, "CCCTA"], 3, 24, 1 << 16, 1 << 18, slot=0)  # the mates are two reads; the two slots overlap
        t.trace(bb, ["CCCTA"], 7, 10, 1 << 16, 1 << 18, slot=1)
        got1, got0 = t.trace_results(1), t.trace_results(0)
        same(got1, host(b[:60], ["CCCTA"], 7, 10))
        same(got0, host(a, [TEL, "CCCTA"], 3, 24))
        assert got0[3] > 100 and got1[3] > 100
        # repeated calls on one slot: more motifs, fewer reads, another penalty; the last call is what results returns
        t.trace(bb, ["CCCTA", TEL, "AAT"], 1, 24, 1 << 16, 1 << 18, slot=0)
        t.trace(ba, ["AAT", TEL], 2, 30, 1 << 16, 1 << 18, slot=0)
        same(t.trace_results(0), host(a, ["AAT", TEL], 2, 30))
        same(t.trace_results(0), host(a, ["AAT", TEL], 2, 30))  # fetching twice changes nothing
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.trace(ba, [TEL], penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.trace(ba, [TEL], 3, 0)
        with pytest.raises(capi.TrewHipError, match="max_items must be at least 1"):
            t.trace(ba, [TEL], 3, 24, 0, 10)
        with pytest.raises(capi.TrewHipError, match="max_rows must be at least 1"):
            t.trace(ba, [TEL], 3, 24, 10, 0)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.trace(ba, ["AAT"] * 9)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.trace(ba, [])
        with pytest.raises(capi.TrewHipError, match=r"k must be in \[3, 32\]"):
            t.trace(ba, [capi.Motif(2, 0, 5)])
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.trace(ba, [TEL], slot=3)
        ni = C.c_uint64(0)
        assert t.lib.trew_hip_trace_results(t.ctx, 0, None, 0, C.byref(ni), None, None, None, None) != 0
        assert b"n_items and n_rows must not be null" in t.lib.trew_hip_last_error(t.ctx)
        assert t.lib.trew_hip_trace_results(t.ctx, 0, None, 3, C.byref(ni), C.byref(ni), None, None, None) != 0
        assert b"items must not be null" in t.lib.trew_hip_last_error(t.ctx)
        # no reads: no items, no rows, no kernel
        t.trace(t.host_batch(*capi.pack_reads([])), [TEL], 3)
        got = t.trace_results()
        assert len(got[0]) == 0 and got[1].shape == (0, 1, 2) and got[2].shape == (0, 1) and got[3:] == (0, 0)


def test_scan_and_align_unchanged_by_trace_calls_in_between():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = host(a, motifs, 3, 24), host(b, [TEL], 5, 30)

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    with fresh() as t:  # without any trace call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.align(ba, motifs, 3)
        alone = t.align_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # trace calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.trace(ba, motifs, 3, 24, 1 << 18, 1 << 20, slot=0)
        t.align(ba, motifs, 3, slot=0)
        t.trace(bb, [TEL], 5, 30, 1 << 18, 1 << 20, slot=1)
        t.submit(bb, slot=1)
        got_1 = t.trace_results(1)
        got_0 = t.trace_results(0)
        got = t.align_results(0)
        tables = t.collect()
    same(got_0, want_a)
    same(got_1, want_b)
    assert (got == alone).all() and (got == got_0[2]).all()  # and trace's records are align's, field for field
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_convenience_entry_point_retries_inside():
    import trew_amd

    unit, reads = fuzz_sets()[3]
    want = host(reads, [unit], 3, 24)
    same(trew_amd.trace(reads, [unit]), want)  # the defaults: penalty 3, min_score 24
    same(trew_amd.trace(reads, [unit], max_items=1, max_rows=1), want)
    same(trew_amd.trace(reads, [unit], penalty=7, min_score=40), host(reads, [unit], 7, 40))


# ---- the `trew trace` subcommand, end to end
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
    # rows formatted from the reference itself for the first reads, from the host definition (equal to it) for all
    same(host(reads[:4], [TEL], 3, 24), T.trace(reads[:4], [TEL], 3, 24))
    want = T.cli_lines(path, reads, [TEL], host3, 3)
    assert len(want) - 6 >= len(reads)  # every read has its planted tract
    assert any(" =" in ln and any(c in ln.split(",")[-1] for c in "ACGT") and any(c in ln.split(",")[-1] for c in "acgt") for ln in want)
    assert run_cli("trace", TEL, path, "-t", "2")[0] == want
    assert run_cli("trace", TEL, path, "-t", "5")[0] == want
    assert run_cli("trace", TEL, path, "-t", "3", "--items")[0] == T.cli_lines(path, reads, [TEL], host3, 3, per_item=True)
    motifs = [TEL, "AAT"]
    traced = host(reads, motifs, 7, 200)
    want = T.cli_lines(path, reads, motifs, traced, 7, min_score=200)
    assert 10 <= len(want) - 8 <= 60
    assert run_cli("trace", ",".join(motifs), path, "--penalty", "7", "--min_score", "200", "-t", "3")[0] == want
    # the file is one batch, whose items outnumber the log's first size (sixteen per read and motif and 1024): it is resubmitted
    # once with the exact numbers, which --stats counts
    assert host3[3] > 16 * len(reads) + 1024
    out, err = run_cli("trace", TEL, path, "-t", "2", "--stats")
    assert out == T.cli_lines(path, reads, [TEL], host3, 3)
    assert "%d items, 1 batch(es) resubmitted with a larger log" % host3[3] in err
