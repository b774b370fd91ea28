"""Units in place for every tract of a read, no motif given, on the GPU (trew_hip_dissect through ctypes) against
trew_dissect_host, which tests/test_dissect_cpu.py checks against the reference of dissect_ref.py on the same case sets, and on
the short reads against that reference itself.  Every record, count and item of every read of every batch is compared, field
for field; the new kernel is also held against the merged ones (tandems, decompose) on the same device."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import dissect_cases as DC
import dissect_ref as X
import oracle as O
from period_cases import junk, noisy
from refine_cases import TEL
from repeat_cases import stack_reads
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 22  # rows (128 MB of workspace): no test batch claims more
PARAMS = ((1, 5), (3, 24), (64, 3))  # (penalty, min_score), those of tests/test_gpu_decompose.py


def same(got, want):
    """(records, items, counts, n_records, n_items, n_rows) of the device against those of the host definition, or against
    dissect_ref.dissect's (records, items, counts, rows)"""
    gr, gi, gc = got[:3]
    wr, wi, wc = want[:3]
    assert len(gr) == len(wr), "%d records, want %d" % (len(gr), len(wr))
    for f in wr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert len(bad) == 0, "record field %s differs at %d: got %s, want %s" % (f, bad[0], gr[bad[0]], wr[bad[0]])
    assert gc.shape == wc.shape
    bad = np.flatnonzero((gc != wc).any(axis=1))
    assert len(bad) == 0, "counts differ at read %d: got %s, want %s" % (bad[0], gc[bad[0]], wc[bad[0]])
    assert len(gi) == len(wi), "%d items, want %d" % (len(gi), len(wi))
    bad = np.flatnonzero(gi != wi)
    assert len(bad) == 0, "item %d differs: got %s, want %s" % (bad[0], gi[bad[0]], wi[bad[0]])
    assert got[5] == want[-1] and got[3] == len(wr) and got[4] == len(wi)


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu(reads, penalty=3, min_score=24, min_period=1, max_period=32, mode=capi.MODE_SHORT, max_records=1 << 16, max_items=1 << 20, max_rows=BIG,
        candidates=1):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.dissect(t.host_batch(words, offsets, lengths), min_period, max_period, penalty, min_score, max_records, max_items, max_rows,
                  candidates=candidates)
        out = t.dissect_results()
    assert out[3] <= max_records and out[4] <= max_items and out[5] <= max_rows
    assert out[3] == len(out[0]) == out[2][:, 0].sum() and out[4] == len(out[1]) == out[2][:, 1].sum()
    return out


def host(reads, penalty=3, min_score=24, min_period=1, max_period=32, candidates=1):
    return capi.dissect_host(reads, min_period, max_period, penalty, min_score, candidates=candidates)


@pytest.fixture(scope="module")
def two_tract():
    """(the two-tract reads, the host definition at the defaults), computed once"""
    reads = [r for r, _ in DC.two_tract_set()]
    want = host(reads)
    assert want[3] == 60 and want[5] == 29359
    return reads, want


def test_hand_vectors_short_units_three_tracts_and_the_end_phase_tie_in_a_child():
    reads = DC.HAND_READS + DC.short_unit_reads() + DC.three_tract_reads()
    for penalty, min_score in PARAMS:
        want = host(reads, penalty, min_score)
        same(gpu(reads, penalty, min_score), want)
        same(want, X.dissect(reads, 1, 32, penalty, min_score))  # the yardstick itself against the reference
    got = gpu(reads)
    weak_first = 2  # its only record is at depth 1, below a piece with no record and no rows
    assert [int(d) for d in got[0]["depth"][got[0]["read"] == weak_first]] == [1] and tuple(got[2][1]) == (0, 0) and tuple(got[2][4]) == (0, 0)
    n_hand, n_short = len(DC.HAND_READS), len(DC.short_unit_reads())
    assert sorted(int(p) for p in got[0]["period"][(got[0]["read"] >= n_hand) & (got[0]["read"] < n_hand + n_short)]).count(1) >= 2
    assert (got[2][n_hand + n_short:, 0] == 3).all()  # three tracts: the stack holds an entry while a trace runs
    read, penalty, min_score, phases, _ = DC.end_tie_child()
    want = X.dissect([read, read[3:] + "ACGT"], 1, 32, penalty, min_score)
    assert want[2][0, 0] == 2
    same(gpu([read, read[3:] + "ACGT"], penalty, min_score), want)


@pytest.mark.parametrize("k", DC.GPU_KS)
def test_a_traced_tract_in_a_child_piece_at_word_and_seam_bounds(k):
    """lo or hi of the child piece at bit 31, 0 and 1 of a word and either side of the 64-word seam: the row table restarts at a
    start that is not the read's, and the items come out in read coordinates"""
    b_reads, b_want = DC.piece_bound_reads(k)
    h_reads, h_want = DC.piece_hi_reads(k)
    reads = b_reads + h_reads
    for penalty, min_score in PARAMS:
        want = host(reads, penalty, min_score)
        same(gpu(reads, penalty, min_score), want)
    want = host(reads)
    recs, items = want[0], want[1]
    for i, (lo, at_start) in enumerate(b_want):  # the child's tract starts at lo or ends at n, and has items
        mine = recs[(recs["read"] == i) & (recs["depth"] == 1)]
        assert len(mine) == 1 and (mine["start"][0] == lo if at_start else mine["end"][0] == len(reads[i]))
        its = items[(items["read"] == i) & (items["motif"] == 1)]
        assert len(its) and its["start"][0] == mine["start"][0] and its["start"][-1] + its["bases"][-1] == mine["end"][0]
    for q, (lo, hi, shape) in enumerate(h_want):
        i = len(b_reads) + q
        assert ((recs["read"] == i) & (recs["end"] == hi)).sum() == 1
    pick = [r for r in reads if len(r) < 700][:6]
    same(host(pick), X.dissect(pick))


def test_child_tracts_around_the_row_block():
    """child tracts of 64 q - 1, 64 q and 64 q + 1 bases behind a depth-0 tract of 200 bases of AATGG, and the refused
    workspace (max_rows = 1) on the same reads: the walk fills every block by computing the rows again"""
    reads = DC.child_block_reads()
    want = host(reads, 3, 20)
    child = want[0][want[0]["depth"] == 1]
    lens = {int(r["end"]) - int(r["start"]) for r in child}
    for q in (1, 2, 3):
        assert {64 * q - 1, 64 * q, 64 * q + 1} <= lens
    assert (want[0]["start"][want[0]["depth"] == 0] == 0).all() and len(child) >= len(reads) - 20
    same(gpu(reads, 3, 20), want)
    same(want, X.dissect(reads, 1, 32, 3, 20))
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        t.dissect(b, 1, 32, 3, 20, 1 << 16, 1 << 20, 1)
        got = t.dissect_results()
        assert len(got[0]) == 0 and len(got[1]) == 0 and got[3:] == (want[3], want[4], want[5]) and (got[2] == want[2]).all()
        t.dissect(b, 1, 32, 3, 20, got[3], got[4], got[5])
        same(t.dissect_results(), want)


def test_two_tract_set_and_cross_checks_against_tandems_and_decompose_on_the_gpu(two_tract):
    """the records equal trew_hip_tandems' but for reserved; the depth-0 items equal trew_hip_decompose's; every depth-1 tract's
    items equal trew_hip_decompose run on the piece's substring as a read, offset: the new kernel against the merged ones"""
    reads, want = two_tract
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        t.dissect(b, 1, 32, 3, 24, 1 << 12, 1 << 20, BIG)
        got = t.dissect_results()
        same(got, want)
        recs, items = got[0], got[1]
        t.tandems(b, 1, 32, 3, 24, 1 << 12)
        tan = t.tandems_results()
        assert tan[2] == len(recs)
        for f in recs.dtype.names:
            assert f == "reserved" or (tan[0][f] == recs[f]).all(), f
        t.decompose(b, 1, 32, 3, 24, 1 << 20, BIG)
        d_items, d_counts, d_recs, _, _ = t.decompose_results()
        pieces, where = [], []
        for i, read in enumerate(reads):
            mine = recs[recs["read"] == i]
            top = int(np.flatnonzero(mine["depth"] == 0)[0])
            mine_top = items[(items["read"] == i) & (items["motif"] == top)]
            theirs = d_items[d_items["read"] == i]
            assert mine[top]["reserved"] == d_recs["reserved"][i] and len(mine_top) == len(theirs)
            for f in ("start", "bases", "count", "phase", "consumed", "mismatches", "insertions", "deletions", "strand"):
                assert (mine_top[f] == theirs[f]).all()
            for q, x in enumerate(mine):
                if x["depth"] == 1:
                    lo, hi = (0, int(mine[top]["start"])) if x["start"] < mine[top]["start"] else (int(mine[top]["end"]), len(read))
                    pieces.append(read[lo:hi])
                    where.append((i, q, lo))
        assert len(pieces) == 30
        t.decompose(t.host_batch(*capi.pack_reads(pieces)), 1, 32, 3, 24, 1 << 20, BIG)
        p_items, p_counts, p_recs, _, _ = t.decompose_results()
        for p, (i, q, lo) in enumerate(where):
            mine = items[(items["read"] == i) & (items["motif"] == q)]
            theirs = p_items[p_items["read"] == p]
            x = recs[recs["read"] == i][q]
            assert p_recs["start"][p] + lo == x["start"] and p_recs["end"][p] + lo == x["end"] and p_recs["reserved"][p] == x["reserved"]
            assert len(mine) == len(theirs) == p_counts[p] and (theirs["start"] + lo == mine["start"]).all()
            for f in ("bases", "count", "phase", "consumed", "mismatches", "insertions", "deletions"):
                assert (mine[f] == theirs[f]).all()
    for penalty, min_score in ((1, 5), (64, 3)):
        same(gpu(reads, penalty, min_score), host(reads, penalty, min_score))


def test_one_long_read_with_three_long_tracts():
    read = DC.long_read()
    want = host([read])
    assert want[3] == 3 and ((want[0]["end"] - want[0]["start"]) > 2048).all() and want[4] > 1000
    same(gpu([read], mode=capi.MODE_LONG), want)


def test_a_deep_stack_with_a_trace_at_every_level():
    """repeat_cases.stack_reads(): six tracts as a right-deep chain, a left-deep chain and a balanced tree, and a read of 64
    tracts: entries stay on the stack while tract after tract is traced, up to 64 traces in one read; refine's record of a
    piece and resolve's"""
    reads = stack_reads()
    assert [len(r) for r in reads] == [1767, 1767, 1767, 5672]
    for candidates in (1, 2):
        want = host(reads, candidates=candidates)
        recs, counts = want[0], want[2]
        assert counts[:, 0].tolist() == [6, 6, 6, 64]
        assert (counts[:3, 1] >= 18).all() and counts[3, 1] >= 64
        depth = [int(recs[recs["read"] == r]["depth"].max()) for r in range(4)]
        assert depth[:3] == [5, 5, 2] and depth[3] >= 4
        same(gpu(reads, candidates=candidates), want)
        same(gpu(reads * 3, 64, 8, candidates=candidates), host(reads * 3, 64, 8, candidates=candidates))


def test_overflow_of_each_capacity(two_tract):
    """(1, 1, 1), each capacity alone, and each one short of enough: nothing is copied, a raw buffer is left untouched, the three
    numbers and the counts are exact, and the retry with exactly what was reported succeeds"""
    reads, want = two_tract
    nr, ni, nw = want[3], want[4], want[5]
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        for room in ((1, 1, 1), (1, 1 << 20, BIG), (1 << 12, 1, BIG), (1 << 12, 1 << 20, 1), (nr - 1, ni, nw), (nr, ni - 1, nw), (nr, ni, nw - 1),
                     (nr - 1, ni - 1, nw - 1)):
            t.dissect(b, 1, 32, 3, 24, *room)
            got = t.dissect_results()
            assert len(got[0]) == 0 and len(got[1]) == 0 and got[3:] == (nr, ni, nw) and (got[2] == want[2]).all()
            rbuf, ibuf = np.full(4, 7, dtype=capi.TANDEM_DTYPE), np.full(4, 7, dtype=capi.TRACE_DTYPE)
            a, c, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
            assert t.lib.trew_hip_dissect_results(t.ctx, 0, rbuf.ctypes.data, 4, ibuf.ctypes.data, 4, C.byref(a), C.byref(c), C.byref(d), None, None) == 0
            assert (a.value, c.value, d.value) == (nr, ni, nw) and (rbuf["read"] == 7).all() and (ibuf["read"] == 7).all()
            t.dissect(b, 1, 32, 3, 24, got[3], got[4], got[5])  # the retry: exactly what was reported
            same(t.dissect_results(), want)
        # buffers smaller than what was found: the first ones of the sorted orders
        rbuf, ibuf = np.zeros(3, dtype=capi.TANDEM_DTYPE), np.zeros(5, dtype=capi.TRACE_DTYPE)
        a, c, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert t.lib.trew_hip_dissect_results(t.ctx, 0, rbuf.ctypes.data, 3, ibuf.ctypes.data, 5, C.byref(a), C.byref(c), C.byref(d), None, None) == 0
        assert (a.value, c.value) == (nr, ni) and (rbuf == want[0][:3]).all() and (ibuf == want[1][:5]).all()


def test_the_fits_decision_is_taken_per_tract():
    """a batch of one read with two tracts, so the claim order is the walk's: depth 0 first.  max_rows = the rows of that tract:
    it is fetched from the workspace, the other is recomputed; the call reports overflow, and the retry equals the reference"""
    read = DC.behind_first(noisy(random.Random(2), "TTAGGC", 150, 0.02, 0.04))
    want = X.dissect([read])
    recs = want[0]
    assert len(recs) == 2 and list(recs["depth"]) == [0, 1]
    first_rows = int(recs["end"][0] - recs["start"][0])
    words, offsets, lengths = capi.pack_reads([read])
    with ctx(words=len(words) + 64, reads=16) as t:
        b = t.host_batch(words, offsets, lengths)
        t.dissect(b, 1, 32, 3, 24, 16, 1 << 12, first_rows)
        got = t.dissect_results()
        assert len(got[0]) == 0 and len(got[1]) == 0 and got[3:] == (2, len(want[1]), want[3]) and got[5] > first_rows
        assert (got[2] == want[2]).all()  # both tracts were traced: the counts are exact
        t.dissect(b, 1, 32, 3, 24, got[3], got[4], got[5])
        same(t.dissect_results(), want)


def test_a_reads_output_does_not_depend_on_the_batch(two_tract):
    reads, want = two_tract
    for r in (0, 13, 29):
        alone = gpu([reads[r]])
        mine_r, mine_i = want[0][want[0]["read"] == r].copy(), want[1][want[1]["read"] == r].copy()
        mine_r["read"] = 0
        mine_i["read"] = 0
        assert (alone[0] == mine_r).all() and (alone[1] == mine_i).all()
    none = gpu(reads, 3, 5000)  # min_score above every score: nothing, and no rows
    assert none[3:] == (0, 0, 0) and none[2].sum() == 0


def long_reads(n):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def test_batch_shapes(two_tract):
    reads, want = two_tract
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=64) as t:  # ragged and contiguous host batches
        t.dissect(t.host_batch(words, offsets, lengths), 1, 32, 3, 24, 1 << 12, 1 << 20, BIG)
        same(t.dissect_results(), want)
        t.dissect(t.host_batch(words, offsets, lengths, contiguous=True), 1, 32, 3, 24, 1 << 12, 1 << 20, BIG)
        same(t.dissect_results(), want)
    # device-resident generator reads, the longest read unknown
    full = long_reads(40)
    with ctx(mode=capi.MODE_LONG, reads=64, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, 40)
        b.max_length = 0
        t.dissect(b, 1, 32, 3, 24, 1 << 16, 1 << 20, BIG)
        got = t.dissect_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert got[6] > 0
    want = host(full)
    assert want[3] > 0
    same(got, want)
    # a uniform 150-base device batch
    n, L = 4000, 150
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    short = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = host(short)
    assert want[3] >= 20
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.dissect(t.device_uniform_batch(d, n, L), 1, 32, 3, 24, 1 << 16, 1 << 20, BIG)
        got = t.dissect_results()
        t.free(d)
    same(got, want)


def test_pair_mode_two_slots_repeated_calls_and_errors():
    rnd = random.Random(6)
    a = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, TEL, rnd.randint(0, 300), 0.03, 0.06, 0.01) + junk(rnd, 20) + noisy(rnd, "AATGG", rnd.randint(0, 200), 0.03, 0.06)
         for _ in range(100)]
    b = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, "CCCTA", rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(61)]
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_dissect"):
            t.dissect_results()
        t.tandems(ba)  # neither a tandems nor a decompose call is a dissect call: the buffers are separate
        t.tandems_results()
        t.decompose(ba)
        t.decompose_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_dissect"):
            t.dissect_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.dissect(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:60]))
        t.dissect(ba, 1, 32, 3, 24, 1 << 12, 1 << 16, 1 << 18, slot=0)  # the mates are two reads; the two slots overlap
        t.dissect(bb, 2, 9, 7, 10, 1 << 12, 1 << 16, 1 << 18, slot=1)
        got1, got0 = t.dissect_results(1), t.dissect_results(0)
        same(got1, host(b[:60], 7, 10, 2, 9))
        same(got0, host(a))
        assert got0[3] > 100 and got1[3] > 30
        # repeated calls on one slot: fewer reads, another penalty; the last call is what results returns
        t.dissect(bb, 1, 32, 1, 24, 1 << 12, 1 << 16, 1 << 18, slot=0)
        t.dissect(ba, 1, 16, 2, 30, 1 << 12, 1 << 16, 1 << 18, slot=0)
        same(t.dissect_results(0), host(a, 2, 30, 1, 16))
        same(t.dissect_results(0), host(a, 2, 30, 1, 16))  # fetching twice changes nothing
        for lo, hi in ((0, 32), (1, 33), (7, 6)):
            with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
                t.dissect(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.dissect(ba, 1, 32, penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.dissect(ba, 1, 32, 3, 0)
        with pytest.raises(capi.TrewHipError, match="max_records must be at least 1"):
            t.dissect(ba, 1, 32, 3, 24, 0, 10, 10)
        with pytest.raises(capi.TrewHipError, match="max_items must be at least 1"):
            t.dissect(ba, 1, 32, 3, 24, 10, 0, 10)
        with pytest.raises(capi.TrewHipError, match="max_rows must be at least 1"):
            t.dissect(ba, 1, 32, 3, 24, 10, 10, 0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.dissect(ba, slot=3)
        n = C.c_uint64(0)
        assert t.lib.trew_hip_dissect_results(t.ctx, 0, None, 0, None, 0, C.byref(n), C.byref(n), None, None, None) != 0
        assert b"n_records, n_items and n_rows must not be null" in t.lib.trew_hip_last_error(t.ctx)
        assert t.lib.trew_hip_dissect_results(t.ctx, 0, None, 3, None, 0, C.byref(n), C.byref(n), C.byref(n), None, None) != 0
        assert b"records must not be null" in t.lib.trew_hip_last_error(t.ctx)
        assert t.lib.trew_hip_dissect_results(t.ctx, 0, None, 0, None, 3, C.byref(n), C.byref(n), C.byref(n), None, None) != 0
        assert b"items must not be null" in t.lib.trew_hip_last_error(t.ctx)
        # no reads: nothing found, no kernel
        t.dissect(t.host_batch(*capi.pack_reads([])))
        got = t.dissect_results()
        assert len(got[0]) == 0 and len(got[1]) == 0 and got[2].shape == (0, 2) and got[3:] == (0, 0, 0)


def test_scan_tandems_and_decompose_unchanged_by_dissect_calls_in_between():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]
    want_a, want_b = host(a), host(b, 5, 30)

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    with fresh() as t:  # without any dissect call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.tandems(ba)
        alone = t.tandems_results()
        t.decompose(ba, 1, 32, 3, 24, 1 << 18, 1 << 20)
        alone_dec = t.decompose_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # dissect calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.dissect(ba, 1, 32, 3, 24, 1 << 14, 1 << 18, 1 << 20, slot=0)
        t.tandems(ba, slot=0)
        t.decompose(ba, 1, 32, 3, 24, 1 << 18, 1 << 20, slot=0)
        t.dissect(bb, 1, 32, 5, 30, 1 << 14, 1 << 18, 1 << 20, slot=1)
        t.submit(bb, slot=1)
        got_1 = t.dissect_results(1)
        got_0 = t.dissect_results(0)
        got = t.tandems_results(0)
        got_dec = t.decompose_results(0)
        tables = t.collect()
    same(got_0, want_a)
    same(got_1, want_b)
    assert (got[0] == alone[0]).all() and (got[1] == alone[1]).all() and got[2] == alone[2]
    assert (got_dec[0] == alone_dec[0]).all() and (got_dec[1] == alone_dec[1]).all() and (got_dec[2] == alone_dec[2]).all() and got_dec[3:] == alone_dec[3:]
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_convenience_entry_point_retries_inside(two_tract):
    import trew_amd

    reads, want = two_tract
    for got in (trew_amd.dissect(reads), trew_amd.dissect(reads, max_records=1, max_items=1, max_rows=1)):
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all()
    got = trew_amd.dissect(reads[:8], penalty=7, min_score=40)
    w = host(reads[:8], 7, 40)
    assert (got[0] == w[0]).all() and (got[1] == w[1]).all() and (got[2] == w[2]).all()


# ---- the `trew dissect` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r.encode() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args, env=None):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


def test_cli_two_tract_reads(tmp_path):
    reads = DC.cli_reads()
    path = str(tmp_path / "two.fastq")
    write_fastq(path, reads)
    host3 = host(reads)
    few = [r for r in reads if len(r) < 250][:8]  # rows formatted from the reference itself for the shortest reads
    same(host(few), X.dissect(few))
    rows, tail = X.cli_lines(path, reads, host3, 3)
    assert len(rows) - 2 == host3[3] >= 60 + 18 and len(tail) >= 5
    assert any(" =" in ln and any(c in ln.split(",")[-1] for c in "ACGT") and any(c in ln.split(",")[-1] for c in "acgt") for ln in rows)
    assert {ln.split(",")[-4] for ln in rows[2:]} == {"+", "-"}
    assert run_cli("dissect", path, "-t", "2")[0] == rows + tail
    assert run_cli("dissect", path, "-t", "5")[0] == rows + tail
    irows, itail = X.cli_lines(path, reads, host3, 3, per_item=True)
    assert itail == tail and len(irows) - 2 == host3[4] and run_cli("dissect", path, "-t", "3", "--items")[0] == irows + itail
    other = host(reads, 7, 60, 3, 12)
    rows2, tail2 = X.cli_lines(path, reads, other, 7)
    assert 5 <= len(rows2) - 2 < len(rows) - 2
    assert run_cli("dissect", path, "--penalty", "7", "--min_score", "60", "--min_period", "3", "--max_period", "12", "-t", "3")[0] == rows2 + tail2
    env = dict(os.environ, TREW_MEASURE_CHUNK_BYTES="4096")  # many small batches: the rows are the same
    assert run_cli("dissect", path, "-t", "4", env=env)[0] == rows + tail
    # the file is one batch, whose items outnumber the log's first size (sixteen per read): it is resubmitted once with the exact
    # numbers, which --stats counts
    assert host3[4] > 16 * len(reads) and host3[3] <= 4 * len(reads) + 16
    out, err = run_cli("dissect", path, "-t", "2", "--stats")
    assert out == rows + tail
    assert "%d items, 1 batch(es) resubmitted with a larger log" % host3[4] in err
