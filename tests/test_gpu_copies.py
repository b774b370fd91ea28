"""Copies in place for units of up to 256 bases on the GPU (trew_hip_copies through ctypes) against trew_copies_host, which
tests/test_copies_cpu.py checks against the brute-force reference of copies_ref.py.  Every item, count, record and n_rows of
every read of every batch is compared, field for field."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import copies_cases as CC
import copies_ref as R
import monomer_cases as MC
import oracle as O
from align_cases import TEL, fuzz_sets, revcomp
from period_cases import junk, noisy, rep
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 20  # rows (at most 256 MB of workspace): no test batch claims more
unit_of, q_of = CC.unit_of, CC.q_of


def same(got, want):
    """(items, counts, records[, n_items, n_rows]) of the device against those of the host definition"""
    gi, gc, gr = got[:3]
    wi, wc, wr = want[:3]
    assert gr.shape == wr.shape and gc.shape == wc.shape
    for f in wr.dtype.names:
        bad = np.argwhere(gr[f] != wr[f])
        assert len(bad) == 0, "record %s differs at (read, unit) %s: got %s, want %s" % (f, bad[0].tolist(), gr[tuple(bad[0])], wr[tuple(bad[0])])
    bad = np.argwhere(gc != wc)
    assert len(bad) == 0, "counts differ at (read, unit, strand) %s: got %d, want %d" % (bad[0].tolist(), gc[tuple(bad[0])], wc[tuple(bad[0])])
    assert len(gi) == len(wi)
    bad = np.flatnonzero(gi != wi)
    assert len(bad) == 0, "item %d differs: got %s, want %s" % (bad[0], gi[bad[0]], wi[bad[0]])
    if len(got) > 4 and len(want) > 4:
        assert tuple(got[3:5]) == tuple(want[3:5])  # n_items, n_rows


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18, flags=0):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16, flags=flags)


def gpu(reads, units, penalty=3, min_score=24, mode=capi.MODE_SHORT, max_items=1 << 20, max_rows=BIG):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.copies(t.host_batch(words, offsets, lengths), units, penalty, min_score, max_items, max_rows)
        out = t.copies_results()
    assert out[3] <= max_items and out[4] <= max_rows and out[3] == len(out[0]) == out[1].sum()
    return out


def host(reads, units, penalty=3, min_score=24):
    return capi.copies_host(reads, units, penalty, min_score)


def check(reads, units, settings=((1, 8), (3, 24), (64, 3)), least=1):
    for penalty, min_score in settings:
        want = host(reads, units, penalty, min_score)
        assert want[3] >= least
        same(gpu(reads, units, penalty, min_score), want)


@pytest.mark.parametrize("k", CC.GPU_KS)
def test_unit_and_read_lengths(k):
    """reads of 0, 1, k - 1, k, k + 1, 2 k + 1 bases and around a 32-base word and the 64-word seam"""
    unit, reads = CC.shape_reads(k)
    assert {0, 1, k - 1, k, k + 1, 2 * k + 1, 31, 32, 33, 2047, 2048, 2049} <= {len(r) for r in reads}
    check(reads, [unit], least=20)


@pytest.mark.parametrize("k", [33, 64, 65, 128, 171, 256])
def test_tracts_around_the_walk_block(k):
    """tracts of B - 1, B, B + 1 and 2 B + 1 rows around the block of B = 64 / Q rows the walk fetches at a time, with the
    workspace and, max_rows = 1, with every block computed again"""
    unit, reads = CC.block_reads(k)
    B = CC.block_of(k)
    want = host(reads, [unit], 3, 8)
    lens = {int(r["end_fwd"]) - int(r["start_fwd"]) for r in want[2][:, 0]} | {int(r["end_rev"]) - int(r["start_rev"]) for r in want[2][:, 0]}
    assert {B - 1, B, B + 1, 2 * B + 1} <= lens
    assert (want[1][:, 0, 0] > 0).any() and (want[1][:, 0, 1] > 0).any()
    same(gpu(reads, [unit], 3, 8), want)
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        t.copies(b, [unit], 3, 8, 1 << 20, 1)
        got = t.copies_results()
        assert len(got[0]) == 0 and (got[3], got[4]) == (want[3], want[4])
        assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
        t.copies(b, [unit], 3, 8, got[3], got[4])
        same(t.copies_results(), want)


@pytest.mark.parametrize("k", [65, 256])
def test_runs_of_deleted_and_inserted_bases(k):
    """d in {1, Q, 63, 64, k - 1} deleted and inserted bases in a row, across phase k - 1 -> 0 and across a lane seam"""
    unit, reads = CC.run_reads(k)
    want = host(reads, [unit], 1, 24)
    # at P = 1 a run of d deleted bases stays d deletions while d < 2 (k - d); a longer one is cheaper as k - d inserted bases
    kept = max(d for d in (1, q_of(k), 63, 64, k - 1) if 3 * d < 2 * k)
    assert int(want[0]["deletions"].max()) >= kept and int(want[0]["insertions"].max()) >= 1
    same(gpu(reads, [unit], 1, 24), want)
    same(gpu(reads, [unit], 3, 24), host(reads, [unit], 3, 24))


def test_special_reads():
    """the end-phase tie read; N inside a tract; a perfect 20 000-base repeat at k = 171; a 60 000-base noisy read at k = 256"""
    got = gpu([CC.TIE_READ, "ACGT" + CC.TIE_READ + "C"], [CC.TIE_UNIT], 3, 24)
    assert [tuple(int(x) for x in it)[3:11] for it in got[0] if it["read"] == 0 and it["strand"] == 0] == [
        (0, 51, 1, 15, 51, 0, 0, 0), (51, 66, 1, 0, 66, 0, 0, 0), (117, 3, 1, 0, 3, 0, 0, 0)]
    same(got, host([CC.TIE_READ, "ACGT" + CC.TIE_READ + "C"], [CC.TIE_UNIT], 3, 24))
    rnd = random.Random(4)
    u100, u171, u256 = unit_of(100, 1), unit_of(171, 1), unit_of(256, 1)
    with_n = [rep(u100, 150, 3) + "N" + rep(u100, 200, 54), rep(u100, 120, 0) + "NNN" + rep(u100, 130, 20), "N" * 40 + rep(u100, 250, 9) + "N"]
    want = host(with_n, [u100], 3, 24)
    assert want[3] >= 6
    same(gpu(with_n, [u100], 3, 24), want)
    perfect = rep(u171, 20_000, 2)
    got = gpu([perfect], [u171], 3, 24, mode=capi.MODE_LONG)
    fwd = [tuple(int(x) for x in it)[3:11] for it in got[0] if it["strand"] == 0]
    assert fwd == [(0, 169, 1, 2, 169, 0, 0, 0), (169, 115 * 171, 115, 0, 115 * 171, 0, 0, 0), (169 + 115 * 171, 166, 1, 0, 166, 0, 0, 0)]
    same(got, host([perfect], [u171], 3, 24))
    noisy_read = (junk(rnd, 1000) + noisy(rnd, u256, 60_000, 0.02, 0.03) + junk(rnd, 500))[:60_000]
    want = host([noisy_read], [u256], 3, 24)
    assert want[3] > 200 and int(want[2]["end_fwd"][0, 0]) - int(want[2]["start_fwd"][0, 0]) > 55_000
    same(gpu([noisy_read], [u256], 3, 24, mode=capi.MODE_LONG), want)


def test_one_deleted_and_one_inserted_base_at_every_position():
    unit = CC.edit_unit()
    reads = [c[0] for c in CC.edit_reads(unit)]
    check(reads, [unit], settings=((3, 24),), least=2 * len(reads))


def test_eight_monomers_of_mixed_lengths():
    """Q = 4 with small k in it: every monomer of the call runs on the layout the largest one picks"""
    rnd = random.Random(2025)
    units = [unit_of(k, 5) for k in (6, 33, 64, 65, 128, 171, 255, 256)]
    reads = []
    for i in range(40):
        u = units[i % 8] if i % 3 else revcomp(units[i % 8])
        reads.append(junk(rnd, rnd.randint(0, 100), "ACGTACGTACGTN") + noisy(rnd, u, rnd.randint(100, 700), 0.03, 0.06, 0.003) + junk(rnd, rnd.randint(0, 100)))
    for penalty in (2, 3):
        want = host(reads, units, penalty, 24)
        assert all(want[1][:, mi].sum() > 0 for mi in range(8))
        same(gpu(reads, units, penalty, 24), want)
    # the same small units on the layouts of Q = 1 and Q = 2
    same(gpu(reads, units[:3], 3, 24), host(reads, units[:3], 3, 24))
    same(gpu(reads, units[:5], 3, 24), host(reads, units[:5], 3, 24))


def two_strand_reads(unit, seed=11, n=12):
    """a noisy array of the unit and, behind a spacer, one of its reverse complement: both strands reach min_score, with
    different ranges; every third read has only one of them"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        a = noisy(rnd, unit, rnd.randint(150, 400), 0.03, 0.06)
        b = noisy(rnd, revcomp(unit), rnd.randint(150, 400), 0.03, 0.06)
        out.append(junk(rnd, rnd.randint(0, 40)) + a + (junk(rnd, 50) + b if i % 3 else "") + junk(rnd, rnd.randint(0, 40)))
    return out


def test_both_strands_one_strand_and_none():
    unit = unit_of(70, 9)
    reads = two_strand_reads(unit)
    want = host(reads, [unit], 3, 24)
    both = (want[1][:, 0, 0] > 0) & (want[1][:, 0, 1] > 0)
    one = (want[1][:, 0, 0] > 0) ^ (want[1][:, 0, 1] > 0)
    assert both.sum() >= 4 and one.sum() >= 2
    got = gpu(reads, [unit], 3, 24)
    same(got, want)
    a = want[2].astype([(f, "<i8") for f in capi.ALIGN_DTYPE.names])
    rows = int((a["end_fwd"] - a["start_fwd"])[a["score_fwd"] >= 24].sum() + (a["end_rev"] - a["start_rev"])[a["score_rev"] >= 24].sum())
    assert got[4] == rows  # per key: the strands claim their rows one after the other
    for r in (0, 1, 5):  # a key's items do not depend on the rest of the batch
        alone = gpu([reads[r]], [unit], 3, 24)
        mine = got[0][got[0]["read"] == r].copy()
        mine["read"] = 0
        assert (alone[0] == mine).all()
    top = int(max(want[2]["score_fwd"].max(), want[2]["score_rev"].max()))
    none = gpu(reads, [unit], 3, top + 1)
    assert none[3] == 0 and none[4] == 0 and len(none[0]) == 0 and none[1].sum() == 0
    for f in want[2].dtype.names:
        assert (none[2][f] == want[2][f]).all()
    exactly = gpu(reads, [unit], 3, top)
    assert exactly[3] > 0 and (exactly[1] > 0).sum() == 1


def test_overflow_of_the_log_and_of_the_workspace():
    """max_items = 1 and max_rows = 1, each alone and one short of enough: nothing is copied, the numbers are exact, and the
    retry with them succeeds"""
    u70, u171 = unit_of(70, 9), unit_of(171, 9)
    rnd = random.Random(12)
    reads = two_strand_reads(u70, 3, 8) + [junk(rnd, 30) + noisy(rnd, u171, rnd.randint(200, 900), 0.03, 0.06) for _ in range(8)]
    units = [u70, u171]
    want = host(reads, units, 3, 24)
    full = gpu(reads, units, 3, 24)
    same(full, want)
    n_items, n_rows = full[3], full[4]
    assert n_items > 50 and n_rows > 500
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads)) as t:
        b = t.host_batch(words, offsets, lengths)
        for max_items, max_rows in ((1, 1), (1, BIG), (1 << 20, 1), (n_items - 1, n_rows), (n_items, n_rows - 1)):
            t.copies(b, units, 3, 24, max_items, max_rows)
            got = t.copies_results()
            assert len(got[0]) == 0 and (got[3], got[4]) == (n_items, n_rows)
            assert (got[1] == want[1]).all() and (got[2] == want[2]).all()
            buf = np.full(4, 7, dtype=capi.TRACE_DTYPE)  # the raw call: a buffer is left untouched
            ni, nr = C.c_uint64(0), C.c_uint64(0)
            assert t.lib.trew_hip_copies_results(t.ctx, 0, buf.ctypes.data, 4, C.byref(ni), C.byref(nr), None, None, None) == 0
            assert (ni.value, nr.value) == (n_items, n_rows) and (buf["read"] == 7).all()
            t.copies(b, units, 3, 24, got[3], got[4])  # the retry: exactly what was reported
            same(t.copies_results(), want)
        buf = np.zeros(5, dtype=capi.TRACE_DTYPE)  # cap below the number of items: the first ones of the sorted order
        ni, nr = C.c_uint64(0), C.c_uint64(0)
        assert t.lib.trew_hip_copies_results(t.ctx, 0, buf.ctypes.data, 5, C.byref(ni), C.byref(nr), None, None, None) == 0
        assert ni.value == n_items and (buf == want[0][:5]).all()


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_items_equal_trace_up_to_32_bases(penalty):
    with ctx(words=1 << 16, reads=64) as t:
        for unit, reads in fuzz_sets():
            b = t.host_batch(*capi.pack_reads(reads))
            t.copies(b, [unit], penalty, 24, 1 << 16, 1 << 18)
            t.trace(b, [unit], penalty, 24, 1 << 16, 1 << 18)
            got, want = t.copies_results(), t.trace_results()
            same(got[:4], want[:4])
            same(got, host(reads, [unit], penalty, 24))


def long_reads(n):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def planted_reads(unit, n=24, seed=8):
    """generator long reads, cut to at most 4.5 kb, with a planted noisy array of the unit of 0.4 - 1.5 kb (one in four
    reverse-complemented)"""
    rnd = random.Random(seed)
    out = []
    for i, r in enumerate(long_reads(n)):
        body = r.decode()[:rnd.randint(300, 4500)]
        s = body + noisy(rnd, unit, rnd.randint(400, 1500), 0.03, 0.06, 0.002)
        out.append((revcomp(s.upper().replace("R", "N")) if i % 4 == 3 else s).encode())
    return out


@pytest.fixture(scope="module")
def planted():
    unit = unit_of(171, 6)
    reads = planted_reads(unit)
    want = host(reads, [unit], 3, 24)
    assert ((want[1][:, 0, 0] >= 3) | (want[1][:, 0, 1] >= 3)).all()  # every planted array is found and cut into copies
    return unit, reads, want


def test_every_batch_shape(planted):
    unit, reads, want = planted
    same(gpu(reads, [unit], 3, 24, mode=capi.MODE_LONG), want)
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=64) as t:
        t.copies(t.host_batch(words, offsets, lengths, contiguous=True), [unit], 3, 24, 1 << 20, BIG)
        same(t.copies_results(), want)
    # device-resident generator reads, the longest read unknown
    full = long_reads(12)
    u66 = unit_of(66, 6)
    with ctx(mode=capi.MODE_LONG, reads=64, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, 12)
        b.max_length = 0
        t.copies(b, [u66], 1, 24, 1 << 20, BIG)
        got = t.copies_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert got[5] > 0
    want66 = host(full, [u66], 1, 24)
    assert want66[3] > 0
    same(got, want66)
    # uniform short reads: device-resident, and host words without offsets and lengths
    n, L = 1500, 150
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    short = [buf[s:e + 1] for s, e in zip(st, nd)]
    units = [TEL, unit_of(130, 6)]
    want_short = host(short, units, 3, 24)
    assert want_short[3] > 10
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.copies(t.device_uniform_batch(d, n, L), units, 3, 24, 1 << 20, BIG)
        got = t.copies_results()
        t.free(d)
    same(got, want_short)
    w = np.ascontiguousarray(capi.pack_reads(short)[0], dtype=np.uint32)
    with ctx() as t:
        t.copies(capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0), units, 3, 24, 1 << 20, BIG)
        same(t.copies_results(), want_short)


def test_pair_mode_two_slots_repeated_calls_and_errors():
    rnd = random.Random(6)
    u40, u70, u200 = unit_of(40, 7), unit_of(70, 7), unit_of(200, 7)
    a = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, u70, rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(100)]
    b = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, u200, rnd.randint(0, 500), 0.03, 0.06, 0.01) for _ in range(61)]
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_copies"):
            t.copies_results()
        t.monomers(ba, [u70], 3)  # a monomers call is no copies call: the buffers are separate
        t.monomers_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_copies"):
            t.copies_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.copies(t.host_batch(*capi.pack_reads(b)), [u70])
        bb = t.host_batch(*capi.pack_reads(b[:60]))
        t.copies(ba, [u70, u40], 3, 24, 1 << 16, 1 << 18, slot=0)  # the mates are two reads; the two slots overlap
        t.copies(bb, [u200], 7, 10, 1 << 16, 1 << 18, slot=1)
        got1, got0 = t.copies_results(1), t.copies_results(0)
        same(got1, host(b[:60], [u200], 7, 10))
        same(got0, host(a, [u70, u40], 3, 24))
        assert got0[3] > 100 and got1[3] > 50
        # repeated calls on one slot: more units and a larger Q, then fewer; the last call is what results returns
        t.copies(bb, [u200, u70, "AAT"], 2, 24, 1 << 16, 1 << 18, slot=0)
        t.copies(ba, ["AAT", u70], 2, 30, 1 << 16, 1 << 18, slot=0)
        same(t.copies_results(0), host(a, ["AAT", u70], 2, 30))
        same(t.copies_results(0), host(a, ["AAT", u70], 2, 30))  # fetching twice changes nothing
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.copies(ba, [u70], penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.copies(ba, [u70], 3, 0)
        with pytest.raises(capi.TrewHipError, match="max_items must be at least 1"):
            t.copies(ba, [u70], 3, 24, 0, 10)
        with pytest.raises(capi.TrewHipError, match="max_rows must be at least 1"):
            t.copies(ba, [u70], 3, 24, 10, 0)
        for units in (["AAT"] * 9, []):
            with pytest.raises(capi.TrewHipError, match=r"n_monomers must be in \[1, 8\]"):
                t.copies(ba, units)
        with pytest.raises(capi.TrewHipError, match=r"monomer: k must be in \[3, 256\]"):
            t.copies(ba, [capi.Monomer(2, 0, (C.c_uint32 * 16)())])
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.copies(ba, [u70], slot=3)
        ni = C.c_uint64(0)
        assert t.lib.trew_hip_copies_results(t.ctx, 0, None, 0, C.byref(ni), None, None, None, None) != 0
        assert b"trew_hip_copies_results: n_items and n_rows must not be null" in t.lib.trew_hip_last_error(t.ctx)
        assert t.lib.trew_hip_copies_results(t.ctx, 0, None, 3, C.byref(ni), C.byref(ni), None, None, None) != 0
        assert b"trew_hip_copies_results: items must not be null" in t.lib.trew_hip_last_error(t.ctx)
        # no reads: no items, no rows, no kernel
        t.copies(t.host_batch(*capi.pack_reads([])), [u70], 3)
        got = t.copies_results()
        assert len(got[0]) == 0 and got[1].shape == (0, 1, 2) and got[2].shape == (0, 1) and got[3:] == (0, 0)


@pytest.mark.parametrize("k", [40, 100, 200])
def test_waves_go_well_past_their_first_read(k):
    """TREW_FLAG_DEBUG_ONE_CU: 32 waves for a few thousand short reads, about a hundred reads a wave"""
    rnd = random.Random(k)
    unit = unit_of(k, 8)
    reads = [junk(rnd, rnd.randint(0, 20), "ACGTN") + noisy(rnd, unit, rnd.randint(0, 90), 0.03, 0.06, 0.01) for _ in range(3000)]
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads), flags=capi.FLAG_DEBUG_ONE_CU) as t:
        assert t.debug_measure_grid(len(reads)) == 8
        t.copies(t.host_batch(words, offsets, lengths), [unit, unit_of(7, 8)], 3, 12, 1 << 18, BIG)
        want = host(reads, [unit, unit_of(7, 8)], 3, 12)
        assert want[3] > 1000
        same(t.copies_results(), want)


def test_scan_monomers_and_trace_unchanged_by_copies_calls_in_between():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 5000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3000], reads[3000:]
    units = [unit_of(70, 3), TEL]

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    with fresh() as t:  # without any copies call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.monomers(ba, units, 3)
        alone_m = t.monomers_results()
        t.trace(ba, [TEL], 3, 24, 1 << 18, 1 << 20)
        alone_t = t.trace_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # copies calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.copies(ba, units, 3, 24, 1 << 18, 1 << 20, slot=0)
        t.monomers(ba, units, 3, slot=0)
        t.trace(ba, [TEL], 3, 24, 1 << 18, 1 << 20, slot=0)
        t.copies(bb, [TEL], 5, 30, 1 << 18, 1 << 20, slot=1)
        t.submit(bb, slot=1)
        got_1 = t.copies_results(1)
        got_0 = t.copies_results(0)
        got_m = t.monomers_results(0)
        got_t = t.trace_results(0)
        tables = t.collect()
    same(got_0, host(a, units, 3, 24))
    same(got_1, host(b, [TEL], 5, 30))
    assert (got_m == alone_m).all() and (got_m == got_0[2]).all()  # and copies' records are monomers', field for field
    same(got_t, alone_t)
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_convenience_entry_point_retries_inside():
    import trew_amd

    unit, reads = CC.host_fuzz()[7]
    want = host(reads, [unit], 3, 24)
    same(trew_amd.copies(reads, [unit]), want)  # the defaults: penalty 3, min_score 24
    same(trew_amd.copies(reads, [unit], max_items=1, max_rows=1), want)
    same(trew_amd.copies(reads, [unit, TEL], penalty=7, min_score=40), host(reads, [unit, TEL], 7, 40))


# ---- the `trew copies` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


def test_cli_generator_long_reads_with_planted_arrays(tmp_path, planted):
    unit, reads, host3 = planted
    path = str(tmp_path / "arrays.fastq")
    write_fastq(path, reads)
    want = R.cli_lines(path, reads, [unit], [unit], host3, 3)
    assert len(want) - 6 >= len(reads)  # every read has its planted array
    assert any(":" in ln.split(",")[-1] and "(" in ln.split(",")[-1] for ln in want)  # edited copies and end pieces, as counts
    assert run_cli("copies", unit, path, "-t", "2")[0] == want
    assert run_cli("copies", unit, path, "-t", "5", "--bases")[0] == R.cli_lines(path, reads, [unit], [unit], host3, 3, bases=True)
    assert run_cli("copies", unit, path, "-t", "3", "--items")[0] == R.cli_lines(path, reads, [unit], [unit], host3, 3, per_item=True)
    assert run_cli("copies", unit, path, "--items", "--bases")[0] == R.cli_lines(path, reads, [unit], [unit], host3, 3, per_item=True, bases=True)
    # by --fasta: two records, the first over several lines, names in the motif column; a unit of at most 32 bases prints
    # trace's signature; another penalty and threshold
    fasta = str(tmp_path / "units.fa")
    with open(fasta, "w") as f:
        f.write(">alpha the 171-mer\n" + unit[:70] + "\n" + unit[70:140] + "\n" + unit[140:] + "\n\n>beta\n" + TEL + "\n")
    both = host(reads, [unit, TEL], 2, 150)
    want = R.cli_lines(path, reads, ["alpha", "beta"], [unit, TEL], both, 2, min_score=150)
    assert 10 <= len(want) - 8 <= 60
    assert run_cli("copies", "--fasta", fasta, path, "--penalty", "2", "--min_score", "150", "-t", "3")[0] == want
    assert run_cli("copies", unit + "," + TEL, path, "--penalty", "2", "--min_score", "150", "--items")[0] == R.cli_lines(
        path, reads, [unit, TEL], [unit, TEL], both, 2, min_score=150, per_item=True)
    out, err = run_cli("copies", unit, path, "-t", "2", "--stats")
    assert out == R.cli_lines(path, reads, [unit], [unit], host3, 3)
    assert "%d items, " % host3[3] in err
