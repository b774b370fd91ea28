"""Ordered unit chain on the GPU (trew_hip_chain through ctypes) against trew_chain_host, which test_chain_cpu.py checks
against the brute-force reference of chain_ref.py: every item and every count, integer for integer; the constructed cases
also name the item they were built for."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as A
import chain_ref as R
import interval_ref as I
import oracle as O
import tract_ref as T
import variant_ref as V
from chain_cases import (EDGE_BITS, EDGE_MOTIFS, EDGE_WORDS, K32, MOTIFS, NONE, TEL, cli_lines, dirty_planes, filler, key_items, noisy_reads, run_end_read,
                         run_start_read, same, subst, variant_back_anchor_read, variant_fwd_anchor_read)
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 20


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_chain(reads_or_packed, motifs, mode=capi.MODE_SHORT, max_events=BIG):
    """(items, counts, n_items, n_events) of one call with a log that is large enough"""
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16)) as t:
        t.chain(t.host_batch(words, offsets, lengths), motifs, max_events)
        return t.chain_results()


def check(reads, motifs, **kw):
    want = capi.chain_host(reads, motifs)
    got = gpu_chain(reads, motifs, **kw)
    same(got, want)
    assert got[2] == want[2] == len(want[0]) and got[2] <= got[3] <= 2 * got[2]
    return want


def short_reads(n):
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, 150)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def long_reads(n):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


# ---- word and iteration seams
@pytest.mark.parametrize("unit", EDGE_MOTIFS, ids=lambda m: "k%d" % len(m))
def test_run_starts_and_ends_at_word_edges(unit):
    k = len(unit)
    reads, expect = [], []
    for w in EDGE_WORDS:
        for bit in EDGE_BITS:
            p = 32 * w + bit
            reads.append(run_start_read(unit, p))
            expect.append((p, 3, NONE))
            read, r = run_end_read(unit, p)
            reads.append(read)
            expect.append((p - (r - 1) * k, r, NONE))
    want = check(reads, [unit])
    for r, item in enumerate(expect):
        assert item in key_items(want[0], r, 0, 0), (r, item)
    # the same seams on the reverse strand
    rc = [R.revcomp(x) for x in reads]
    want = check(rc, [unit])
    assert (want[1][:, 0, 1, 0] >= 1).all()


@pytest.mark.parametrize("unit", EDGE_MOTIFS, ids=lambda m: "k%d" % len(m))
def test_variant_at_word_edges_with_its_only_anchor_in_the_neighbouring_word(unit):
    k = len(unit)
    reads, expect = [], []
    for w in EDGE_WORDS:
        for bit in EDGE_BITS:
            p = 32 * w + bit
            reads.append(variant_fwd_anchor_read(unit, p) if bit >= 30 else variant_back_anchor_read(unit, p))
            expect.append(p)
            assert (p + k) // 32 > p // 32 if bit >= 30 else (p - k) // 32 < p // 32
    want = check(reads, [unit])
    for r, p in enumerate(expect):
        items = key_items(want[0], r, 0, 0)
        assert [x for x in items if x[0] == p and x[2] != NONE], (r, p, items)
        assert want[1][r, 0, 0].tolist() == [1, 1]  # the one anchor (a one-unit run) and the variant
    rc = [R.revcomp(x) for x in reads]
    want = check(rc, [unit])
    assert (want[1][:, 0, 1] == 1).all()


def test_k32_variant_whose_anchor_reaches_two_words_on():
    reads = [variant_fwd_anchor_read(K32, 32 * w + 31) for w in (0, 1, 61, 62, 63, 64, 125, 126)]
    want = check(reads, [K32])
    assert (want[1][:, 0, 0] == 1).all()


def test_one_run_over_three_iterations_is_two_events():
    read = filler(TEL, 5) + TEL * 684 + filler(TEL, 7)  # 4104 bases of tract: words 0 .. 128, iterations of 63 words
    want = capi.chain_host([read], [TEL])
    assert key_items(want[0], 0, 0, 0) == [(5, 684, NONE)] and want[2] == 1
    got = gpu_chain([read], [TEL])
    same(got, want)
    assert got[2] == 1 and got[3] == 2  # one item, a start event and an end event
    got = gpu_chain([R.revcomp(read)], [TEL])
    assert key_items(got[0], 0, 0, 1) == [(7, 684, NONE)] and got[2:] == (1, 2)


def test_one_unit_run_is_one_event():
    reads = [filler(TEL, 40) + TEL + filler(TEL, 40), TEL, filler(TEL, 2016) + TEL, filler(TEL, 2015 - 3) + TEL + filler(TEL, 9)]
    for read in reads:
        got = gpu_chain([read], [TEL])
        same(got, capi.chain_host([read], [TEL]))
        assert got[2:] == (1, 1) and key_items(got[0], 0, 0, 0)[0][1:] == (1, NONE)


def test_interleaved_residue_classes_in_one_word():
    reads = ["TGTGTGT", "TGTGT", "TG" * 40 + "T", "A" * 12, "A" * 100, "C" * 30 + "A" * 2100 + "C" * 3, "AC" * 1100, "ACG" * 20 + "ACGACGAC" * 9]
    motifs = ["TGT", "AAA", "ACAC", "ACGACG"]
    want = check(reads, motifs)
    assert key_items(want[0], 0, 0, 0) == [(0, 1, NONE), (2, 1, NONE), (4, 1, NONE)]
    assert key_items(want[0], 3, 1, 0) == [(0, 4, NONE), (1, 3, NONE), (2, 3, NONE)]
    # three runs across two iterations, between the variants CAA and AAC at the tract's ends
    assert key_items(want[0], 5, 1, 0) == [(29, 1, 4 * 0 + 2), (30, 700, NONE), (31, 699, NONE), (32, 699, NONE), (2128, 1, 4 * 2 + 2)]
    assert key_items(want[0], 6, 2, 0) == [(0, 550, NONE), (2, 549, NONE)]


def test_read_end_pairs_and_small_reads():
    reads = []
    for unit in EDGE_MOTIFS:
        k = len(unit)
        var = subst(unit, 1, "C" if unit[1] != "C" else "A")
        for n in (2 * k, 63, 64, 65, 2015, 2016, 2017, 2047, 2048, 2049):
            if n < 2 * k:
                continue
            full = filler(unit, n - 2 * k) + var + unit  # the forward anchor is the last window; one base shorter it is gone
            reads += [full, full[:-1]]
    reads += ["", "T", "TT", "TTAGG", TEL, TEL + "TCAGGG", "TCAGGG" + TEL, "N" * 31, "N" * 5000, "A" * 33, "ttagggTCAGGGttaggg", (TEL * 700)[:2016] + "N" + (TEL * 700)[2017:4000]]
    want = check(reads, EDGE_MOTIFS)
    m = 1
    i = 2 * len([n for n in (6, 63, 64, 65, 2015, 2016, 2017, 2047, 2048, 2049) if n >= 6])  # the TEL pairs come second
    assert want[1][i, m, 0].tolist() == [1, 1] and want[1][i + 1, m, 0].tolist() == [0, 0]


def test_dirty_bits_past_the_end():
    rnd = random.Random(7)
    reads = [(TEL * 400)[:n] for n in (6, 11, 12, 33, 63, 65, 2017, 2047, 4033)] + [(K32 * 70)[:n] for n in (32, 63, 65, 2047)] + noisy_reads(60, seed=2)
    words, offsets, lengths = capi.pack_reads(reads)
    dirty = dirty_planes(words, offsets, lengths, rnd)
    assert (dirty != words).any()
    want = capi.chain_host(reads, [TEL, K32, "GGG"])
    same(capi.chain_host((dirty, offsets, lengths), [TEL, K32, "GGG"]), want)
    same(gpu_chain((dirty, offsets, lengths), [TEL, K32, "GGG"]), want)


def test_many_copies_of_one_read():
    read = "ACGTACGT" + TEL * 3 + "TCAGGG" + TEL * 2 + "TGAGGG" + "TTGGGG" + TEL + "A" + TEL * 30 + R.revcomp(TEL * 2 + "TCAGGG" + TEL)
    one = capi.chain_host([read], [TEL, "TTAGGC"])
    assert one[2] >= 9
    items, counts, n_items, n_events = gpu_chain([read] * 4096, [TEL, "TTAGGC"])
    assert n_items == 4096 * one[2] and (counts == one[1][0]).all()
    assert (items["read"] == np.repeat(np.arange(4096, dtype=np.uint32), one[2])).all()
    for f in R.FIELDS[1:]:
        assert (items[f].reshape(4096, one[2]) == one[0][f]).all(), f


# ---- the overflow protocol
def test_overflow_protocol():
    reads = noisy_reads(200, seed=8)
    motifs = MOTIFS[:3]
    want = capi.chain_host(reads, motifs)
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads(reads))
        t.chain(b, motifs, BIG)
        need = t.chain_results()[3]
        assert want[2] < need <= 2 * want[2] and need > 100
        for cap in (1, need // 2, need - 1):  # below the need: no items, everything else exact
            t.chain(b, motifs, cap)
            items, counts, n_items, n_events = t.chain_results()
            assert len(items) == 0 and n_items == want[2] and n_events == need and (counts == want[1]).all()
            # a buffer handed in anyway stays untouched
            buf = np.full(4, 0xAB, dtype=capi.CHAIN_DTYPE)
            ni, ne = C.c_uint64(0), C.c_uint64(0)
            assert t.lib.trew_hip_chain_results(t.ctx, 0, buf.ctypes.data, 4, C.byref(ni), C.byref(ne), None, None) == 0
            assert (ni.value, ne.value) == (want[2], need) and (buf == np.full(4, 0xAB, dtype=capi.CHAIN_DTYPE)).all()
            t.chain(b, motifs, n_events)  # the retry with the reported number is complete
            same(t.chain_results(), want)
        for cap in (need, need + 1):  # at and above the need
            t.chain(b, motifs, cap)
            got = t.chain_results()
            same(got, want)
            assert got[2:] == (want[2], need)
        # a caller's buffer smaller than the items: the first ones of the sorted order
        t.chain(b, motifs, need)
        few = np.zeros(5, dtype=capi.CHAIN_DTYPE)
        ni, ne = C.c_uint64(0), C.c_uint64(0)
        assert t.lib.trew_hip_chain_results(t.ctx, 0, few.ctypes.data, 5, C.byref(ni), C.byref(ne), None, None) == 0
        assert ni.value == want[2] and (few == want[0][:5]).all()
    import trew_amd
    same(trew_amd.chain(reads, motifs, max_events=3), want)  # the retry inside the Python entry
    same(trew_amd.chain(reads, motifs), want)


def test_repeated_calls():
    reads = noisy_reads(200, seed=9)
    want = capi.chain_host(reads, MOTIFS[:3])
    few = capi.chain_host(reads[:7], [TEL])
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads(reads))
        t.chain(b, MOTIFS[:3], BIG)
        t.chain(b, MOTIFS[:3], BIG)
        same(t.chain_results(), want)
        same(t.chain_results(), want)  # reading twice changes nothing
        t.chain(t.host_batch(*capi.pack_reads(reads[:7])), [TEL], BIG)  # fewer reads and motifs than the call before
        same(t.chain_results(), few)
        t.chain(t.host_batch(*capi.pack_reads([])), [TEL], 1)  # no reads: nothing
        items, counts, n_items, n_events = t.chain_results()
        assert len(items) == 0 and counts.shape == (0, 1, 2, 2) and (n_items, n_events) == (0, 0)


# ---- against the host at large
def fuzz_case(seed):
    rnd = random.Random(seed)
    motifs = ["".join(rnd.choice("ACGT") for _ in range(k)) for k in (3, 4, 6, 9, 13, 24, 31, 32)]
    reads = []
    for i in range(160):
        n = rnd.randint(50, 5000)
        unit = rnd.choice(motifs)
        unit = unit if i % 2 else R.revcomp(unit)
        rate = rnd.choice([0.005, 0.02, 0.08])
        tract = [rnd.choice("ACGTN") if rnd.random() < rate else c for c in unit * (n // len(unit) + 1)]
        if i % 5 == 0:
            del tract[rnd.randrange(len(tract))]  # an indel shifts the phase
        head = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 200)))
        reads.append((head + "".join(tract))[:n] if i % 7 else "".join(rnd.choice("ACGT") for _ in range(n)))
    return reads, motifs


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_over_ragged_reads(seed):
    reads, motifs = fuzz_case(seed)
    want = check(reads, motifs)
    assert (want[1].sum(axis=(0, 2)) >= 10).all()  # runs and variants for every motif
    ref = R.chain(reads[:12], motifs, R.chain_read_walk)  # the host twin itself against the reference
    head = want[0][want[0]["read"] < 12]
    same((head, want[1][:12]), ref)


def test_eight_motifs_in_one_call():
    reads = noisy_reads()
    want = check(reads, MOTIFS)
    assert (want[1].sum(axis=0) >= 5).all()


def test_generator_long_reads_device_resident():
    n = 2000
    reads = long_reads(n)
    want = capi.chain_host(capi.pack_reads(reads), [TEL])
    assert (want[1].sum(axis=(0, 1)) >= 300).all()
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        b.max_length = 0  # unknown longest read
        t.chain(b, [TEL])  # the default log: four events per read
        items, counts, n_items, n_events, ms = t.chain_results(want_ms=True)
        if n_events > 4 * n:
            assert len(items) == 0
            t.chain(b, [TEL], n_events)
            items, counts, n_items, n_events, ms = t.chain_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same((items, counts), want)


# ---- batch plumbing
@pytest.fixture(scope="module")
def uniform150():
    reads = short_reads(4000)  # text from the generator, packed on the host
    want = capi.chain_host(reads, [TEL, "CCCTAA"])
    assert want[1][:, 0, 0, 0].sum() >= 100 and want[1][:, 0, 1, 0].sum() >= 100
    return reads, want


@pytest.mark.parametrize("shape", ["host_ragged", "contiguous", "host_uniform", "device_uniform"])
def test_batch_shapes(uniform150, shape):
    n, L = 4000, 150
    reads, want = uniform150
    words, offsets, lengths = capi.pack_reads(reads)
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 20) as t:
        d = None
        if shape == "host_ragged":
            b = t.host_batch(words, offsets, lengths)
        elif shape == "contiguous":
            b = t.host_batch(words, offsets, lengths, contiguous=True)
        elif shape == "host_uniform":
            w = np.ascontiguousarray(words, dtype=np.uint32)
            b = capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0)
            b._keep = (w,)
        else:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(20250218, 0, n, L, d)
            b = t.device_uniform_batch(d, n, L)
        t.chain(b, [TEL, "CCCTAA"], BIG)
        got = t.chain_results()
        if d is not None:
            t.free(d)
    same(got, want)


def test_pair_mode_context_and_two_slots():
    reads = noisy_reads(400, seed=6)
    a, b = reads[:250], reads[250:]
    want_a, want_b = capi.chain_host(a, [TEL, "AAT"]), capi.chain_host(b, [K32])
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.chain(ba, [TEL, "AAT"], BIG, slot=0)
        t.chain(bb, [K32], BIG, slot=1)
        same(t.chain_results(1), want_b)
        same(t.chain_results(0), want_a)


# ---- independence
def test_scan_and_the_other_measures_are_unchanged_by_a_chain_call_in_between():
    reads = short_reads(12000)
    a, b = reads[:7000], reads[7000:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = capi.chain_host(a, motifs), capi.chain_host(b, motifs)
    IV = 1 << 16
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        # without any chain call
        t.annotate(ba, motifs)
        alone_a = t.annotate_results()
        t.tracts(ba, motifs, 3)
        alone_t = t.tracts_results()
        t.intervals(ba, motifs, 6, 12, IV)
        alone_i = t.intervals_results()
        t.variants(ba, motifs)
        alone_v = t.variants_results()
        t.periods(ba, 1, 32, 3, 24)
        alone_p = t.periods_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        # everything interleaved on slot 0, chain and a scan on slot 1; nothing collected until the end
        t.submit(ba, slot=0)
        t.chain(ba, motifs, BIG, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.chain(bb, motifs, BIG, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.intervals(ba, motifs, 6, 12, IV, slot=0)
        t.variants(ba, motifs, slot=0)
        t.chain(ba, motifs, BIG, slot=0)
        t.periods(ba, 1, 32, 3, 24, slot=0)
        t.submit(bb, slot=1)
        got_c1 = t.chain_results(1)
        got_c0 = t.chain_results(0)
        got_a = t.annotate_results(0)
        got_t = t.tracts_results(0)
        got_i = t.intervals_results(0)
        got_v = t.variants_results(0)
        got_p = t.periods_results(0)
        tables = t.collect()
    same(got_c0, want_a)
    same(got_c1, want_b)
    assert (got_a == alone_a).all() and (alone_a == A.annotate(a, motifs)).all()
    assert (got_t == alone_t).all() and (alone_t == T.tracts(a, motifs, 3)).all()
    assert (got_i[0] == alone_i[0]).all() and (got_i[1] == alone_i[1]).all() and got_i[2] == alone_i[2]
    assert (alone_i[0] == I.intervals(a, motifs, 6, 12)[0]).all()
    assert all((x == y).all() for x, y in zip(got_v, alone_v)) and (alone_v[1] == V.variants(a, motifs)[1]).all()
    assert (got_p == alone_p).all() and (alone_p["period"] > 0).any()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0
    # and the chain agrees with the variants of the same batch
    runs = got_c0[0][got_c0[0]["bin"] == NONE]
    units = np.zeros((len(a), 2, 2), dtype=np.uint64)
    np.add.at(units, (runs["read"], runs["motif"], runs["strand"]), runs["count"])
    assert (units[:, :, 0] == got_v[0]["units_fwd"]).all() and (units[:, :, 1] == got_v[0]["units_rev"]).all()
    assert (got_c0[1][:, :, 0, 1] == got_v[0]["variants_fwd"]).all() and (got_c0[1][:, :, 1, 1] == got_v[0]["variants_rev"]).all()


def test_errors():
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads([b"TTAGGGTCAGGG"]))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_chain"):
            t.chain_results()
        t.variants(b, [TEL])  # a variants call is no chain call: the buffers are separate
        t.variants_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_chain"):
            t.chain_results()
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.chain(b, ["AAT"] * 9)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.chain(b, [])
        with pytest.raises(capi.TrewHipError, match=r"k must be in \[3, 32\]"):
            t.chain(b, [capi.Motif(2, 0, 5)])
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.chain(b, [TEL], slot=3)
        with pytest.raises(capi.TrewHipError, match="max_events must be at least 1"):
            t.chain(b, [TEL], 0)
        t.chain(b, [TEL, "CCCTAA"], 16)
        ni, ne = C.c_uint64(0), C.c_uint64(0)
        assert t.lib.trew_hip_chain_results(t.ctx, 0, None, 0, None, C.byref(ne), None, None) != 0
        assert b"must not be null" in t.lib.trew_hip_last_error(t.ctx)
        assert t.lib.trew_hip_chain_results(t.ctx, 0, None, 1, C.byref(ni), C.byref(ne), None, None) != 0
        assert b"out must not be null" in t.lib.trew_hip_last_error(t.ctx)
        assert t.lib.trew_hip_chain_results(t.ctx, 0, None, 0, C.byref(ni), C.byref(ne), None, None) == 0 and (ni.value, ne.value) == (4, 4)
        items, counts, n_items, n_events = t.chain_results()
        # TTAGGG forward, and the reverse strand of CCCTAA, whose target is TTAGGG again: CCCTGA is (4, G) of CCCTAA, bin 17
        assert [tuple(int(v) for v in x) for x in items] == [(0, 0, 0, 0, 1, NONE), (0, 0, 0, 6, 1, 6), (0, 1, 1, 0, 1, NONE), (0, 1, 1, 6, 1, 17)]


# ---- the `trew chain` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)


expected_cli = cli_lines


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


def test_cli_end_to_end(tmp_path):
    """generator long reads with noisy telomere tails, two files (one gzipped), two motifs; rows, --items, the summary, the
    resubmits that --stats counts"""
    reads = long_reads(300)
    pa, pb = str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq.gz")
    write_fastq(pa, reads[:180])
    write_fastq(pb, reads[180:])
    motifs = [TEL, "TTAGGGC"]
    files = [(pa, reads[:180]), (pb, reads[180:])]
    want = expected_cli(files, motifs, min_units=50)
    assert sum(1 for ln in want if ln[0].isdigit()) >= 10 and any(" TCAGGG " in ln or " TTGGGG " in ln for ln in want)
    out, err = run_cli("chain", ",".join(motifs), pa, pb, "--min_units", "50", "-t", "2", "--stats")
    assert out == want
    assert "batch(es) resubmitted with a larger log" in err and ", 0 batch(es)" not in err  # far more than four events a read
    assert run_cli("chain", ",".join(motifs), pa, pb, "--min_units", "50", "-t", "8")[0] == want
    items = expected_cli(files, motifs, min_units=50, per_item=True)
    assert len(items) > len(want)
    assert run_cli("chain", ",".join(motifs), pa, pb, "--min_units", "50", "--items", "-t", "3")[0] == items
    # the default MIN_UNITS and a file without a read
    empty = str(tmp_path / "empty.fastq")
    write_fastq(empty, [])
    assert run_cli("chain", TEL, pa, empty)[0] == expected_cli([(pa, reads[:180]), (empty, [])], [TEL])
