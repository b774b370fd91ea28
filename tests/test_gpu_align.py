"""Indel-aware motif tract per read on the GPU (trew_hip_align through ctypes) against the reference of align_ref.py, or, where
that is too slow, against trew_align_host (which tests/test_align_cpu.py checks against the reference).  Every read of every
batch is compared, field for field."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_ref as R
import oracle as O
from align_cases import GPU_KS, HAND, TEL, UNITS, fuzz_sets, revcomp, rotations, with_deletion, with_insertion
from period_cases import junk, noisy, rep
from trew_amd import capi

pytestmark = pytest.mark.gpu
assert tuple(capi.ALIGN_DTYPE.names) == R.FIELDS  # the reference and the record name their fields alike, in the same order
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
LONG_N = 300


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, motif) %s: got %s, want %s" % (
            f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def rec(x):
    return tuple(int(v) for v in x)


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_align(reads, motifs, penalty=3, mode=capi.MODE_SHORT):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.align(t.host_batch(words, offsets, lengths), motifs, penalty)
        return t.align_results()


def long_reads(n=LONG_N):
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
    want = capi.align_host(reads, [TEL], 3)
    cols = capi.align_columns(want, 6, 3)
    best = np.where(want["score_fwd"] >= want["score_rev"], cols["deletions_fwd"] + cols["insertions_fwd"], cols["deletions_rev"] + cols["insertions_rev"])
    assert (best[:, 0] >= 5).sum() >= len(reads) // 2  # the planted tails are found through their indels
    return reads, want


def test_hand_worked_vectors():
    for penalty in sorted({p for _, _, p, _, _ in HAND}):
        for motif in sorted({m for _, m, p, _, _ in HAND if p == penalty}):
            rows = [(r, f + v) for r, m, p, f, v in HAND if p == penalty and m == motif]
            got = gpu_align([r.encode() for r, _ in rows], [motif], penalty)
            assert [rec(g) for g in got[:, 0]] == [w for _, w in rows]


def shape_reads(unit, seed):
    """The read lengths at which a wave-per-read kernel goes wrong (word and 64-word seams, reads shorter than the motif), as
    perfect repeats, as noisy repeats and with one deleted / one inserted base at bits 31 and 0 of a word and at base 2047 /
    2048"""
    rnd = random.Random(seed)
    k = len(unit)
    reads = []
    for n in (0, 1, k - 1, k, 31, 32, 33, 2047, 2048, 2049):
        reads.append(rep(unit, n))
        reads.append(rep(unit, n, 1 % k))
        reads.append(noisy(rnd, unit, n, 0.03, 0.06, 0.005))
        reads.append(junk(rnd, n, "ACGTN"))
    base = rep(unit, 2200)
    for at in (31, 32, 63, 64, 2047, 2048):
        reads.append(with_deletion(base, at))
        reads.append(with_insertion(base, at, "ACGT"[(at + 1) % 4]))
        reads.append(with_insertion(with_deletion(base, at), at + 40, "A"))
    return reads


@pytest.mark.parametrize("k", GPU_KS)
def test_motif_and_read_lengths(k):
    unit = UNITS[k]
    reads = shape_reads(unit, k)
    short = [r for r in reads if len(r) <= 33]
    for penalty in (1, 3, 64):
        want = capi.align_host(reads, [unit], penalty)
        same(gpu_align(reads, [unit], penalty), want)
    # the yardstick itself against the reference, on the short reads and on the two longest kinds
    pick = short + reads[-18:-12]
    same(capi.align_host(pick, [unit], 3), R.align(pick, [unit], 3))


@pytest.mark.parametrize("k", GPU_KS)
def test_runs_of_deleted_and_inserted_bases(k):
    """d deleted motif bases in a row for every d < k: d deletions at P = 1 while d < 2 (k - d), and k - d inserted bases (the rest
    of the broken unit, which costs k - d and loses k - d matches) once that is cheaper; k deleted bases leave no trace; runs of inserted bases"""
    unit = UNITS[k]
    base = rep(unit, 40 * k)
    mid = 20 * k + 1
    reads = [with_deletion(base, mid, d) for d in range(1, k + 1)]
    reads += [with_insertion(base, mid, junk(random.Random(d), d)) for d in (1, 2, 3, 5, 8)]
    want = R.align(reads, [unit], 1)
    cols = capi.align_columns(want, k, 1)
    for d in range(1, k):
        got = (int(cols["deletions_fwd"][d - 1, 0]), int(cols["insertions_fwd"][d - 1, 0]), int(cols["mismatches_fwd"][d - 1, 0]))
        if 3 * d != 2 * k:
            assert got == ((d, 0, 0) if 3 * d < 2 * k else (0, k - d, 0)), (d, got)
        assert (int(want["start_fwd"][d - 1, 0]), int(want["end_fwd"][d - 1, 0])) == (0, 40 * k - d)
    assert rec(want[k - 1, 0])[:5] == (39 * k, 0, 39 * k, 39 * k, 39 * k)
    same(gpu_align(reads, [unit], 1), want)
    for penalty in (3, 64):
        same(gpu_align(reads, [unit], penalty), capi.align_host(reads, [unit], penalty))


def test_ties_and_n():
    """P = 1: a zero-sum prefix (a match and a mismatch, ...) in front of a tract and behind it: the later start and the earlier
    end win.  Equal scores in different phases: two tracts of 36 bases in different phases of the motif, 40 bases that match
    nothing apart; the one that ends earlier is reported.  An N inside a tract is a mismatch."""
    t = TEL * 6
    reads = ["TC" + t, "TCTC" + t, t + "CT", t + "CTCT", "T" + "C" + "T" + "A" + "C" + t,
             t + "C" * 40 + t[3:] + "TTA", t[3:] + "TTA" + "C" * 40 + t, t[:17] + "N" + t[18:], "N" * 5 + t + "N" + t + "NN"]
    for penalty in (1, 3):
        want = R.align(reads, [TEL], penalty)
        if penalty == 1:
            assert rec(want[0, 0])[:3] == (36, 2, 38) and rec(want[1, 0])[:3] == (36, 4, 40)
            assert rec(want[2, 0])[:3] == (36, 0, 36) and rec(want[3, 0])[:3] == (36, 0, 36)
            assert rec(want[5, 0])[:3] == (36, 0, 36) and rec(want[6, 0])[:3] == (36, 0, 36)
        same(gpu_align(reads, [TEL], penalty), want)
        same(gpu_align([revcomp(r) for r in reads], [TEL], penalty), R.align([revcomp(r) for r in reads], [TEL], penalty))


def test_fields_beyond_16_bits():
    """a perfect repeat of 70 000 bases (every field passes 2^16) and a 200 000-base noisy read at P = 64"""
    rnd = random.Random(4)
    perfect = rep(TEL, 70_000, 2)
    noisy_read = junk(rnd, 3000) + noisy(rnd, TEL, 200_000, 0.002, 0.002) + junk(rnd, 500)
    noisy_read = noisy_read[:200_000]
    got = gpu_align([perfect], [TEL], 3, mode=capi.MODE_LONG)
    assert rec(got[0, 0])[:5] == (70_000, 0, 70_000, 70_000, 70_000)
    same(got, capi.align_host([perfect], [TEL], 3))
    want = capi.align_host([noisy_read], [TEL], 64)
    assert int(want["score_fwd"][0, 0]) > 1 << 16 and int(want["end_fwd"][0, 0]) - int(want["start_fwd"][0, 0]) > 1 << 16
    same(gpu_align([noisy_read], [TEL], 64, mode=capi.MODE_LONG), want)


@pytest.mark.parametrize("k", (6, 17, 32))
def test_every_rotation_and_the_other_strand(k):
    rnd = random.Random(k)
    unit = UNITS[k]
    reads = [junk(rnd, 30) + noisy(rnd, unit, 400, 0.03, 0.06, 0.003) + junk(rnd, 20) for _ in range(6)]
    want = capi.align_host(reads, [unit], 3)
    rots = rotations(unit)
    for lo in range(0, k, 8):
        got = gpu_align(reads, rots[lo:lo + 8], 3)
        for m in range(got.shape[1]):
            same(got[:, m:m + 1], want)
    rc = gpu_align([revcomp(r) for r in reads], [unit], 3)
    assert (rc["score_rev"] == want["score_fwd"]).all() and (rc["score_fwd"] == want["score_rev"]).all()
    same(rc, capi.align_host([revcomp(r) for r in reads], [unit], 3))


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_fuzz_sets(penalty):
    for unit, reads in fuzz_sets():
        same(gpu_align(reads, [unit], penalty), capi.align_host(reads, [unit], penalty))


def test_eight_motifs_at_once():
    rnd = random.Random(2025)
    motifs = [UNITS[k] for k in GPU_KS]
    reads = []
    for i in range(48):
        unit = motifs[i % 8] if i % 3 else revcomp(motifs[i % 8])
        reads.append(junk(rnd, rnd.randint(0, 100), "ACGTACGTACGTN") + noisy(rnd, unit, rnd.randint(100, 500), 0.03, 0.06, 0.003) + junk(rnd, rnd.randint(0, 100)))
    for penalty in (1, 3, 64):
        want = capi.align_host(reads, motifs, penalty)
        if penalty == 3:
            for mi in range(8):
                assert max(want["score_fwd"][:, mi].max(), want["score_rev"][:, mi].max()) >= 60
        same(gpu_align(reads, motifs, penalty), want)
    few = sorted(reads, key=len)[:3]
    same(capi.align_host(few, motifs, 3), R.align(few, motifs, 3))


def test_generator_long_reads_every_batch_shape(tails):
    reads, want = tails
    same(gpu_align(reads, [TEL], 3, mode=capi.MODE_LONG), want)
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=64) as t:
        t.align(t.host_batch(words, offsets, lengths, contiguous=True), [TEL], 3)
        same(t.align_results(), want)
    # device-resident generator reads, the longest read unknown
    full = long_reads(60)
    with ctx(mode=capi.MODE_LONG, reads=64, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, 60)
        b.max_length = 0
        t.align(b, [TEL], 3)
        got, ms = t.align_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, capi.align_host(full, [TEL], 3))


def test_uniform_short_reads():
    n, L = 4000, 150
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.align_host(reads, [TEL], 3)
    assert (want["score_fwd"][:, 0] >= 100).sum() >= 10 and (want["score_rev"][:, 0] >= 100).sum() >= 10
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.align(t.device_uniform_batch(d, n, L), [TEL], 3)
        got = t.align_results()
        t.free(d)
    same(got, want)
    words, offsets, lengths = capi.pack_reads(reads)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    with ctx() as t:
        b = capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0)
        t.align(b, [TEL], 3)
        same(t.align_results(), want)


def test_pair_mode_two_slots_repeated_calls_and_errors():
    rnd = random.Random(6)
    a = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, TEL, rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(100)]
    b = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, "CCCTA", rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(61)]
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_align"):
            t.align_results()
        t.tracts(ba, [TEL], 3)  # a tracts call is no align call: the buffers are separate
        t.tracts_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_align"):
            t.align_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.align(t.host_batch(*capi.pack_reads(b)), [TEL])
        bb = t.host_batch(*capi.pack_reads(b[:60]))
        t.align(ba, [TEL, "CCCTA"], 3, slot=0)  # the mates are two reads; the two slots overlap
        t.align(bb, ["CCCTA"], 7, slot=1)
        got1, got0 = t.align_results(1), t.align_results(0)
        same(got1, capi.align_host(b[:60], ["CCCTA"], 7))
        same(got0, capi.align_host(a, [TEL, "CCCTA"], 3))
        # repeated calls on one slot: more motifs, fewer reads, another penalty; the last call is what results returns
        t.align(bb, ["CCCTA", TEL, "AAT"], 1, slot=0)
        t.align(ba, ["AAT"], 64, slot=0)
        same(t.align_results(0), capi.align_host(a, ["AAT"], 64))
        same(t.align_results(0), capi.align_host(a, ["AAT"], 64))  # fetching twice changes nothing
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.align(ba, [TEL], penalty)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.align(ba, ["AAT"] * 9)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.align(ba, [])
        with pytest.raises(capi.TrewHipError, match=r"k must be in \[3, 32\]"):
            t.align(ba, [capi.Motif(2, 0, 5)])
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.align(ba, [TEL], slot=3)
        # results larger than the caller's buffer: the count is reported, cap records are copied
        t.align(ba, ["ACG", TEL], 3)
        n = C.c_uint64(0)
        one = np.zeros(1, dtype=capi.ALIGN_DTYPE)
        assert t.lib.trew_hip_align_results(t.ctx, 0, one.ctypes.data, 1, C.byref(n), None) == 0
        assert n.value == 200 and rec(one[0]) == rec(capi.align_host(a[:1], ["ACG"], 3)[0, 0])
        assert t.lib.trew_hip_align_results(t.ctx, 0, None, 0, C.byref(n), None) == 0 and n.value == 200
        # no reads: no records, no kernel
        t.align(t.host_batch(*capi.pack_reads([])), [TEL], 3)
        assert t.align_results().shape == (0, 1)


def test_independent_of_scan_and_the_other_measures():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = capi.align_host(a, motifs, 3), capi.align_host(b, [TEL], 5)
    LOG = 1 << 16

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    def fetch(t, slot=0):
        return ((t.annotate_results(slot), t.tracts_results(slot)) + t.intervals_results(slot) + t.variants_results(slot) + (t.periods_results(slot),) +
                t.chain_results(slot) + t.repeats_results(slot) + t.satellites_results(slot))

    with fresh() as t:  # without any align call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.annotate(ba, motifs)
        t.tracts(ba, motifs, 3)
        t.intervals(ba, motifs, 6, 12, LOG)
        t.variants(ba, motifs)
        t.periods(ba)
        t.chain(ba, motifs, 8 * LOG)
        t.repeats(ba, max_records=LOG)
        t.satellites(ba, 1, 64, max_records=LOG)
        alone = fetch(t)
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # align calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.align(ba, motifs, 3, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.align(bb, [TEL], 5, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.intervals(ba, motifs, 6, 12, LOG, slot=0)
        t.variants(ba, motifs, slot=0)
        t.periods(ba, slot=0)
        t.chain(ba, motifs, 8 * LOG, slot=0)
        t.repeats(ba, max_records=LOG, slot=0)
        t.satellites(ba, 1, 64, max_records=LOG, slot=0)
        t.submit(bb, slot=1)
        got_1 = t.align_results(1)
        got_0 = t.align_results(0)
        got = fetch(t)
        tables = t.collect()
    same(got_0, want_a)
    same(got_1, want_b)
    assert len(got) == len(alone)
    for x, y in zip(got, alone):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_convenience_entry_point():
    import trew_amd

    unit, reads = fuzz_sets()[3]
    same(trew_amd.align(reads, [unit], penalty=7), capi.align_host(reads, [unit], 7))
    same(trew_amd.align(reads, [unit]), capi.align_host(reads, [unit], 3))  # the default penalty is 3


# ---- the `trew align` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


expected_cli = R.cli_lines


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_cli_generator_long_reads_with_noisy_tails(tmp_path, tails):
    reads, host3 = tails
    path = str(tmp_path / "tails.fastq")
    write_fastq(path, reads)
    # rows formatted from the reference itself for the first reads, from the host definition (equal to it) for all
    head = R.align(reads[:4], [TEL], 3)
    same(host3[:4], head)
    want = expected_cli(path, reads, [TEL], host3, 3)
    assert len(want) - 6 >= len(reads)  # every read has its planted tract
    assert run_cli("align", TEL, path, "-t", "2") == want
    assert run_cli("align", TEL, path, "-t", "5") == want
    motifs = [TEL, "AAT"]
    want = expected_cli(path, reads, motifs, capi.align_host(reads, motifs, 7), 7, min_score=200)
    assert 10 <= len(want) - 8 <= 60
    assert run_cli("align", ",".join(motifs), path, "--penalty", "7", "--min_score", "200", "-t", "3") == want
