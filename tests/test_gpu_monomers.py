"""Wraparound alignment for units of up to 256 bases on the GPU (trew_hip_monomers through ctypes) against trew_monomers_host
(which tests/test_monomers_cpu.py checks against the brute-force definition and the numpy form of monomer_ref.py).  Every read
of every batch is compared, field for field.  The shapes are the smallest at which monomers_wave_kernel<Q> can go wrong: both
ends of each Q, every k mod Q, a last lane with one live slot, reads around k, around a word and around the 64-word seam."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_cases as AC
import monomer_cases as MC
import monomer_ref as R
import oracle as O
from align_cases import revcomp, rotations, with_deletion, with_insertion
from monomer_cases import q_of, unit_of
from period_cases import junk, noisy, rep
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, unit) %s: got %s, want %s" % (f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def rec(x):
    return tuple(int(v) for v in x)


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18, flags=0):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16, flags=flags)


def gpu(reads, units, penalty=3, mode=capi.MODE_SHORT, flags=0):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16), flags=flags) as t:
        t.monomers(t.host_batch(words, offsets, lengths), units, penalty)
        return t.monomers_results()


def check(reads, units, penalties=(1, 3, 64), **kw):
    for penalty in penalties:
        same(gpu(reads, units, penalty, **kw), capi.monomers_host(reads, units, penalty))


def shape_reads(unit, seed):
    """read lengths around the unit, a word and the 64-word seam: perfect, shifted by one phase, noisy, random with N; one
    deleted and one inserted base at bits 31 and 0 of a word, at the 64-word seam, and where the tract's phase is 0, Q - 1, Q,
    k - 1"""
    rnd = random.Random(seed)
    k, q = len(unit), q_of(len(unit))
    lens = [0, 1, k - 1, k, k + 1, 31, 32, 33, 2 * k + 5] + ([2047, 2048, 2049] if k in (33, 171, 256) else [])
    reads = []
    for n in lens:
        reads += [rep(unit, n), rep(unit, n, 1 % k), noisy(rnd, unit, n, 0.03, 0.06, 0.005), junk(rnd, n, "ACGTN")]
    base = rep(unit, 2200)
    for at in (31, 32, 63, 64, 2047, 2048):
        reads += [with_deletion(base, at), with_insertion(base, at, "ACGT"[(at + 1) % 4]), with_insertion(with_deletion(base, at), at + 40, "A")]
    base = rep(unit, 5 * k + 7)
    for phase in sorted({0, q - 1, q, k - 1}):
        at = 2 * k + phase
        other = next(b for b in "ACGT" if b != base[at])
        reads += [with_deletion(base, at), with_insertion(base, at, other)]
    return reads


@pytest.mark.parametrize("k", MC.GPU_KS)
def test_unit_and_read_lengths(k):
    check(shape_reads(unit_of(k, 1), k), [unit_of(k, 1)])


@pytest.mark.parametrize("k", MC.GPU_KS)
def test_runs_of_deleted_and_inserted_bases(k):
    """d unit bases deleted in a row, starting where the run crosses phase k - 1 -> 0, where it crosses a lane seam and at
    phase 0; d = k leaves no trace; runs of inserted bases of the same lengths"""
    unit, q = unit_of(k, 2), q_of(k)
    ds = sorted({d for d in (1, q - 1, q, q + 1, 63, 64, 65, k - 2, k - 1, k) if 1 <= d <= k})
    reads, whole = [], []
    for d in ds:
        for phase in sorted({(k - (d + 1) // 2) % k, min(3 * q + q - 1, k - 1), 0}):
            if d == k:
                whole.append(len(reads))
            reads.append(MC.with_deleted_run(unit, phase, d, lead="NN", tail="N"))
            reads.append(MC.with_inserted_run(unit, phase, junk(random.Random(d), d), lead="N"))
    want = capi.monomers_host(reads, [unit], 1)
    for i in whole:  # k deleted bases: a perfect repeat
        n = len(reads[i]) - 3
        assert rec(want[i, 0])[:5] == (n, 2, 2 + n, n, n)
    # at P = 1 a run of d is d deletions while 3 d < 2 k (beyond that the k - d bases of the broken copy are cheaper as insertions)
    cols = capi.align_columns(want, k, 1)
    assert int(cols["deletions_fwd"].max()) >= max(d for d in ds if 3 * d < 2 * k) and int(cols["insertions_fwd"].max()) >= 1
    same(gpu(reads, [unit], 1), want)
    check(reads, [unit], (3,))


def test_ties_and_n():
    """Equal scores in two slots of one lane and in two lanes: two equal tracts of less than a copy that end in chosen phases,
    40 N apart (the earlier end wins); zero-sum prefixes at P = 1; an N inside a tract; and reads over a two-letter
    alphabet against a two-letter unit, where equal scores are everywhere."""
    for k in (6, 66, 130):
        unit, q = unit_of(k, 3), q_of(k)
        m = min(k - 2, 40)
        reads = []
        for a, b in ((0, 1), (1, 0), (0, q), (q, 0), (2, k - m), (k - 1, 0), (0, k - 1)):
            reads.append(rep(unit, m, a % k) + "N" * 40 + rep(unit, m, b % k))
        t = rep(unit, 3 * k)
        x, y = next(b for b in "ACGT" if b != unit[k - 1]), next(b for b in "ACGT" if b != unit[0])
        reads += [unit[-1] + x + t, unit[-2:] + x + x + t, t + unit[0] + y, t[:k + 5] + "N" + t[k + 6:], "N" * 5 + t + "N" + t + "NN"]
        reads += [revcomp(r) for r in reads]
        want = capi.monomers_host(reads, [unit], 1)
        for i in range(7):
            assert rec(want[i, 0])[:3] == (m, 0, m)
        check(reads, [unit], (1, 3))
    rnd = random.Random(77)
    for k in (5, 64, 129, 256):
        unit = junk(rnd, k, "AC")
        reads = [junk(rnd, rnd.randint(1, 3 * k), "ACACACN") for _ in range(60)]
        check(reads, [unit], (1, 2))


def test_long_reads_and_fields_beyond_16_bits():
    rnd = random.Random(4)
    u171, u256 = unit_of(171, 1), unit_of(256, 1)
    perfect = rep(u171, 70_000, 2)
    got = gpu([perfect], [u171], 3, mode=capi.MODE_LONG)
    assert rec(got[0, 0])[:5] == (70_000, 0, 70_000, 70_000, 70_000)
    same(got, capi.monomers_host([perfect], [u171], 3))
    noisy_read = (junk(rnd, 3000) + noisy(rnd, u256, 100_000, 0.002, 0.002) + junk(rnd, 500))[:100_000]
    want = capi.monomers_host([noisy_read], [u256], 64)
    assert int(want["score_fwd"][0, 0]) > 1 << 16 and int(want["end_fwd"][0, 0]) - int(want["start_fwd"][0, 0]) > 1 << 16
    same(gpu([noisy_read], [u256], 64, mode=capi.MODE_LONG), want)


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_records_equal_align_up_to_32_bases(penalty):
    words = 1 << 16
    with ctx(words=words, reads=64) as t:
        for unit, reads in AC.fuzz_sets():
            b = t.host_batch(*capi.pack_reads(reads))
            t.align(b, [unit], penalty)
            t.monomers(b, [unit], penalty)
            a = t.align_results()
            same(t.monomers_results(), a)
            same(a, capi.monomers_host(reads, [unit], penalty))


@pytest.mark.parametrize("k", (66, 171, 256))
def test_every_rotation_and_the_other_strand(k):
    rnd = random.Random(k)
    unit = unit_of(k, 4)
    reads = [junk(rnd, 30) + noisy(rnd, unit, 2 * k + 60, 0.03, 0.06, 0.003) + junk(rnd, 20) for _ in range(3)]
    want = capi.monomers_host(reads, [unit], 3)
    rots = rotations(unit)
    for lo in range(0, k, 40):
        got = gpu(reads, rots[lo:lo + 8], 3)
        for m in range(got.shape[1]):
            same(got[:, m:m + 1], want)
    rc = gpu([revcomp(r) for r in reads], [unit], 3)
    assert (rc["score_rev"] == want["score_fwd"]).all() and (rc["score_fwd"] == want["score_rev"]).all()
    cols = capi.align_columns(rc, k, 3)
    assert all((v >= 0).all() for v in cols.values())


def test_eight_monomers_of_mixed_lengths():
    """Q = 4 with small k in it: every monomer of the call runs on the layout the largest one picks"""
    rnd = random.Random(2025)
    units = [unit_of(k, 5) for k in (6, 33, 64, 65, 128, 171, 255, 256)]
    reads = []
    for i in range(32):
        unit = units[i % 8] if i % 3 else revcomp(units[i % 8])
        reads.append(junk(rnd, rnd.randint(0, 60), "ACGTACGTACGTN") + noisy(rnd, unit, rnd.randint(100, 600), 0.03, 0.06, 0.003) + junk(rnd, rnd.randint(0, 60)))
    want = capi.monomers_host(reads, units, 3)
    for mi in range(8):
        assert max(want["score_fwd"][:, mi].max(), want["score_rev"][:, mi].max()) >= 60
    check(reads, units)
    check(reads, units[:5] + [unit_of(3, 5)], (3,))  # Q = 2
    few = sorted(reads, key=len)[:2]
    same(capi.monomers_host(few, units, 3), R.monomers(few, units, 3))


def test_the_array_of_diverged_monomers():
    consensus, read, begin, end, background = MC.diverged_array()
    for penalty in (2, 3):
        same(gpu([read, background], [consensus], penalty), capi.monomers_host([read, background], [consensus], penalty))
    got = gpu([read, background], [consensus], 2)
    assert abs(int(got["start_fwd"][0, 0]) - begin) <= 10 and abs(int(got["end_fwd"][0, 0]) - end) <= 10
    assert max(int(got["score_fwd"][1, 0]), int(got["score_rev"][1, 0])) < 24


def long_reads(n):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def planted_reads(unit, n=24, seed=8):
    """generator long reads, cut to at most 6 kb, with a planted noisy array of the unit of 0.4 - 1.5 kb (one in four
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
    want = capi.monomers_host(reads, [unit], 3)
    assert (np.maximum(want["score_fwd"], want["score_rev"])[:, 0] >= 100).all()  # every planted array is found
    return unit, reads, want


def test_every_batch_shape(planted):
    unit, reads, want = planted
    same(gpu(reads, [unit], 3, mode=capi.MODE_LONG), want)
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=64) as t:
        t.monomers(t.host_batch(words, offsets, lengths, contiguous=True), [unit], 3)
        same(t.monomers_results(), want)
    # device-resident generator reads, the longest read unknown
    full = long_reads(12)
    u66 = unit_of(66, 6)
    with ctx(mode=capi.MODE_LONG, reads=64, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, 12)
        b.max_length = 0
        t.monomers(b, [u66], 3)
        got, ms = t.monomers_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, capi.monomers_host(full, [u66], 3))
    # uniform short reads: device-resident, and host words without offsets and lengths
    n, L = 1500, 150
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    short = [buf[s:e + 1] for s, e in zip(st, nd)]
    units = [unit_of(33, 6), unit_of(130, 6)]
    want_short = capi.monomers_host(short, units, 3)
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.monomers(t.device_uniform_batch(d, n, L), units, 3)
        got = t.monomers_results()
        t.free(d)
    same(got, want_short)
    w = np.ascontiguousarray(capi.pack_reads(short)[0], dtype=np.uint32)
    with ctx() as t:
        t.monomers(capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0), units, 3)
        same(t.monomers_results(), want_short)


def test_pair_mode_two_slots_repeated_calls_and_errors():
    rnd = random.Random(6)
    u40, u70, u200 = unit_of(40, 7), unit_of(70, 7), unit_of(200, 7)
    a = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, u70, rnd.randint(0, 300), 0.03, 0.06, 0.01) for _ in range(100)]
    b = [junk(rnd, rnd.randint(0, 90)) + noisy(rnd, u200, rnd.randint(0, 500), 0.03, 0.06, 0.01) for _ in range(61)]
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_monomers"):
            t.monomers_results()
        t.align(ba, ["TTAGGG"], 3)  # an align call is no monomers call: the buffers are separate
        t.align_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_monomers"):
            t.monomers_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.monomers(t.host_batch(*capi.pack_reads(b)), [u70])
        bb = t.host_batch(*capi.pack_reads(b[:60]))
        t.monomers(ba, [u70, u200], 3, slot=0)  # the mates are two reads; the two slots overlap
        t.monomers(bb, [u200], 7, slot=1)
        got1, got0 = t.monomers_results(1), t.monomers_results(0)
        same(got1, capi.monomers_host(b[:60], [u200], 7))
        same(got0, capi.monomers_host(a, [u70, u200], 3))
        # repeated calls on one slot: more monomers, fewer reads, another penalty and another Q; the last call is what results returns
        t.monomers(bb, [u200, u70, u40], 1, slot=0)
        same(t.monomers_results(0), capi.monomers_host(b[:60], [u200, u70, u40], 1))
        t.monomers(ba, [u40], 64, slot=0)
        same(t.monomers_results(0), capi.monomers_host(a, [u40], 64))
        t.monomers(ba, [u70], 2, slot=0)  # one monomer again, another unit: the staged table is replaced
        same(t.monomers_results(0), capi.monomers_host(a, [u70], 2))
        same(t.monomers_results(0), capi.monomers_host(a, [u70], 2))  # fetching twice changes nothing
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.monomers(ba, [u70], penalty)
        for units in ([u40] * 9, []):
            with pytest.raises(capi.TrewHipError, match=r"n_monomers must be in \[1, 8\]"):
                t.monomers(ba, units)
        zero = (C.c_uint32 * 16)()
        for k in (2, 257):
            with pytest.raises(capi.TrewHipError, match=r"monomer: k must be in \[3, 256\]"):
                t.monomers(ba, [capi.Monomer(k, 0, zero)])
        high = (C.c_uint32 * 16)()
        high[2] = 1
        with pytest.raises(capi.TrewHipError, match="bits at or above base k"):
            t.monomers(ba, [capi.Monomer(32, 0, high)])
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.monomers(ba, [u70], slot=3)
        same(t.monomers_results(0), capi.monomers_host(a, [u70], 2))  # a refused call leaves the last results alone
        # results larger than the caller's buffer: the count is reported, cap records are copied
        t.monomers(ba, [u40, u70], 3)
        n = C.c_uint64(0)
        one = np.zeros(1, dtype=capi.ALIGN_DTYPE)
        assert t.lib.trew_hip_monomers_results(t.ctx, 0, one.ctypes.data, 1, C.byref(n), None) == 0
        assert n.value == 200 and rec(one[0]) == rec(capi.monomers_host(a[:1], [u40], 3)[0, 0])
        assert t.lib.trew_hip_monomers_results(t.ctx, 0, None, 0, C.byref(n), None) == 0 and n.value == 200
        # no reads: no records, no kernel
        t.monomers(t.host_batch(*capi.pack_reads([])), [u70], 3)
        assert t.monomers_results().shape == (0, 1)


@pytest.mark.parametrize("k", (40, 100, 171))
def test_waves_go_well_past_their_first_read(k):
    """TREW_FLAG_DEBUG_ONE_CU: 32 waves for a few thousand short reads, about a hundred reads a wave"""
    rnd = random.Random(k)
    unit = unit_of(k, 8)
    reads = [junk(rnd, rnd.randint(0, 20), "ACGTN") + noisy(rnd, unit, rnd.randint(0, 90), 0.03, 0.06, 0.01) for _ in range(3000)]
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=len(words) + 64, reads=len(reads), flags=capi.FLAG_DEBUG_ONE_CU) as t:
        assert t.debug_measure_grid(len(reads)) == 8
        t.monomers(t.host_batch(words, offsets, lengths), [unit, unit_of(7, 8)], 3)
        same(t.monomers_results(), capi.monomers_host(reads, [unit, unit_of(7, 8)], 3))


def test_independent_of_scan_and_of_align():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 5000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3000], reads[3000:]
    motifs = ["TTAGGG", "CCCTA"]
    units = [unit_of(100, 9), unit_of(36, 9)]

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    with fresh() as t:  # without any monomers call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.align(ba, motifs, 3)
        alone = t.align_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # monomers calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.monomers(ba, units, 3, slot=0)
        t.align(ba, motifs, 3, slot=0)
        t.monomers(bb, units[:1], 5, slot=1)
        t.submit(bb, slot=1)
        got_1 = t.monomers_results(1)
        got_0 = t.monomers_results(0)
        got = t.align_results(0)
        tables = t.collect()
    same(got_0, capi.monomers_host(a, units, 3))
    same(got_1, capi.monomers_host(b, units[:1], 5))
    same(got, alone)
    same(alone, capi.align_host(a, motifs, 3))
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_convenience_entry_point():
    import trew_amd

    unit, reads = MC.host_fuzz()[9]
    assert len(unit) == 171
    same(trew_amd.monomers(reads, [unit], penalty=7), capi.monomers_host(reads, [unit], 7))
    same(trew_amd.monomers(reads, [unit]), capi.monomers_host(reads, [unit], 3))  # the default penalty is 3


# ---- the `trew monomers` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def expected_cli(path, reads, names, units, a, penalty, min_score=24):
    """R.cli_lines prints the motif's text and takes k from its length: hand it stand-ins of the units' lengths, then put the names in"""
    lines = R.cli_lines(path, reads, ["\x00%d\x00" % m + "x" * (len(u) - len("\x00%d\x00" % m)) for m, u in enumerate(units)], a, penalty, min_score)
    for m, (name, u) in enumerate(zip(names, units)):
        stand_in = "\x00%d\x00" % m + "x" * (len(u) - len("\x00%d\x00" % m))
        lines = [ln.replace(stand_in, name) for ln in lines]
    return lines


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_cli_generator_long_reads_with_planted_arrays(tmp_path, planted):
    unit, reads, host3 = planted
    path = str(tmp_path / "arrays.fastq")
    write_fastq(path, reads)
    want = expected_cli(path, reads, [unit], [unit], host3, 3)
    assert len(want) - 6 >= len(reads)  # every read has its planted array
    assert run_cli("monomers", unit, path, "-t", "2") == want
    assert run_cli("monomers", unit.lower(), path, "-t", "5") == [ln.replace(unit, unit.lower()) for ln in want]
    # by --fasta: two records, the first over several lines, names in the motif column; another penalty and threshold
    other = unit_of(48, 6)
    fasta = str(tmp_path / "units.fa")
    with open(fasta, "w") as f:
        f.write(">alpha the 171-mer\n" + unit[:70] + "\n" + unit[70:140] + "\n" + unit[140:] + "\n\n>beta\n" + other + "\n")
    both = capi.monomers_host(reads, [unit, other], 2)
    want = expected_cli(path, reads, ["alpha", "beta"], [unit, other], both, 2, min_score=150)
    assert 10 <= len(want) - 8 <= 60
    assert run_cli("monomers", "--fasta", fasta, path, "--penalty", "2", "--min_score", "150", "-t", "3") == want
    assert run_cli("monomers", unit + "," + other, path, "--penalty", "2", "--min_score", "150") == expected_cli(
        path, reads, [unit, other], [unit, other], both, 2, min_score=150)
