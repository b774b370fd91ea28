"""Per-read motif annotation on the GPU (trew_hip_annotate through ctypes) against the brute-force reference of annot_ref.py.
Every read of every batch is compared, integer for integer; both kernels (lane per read, wave per read) see every workload."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as R
import oracle as O
from trew_amd import capi
from conftest import GOLDEN, read_fastq

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
PATHS = [pytest.param(0, id="lane"), pytest.param(capi.FLAG_DEBUG_ANNOT_GENERAL, id="wave")]


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, motif) %s: got %s, want %s" % (
            f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def ctx(flags=0, mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, flags=flags, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_annotate(reads, motifs, flags=0, mode=capi.MODE_SHORT, contiguous=False):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(flags, mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.annotate(t.host_batch(words, offsets, lengths, contiguous=contiguous), motifs)
        return t.annotate_results()


def short_reads(n=20000):
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, 150)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def long_reads(n=200):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def ragged_reads(n=2000):
    rnd = random.Random(77)
    out = []
    for i in range(n):
        ln = rnd.randint(0, 1000)
        if i % 3 == 0:
            unit = rnd.choice(["TTAGGG", "CCCTAA", "AAT", "TGTG", "ACGTT"])
            s = (unit * (ln // len(unit) + 2))[rnd.randint(0, 5):][:ln]
            s = "".join(rnd.choice("ACGTNacgtn") if rnd.random() < 0.02 else c for c in s)
        else:
            s = "".join(rnd.choice("ACGTACGTACGTACGTNacgtnR") for _ in range(ln))
        out.append(s.encode())
    return out


def eight_motifs(reads):
    """k = 3, 4, 5, 6, 7, 12, 31, 32; the long ones are cut from the reads so that they match somewhere"""
    def cut(k):
        for r in reads:
            s = r[:k].decode().upper()
            if len(s) == k and set(s) <= set("ACGT"):
                return s
        raise AssertionError("no clean read")
    return ["AAT", "TGTG", "CCCTA", "TTAGGG", "GGGTTAG", cut(12), cut(31), cut(32)]


@pytest.mark.parametrize("flags", PATHS)
def test_short_one_motif(flags):
    reads = short_reads()
    want = R.annotate(reads, ["TTAGGG"])
    assert (want["tract_len_fwd"] >= 24).sum() >= 50 and (want["tract_len_rev"] >= 24).sum() >= 50
    same(gpu_annotate(reads, ["TTAGGG"], flags), want)


@pytest.mark.parametrize("flags", PATHS)
def test_short_eight_motifs(flags):
    reads = short_reads()
    motifs = eight_motifs(reads)
    want = R.annotate(reads, motifs)
    for mi in range(len(motifs)):
        assert want["windows_fwd"][:, mi].sum() > 0
    same(gpu_annotate(reads, motifs, flags), want)


@pytest.mark.parametrize("flags", PATHS)
def test_ragged(flags):
    reads = ragged_reads()
    motifs = ["TTAGGG", "AAT", "TGTG", "AAAA", "ACGTT"]
    # the longest read has more than 256 bases: both contexts take the wave-per-read kernel here; the lane kernel gets
    # the same reads cut to 256 and to 160 bases below
    same(gpu_annotate(reads, motifs, flags), R.annotate(reads, motifs))
    for cap in (256, 160):
        cut = [r[:cap] for r in reads]
        same(gpu_annotate(cut, motifs, flags), R.annotate(cut, motifs))


@pytest.mark.parametrize("flags", PATHS)
def test_long(flags):
    reads = long_reads()
    motifs = ["TTAGGG", "AAT"]
    want = R.annotate(reads, motifs)
    assert want["tract_len_fwd"][:, 0].max() >= 24 and want["tract_len_rev"][:, 0].max() >= 24
    same(gpu_annotate(reads, motifs, flags), want)


def edge_cases():
    rnd = random.Random(11)

    def junk(n):
        return "".join(rnd.choice("ACGT") for _ in range(n))

    tel = "TTAGGG"
    cases = []
    # a tract that ends with the last base
    for n in (40, 150, 160, 256, 300):
        cases.append((junk(n - 30) + tel * 5, tel))
    # tracts that cross bit 31/32, 63/64, 159/160, 255/256
    for edge in (32, 64, 160, 256):
        for before in (1, 5, 17):
            s = junk(edge - before) + tel * 6
            cases.append((s + junk(7), tel))
            cases.append((s, tel))
    # two tracts of equal length: the earliest wins
    cases.append((tel * 4 + "N" + tel * 4 + junk(9), tel))
    cases.append((junk(3) + tel * 4 + "ACAC" + tel * 4, tel))
    cases.append((junk(100) + tel * 5 + "C" + tel * 5 + junk(200), tel))
    # a tract cut by one N
    cases.append((tel * 6 + "N" + tel * 9, tel))
    cases.append((tel * 12 + "N" + tel * 12 + junk(150) + tel * 40, tel))
    # read lengths around k, the word edges and the kernels' limits
    for k, unit in ((6, tel), (3, "AAT"), (32, junk(32))):
        for n in (k - 1, k, k + 1, 32, 33, 160, 161, 256, 257, 1000):
            cases.append(((unit * (n // k + 2))[2:2 + n], unit))
            cases.append((junk(n), unit))
    # k = 3 and k = 32 inside junk
    cases.append((junk(50) + "AAT" * 20 + junk(31), "AAT"))
    u32 = junk(32)
    cases.append((junk(70) + u32 * 3 + junk(5), u32))
    # self-reverse-complementary, non-primitive, homopolymer
    cases.append((junk(10) + "ACGT" * 9 + junk(10), "ACGT"))
    cases.append((junk(10) + "AATT" * 9 + junk(300), "AATT"))
    cases.append((junk(20) + "TGTG" * 10 + junk(20), "TGTG"))
    cases.append((junk(20) + "TG" * 21 + junk(20), "TGTG"))
    cases.append((junk(20) + "A" * 40 + junk(20) + "T" * 50, "AAAA"))
    cases.append(("A" * 1000, "AAA"))
    cases.append(("A" * 256, "AAA"))
    cases.append(("T" * 160, "AAAAA"))
    # whole words of matches: runs that cover several lanes of the wave-per-read kernel, and more than 64 words
    cases.append((junk(13) + tel * 700 + junk(40), tel))
    cases.append((tel * 1200, "CCCTAA"))
    cases.append(("N" + "AT" * 2100 + "N" + "AT" * 2100, "ATAT"))
    return cases


@pytest.mark.parametrize("flags", PATHS)
def test_edge_reads(flags):
    cases = edge_cases()
    by_motif = {}
    for read, motif in cases:
        by_motif.setdefault(motif, []).append(read.encode())
    for motif, reads in by_motif.items():
        want = R.annotate(reads, [motif])
        for r, w in zip(reads[:4], want[:4]):  # the numpy reference against the plain-Python one
            assert tuple(w[0]) == R.annotate_read(r, motif)
        same(gpu_annotate(reads, [motif], flags), want)
        # cut to the limits of the two lane kernels (NW = 5 and NW = 8): no read of these batches takes the wave kernel by length
        for cap in (160, 256):
            cut = [r[:cap] for r in reads]
            same(gpu_annotate(cut, [motif], flags), R.annotate(cut, [motif]))


def test_hand_worked_vectors():
    tel = "TTAGGG"
    reads = [b"TTAGGG" * 5, b"CCCTAA" * 5 + b"N" + b"TTAGGG" * 3, b"TTAGG", b"GGTTAG"]
    got = gpu_annotate(reads, [tel])
    assert [tuple(x) for x in got[:, 0]] == [(25, 0, 0, 30, 0, 0), (13, 25, 31, 18, 0, 30), (0, 0, 0, 0, 0, 0), (1, 0, 0, 6, 0, 0)]
    assert tuple(gpu_annotate([b"ACGT" * 4], ["ACGT"])[0, 0]) == (13, 13, 0, 16, 0, 16)


@pytest.mark.parametrize("flags", PATHS)
@pytest.mark.parametrize("shape", ["offsets_lengths_words", "words_offsets_lengths", "three_arrays", "uniform_host"])
def test_batch_shapes(shape, flags):
    reads = short_reads(5000)
    motifs = ["TTAGGG", "AAT"]
    want = R.annotate(reads, motifs)
    words, offsets, lengths = capi.pack_reads(reads)
    n = len(reads)
    with ctx(flags) as t:
        if shape == "offsets_lengths_words":
            b = t.host_batch(words, offsets, lengths, contiguous=True)
        elif shape == "words_offsets_lengths":
            buf = np.concatenate([words, offsets, lengths]).astype(np.uint32)
            base = buf.ctypes.data
            b = capi.Batch(base, len(words), base + 4 * len(words), base + 4 * (len(words) + n), 0, 0, n, 0, 0)
            b._keep = (buf,)
        elif shape == "three_arrays":
            b = t.host_batch(words, offsets, lengths)
        else:
            stride = 3 * ((150 + 31) // 32)
            assert (offsets == np.arange(n) * stride).all()
            w = np.ascontiguousarray(words, dtype=np.uint32)
            b = capi.Batch(w.ctypes.data, len(w), None, None, 150, stride, n, 0, 0)
            b._keep = (w,)
        t.annotate(b, motifs)
        same(t.annotate_results(), want)


@pytest.mark.parametrize("flags", PATHS)
def test_uniform_device_resident(flags):
    n, L = 1000000, 150
    stride = 3 * ((L + 31) // 32)
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    packed = capi.pack_reads([buf[s:e + 1] for s, e in zip(st, nd)])
    want = capi.annotate_host(packed, ["TTAGGG"])
    head = R.annotate([buf[s:e + 1] for s, e in zip(st[:20000], nd[:20000])], ["TTAGGG"])
    same(want[:20000], head)  # the host twin itself against the reference
    with ctx(flags, reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.annotate(t.device_uniform_batch(d, n, L), ["TTAGGG"])
        got, ms = t.annotate_results(want_ms=True)
        t.free(d)
    assert ms > 0
    same(got, want)


@pytest.mark.parametrize("flags", PATHS)
def test_long_device_resident(flags):
    n = 300
    reads = long_reads(n)
    want = R.annotate(reads, ["TTAGGG"])
    with ctx(flags, mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        t.annotate(b, ["TTAGGG"])
        got = t.annotate_results()
        b.max_length = 0  # unknown longest read: the wave-per-read kernel
        t.annotate(b, ["TTAGGG"])
        got0 = t.annotate_results()
        for p in ptrs:
            t.free(p)
    same(got, want)
    same(got0, want)


def test_pair_mode_mates_are_two_reads():
    reads = short_reads(2000)
    same(gpu_annotate(reads, ["TTAGGG"], mode=capi.MODE_PAIR), R.annotate(reads, ["TTAGGG"]))


def test_independent_of_the_scan():
    reads = short_reads(20000)
    a, b = reads[:12000], reads[12000:]
    motifs = ["TTAGGG", "CCCTA"]
    want_a, want_b = R.annotate(a, motifs), R.annotate(b, motifs)
    p = O.OracleParams()
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        bb = t.host_batch(*capi.pack_reads(b))
        # serial results first
        t.annotate(ba, motifs, slot=0)
        ser_a = t.annotate_results(0)
        t.annotate(bb, motifs, slot=1)
        ser_b = t.annotate_results(1)
        same(ser_a, want_a)
        same(ser_b, want_b)
        # scan, annotate on both slots, scan again, all queued before anything is collected
        t.submit(ba, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.annotate(bb, motifs, slot=1)
        t.submit(bb, slot=0)
        got_a = t.annotate_results(0)
        got_b = t.annotate_results(1)
        tables = t.collect()
        timing = t.last_timing(0)
    same(got_a, ser_a)
    same(got_b, ser_b)
    assert tables == O.run_short(p, reads)
    assert timing[0] > 0 and timing[1] > 0


def test_errors():
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads([b"ACGTACGTAC"]))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_annotate"):
            t.annotate_results()
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.annotate(b, ["TTAGGG"], slot=3)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.annotate(b, ["AAT"] * 9)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.annotate(b, [])
        with pytest.raises(capi.TrewHipError, match=r"k must be in \[3, 32\]"):
            t.annotate(b, [capi.Motif(2, 0, 5)])
        with pytest.raises(capi.TrewHipError, match="bits above 2k"):
            t.annotate(b, [capi.Motif(3, 0, 1 << 6)])
        # results larger than the caller's buffer: the count is reported, cap records are copied
        t.annotate(b, ["ACG", "CGT"])
        n = C.c_uint64(0)
        one = np.zeros(1, dtype=capi.ANNOT_DTYPE)
        assert t.lib.trew_hip_annotate_results(t.ctx, 0, one.ctypes.data, 1, C.byref(n), None) == 0
        assert n.value == 2 and tuple(one[0]) == R.annotate_read(b"ACGTACGTAC", "ACG")


def test_convenience_entry_point():
    import trew_amd

    reads = short_reads(300)
    same(trew_amd.annotate(reads, ["TTAGGG"]), R.annotate(reads, ["TTAGGG"]))


# ---- the `trew annotate` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)


def expected_cli(path, reads, motifs, min_tract=None):
    """stdout of `trew annotate`, formatted from the reference"""
    return R.cli_lines(path, reads, motifs, R.annotate(reads, motifs), min_tract)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("suffix", [".fastq", ".fastq.gz"])
@pytest.mark.parametrize("kind", ["short", "long"])
def test_cli_synthetic(tmp_path, kind, suffix):
    reads = short_reads() if kind == "short" else long_reads()
    path = str(tmp_path / (kind + suffix))
    write_fastq(path, reads)
    want = expected_cli(path, reads, ["TTAGGG"])
    assert len(want) - 4 >= (300 if kind == "short" else 5)  # rows: 171 + 156 reads of the short file, a dozen long reads
    for threads in ("2", "8"):
        assert run_cli("annotate", "TTAGGG", path, "-t", threads) == want


@pytest.mark.parametrize("name,aat,tel", [("test.fastq", 11, 0), ("test.fastq.gz", 11, 0), ("test_long.fastq", 3, 1), ("test_long.fastq.gz", 3, 1)])
def test_cli_fixtures(name, aat, tel):
    """The bundled fixtures hold no telomeric tract.  By the brute-force reference, at --min_tract 9 AAT reports 11 of the 100
    reads of test.fastq (246 bases each: the NW = 8 lane kernel) and 3 of the 10 of test_long.fastq; TTAGGG reports none in
    test.fastq (an empty motif section) and one read in test_long.fastq, whose GGGTTAGGG at base 570 is four windows = 9 bases."""
    path = os.path.join(GOLDEN, name)
    reads = read_fastq(path)
    want = expected_cli(path, reads, ["AAT", "TTAGGG"], min_tract=9)
    assert sum(",AAT," in w for w in want[2:-4]) == aat and sum(",TTAGGG," in w for w in want[2:-4]) == tel
    assert len(want) == 2 + aat + tel + 4
    for threads in ("2", "8"):
        assert run_cli("annotate", "AAT,TTAGGG", path, "--min_tract", "9", "-t", threads) == want
