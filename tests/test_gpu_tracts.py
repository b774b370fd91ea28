"""Error-tolerant terminal motif tracts on the GPU (trew_hip_tracts through ctypes) against the brute-force reference of
tract_ref.py.  Every read of every batch is compared, integer for integer."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as A
import oracle as O
import tract_ref as R
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
LONG_N = 300  # see test_tracts_cpu.py: 9 tails and 9 reverse-complemented tails of >= 1500 bases
TEL = "TTAGGG"


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, motif) %s: got %s, want %s" % (
            f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_tracts(reads, motifs, penalty, mode=capi.MODE_SHORT):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.tracts(t.host_batch(words, offsets, lengths), motifs, penalty)
        return t.tracts_results()


def short_reads(n=20000):
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, 150)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def long_reads(n=LONG_N):
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


def noisy(unit, n, rate, rnd):
    s = (unit * (n // len(unit) + 2))[rnd.randint(0, len(unit) - 1):][:n]
    return "".join(rnd.choice([x for x in "ACGT" if x != c]) if rnd.random() < rate else c for c in s)


@pytest.fixture(scope="module")
def ragged():
    reads = ragged_reads()
    motifs = ["AAT", "TGTG", "ACGTT", "TTAGGG"]
    return reads, motifs, {p: R.tracts(reads, motifs, p) for p in (1, 3, 7, 64)}


@pytest.fixture(scope="module")
def generator_long():
    reads = long_reads()
    want = R.tracts(reads, [TEL], 3)
    assert (want["tail_len_fwd"][:, 0] >= 1500).sum() >= 5 and (want["head_len_rev"][:, 0] >= 1500).sum() >= 5
    return reads, want


HAND = [
    (b"TTAGGG" * 5, 3, (30, 30, 30, 30, 30, 0, 0, 0, 0, 0)),
    (b"TTAGGGTTAGGGTCAGGGTTAGGGACGTACGTACGT", 3, (23, 24, 23, 0, 0, 0, 0, 0, 0, 0)),
    (b"ACGTACGTACTTAGGGTTAGGG", 3, (12, 0, 0, 12, 12, 0, 0, 0, 0, 0)),
    (b"TTAGGGTTAGGGACGACGACGATTAGGGTTAGGG", 1, (24, 34, 24, 34, 24, 0, 0, 0, 0, 0)),
    (b"TTAGGGTTAGGGACGACGACGATTAGGGTTAGGG", 3, (24, 12, 12, 12, 12, 0, 0, 0, 0, 0)),
    (b"TTAGGGACACACTTAGGG", 1, (12, 6, 6, 6, 6, 0, 0, 0, 0, 0)),
    (b"TTAGGGTTAGGGTTAGGGNTTAGGGTTAGGG", 3, (30, 31, 30, 31, 30, 0, 0, 0, 0, 0)),
    (b"CCCTAACCCTAACCCTAAGATTACAGATTACA", 3, (0, 0, 0, 0, 0, 18, 18, 18, 0, 0)),
    (b"GATTACATTAGGGTTAGGGTTACGGTTAGGGTTAGGG", 7, (29, 0, 0, 30, 29, 0, 0, 0, 0, 0)),
    (b"TTAGG", 3, (0,) * 10),
]


def test_hand_worked_vectors():
    for penalty in sorted({p for _, p, _ in HAND}):
        rows = [(r, w) for r, p, w in HAND if p == penalty]
        got = gpu_tracts([r for r, _ in rows], [TEL], penalty)
        assert [tuple(int(x) for x in g) for g in got[:, 0]] == [w for _, w in rows]
    assert tuple(int(x) for x in gpu_tracts([b"ACGT" * 4], ["ACGT"], 3)[0, 0]) == (16,) * 10


def boundary_reads(unit, seed):
    """The shapes at which a wave-per-read kernel goes wrong: word (32), iteration (2048) and read ends."""
    rnd = random.Random(seed)
    k = len(unit)

    def junk(n):
        return "".join(rnd.choice("ACGT") for _ in range(n))

    def rep(n):
        return (unit * (n // k + 2))[:n]

    reads = []
    for n in (0, 1, k - 1, k, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 2048 + k - 1, 4095, 4096, 4097, 6200):
        reads.append(rep(n))  # (a) a perfect repeat throughout
        for h in (2040, 2048, 2053):  # (b) a repeat only in the first h or the last h bases
            h = min(h, n)
            reads.append(rep(h) + junk(n - h))
            reads.append(junk(n - h) + rep(h))
        # (c) random sequence with one matching window: over a word edge, an iteration edge, two iterations in, at the end
        for at in (32 - k // 2, 2048 - k // 2, 4096 - k // 2, 32 - k + 1, 2048 - 1, n - k):
            if 0 <= at and at + k <= n:
                s = junk(n)
                reads.append(s[:at] + unit + s[at + k:])
    reads.append("N" * 5000)
    reads.append("N" * 31)
    s = rep(6200)
    reads.append(s[:2048] + "N" + s[2049:])  # the only N at base 2048, inside a repeat
    reads.append(s[:2047] + "N" + s[2048:])
    reads.append(s[:31] + "N" + s[32:4100])
    return [r.encode() for r in reads]


@pytest.mark.parametrize("unit", ["AAT", TEL, "GATTACAGGCTTAACGGTCATTGCAAGCTAGG"], ids=["k3", "k6", "k32"])
def test_boundary_shapes(unit):
    assert len(unit) in (3, 6, 32)
    reads = boundary_reads(unit, len(unit))
    for r in reads[:6] + reads[-3:-2]:  # the numpy reference against the plain-Python one
        assert tuple(int(x) for x in R.tracts([r], [unit], 3)[0, 0]) == R.tracts_read(r, unit, 3)
    for penalty in (1, 3, 64):
        same(gpu_tracts(reads, [unit], penalty), R.tracts(reads, [unit], penalty))


def test_ties_take_the_shorter_tract():
    """Penalty 1: a run of x covered bases, a gap of g uncovered ones and a run of g bring S back to x (head tie), the mirror
    image brings it back to 0 (tail tie).  The equal extremes sit in different words (g = 18, 30) or in different iterations
    (g = 1080, 2400); `pre` moves the first extreme onto and around a word edge."""
    reads, want_head, want_tail = [], [], []
    for pre in (6, 30, 32, 36):
        for g in (18, 30, 1080, 2400):
            first = (TEL * 7)[:pre]
            head = first + "CA" * (g // 2) + (TEL * (g // 6 + 1))[:g]
            reads.append(head)
            want_head.append(pre)
            reads.append(A.revcomp(head))  # the same tie at the 3' end of the other strand
            want_tail.append(pre)
    want = R.tracts(reads, [TEL], 1)
    assert want["head_len_fwd"][0::2, 0].tolist() == want_head  # the tie is there and the reference takes the shorter tract
    assert want["tail_len_rev"][1::2, 0].tolist() == want_tail
    for r in reads[:4]:
        assert tuple(int(x) for x in R.tracts([r], [TEL], 1)[0, 0]) == R.tracts_read(r, TEL, 1)
    same(gpu_tracts(reads, [TEL], 1), want)
    # the tail tie on the forward strand: S falls back to 0 = S(0) in front of a last run of `pre` bases
    tails = [(TEL * (g // 6 + 1))[:g] + "AC" * (g // 2) + "TTAGGG" * (pre // 6) for pre in (6, 30, 36) for g in (18, 30, 1080, 2400)]
    want = R.tracts(tails, [TEL], 1)
    assert want["tail_len_fwd"][:, 0].tolist() == [pre for pre in (6, 30, 36) for g in range(4)]
    same(gpu_tracts(tails, [TEL], 1), want)


def test_running_sum_beyond_32_bits():
    """34 M uncovered bases at penalty 64 take S below -2^31 between a head and a tail tract: the running sum has to be carried
    in 64 bits.  Too large for the Python reference: trew_tracts_host (itself checked against it on every other input) is
    the yardstick here, and the ends are known by construction."""
    read = (TEL * 200 + "A" * 34_000_000 + TEL * 1000).encode()
    assert 64 * 34_000_000 > 2 ** 31
    packed = capi.pack_reads([read])
    want = capi.tracts_host(packed, [TEL], 64)
    assert (int(want["head_len_fwd"][0, 0]), int(want["tail_len_fwd"][0, 0]), int(want["covered_fwd"][0, 0])) == (1200, 6000, 7200)
    words, offsets, lengths = packed
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=16) as t:
        t.tracts(t.host_batch(words, offsets, lengths), [TEL], 64)
        same(t.tracts_results(), want)


@pytest.mark.parametrize("penalty", [1, 3, 7, 64])
def test_ragged(ragged, penalty):
    reads, motifs, want = ragged
    same(gpu_tracts(reads, motifs, penalty), want[penalty])


def test_planted_noisy_tracts_eight_motifs():
    rnd = random.Random(2025)
    u12, u31, u32 = ("".join(rnd.choice("ACGT") for _ in range(k)) for k in (12, 31, 32))
    motifs = ["AAT", "TGTG", "CCCTA", TEL, "GGGTTAG", u12, u31, u32]
    assert [len(m) for m in motifs] == [3, 4, 5, 6, 7, 12, 31, 32]
    reads = []
    for i in range(64):
        n = rnd.randint(1000, 10000)
        unit = motifs[i % 8] if i % 3 else A.revcomp(motifs[i % 8])
        h, t = rnd.randint(0, n // 2), rnd.randint(0, n // 2)
        body = "".join(rnd.choice("ACGTACGTACGTN") for _ in range(n - h - t))
        rate = min(0.05, 0.2 / len(unit))  # a substitution removes k windows: long motifs get fewer of them
        reads.append(noisy(unit, h, rate, rnd) + body + noisy(unit, t, rate, rnd))
    for penalty in (1, 3, 64):
        want = R.tracts(reads, motifs, penalty)
        if penalty == 3:
            for mi in range(8):
                assert max(want["head_len_fwd"][:, mi].max(), want["head_len_rev"][:, mi].max()) >= 200
        same(gpu_tracts(reads, motifs, penalty), want)


def test_generator_long_reads(generator_long):
    reads, want = generator_long
    same(gpu_tracts(reads, [TEL], 3, mode=capi.MODE_LONG), want)


def test_generator_long_reads_device_resident(generator_long):
    reads, want = generator_long
    with ctx(mode=capi.MODE_LONG, reads=LONG_N, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, LONG_N)
        b.max_length = 0  # unknown longest read
        t.tracts(b, [TEL], 3)
        got, ms = t.tracts_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, want)


def test_uniform_short_reads():
    n, L = 20000, 150
    reads = short_reads(n)
    want = R.tracts(reads, [TEL], 3)
    assert (want["covered_fwd"][:, 0] >= 100).sum() >= 50 and (want["covered_rev"][:, 0] >= 100).sum() >= 50
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        t.tracts(t.device_uniform_batch(d, n, L), [TEL], 3)
        got = t.tracts_results()
        t.free(d)
    same(got, want)
    # the same reads as a uniform host batch
    words, offsets, lengths = capi.pack_reads(reads)
    w = np.ascontiguousarray(words, dtype=np.uint32)
    with ctx() as t:
        b = capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0)
        t.tracts(b, [TEL], 3)
        same(t.tracts_results(), want)


def test_independent_of_scan_and_annotate():
    reads = short_reads(12000)
    motifs = [TEL, "CCCTA"]
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        b = t.host_batch(*capi.pack_reads(reads))
        t.tracts(b, motifs, 3)
        alone_t = t.tracts_results()
        t.annotate(b, motifs)
        alone_a = t.annotate_results()
        # scan, tracts, annotate, the same scan again: all queued on the one slot before anything is collected
        t.submit(b)
        t.tracts(b, motifs, 3)
        t.annotate(b, motifs)
        t.submit(b)
        got_t = t.tracts_results()
        got_a = t.annotate_results()
        tables = t.collect()
    same(alone_t, R.tracts(reads, motifs, 3))
    same(got_t, alone_t)
    assert (got_a == alone_a).all() and (alone_a == A.annotate(reads, motifs)).all()
    single = O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in single.values()) > 0
    assert tables == {name: {key: 2 * c for key, c in rows.items()} for name, rows in single.items()}


def test_errors():
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads([b"ACGTACGTAC"]))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_tracts"):
            t.tracts_results()
        t.annotate(b, ["ACG"])  # an annotate is no tracts call: the buffers are separate
        t.annotate_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_tracts"):
            t.tracts_results()
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.tracts(b, [TEL], penalty)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.tracts(b, ["AAT"] * 9)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.tracts(b, [])
        with pytest.raises(capi.TrewHipError, match=r"k must be in \[3, 32\]"):
            t.tracts(b, [capi.Motif(2, 0, 5)])
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.tracts(b, [TEL], slot=3)
        # results larger than the caller's buffer: the count is reported, cap records are copied
        t.tracts(b, ["ACG", "CGT"], 3)
        n = C.c_uint64(0)
        one = np.zeros(1, dtype=capi.TRACT_DTYPE)
        assert t.lib.trew_hip_tracts_results(t.ctx, 0, one.ctypes.data, 1, C.byref(n), None) == 0
        assert n.value == 2 and tuple(int(x) for x in one[0]) == R.tracts_read(b"ACGTACGTAC", "ACG", 3)


def test_convenience_entry_point(ragged):
    import trew_amd

    reads, motifs, want = ragged
    same(trew_amd.tracts(reads[:300], motifs, penalty=7), want[7][:300])
    same(trew_amd.tracts(reads[:300], motifs), want[3][:300])  # the default penalty is 3


# ---- the `trew tracts` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)


expected_cli = R.cli_lines


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("suffix", [".fastq", ".fastq.gz"])
def test_cli_synthetic_long(tmp_path, generator_long, suffix):
    reads, want3 = generator_long
    path = str(tmp_path / ("long" + suffix))
    write_fastq(path, reads)
    want = expected_cli(path, reads, [TEL], want3)
    assert len(want) - 4 >= 18  # rows: the reads with a planted tail and a few chance tracts of 24 bases
    assert run_cli("tracts", TEL, path, "-t", "2") == want
    assert run_cli("tracts", TEL, path, "-t", "8") == want
    if suffix == ".fastq":  # two motifs, another penalty, a threshold of its own
        motifs = [TEL, "AAT"]
        want = expected_cli(path, reads, motifs, R.tracts(reads, motifs, 7), min_tract=1500)
        assert 10 <= len(want) - 5 <= 40
        assert run_cli("tracts", ",".join(motifs), path, "--penalty", "7", "--min_tract", "1500", "-t", "3") == want
