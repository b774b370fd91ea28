"""Telomere variant repeats on the GPU (trew_hip_variants through ctypes) against the brute-force reference of
variant_ref.py: every record and both batch histograms, integer for integer.  The large cases are compared with
trew_variants_host, which test_variants_cpu.py checks against the same reference."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as A
import interval_ref as I
import oracle as O
import tract_ref as T
import variant_ref as R
from variant_cases import MOTIFS, noisy_reads, same
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
GOLDEN_LONG = os.path.join(ROOT, "tests", "golden", "test_long.fastq")
TEL = "TTAGGG"
K31 = MOTIFS[6]
K32 = MOTIFS[7]
# the kernel's iteration covers 63 words (seams at bases 2016 and 4032); 2048 and 4096 are those of a 64-word iteration
SEAMS = (32, 64, 2016, 2048, 4032, 4096)


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_variants(reads, motifs, mode=capi.MODE_SHORT):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.variants(t.host_batch(words, offsets, lengths), motifs)
        return t.variants_results()


def check(got, want):
    """got = (records, hist, reads_with); want the same three (a fourth element is ignored)"""
    same(got[0], want[0])
    assert (got[1] == want[1]).all(), "hist differs at (motif, strand, bin) %s" % np.argwhere(got[1] != want[1])[0].tolist()
    assert (got[2] == want[2]).all(), "reads_with differs at (motif, strand, bin) %s" % np.argwhere(got[2] != want[2])[0].tolist()


def short_reads(n=20000):
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, 150)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def long_reads(n):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def other_base(c, rnd=None):
    return rnd.choice([x for x in "ACGT" if x != c]) if rnd else ("C" if c != "C" else "A")


def subst(unit, j, c):
    return unit[:j] + c + unit[j + 1:]


# ---- seams
def seam_read(unit, p, anchors, rnd, after=4):
    """A perfect repeat of `unit` behind p mod k bases of filler, whose unit at base p carries one substitution.  anchors:
    'both', 'fwd' (the unit in front is spoiled by a C, so only the window at p + k anchors) or 'back'."""
    k = len(unit)
    o, a = p % k, p // k
    units = [unit] * (a + 1 + after)
    j = rnd.randrange(k)
    units[a] = subst(unit, j, other_base(unit[j], rnd))
    spoil = a - 1 if anchors == "fwd" else a + 1 if anchors == "back" else None
    if spoil is not None and spoil >= 0:
        units[spoil] = subst(unit, k // 2, other_base(unit[k // 2]))
    return "".join(rnd.choice("ACGT") for _ in range(o)) + "".join(units)


def seam_reads(unit):
    rnd = random.Random(len(unit))
    k = len(unit)
    reads = []
    for S in SEAMS:
        for p in (S - 2, S - 1, S, S + 1, S - k // 2, 2047 if S == 2048 else S + 31):
            for anchors in ("both", "fwd", "back"):
                reads.append(seam_read(unit, p, anchors, rnd))
    # the read-end pair: the forward anchor is the last window (i + k = n - k), and the read one base shorter; the read end
    # at and next to a word seam and an iteration seam
    for n in (63, 64, 65, 2015, 2016, 2017, 2047, 2048, 2049):
        if n < 2 * k:
            continue
        full = seam_read(unit, n - 2 * k, "fwd", rnd, after=1)
        assert len(full) == n
        reads += [full, full[:-1]]
    return reads


@pytest.mark.parametrize("unit", ["AAT", TEL, K31, K32], ids=["k3", "k6", "k31", "k32"])
def test_seams(unit):
    reads = seam_reads(unit)
    want = R.variants(reads, [unit])
    # the reference sees what the construction meant: a variant in every read except the shortened ones of the read-end pairs
    nv = want[0]["variants_fwd"][:, 0]
    assert (nv[:len(SEAMS) * 18] >= 1).all()
    pairs = nv[len(SEAMS) * 18:]
    assert len(pairs) >= 12 and (pairs[0::2] >= 1).all() and (pairs[1::2] == pairs[0::2] - 1).all()
    for r in (0, 1, 2, len(reads) - 2, len(reads) - 1):
        assert tuple(int(x) for x in want[0][r, 0]) == R.variants_read(reads[r], unit)[0]
    check(gpu_variants(reads, [unit]), want)
    # the same seams on the reverse strand
    rc = [R.revcomp(r) for r in reads]
    want_rc = R.variants(rc, [unit])
    assert (want_rc[1][:, 1] == want[1][:, 0]).all()
    check(gpu_variants(rc, [unit]), want_rc)


def test_k32_anchor_two_words_on():
    """k = 32, the variant window at bit 31 of a word: its forward anchor is bit 31 of the next word and reaches into the
    word after that; the backward anchor is spoiled"""
    rnd = random.Random(5)
    reads = [seam_read(K32, 32 * w + 31, "fwd", rnd) for w in (0, 1, 61, 62, 63, 64, 125, 126)]
    want = R.variants(reads, [K32])
    assert (want[0]["variants_fwd"][:, 0] >= 1).all()
    check(gpu_variants(reads, [K32]), want)


# ---- bins
def all_bins_read(unit, repeat=lambda b: 1):
    """every variant bin of `unit` in one read, each variant unit between two exact units; repeat(bin) copies of it"""
    parts, bins = [unit], []
    for j in range(len(unit)):
        for c in "TGCA":
            if c != unit[j]:
                b = R.bin_of(j, c)
                bins.append(b)
                parts += [subst(unit, j, c), unit] * repeat(b)
    return "".join(parts), bins


@pytest.mark.parametrize("unit", [TEL, K32], ids=["k6", "k32"])
def test_every_bin_on_both_strands(unit):
    k = len(unit)
    read, bins = all_bins_read(unit)
    assert len(bins) == 3 * k
    tie, _ = all_bins_read(unit, lambda b: 3 if b in (bins[5], bins[-2]) else 1)   # two bins tie at the top
    skew, _ = all_bins_read(unit, lambda b: 1 + b % 3)
    reads = [read, tie, skew, R.revcomp(read), R.revcomp(tie), R.revcomp(skew)]
    want = R.variants(reads, [unit])
    rec, hist, _, per_read = want
    for r, s in ((0, 0), (3, 1)):  # every bin exactly once: all 3 k non-zero, the smallest bin is top
        sfx = "_fwd" if s == 0 else "_rev"
        assert int(rec["distinct" + sfx][r, 0]) == 3 * k and int(rec["top" + sfx][r, 0]) == min(bins) and int(rec["top_count" + sfx][r, 0]) == 1
        assert sorted(np.flatnonzero(per_read[r, 0, s]).tolist()) == sorted(bins)
    assert int(rec["top_fwd"][1, 0]) == min(bins[5], bins[-2]) and int(rec["top_count_fwd"][1, 0]) == 3
    assert int(rec["top_rev"][4, 0]) == min(bins[5], bins[-2]) and int(rec["top_count_rev"][4, 0]) == 3
    check(gpu_variants(reads, [unit]), want)
    for r in range(len(reads)):  # per-read histograms: one read per call
        check(gpu_variants([reads[r]], [unit]), R.variants([reads[r]], [unit]))


# ---- reduction
def test_histogram_of_many_copies():
    read, _ = all_bins_read(TEL, lambda b: 1 + b % 4)
    read = "ACGTACGT" + read + R.revcomp(subst(TEL, 1, "C") + TEL)
    one = R.variants([read], [TEL, "TTAGGC"])
    assert one[1][0, 0].sum() >= 18 and one[1][0, 1].sum() >= 1 and one[1][1].sum() >= 1
    got = gpu_variants([read] * 4096, [TEL, "TTAGGC"])
    assert (got[0] == one[0][0]).all()
    assert (got[1] == 4096 * one[1]).all() and (got[2] == 4096 * one[2]).all()


def test_clean_reads_after_rich_ones():
    """20 000 short reads, more than the grid has waves, rich and clean in a random order: whatever the number of waves, most
    of them meet a clean read behind a rich one and must find their bins empty"""
    rnd = random.Random(99)
    rich = []
    for i in range(16):
        units = [TEL if rnd.random() < 0.6 else subst(TEL, rnd.randrange(6), rnd.choice("ACGT")) for _ in range(25)]
        s = "".join(units)
        rich.append(s if i % 2 else R.revcomp(s))
    clean = ["".join(rnd.choice("AC") for _ in range(150)) for _ in range(16)]  # no T, no G: no unit on either strand
    pick = [(rnd.random() < 0.5, rnd.randrange(16)) for _ in range(20000)]
    reads = [(rich if is_rich else clean)[i] for is_rich, i in pick]
    want_rich = R.variants(rich, [TEL])
    assert (want_rich[0]["variants_fwd"][1::2, 0] >= 3).all() and (want_rich[0]["variants_rev"][0::2, 0] >= 3).all()
    rec, hist, reads_with = gpu_variants(reads, [TEL])
    zero = np.zeros(1, dtype=R.VARIANT_DTYPE)
    zero["top_fwd"] = zero["top_rev"] = R.NONE
    want_hist = np.zeros((1, 2, R.BINS), dtype=np.uint64)
    want_with = np.zeros_like(want_hist)
    for r, (is_rich, i) in enumerate(pick):
        assert rec[r, 0] == (want_rich[0][i, 0] if is_rich else zero[0]), r
        if is_rich:
            want_hist += want_rich[3][i]
            want_with += want_rich[3][i] != 0
    assert (hist == want_hist).all() and (reads_with == want_with).all()


def test_consecutive_calls_do_not_add_up():
    reads = noisy_reads(200, seed=8)
    want = R.variants(reads, MOTIFS[:3])
    few = R.variants(reads[:7], [TEL])
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads(reads))
        t.variants(b, MOTIFS[:3])
        t.variants(b, MOTIFS[:3])
        check(t.variants_results(), want)
        check(t.variants_results(), want)  # reading twice changes nothing
        t.variants(t.host_batch(*capi.pack_reads(reads[:7])), [TEL])  # fewer reads and motifs than the call before
        check(t.variants_results(), few)
        t.variants(t.host_batch(*capi.pack_reads([])), [TEL])  # no reads: no records, empty histograms
        rec, hist, reads_with = t.variants_results()
        assert rec.shape == (0, 1) and hist.sum() == 0 and reads_with.sum() == 0


def test_degenerate_reads():
    rep = TEL * 700
    reads = ["", "T", "TTAGG", "N" * 31, "N" * 5000, "", "T" * 40, "G" * 5000, "A" * 33, TEL, TEL + "TCAGGG", "",
             rep[:2016] + "N" + rep[2017:], rep[:2048] + "N" + rep[2049:], "ttagggTCAGGGttaggg", "n" * 7 + (TEL * 5).lower() + "N"]
    motifs = [TEL, "TTT", "GGGG", "A" * 32]
    want = R.variants(reads, motifs)
    assert int(want[0]["units_fwd"][6, 1]) == 38 and int(want[0]["units_rev"][8, 1]) == 31  # homopolymer motifs on homopolymers
    check(gpu_variants(reads, motifs), want)


# ---- against the reference at large
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
def test_fuzz(seed):
    reads, motifs = fuzz_case(seed)
    want = R.variants(reads, motifs)
    assert (want[1].sum(axis=(1, 2)) >= 10).all()
    check(gpu_variants(reads, motifs), want)


def test_eight_motifs_in_one_call():
    reads = noisy_reads()
    want = R.variants(reads, MOTIFS)
    for m in range(len(MOTIFS)):
        assert want[1][m, 0].sum() >= 5 and want[1][m, 1].sum() >= 5
    check(gpu_variants(reads, MOTIFS), want)
    # a self-reverse-complementary motif: strand rev is strand fwd under (j, c) -> (k-1-j, 3-c)
    rec, hist, _ = gpu_variants(reads, ["AAATTT"])
    assert hist[0, 0].sum() > 0 and (rec["units_fwd"] == rec["units_rev"]).all()
    assert all(hist[0, 1, 4 * (5 - j) + (3 - c)] == hist[0, 0, 4 * j + c] for j in range(6) for c in range(4))


def test_generator_long_reads_device_resident():
    n = 2000
    reads = long_reads(n)
    want = capi.variants_host(capi.pack_reads(reads), [TEL])
    assert want[1][0, 0].sum() >= 300 and want[1][0, 1].sum() >= 300
    head = R.variants(reads[:40], [TEL])
    same(want[0][:40], head[0])  # the host twin itself against the reference
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        b.max_length = 0  # unknown longest read
        t.variants(b, [TEL])
        rec, hist, reads_with, ms = t.variants_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    check((rec, hist, reads_with), want)


# ---- batch plumbing
@pytest.fixture(scope="module")
def uniform150():
    reads = short_reads(4000)  # text from the generator, packed on the host
    want = R.variants(reads, [TEL, "CCCTAA"])
    assert want[0]["units_fwd"][:, 0].sum() >= 500 and want[0]["units_rev"][:, 0].sum() >= 500
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
        t.variants(b, [TEL, "CCCTAA"])
        got = t.variants_results()
        if d is not None:
            t.free(d)
    check(got, want)


def test_ragged_contiguous_with_variants():
    """the generator's short reads hold few variants: the ragged shapes again on reads that are full of them"""
    reads = noisy_reads(300, seed=4)
    want = R.variants(reads, MOTIFS[:4])
    assert want[1].sum() >= 100
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx() as t:
        t.variants(t.host_batch(words, offsets, lengths, contiguous=True), MOTIFS[:4])
        check(t.variants_results(), want)


def test_pair_mode_context_and_two_slots():
    reads = noisy_reads(400, seed=6)
    a, b = reads[:250], reads[250:]
    want_a, want_b = R.variants(a, [TEL, "AAT"]), R.variants(b, [K32])
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.variants(ba, [TEL, "AAT"], slot=0)
        t.variants(bb, [K32], slot=1)
        check(t.variants_results(1), want_b)
        check(t.variants_results(0), want_a)


# ---- independence
def test_independent_of_scan_and_the_other_kernels():
    reads = short_reads(12000)
    a, b = reads[:7000], reads[7000:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = R.variants(a, motifs), R.variants(b, motifs)
    BIG = 1 << 16
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        # without any variants call
        t.annotate(ba, motifs)
        alone_a = t.annotate_results()
        t.tracts(ba, motifs, 3)
        alone_t = t.tracts_results()
        t.intervals(ba, motifs, 6, 12, BIG)
        alone_i = t.intervals_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        # everything interleaved on slot 0, variants and a scan on slot 1; nothing collected until the end
        t.submit(ba, slot=0)
        t.variants(ba, motifs, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.variants(bb, motifs, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.intervals(ba, motifs, 6, 12, BIG, slot=0)
        t.submit(bb, slot=1)
        got_v1 = t.variants_results(1)
        got_v0 = t.variants_results(0)
        got_a = t.annotate_results(0)
        got_t = t.tracts_results(0)
        got_i = t.intervals_results(0)
        tables = t.collect()
    check(got_v0, want_a)
    check(got_v1, want_b)
    assert (got_a == alone_a).all() and (alone_a == A.annotate(a, motifs)).all()
    assert (got_t == alone_t).all() and (alone_t == T.tracts(a, motifs, 3)).all()
    assert (got_i[0] == alone_i[0]).all() and (got_i[1] == alone_i[1]).all() and got_i[2] == alone_i[2]
    assert (alone_i[0] == I.intervals(a, motifs, 6, 12)[0]).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_errors():
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads([b"TTAGGGTCAGGG"]))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_variants"):
            t.variants_results()
        t.tracts(b, [TEL], 3)  # a tracts call is no variants call: the buffers are separate
        t.tracts_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_variants"):
            t.variants_results()
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.variants(b, ["AAT"] * 9)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.variants(b, [])
        with pytest.raises(capi.TrewHipError, match=r"k must be in \[3, 32\]"):
            t.variants(b, [capi.Motif(2, 0, 5)])
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.variants(b, [TEL], slot=3)
        # results larger than the caller's buffer: the count is reported, cap records are copied; the histograms may be NULL
        t.variants(b, [TEL, "CCCTAA"])
        n = C.c_uint64(0)
        one = np.zeros(1, dtype=capi.VARIANT_DTYPE)
        assert t.lib.trew_hip_variants_results(t.ctx, 0, one.ctypes.data, 1, C.byref(n), None, None, None) == 0
        assert n.value == 2 and tuple(int(x) for x in one[0]) == (1, 1, 1, 6, 1, 0, 0, 0, R.NONE, 0)
        assert t.lib.trew_hip_variants_results(t.ctx, 0, None, 1, C.byref(n), None, None, None) != 0
        assert b"out must not be null" in t.lib.trew_hip_last_error(t.ctx)


def test_convenience_entry_point():
    import trew_amd

    reads = noisy_reads(100, seed=12)
    check(trew_amd.variants(reads, MOTIFS[:3]), R.variants(reads, MOTIFS[:3]))


# ---- the `trew variants` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)


def read_fastq(path):
    with (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")) as f:
        return f.read().split(b"\n")[1::4]


expected_cli = R.cli_lines


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_cli_golden_long(suffix):
    path = GOLDEN_LONG + suffix
    reads = read_fastq(path)
    assert len(reads) == 10
    want = expected_cli([(path, reads)], [TEL])
    one = run_cli("variants", TEL, path, "-t", "1")
    assert one == want
    assert run_cli("variants", TEL, path, "-t", "8") == one
    # --min_units is honoured: at 1 every read with a chance unit is listed, at 4294967295 none
    low = expected_cli([(path, reads)], [TEL], min_units=1)
    assert len(low) > len(want)
    assert run_cli("variants", TEL, path, "--min_units", "1", "-t", "3") == low
    assert run_cli("variants", TEL, path, "--min_units", "4294967295") == expected_cli([(path, reads)], [TEL], min_units=4294967295)


def test_cli_synthetic_long_two_files_two_motifs(tmp_path):
    """the golden file holds next to no telomere repeat: generator reads with noisy tails, two files, two motifs"""
    reads = long_reads(300)
    pa, pb = str(tmp_path / "a.fastq"), str(tmp_path / "b.fastq.gz")
    write_fastq(pa, reads[:180])
    write_fastq(pb, reads[180:])
    motifs = [TEL, "TTAGGGC"]
    want = expected_cli([(pa, reads[:180]), (pb, reads[180:])], motifs, min_units=50)
    at = want.index(">Variants")
    assert len(want) - at - 2 >= 18 and sum(1 for ln in want[:at] if ln[0].isdigit()) >= 10
    assert run_cli("variants", ",".join(motifs), pa, pb, "--min_units", "50", "-t", "2") == want
    assert run_cli("variants", ",".join(motifs), pa, pb, "--min_units", "50", "-t", "8") == want
