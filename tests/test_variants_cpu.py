"""Telomere variant repeats, the parts that need no GPU: the brute-force reference against hand-worked vectors and against
itself, the host implementation (trew_variants_host) against the reference, the consequences the definition promises, the
additive ABI, the argument errors of `trew variants`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import variant_ref as R
from variant_cases import MOTIFS, noisy_reads, rc_read, same, swapped
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
NONE = R.NONE
Z = (0, 0, 0, NONE, 0)
U, RU = "TTAGGG", "CCCTAA"


HAND = [
    # TTAGGG x 3 + TCAGGG + TTAGGG x 3: six exact units, one variant (1, C) = bin 6, anchored from both sides
    (U * 3 + "TCAGGG" + U * 3, (6, 1, 1, 6, 1), Z),
    # the same on the reverse strand: CCCTGA is TCAGGG read backwards, bin (1, C) again
    (RU * 3 + "CCCTGA" + RU * 3, Z, (6, 1, 1, 6, 1)),
    # two adjacent variant units, each anchored from outside: bins (1, C) = 6 and (1, G) = 5, the tie goes to the smaller bin
    (U * 2 + "TCAGGG" + "TGAGGG" + U * 2, (4, 2, 2, 5, 1), Z),
    # three adjacent variant units: the middle one has no exact neighbour; (1, C) = 6 and (2, G) = 9 remain
    (U * 2 + "TCAGGG" + "TGAGGG" + "TTGGGG" + U * 2, (4, 2, 2, 6, 1), Z),
    # a window with two mismatches is no variant
    (U * 2 + "TCAGCG" + U * 2, (4, 0, 0, NONE, 0), Z),
    # an N in the variant window
    (U * 2 + "TNAGGG" + U * 2, (4, 0, 0, NONE, 0), Z),
    # an N in the only anchor window: the variant is not anchored; without the N it is
    ("TTAGNG" + "TCAGGG" + "ACGTAC", Z, Z),
    ("TTAGGG" + "TCAGGG" + "ACGTAC", (1, 1, 1, 6, 1), Z),
    # the forward anchor is the last window of the read (i + k = n - k); one base shorter it does not exist
    ("TCAGGG" + "TTAGGG", (1, 1, 1, 6, 1), Z),
    ("TCAGGG" + "TTAGG", Z, Z),
    # a backward anchor at window 0
    ("TTAGGG" + "TCAGGG", (1, 1, 1, 6, 1), Z),
    # n < k, and an empty read
    ("TTAGG", Z, Z),
    ("", Z, Z),
    # lower-case bases are bases
    ("ttagggTCAGGGttaggg", (2, 1, 1, 6, 1), Z),
    # an unanchored exact unit counts as a unit; an unanchored variant does not count
    ("ACGTACTTAGGGACGTACTCAGGGACGTAC", (1, 0, 0, NONE, 0), Z),
]


@pytest.mark.parametrize("read,fwd,rev", HAND)
def test_hand_worked_vectors(read, fwd, rev):
    want = fwd + rev
    rec, _ = R.variants_read(read, U)
    assert rec == want
    assert tuple(int(x) for x in R.variants([read], [U])[0][0, 0]) == want
    assert tuple(int(x) for x in capi.variants_host([read.encode()], [U])[0][0, 0]) == want


def test_top_takes_the_smallest_bin_on_a_tie():
    # (1, C) twice and (1, G) twice: bin 5 wins; one more (1, C) and bin 6 wins
    read = U * 2 + "TCAGGG" + U + "TGAGGG" + U + "TCAGGG" + U + "TGAGGG" + U * 2
    for impl in (lambda r: R.variants([r], [U])[0], lambda r: capi.variants_host([r.encode()], [U])[0]):
        assert tuple(int(x) for x in impl(read)[0, 0])[:5] == (7, 4, 2, 5, 2)
        assert tuple(int(x) for x in impl(read + "TCAGGG" + U)[0, 0])[:5] == (8, 5, 2, 6, 3)
    # the same tie on the reverse strand, in motif coordinates
    rec = capi.variants_host([R.revcomp(read).encode()], [U])[0][0, 0]
    assert tuple(int(x) for x in rec)[5:] == (7, 4, 2, 5, 2)


def test_every_bin_of_k6():
    reads, want_bin = [], []
    for j in range(6):
        for c in "TGCA":
            if c == U[j]:
                continue
            unit = U[:j] + c + U[j + 1:]
            reads.append(U * 2 + unit + U * 2)
            want_bin.append(R.bin_of(j, c))
            assert R.bin_text(U, want_bin[-1]) == unit
    assert len(reads) == 18
    for strand, rs in ((0, reads), (1, [R.revcomp(r) for r in reads])):
        rec, hist, reads_with, per_read = R.variants(rs, [U])
        got, ghist, gwith = capi.variants_host([r.encode() for r in rs], [U])
        same(got, rec)
        assert (ghist == hist).all() and (gwith == reads_with).all()
        sfx = "_fwd" if strand == 0 else "_rev"
        for i, b in enumerate(want_bin):
            assert int(rec["units" + sfx][i, 0]) == 4 and int(rec["variants" + sfx][i, 0]) == 1 and int(rec["top" + sfx][i, 0]) == b
            assert per_read[i, 0, strand, b] == 1 and per_read[i, 0].sum() == 1
        # a bin whose base equals M[j] is always 0
        for j in range(6):
            assert hist[0, strand, R.bin_of(j, U[j])] == 0
        assert hist[0, strand].sum() == 18 and (hist[0, strand] != 0).sum() == 18 and hist[0, 1 - strand].sum() == 0


def test_reference_forms_agree():
    reads = noisy_reads(120, seed=3, max_len=300) + [b"", b"TT", b"N" * 40, b"A" * 50]
    rec, hist, reads_with, per_read = R.variants(reads, MOTIFS)
    for r, read in enumerate(reads):
        for m, motif in enumerate(MOTIFS):
            want, bins = R.variants_read(read, motif)
            assert tuple(int(x) for x in rec[r, m]) == want
            assert per_read[r, m].tolist() == bins
    assert hist.sum() > 50


def test_host_against_reference():
    reads = noisy_reads()
    rec, hist, reads_with, _ = R.variants(reads, MOTIFS)
    # not vacuous: every motif has variants on both strands
    for m in range(len(MOTIFS)):
        assert hist[m, 0].sum() >= 5 and hist[m, 1].sum() >= 5, MOTIFS[m]
    got, ghist, gwith = capi.variants_host(reads, MOTIFS)
    same(got, rec)
    assert (ghist == hist).all() and (gwith == reads_with).all()
    # packed planes give the same
    got2, ghist2, gwith2 = capi.variants_host(capi.pack_reads(reads), MOTIFS)
    same(got2, rec)
    assert (ghist2 == hist).all() and (gwith2 == reads_with).all()


def test_consequences():
    reads = noisy_reads(300, seed=21)
    rec, hist, reads_with = capi.variants_host(reads, MOTIFS)
    # the bins of a histogram sum to the variants
    for m in range(len(MOTIFS)):
        assert hist[m, 0].sum() == rec["variants_fwd"][:, m].sum() and hist[m, 1].sum() == rec["variants_rev"][:, m].sum()
    for r in (0, 1, 2, 4, 5):
        one, h1, w1 = capi.variants_host([reads[r]], MOTIFS)
        assert (h1[:, 0].sum(axis=1) == one["variants_fwd"][0]).all() and (h1[:, 1].sum(axis=1) == one["variants_rev"][0]).all()
        assert ((h1 != 0) == (w1 == 1)).all() and ((h1 != 0).sum(axis=2)[:, 0] == one["distinct_fwd"][0]).all()
    # units <= annotate's windows (an exact window is a rotation of the motif)
    annot = capi.annotate_host(reads, MOTIFS)
    assert (rec["units_fwd"] <= annot["windows_fwd"]).all() and (rec["units_rev"] <= annot["windows_rev"]).all()
    assert (rec["units_fwd"] < annot["windows_fwd"]).any()
    # an exact periodic repeat has no variants
    for m in MOTIFS:
        one, h1, _ = capi.variants_host([(m * 40).encode(), (R.revcomp(m) * 40)[3:].encode()], [m])
        assert h1.sum() == 0 and one["variants_fwd"].sum() == 0 and one["variants_rev"].sum() == 0
        assert int(one["units_fwd"][0, 0]) >= 40 and int(one["units_rev"][1, 0]) >= 39
    # reverse-complement symmetry: records and histograms swap strands
    rrec, rhist, rwith = capi.variants_host([rc_read(r) for r in reads], MOTIFS)
    same(rrec, swapped(rec))
    assert (rhist[:, ::-1] == hist).all() and (rwith[:, ::-1] == reads_with).all()
    # a self-reverse-complementary motif: strand rev is strand fwd under (j, c) -> (k-1-j, 3-c)
    m = MOTIFS.index("AAATTT")
    assert (rec["units_fwd"][:, m] == rec["units_rev"][:, m]).all() and (rec["variants_fwd"][:, m] == rec["variants_rev"][:, m]).all()
    assert hist[m, 0].sum() > 0
    for j in range(6):
        for c in range(4):
            assert hist[m, 1, 4 * (5 - j) + (3 - c)] == hist[m, 0, 4 * j + c]


def test_variant_signature_of_a_tract():
    """82 TCAGGG among 800 units, no three in a row: (1, C) x 82 and nothing else; random sequence gives no anchored variant"""
    units = ["TCAGGG" if i % 9 == 4 and i < 9 * 82 else U for i in range(800)]
    assert units.count("TCAGGG") == 82
    rec, hist, _ = capi.variants_host(["".join(units).encode()], [U])
    assert tuple(int(x) for x in rec[0, 0]) == (718, 82, 1, 6, 82) + Z
    assert hist[0, 0, 6] == 82 and hist.sum() == 82


def test_generator_long_reads():
    buf, st, nd = capi.synth_long_ascii(20250218, 0, 120)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    rec, hist, reads_with, _ = R.variants(reads, [U])
    assert hist[0, 0].sum() >= 20 and hist[0, 1].sum() >= 20  # the generator's noisy tails are there on both strands
    got, ghist, gwith = capi.variants_host(reads, [U])
    same(got, rec)
    assert (ghist == hist).all() and (gwith == reads_with).all()


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.variants_host(reads, ["AAT"] * 9)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.variants_host(reads, [])
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.variants_host(reads, [capi.Motif(33, 0, 0)])
    with pytest.raises(capi.TrewHipError, match="bits above 2k"):
        capi.variants_host(reads, [capi.Motif(3, 0, 64)])
    with pytest.raises(capi.TrewHipError, match="only A, C, G and T"):
        capi.variants_host(reads, ["TTAGGN"])
    lib = capi.load()
    m = capi.motif("AAT")
    w, o, ln = capi.pack_reads(reads)
    assert lib.trew_variants_host(w.ctypes.data, o.ctypes.data, ln.ctypes.data, 1, C.byref(m), 1, None, None, None) != 0
    assert b"null argument" in lib.trew_hip_last_error(None)


def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Variant) == 40 and capi.VARIANT_DTYPE.itemsize == 40
    assert tuple(capi.VARIANT_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.Variant._fields_)
    assert capi.VARIANT_BINS == R.BINS == 128 and capi.VARIANT_NONE == R.NONE
    assert C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Annot) == 24 and C.sizeof(capi.Tract) == 40
    for sym in ("trew_hip_variants", "trew_hip_variants_results", "trew_variants_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_variants.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.variants([b"TTAGGGTTAGGG"], ["TTAGGG"])
    r = subprocess.run([TREW, "variants", "TTAGGG", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["variants"], "MOTIF is required."),
        (["variants", "TTAGGG"], "FASTQ is required."),
        (["variants", "TTAGGN", FQ], "must consist of A, C, G and T."),
        (["variants", "TTAGGG,", FQ], "the length must be in range 3 to 32."),
        (["variants", "AC", FQ], "the length must be in range 3 to 32."),
        (["variants", "A" * 33, FQ], "the length must be in range 3 to 32."),
        (["variants", ",".join(["AAT"] * 9), FQ], "At most 8 motifs can be given."),
        (["variants", "TTAGGG", FQ, "--min_units", "x"], "MIN_UNITS must be a number."),
        (["variants", "TTAGGG", FQ, "--min_units", "-1"], "MIN_UNITS must be a number."),
        (["variants", "TTAGGG", FQ, "--min_units", "0"], "MIN_UNITS must be in range 1 to 4294967295."),
        (["variants", "TTAGGG", FQ, "--min_units", "4294967296"], "MIN_UNITS must be in range 1 to 4294967295."),
        (["variants", "TTAGGG", FQ, "--min_units"], "--min_units: expected 1 argument(s). 0 provided."),
        (["variants", "TTAGGG", FQ, "-t", "0"], "number of threads must be positive."),
        (["variants", "TTAGGG", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["variants", "TTAGGG", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["variants", "TTAGGG", FQ, "--devices", "0,x"], "Usage: variants"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: variants" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_variants():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "variants" in r.stderr and "intervals" in r.stderr and "tracts" in r.stderr and "short" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "variants" in r.stderr
    r = subprocess.run([TREW, "variants", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: variants" in r.stderr and "--min_units" in r.stderr and r.stdout == ""
