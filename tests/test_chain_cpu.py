"""Ordered unit chain, the parts that need no GPU: the two brute-force reference shapes against hand-worked vectors and
against each other, the host implementation (trew_chain_host) against the reference, the consequences the definition
promises (against trew_variants_host), the stand-alone sanitizer harness, the signature formatter, the additive ABI, the
argument errors of the C ABI and of `trew chain`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chain_ref as R
from chain_cases import K31, K32, MOTIFS, NONE, RTEL, TEL, EDGE_MOTIFS, filler, key_items, mirrored, noisy_reads, rc_read, same
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
U, RU = TEL, RTEL
B_C1, B_G1, B_G2 = 4 * 1 + 2, 4 * 1 + 1, 4 * 2 + 1  # TCAGGG, TGAGGG, TTGGGG

HAND = [
    # TTAGGG x 3 + TCAGGG + TTAGGG x 3
    (U * 3 + "TCAGGG" + U * 3, [(0, 3, NONE), (18, 1, B_C1), (24, 3, NONE)], [], "=3 TCAGGG =3", ""),
    # the same on the reverse strand: read coordinates, the variant's text in motif orientation
    (RU * 3 + "CCCTGA" + RU * 3, [], [(0, 3, NONE), (18, 1, B_C1), (24, 3, NONE)], "", "=3 TCAGGG =3"),
    # two adjacent variants, each anchored from outside
    (U * 2 + "TCAGGG" + "TGAGGG" + U * 2, [(0, 2, NONE), (12, 1, B_C1), (18, 1, B_G1), (24, 2, NONE)], [], "=2 TCAGGG TGAGGG =2", ""),
    # three adjacent variants: the middle one has no exact neighbour, is absent and leaves a +6
    (U * 2 + "TCAGGG" + "TGAGGG" + "TTGGGG" + U * 2, [(0, 2, NONE), (12, 1, B_C1), (24, 1, B_G2), (30, 2, NONE)], [], "=2 TCAGGG +6 TTGGGG =2", ""),
    # a unit with an N: neither exact nor variant
    (U * 2 + "TNAGGG" + U * 2, [(0, 2, NONE), (18, 2, NONE)], [], "=2 +6 =2", ""),
    # a one-unit run between two variants' worth of junk
    ("ACGTAC" + U + "ACGTAC", [(6, 1, NONE)], [], "=1", ""),
    # an unanchored exact unit is a one-unit run; an unanchored variant is nothing
    ("ACGTACTTAGGGACGTACTCAGGGACGTAC", [(6, 1, NONE)], [], "=1", ""),
    # the read-end anchor pair: the forward anchor is the last window (i + k = n - k); one base shorter it does not exist
    ("TCAGGG" + "TTAGGG", [(0, 1, B_C1), (6, 1, NONE)], [], "TCAGGG =1", ""),
    ("TCAGGG" + "TTAGG", [], [], "", ""),
    # a backward anchor at window 0
    ("TTAGGG" + "TCAGGG", [(0, 1, NONE), (6, 1, B_C1)], [], "=1 TCAGGG", ""),
    # n < k, and the empty read
    ("TTAGG", [], [], "", ""),
    ("", [], [], "", ""),
    # lower-case bases are bases
    ("ttagggTCAGGGttaggg", [(0, 1, NONE), (6, 1, B_C1), (12, 1, NONE)], [], "=1 TCAGGG =1", ""),
    # a phase shift by an inserted base shows as a gap token
    (U * 2 + "A" + U * 2, [(0, 2, NONE), (13, 2, NONE)], [], "=2 +1 =2", ""),
]


def host_items(read, motif):
    items, counts, n = capi.chain_host([read.encode() if isinstance(read, str) else read], [motif])
    assert n == len(items) == int(counts.sum())
    return [key_items(items, 0, 0, s) for s in (0, 1)], counts


@pytest.mark.parametrize("read,fwd,rev,sig_f,sig_r", HAND)
def test_hand_worked_vectors(read, fwd, rev, sig_f, sig_r):
    assert R.chain_read_marks(read, U) == [fwd, rev]
    assert R.chain_read_walk(read, U) == [fwd, rev]
    got, counts = host_items(read, U)
    assert got == [fwd, rev]
    for s, want in enumerate((fwd, rev)):
        assert counts[0, 0, s].tolist() == [sum(1 for x in want if x[2] == NONE), sum(1 for x in want if x[2] != NONE)]
    assert R.signature(fwd, U) == sig_f and R.signature(rev, U) == sig_r
    items = capi.chain_host([read.encode()], [U])[0]
    assert capi.chain_signature(items[items["strand"] == 0], U) == sig_f
    assert capi.chain_signature(items[items["strand"] == 1], U) == sig_r


def test_overlapping_residue_classes():
    # TGT in TGTGTGT: windows 0, 2 and 4 are exact, one one-unit run in each of the classes 0, 2, 1; items overlap
    want = [(0, 1, NONE), (2, 1, NONE), (4, 1, NONE)]
    assert R.chain_read_marks("TGTGTGT", "TGT")[0] == want and R.chain_read_walk("TGTGTGT", "TGT")[0] == want
    assert host_items("TGTGTGT", "TGT")[0][0] == want
    assert R.signature(want, "TGT") == "=1 -1 =1 -1 =1"
    # a homopolymer: every window exact, k runs interleaved
    want = [(0, 4, NONE), (1, 3, NONE), (2, 3, NONE)]
    assert R.chain_read_walk("A" * 12, "AAA")[0] == want and host_items("A" * 12, "AAA")[0][0] == want
    # TGTGT as the issue has it
    assert host_items("TGTGT", "TGT")[0][0] == [(0, 1, NONE), (2, 1, NONE)]


def test_reference_shapes_agree():
    reads = noisy_reads(120, seed=3, max_len=300) + [b"", b"TT", b"N" * 40, b"A" * 50, b"TGTGTGTGTGTGT"]
    motifs = MOTIFS + ["TGT"]
    a = R.chain(reads, motifs, R.chain_read_marks)
    b = R.chain(reads, motifs, R.chain_read_walk)
    same(a, b)
    assert len(a[0]) > 200 and a[1][..., 1].sum() > 20


@pytest.mark.parametrize("motif", ["AAT", "ACGTT", TEL, "TTAGGGC", "TTAGGGTTAGGGTCAG", K31, K32], ids=lambda m: "k%d" % len(m))
def test_host_against_reference(motif):
    reads = noisy_reads()
    want = R.chain(reads, [motif])
    # not vacuous: runs and variants on both strands
    assert (want[1].sum(axis=(0, 1))[:, 0] >= 5).all() and (want[1].sum(axis=(0, 1))[:, 1] >= 5).all()
    got = capi.chain_host(reads, [motif])
    same(got, want)
    assert got[2] == len(want[0])
    same(capi.chain_host(capi.pack_reads(reads), [motif]), want)  # packed planes give the same


def test_host_eight_motifs_and_cap():
    reads = noisy_reads(150, seed=17)
    want = R.chain(reads, MOTIFS)
    got = capi.chain_host(reads, MOTIFS)
    same(got, want)
    few = capi.chain_host(reads, MOTIFS, cap=7)  # the first ones of the sorted order; the number and the counts stay exact
    assert few[2] == len(want[0]) and (few[0] == want[0][:7]).all() and (few[1] == want[1]).all()


def test_generator_long_reads():
    buf, st, nd = capi.synth_long_ascii(20250218, 0, 60)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = R.chain(reads, [TEL], R.chain_read_walk)
    assert (want[1].sum(axis=(0, 1)) >= 20).all()  # the generator's noisy tails are there on both strands
    same(capi.chain_host(reads, [TEL]), want)


def test_consequences_against_variants_host():
    reads = noisy_reads(300, seed=21)
    items, counts, n = capi.chain_host(reads, MOTIFS)
    vrec, hist, reads_with = capi.variants_host(reads, MOTIFS)
    runs = items[items["bin"] == NONE]
    var = items[items["bin"] != NONE]
    assert (var["bin"] < 128).all() and (var["count"] == 1).all() and (runs["count"] >= 1).all()
    for s, sfx in ((0, "_fwd"), (1, "_rev")):
        units = np.zeros((len(reads), len(MOTIFS)), dtype=np.uint64)
        x = runs[runs["strand"] == s]
        np.add.at(units, (x["read"], x["motif"]), x["count"])
        assert (units == vrec["units" + sfx]).all()                    # the sum of the runs' counts is units_s
        assert (counts[:, :, s, 1] == vrec["variants" + sfx]).all()    # the variant items number variants_s
        per_read = np.zeros((len(reads), len(MOTIFS), 128), dtype=np.uint64)
        y = var[var["strand"] == s]
        np.add.at(per_read, (y["read"], y["motif"], y["bin"]), 1)
        assert (per_read.sum(axis=0) == hist[:, s]).all()               # their bins, summed over the batch, are hist
        assert ((per_read != 0).sum(axis=0) == reads_with[:, s]).all()
        assert ((per_read != 0).sum(axis=2) == vrec["distinct" + sfx]).all()  # and per read the read's bins
    # no two items of a key share a start, and the order is total
    key = np.stack([items[f].astype(np.int64) for f in ("read", "motif", "strand", "start")], axis=1)
    assert (np.lexsort(key.T[::-1]) == np.arange(len(key))).all() and len(np.unique(key, axis=0)) == len(key)
    # a primitive M repeated r times has exactly one forward item
    for m in MOTIFS:
        one = capi.chain_host([(m * 40).encode()], [m])[0]
        assert key_items(one, 0, 0, 0) == [(0, 40, NONE)]
    # reverse-complement symmetry
    ks = [len(m) for m in MOTIFS]
    rc = capi.chain_host([rc_read(r) for r in reads], MOTIFS)
    same(rc, mirrored(items, counts, [len(r) for r in reads], ks))
    # an item does not depend on the rest of the batch
    for r in (0, 1, 2, 5, 9, 250):
        alone = capi.chain_host([reads[r]], MOTIFS)
        sub = items[items["read"] == r].copy()
        sub["read"] = 0
        same(alone, (sub, counts[r:r + 1]))


def test_signature_formatter():
    it = lambda *rows: np.array([(0, 0, 0) + r for r in rows], dtype=capi.CHAIN_DTYPE)  # noqa: E731
    assert capi.chain_signature(it(), TEL) == ""
    assert capi.chain_signature(it((0, 41, NONE), (246, 1, B_C1), (252, 3, NONE), (270, 1, B_C1), (276, 1, B_G1), (282, 212, NONE)), TEL) == \
        "=41 TCAGGG =3 TCAGGG TGAGGG =212"
    assert capi.chain_signature(it((5, 2, NONE), (18, 1, B_G2), (23, 1, NONE)), TEL) == "=2 +1 TTGGGG -1 =1"
    assert capi.chain_signature(it((0, 1, NONE), (2, 1, NONE)), "TGT") == "=1 -1 =1"
    assert capi.chain_signature(it((0, 1, 4 * 31 + 0)), K32.lower()) == K32[:31] + "T"
    assert capi.chain_unit_text("ttaggg", B_C1) == "TCAGGG"
    # and the reference's own formatter says the same on real items
    reads = noisy_reads(60, seed=5)
    items = capi.chain_host(reads, [TEL])[0]
    for r in range(len(reads)):
        for s in (0, 1):
            sub = items[(items["read"] == r) & (items["strand"] == s)]
            assert capi.chain_signature(sub, TEL) == R.signature(key_items(items, r, 0, s), TEL)


def test_fillers_hold_no_unit():
    for unit in EDGE_MOTIFS + [RTEL]:
        f = filler(unit, 200)
        assert len(f) == 200 and len(R.chain([f], [unit])[0]) == 0


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path):
    exe = str(tmp_path / "chain_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "chain_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.decode().upper().encode() for r in noisy_reads(200, seed=31)] + [b"", b"A", TEL.encode() * 400, b"TGTGTGT"]

    def text(items, counts, n):
        return "items %d\n" % n + "".join(" ".join(str(int(x[f])) for f in R.FIELDS) + "\n" for x in items) + \
            "counts" + "".join(" %d" % c for c in counts.ravel().tolist()) + "\n"

    for motifs in ([TEL], ["AAT", K32], MOTIFS):
        r = subprocess.run([exe, ",".join(motifs)], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        assert r.stdout.decode() == text(*capi.chain_host(reads, motifs))
    r = subprocess.run([exe, TEL, "5"], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.decode() == text(*capi.chain_host(reads, [TEL], cap=5))
    r = subprocess.run([exe, TEL], input=b"", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"items 0\ncounts\n" and r.stderr == b""


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.ChainItem) == 24 and capi.CHAIN_DTYPE.itemsize == 24
    assert tuple(capi.CHAIN_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.ChainItem._fields_)
    assert capi.VARIANT_NONE == R.NONE
    assert C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Variant) == 40 and C.sizeof(capi.Interval) == 24
    for sym in ("trew_hip_chain", "trew_hip_chain_results", "trew_chain_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    import trew_amd
    assert trew_amd.chain is capi.chain


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.chain_host(reads, ["AAT"] * 9)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.chain_host(reads, [])
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.chain_host(reads, [capi.Motif(33, 0, 0)])
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.chain_host(reads, [capi.Motif(2, 0, 0)])
    with pytest.raises(capi.TrewHipError, match="bits above 2k"):
        capi.chain_host(reads, [capi.Motif(3, 0, 64)])
    with pytest.raises(capi.TrewHipError, match="only A, C, G and T"):
        capi.chain_host(reads, ["TTAGGN"])
    lib = capi.load()
    m = capi.motif("AAT")
    w, o, ln = capi.pack_reads(reads)
    n = C.c_uint64(0)
    assert lib.trew_chain_host(w.ctypes.data, o.ctypes.data, ln.ctypes.data, 1, C.byref(m), 1, None, 0, None, None) != 0
    assert b"null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_chain_host(w.ctypes.data, o.ctypes.data, ln.ctypes.data, 1, C.byref(m), 1, None, 3, C.byref(n), None) != 0
    assert b"null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_chain_host(None, None, None, 1, C.byref(m), 1, None, 0, C.byref(n), None) != 0
    assert lib.trew_chain_host(None, None, None, 0, C.byref(m), 1, None, 0, C.byref(n), None) == 0 and n.value == 0
    # the device entry points without a context
    assert lib.trew_hip_chain(None, None, 0, C.byref(m), 1, 4) != 0
    assert lib.trew_hip_chain_results(None, 0, None, 0, C.byref(n), C.byref(n), None, None) != 0


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_chain.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.chain([b"TTAGGGTTAGGG"], ["TTAGGG"])
    r = subprocess.run([TREW, "chain", "TTAGGG", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["chain"], "MOTIF is required."),
        (["chain", "TTAGGG"], "FASTQ is required."),
        (["chain", "TTAGGN", FQ], "must consist of A, C, G and T."),
        (["chain", "TTAGGG,", FQ], "the length must be in range 3 to 32."),
        (["chain", "AC", FQ], "the length must be in range 3 to 32."),
        (["chain", "A" * 33, FQ], "the length must be in range 3 to 32."),
        (["chain", ",".join(["AAT"] * 9), FQ], "At most 8 motifs can be given."),
        (["chain", "TTAGGG", FQ, "--min_units", "x"], "MIN_UNITS must be a number."),
        (["chain", "TTAGGG", FQ, "--min_units", "-1"], "MIN_UNITS must be a number."),
        (["chain", "TTAGGG", FQ, "--min_units", "0"], "MIN_UNITS must be in range 1 to 4294967295."),
        (["chain", "TTAGGG", FQ, "--min_units", "4294967296"], "MIN_UNITS must be in range 1 to 4294967295."),
        (["chain", "TTAGGG", FQ, "--items", "--min_units"], "--min_units: expected 1 argument(s). 0 provided."),
        (["chain", "TTAGGG", FQ, "-t", "0"], "number of threads must be positive."),
        (["chain", "TTAGGG", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["chain", "TTAGGG", FQ, "--max_gap", "3"], "Unknown argument: --max_gap"),
        (["chain", "TTAGGG", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["chain", "TTAGGG", FQ, "--devices", "0,x"], "Usage: chain"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: chain" in r.stderr
    assert r.stdout == ""


def test_items_flag_belongs_to_chain_alone():
    r = subprocess.run([TREW, "variants", "TTAGGG", FQ, "--items"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "Unknown argument: --items" in r.stderr and r.stdout == ""


def test_cli_usage_lists_chain():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "chain" in r.stderr and "variants" in r.stderr and "periods" in r.stderr and "short" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "chain" in r.stderr
    r = subprocess.run([TREW, "chain", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: chain" in r.stderr and "--min_units" in r.stderr and "--items" in r.stderr and r.stdout == ""
