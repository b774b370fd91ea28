"""Indel-aware motif tract per read (wraparound alignment), the parts that need no GPU: the two forms of align_ref.py against
hand-worked vectors and against each other, the consequences of the definition, the host definition (trew_align_host)
against the reference on a fuzz set with substitutions and indels, the stand-alone sanitizer harness, the additive ABI, the
argument errors of the C ABI and of `trew align`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_ref as R
import annot_ref as A
from align_cases import HAND, TEL, fuzz_sets, revcomp, rotations, with_deletion, with_insertion
from period_cases import junk, noisy
from trew_amd import capi

assert tuple(capi.ALIGN_DTYPE.names) == R.FIELDS  # the reference and the record name their fields alike, in the same order
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, motif) %s: got %s, want %s" % (
            f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def rec(x):
    return tuple(int(v) for v in x)


@pytest.fixture(scope="module")
def fuzz():
    """[(motif, reads, {penalty: reference records})], the reference computed once"""
    return [(unit, reads, {p: R.align(reads, [unit], p) for p in (1, 3, 64)}) for unit, reads in fuzz_sets()]


@pytest.mark.parametrize("read,motif,penalty,fwd,rev", HAND)
def test_hand_worked_vectors(read, motif, penalty, fwd, rev):
    want = fwd + rev
    assert R.align_read(read, motif, penalty) == want
    assert rec(R.align([read], [motif], penalty)[0, 0]) == want
    assert rec(capi.align_host([read.encode()], [motif], penalty)[0, 0]) == want


def test_reference_forms_agree():
    """the definition (max over d) against the doubling steps, for every k: short reads, all three penalties"""
    rnd = random.Random(9)
    for k in range(3, 33):
        unit = junk(rnd, k)
        reads = [junk(rnd, rnd.randint(0, 8), "ACGTN") + noisy(rnd, unit, rnd.randint(0, 70), 0.04, 0.1, 0.01) + junk(rnd, rnd.randint(0, 8))
                 for _ in range(3)]
        for penalty in (1, 3, 64):
            got = R.align(reads, [unit], penalty)
            for r, read in enumerate(reads):
                assert rec(got[r, 0]) == R.align_read(read, unit, penalty), (read, unit, penalty)


def test_one_deleted_and_one_inserted_base():
    t10 = TEL * 10
    for at in range(1, 59):
        score, start, end, consumed, matches = R.align_read(with_deletion(t10, at), TEL)[:5]
        c = R.columns(score, start, end, consumed, matches, 6, 3)
        if 6 <= at <= 55:  # further out the flank is no dearer to drop than to bridge, and on a tie the shorter tract wins
            assert (c["deletions"], c["insertions"], c["mismatches"]) == (1, 0, 0) and (start, end) == (0, 59)
            assert consumed == end - start + 1 and score == 59 - 3
        score, start, end, consumed, matches = R.align_read(with_insertion(t10, at, "C"), TEL)[:5]
        c = R.columns(score, start, end, consumed, matches, 6, 3)
        if 4 <= at <= 56:
            assert (c["deletions"], c["insertions"], c["mismatches"]) == (0, 1, 0) and (start, end, consumed) == (0, 61, 60)


def test_every_rotation_gives_the_same_record(fuzz):
    rnd = random.Random(3)
    for unit, reads, _ in fuzz[::4]:
        rots = rotations(unit)
        read = reads[0]
        want = capi.align_host([read], [unit], 3)[0, 0]
        got = capi.align_host([read], rots[:8], 3)
        for m in range(len(rots[:8])):
            assert rec(got[0, m]) == rec(want)
        rot = rnd.choice(rots)
        assert R.align_read(read, rot, 3) == rec(want)


def test_consequences_on_the_fuzz_set(fuzz):
    """score >= annotate's longest exact tract for every P; score_rev(x) = score_fwd(revcomp x); the derived columns are never
    negative and add up; and the fuzz set is what it is meant to be: at P = 3 at least half of the reads have both an insertion
    and a deletion in the winning alignment, and at least half have two or more deletions (by the reference alone)."""
    both = two_del = total = 0
    for unit, reads, want in fuzz:
        annot = A.annotate([r.encode() for r in reads], [unit])
        rc = R.align([revcomp(r) for r in reads], [unit], 3)
        assert (rc["score_fwd"] == want[3]["score_rev"]).all() and (rc["score_rev"] == want[3]["score_fwd"]).all()
        for penalty, w in want.items():
            for sfx in ("_fwd", "_rev"):
                assert (w["score" + sfx][:, 0] >= annot["tract_len" + sfx][:, 0]).all()
            cols = capi.align_columns(w, len(unit), penalty)
            for name, v in cols.items():
                assert (v >= 0).all(), name
            for r in range(len(reads)):
                for s, sfx in enumerate(("_fwd", "_rev")):
                    f = rec(w[r, 0])[5 * s:5 * s + 5]
                    c = R.columns(*f, len(unit), penalty)
                    assert all(int(cols[n + sfx][r, 0]) == c[n] for n in R.COLUMNS)
                    assert f[0] == f[4] - penalty * (c["mismatches"] + c["insertions"] + c["deletions"])
                    assert f[2] - f[1] == f[4] + c["mismatches"] + c["insertions"] and f[3] == f[4] + c["mismatches"] + c["deletions"]
        cols = capi.align_columns(want[3], len(unit), 3)
        for r in range(len(reads)):
            sfx = "_fwd" if want[3]["score_fwd"][r, 0] >= want[3]["score_rev"][r, 0] else "_rev"
            total += 1
            both += cols["insertions" + sfx][r, 0] >= 1 and cols["deletions" + sfx][r, 0] >= 1
            two_del += cols["deletions" + sfx][r, 0] >= 2
    print("reads %d, with an insertion and a deletion %d, with two or more deletions %d" % (total, both, two_del))
    assert 2 * both >= total and 2 * two_del >= total


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_host_against_reference_on_the_fuzz_set(fuzz, penalty):
    for unit, reads, want in fuzz:
        same(capi.align_host(reads, [unit], penalty), want[penalty])


def test_host_many_motifs_packed_planes_and_lower_case():
    rnd = random.Random(12)
    motifs = ["AAT", "TGTG", "ACGTT", TEL, "GGGTTAG", junk(rnd, 12)]
    reads = [junk(rnd, rnd.randint(0, 60), "ACGTacgtNn") + noisy(rnd, rnd.choice(motifs), rnd.randint(0, 120), 0.03, 0.06, 0.01).lower()
             + junk(rnd, rnd.randint(0, 30)) for _ in range(40)] + ["", "A", "N" * 40]
    want = R.align(reads, motifs, 3)
    same(capi.align_host(reads, motifs, 3), want)
    same(capi.align_host(capi.pack_reads(reads), motifs, 3), want)


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path, fuzz):
    exe = str(tmp_path / "align_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "align_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.upper().encode() for _, rs, _ in fuzz[::3] for r in rs[:3]] + [b"", b"A", TEL.encode() * 400]
    motifs = [fuzz[0][0], TEL, fuzz[-2][0], fuzz[-1][0]]
    assert [len(m) for m in motifs] == [3, 6, 31, 32]
    for penalty in (1, 3, 64):
        r = subprocess.run([exe, str(penalty), ",".join(motifs)], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        want = capi.align_host(reads, motifs, penalty)
        assert r.stdout.decode() == "".join(" ".join(str(int(x[f])) for f in R.FIELDS) + "\n" for x in want.reshape(-1))
    r = subprocess.run([exe, "3", TEL], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0 0 0 0 0 0 0 0 0 0\n" * 2 and r.stderr == b""


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Alignment) == 40 and capi.ALIGN_DTYPE.itemsize == 40
    assert tuple(capi.ALIGN_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.Alignment._fields_)
    assert C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Tract) == 40
    for sym in ("trew_hip_align", "trew_hip_align_results", "trew_align_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.align_host(reads, ["AAT"], penalty)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.align_host(reads, ["AAT"] * 9)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.align_host(reads, [])
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.align_host(reads, [capi.Motif(33, 0, 0)])
    with pytest.raises(capi.TrewHipError, match="bits above 2k"):
        capi.align_host(reads, [capi.Motif(3, 0, 64)])
    lib = capi.load()
    arr, nm = capi._motif_array(["AAT"])
    assert lib.trew_align_host(None, None, None, 1, arr, nm, 3, None) != 0
    assert b"trew_align_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_align_host(None, None, None, 0, arr, nm, 3, None) == 0  # no reads: nothing is read or written


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched"""
    lib = capi.load()
    arr, nm = capi._motif_array([TEL])
    n = C.c_uint64(7)
    assert lib.trew_hip_align(None, None, 0, arr, nm, 3) == -1
    assert lib.trew_hip_align_results(None, 0, None, 0, C.byref(n), None) == -1 and n.value == 7


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_align.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.align([b"TTAGGGTTAGGG"], [TEL])
    r = subprocess.run([TREW, "align", TEL, FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["align"], "MOTIF is required."),
        (["align", "TTAGGG"], "FASTQ is required."),
        (["align", "TTAGGN", FQ], "must consist of A, C, G and T."),
        (["align", "TTAGGG,", FQ], "the length must be in range 3 to 32."),
        (["align", "AC", FQ], "the length must be in range 3 to 32."),
        (["align", "A" * 33, FQ], "the length must be in range 3 to 32."),
        (["align", ",".join(["AAT"] * 9), FQ], "At most 8 motifs can be given."),
        (["align", "TTAGGG", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["align", "TTAGGG", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["align", "TTAGGG", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["align", "TTAGGG", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["align", "TTAGGG", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["align", "TTAGGG", FQ, "-t", "0"], "number of threads must be positive."),
        (["align", "TTAGGG", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["align", "TTAGGG", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["align", "TTAGGG", FQ, "--devices", "0,x"], "Usage: align"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: align" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_align():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "align" in r.stderr and "tracts" in r.stderr and "short" in r.stderr and "long" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  align " in r.stderr
    r = subprocess.run([TREW, "align", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: align" in r.stderr and "--penalty" in r.stderr and "--min_score" in r.stderr and r.stdout == ""
