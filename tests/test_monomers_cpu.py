"""Wraparound alignment for units of up to 256 bases (trew_hip_monomers), the parts that need no GPU: the definition by brute
force against the O(n k) numpy form of monomer_ref.py, the host definition (trew_monomers_host) against that form on a fuzz
set with substitutions and indels and against trew_align_host for k <= 32, the consequences of the definition, an array of
diverged monomers, the stand-alone sanitizer harness, the additive ABI, and the argument errors of the C ABI and of
`trew monomers`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_cases as AC
import monomer_cases as MC
import monomer_ref as R
from period_cases import junk, noisy
from trew_amd import capi

assert tuple(capi.ALIGN_DTYPE.names) == R.FIELDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
TEL = AC.TEL


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, unit) %s: got %s, want %s" % (f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def rec(x):
    return tuple(int(v) for v in x)


@pytest.fixture(scope="module")
def fuzz():
    """[(unit, reads, {penalty: reference records})] of monomer_cases.host_fuzz, the O(n k) reference computed once"""
    return [(unit, reads, {p: R.monomers(reads, [unit], p) for p in (1, 3)}) for unit, reads in MC.host_fuzz()]


# ---- the two forms of the reference
@pytest.mark.parametrize("k", [3, 32, 33, 64, 65])
def test_definition_by_brute_force_against_the_numpy_form(k):
    rnd = random.Random(100 + k)
    unit = MC.unit_of(k, 1)
    reads = [junk(rnd, rnd.randint(0, 8), "ACGTN") + noisy(rnd, unit, 2 * k + rnd.randint(10, 30), 0.03, 0.08, 0.01) + junk(rnd, rnd.randint(0, 8))
             for _ in range(2)]
    for penalty in (1, 3, 64):
        got = R.monomers(reads, [unit], penalty)
        for r, read in enumerate(reads):
            assert rec(got[r, 0]) == R.monomer_read(read, unit, penalty), (k, penalty, read)


@pytest.mark.parametrize("k", [171, 256])
def test_definition_by_brute_force_at_the_large_k(k):
    """one read of about 2 k + 40 bases, P = 3, the forward strand (O(n k^2) in Python: seconds a strand)"""
    rnd = random.Random(200 + k)
    unit = MC.unit_of(k, 2)
    read = junk(rnd, 10) + noisy(rnd, unit, 2 * k + 20, 0.03, 0.06, 0.005) + junk(rnd, 10)
    want = R.monomer_read(read, unit, 3, strands=(0,))
    assert want[0] > k  # more than one copy aligned: the path goes round the unit
    assert rec(R.monomers([read], [unit], 3)[0, 0])[:5] == want
    assert rec(capi.monomers_host([read], [unit], 3)[0, 0])[:5] == want


# ---- the host definition
@pytest.mark.parametrize("penalty", [1, 3])
def test_host_against_reference_on_the_fuzz_set(fuzz, penalty):
    assert tuple(len(u) for u, _, _ in fuzz) == MC.HOST_KS
    for unit, reads, want in fuzz:
        same(capi.monomers_host(reads, [unit], penalty), want[penalty])


def test_the_fuzz_set_has_insertions_and_deletions(fuzz):
    """by the reference alone: at least half of the reads have both an insertion and a deletion in the winning forward
    alignment at P = 3"""
    both = total = 0
    for unit, reads, want in fuzz:
        cols = capi.align_columns(want[3], len(unit), 3)
        total += len(reads)
        both += int(((cols["insertions_fwd"][:, 0] >= 1) & (cols["deletions_fwd"][:, 0] >= 1)).sum())
    print("reads %d, with an insertion and a deletion %d" % (total, both))
    assert 2 * both >= total


def test_host_equals_align_host_up_to_32_bases():
    for unit, reads in AC.fuzz_sets():
        for penalty in (1, 3, 64):
            same(capi.monomers_host(reads, [unit], penalty), capi.align_host(reads, [unit], penalty))
    for read, motif, penalty, fwd, rv in AC.HAND:
        assert rec(capi.monomers_host([read.encode()], [motif], penalty)[0, 0]) == fwd + rv
        assert rec(R.monomers([read], [motif], penalty)[0, 0]) == fwd + rv


def test_host_many_monomers_packed_planes_and_lower_case():
    rnd = random.Random(12)
    units = [MC.unit_of(k, 4) for k in (6, 33, 64, 65, 128, 171, 255, 256)]
    reads = [junk(rnd, rnd.randint(0, 30), "ACGTacgtNn") + noisy(rnd, rnd.choice(units), rnd.randint(0, 300), 0.03, 0.06, 0.01).lower()
             + junk(rnd, rnd.randint(0, 30)) for _ in range(12)] + ["", "A", "N" * 40]
    want = R.monomers(reads, units, 3)
    same(capi.monomers_host(reads, units, 3), want)
    same(capi.monomers_host(capi.pack_reads(reads), [u.lower() for u in units], 3), want)


# ---- consequences of the definition
def test_every_rotation_gives_the_same_record():
    rnd = random.Random(171)
    unit = MC.unit_of(171, 5)
    read = junk(rnd, 25) + noisy(rnd, unit, 2 * 171 + 40, 0.03, 0.06, 0.005) + junk(rnd, 25)
    want = rec(capi.monomers_host([read], [unit], 3)[0, 0])
    assert want[0] > 171
    rots = AC.rotations(unit)
    assert len(rots) == 171
    for at in range(0, 171, 8):
        got = capi.monomers_host([read], rots[at:at + 8], 3)
        for m in range(got.shape[1]):
            assert rec(got[0, m]) == want, at + m


def test_strand_mirror_and_derived_columns(fuzz):
    """score_rev(x) = score_fwd(revcomp x), and the derived columns are never negative and add up"""
    for unit, reads, want in fuzz:
        for penalty in (1, 3):
            w = want[penalty]
            rc = capi.monomers_host([AC.revcomp(r) for r in reads], [unit], penalty)
            assert (rc["score_fwd"] == w["score_rev"]).all() and (rc["score_rev"] == w["score_fwd"]).all()
            cols = capi.align_columns(w, len(unit), penalty)
            for name, v in cols.items():
                assert (v >= 0).all(), (name, len(unit), penalty)
            for sfx in ("_fwd", "_rev"):
                errors = cols["mismatches" + sfx] + cols["insertions" + sfx] + cols["deletions" + sfx]
                assert (w["score" + sfx] == w["matches" + sfx] - penalty * errors).all()
                assert (w["end" + sfx] - w["start" + sfx] == w["matches" + sfx] + cols["mismatches" + sfx] + cols["insertions" + sfx]).all()
                assert (w["consumed" + sfx] == w["matches" + sfx] + cols["mismatches" + sfx] + cols["deletions" + sfx]).all()


def test_an_array_of_diverged_monomers_is_found_and_a_random_read_is_not():
    """six copies of a 171-base consensus, each diverged by 18 % substitutions and 2 % indels (monomer_cases.ARRAY_SEED): at
    P = 2 the forward tract begins and ends within 10 bases of the plant; a random read of the same length stays below the
    default min_score of 24 at P = 2 and P = 3 on both strands.  Neighbouring copies are about 0.64 identical: no fixed-phase
    comparison scores them at these penalties."""
    consensus, read, begin, end, background = MC.diverged_array()
    assert len(consensus) == 171 and len(background) == len(read)
    for penalty in (2, 3):
        got = capi.monomers_host([read, background], [consensus], penalty)
        same(got, R.monomers([read, background], [consensus], penalty))
        assert max(int(got["score_fwd"][1, 0]), int(got["score_rev"][1, 0])) < 24
        assert int(got["score_fwd"][0, 0]) >= 150 and int(got["score_rev"][0, 0]) < 24
    got = capi.monomers_host([read], [consensus], 2)[0, 0]
    assert abs(int(got["start_fwd"]) - begin) <= 10 and abs(int(got["end_fwd"]) - end) <= 10
    assert capi.align_columns(got, 171, 2)["copies_fwd"] in (5, 6)


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path, fuzz):
    exe = str(tmp_path / "monomers_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "monomers_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.upper().encode() for _, rs, _ in fuzz[::3] for r in rs[:2]] + [b"", b"A", TEL.encode() * 100]
    units = [TEL] + [fuzz[i][0] for i in (0, 3, 4, 9, 12, 13)]
    assert [len(u) for u in units] == [6, 33, 64, 65, 171, 255, 256]
    for penalty in (1, 3, 64):
        r = subprocess.run([exe, str(penalty), ",".join(units)], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        want = capi.monomers_host(reads, units, penalty)
        assert r.stdout.decode() == "".join(" ".join(str(int(x[f])) for f in R.FIELDS) + "\n" for x in want.reshape(-1))
    r = subprocess.run([exe, "3", "A" * 256], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0 0 0 0 0 0 0 0 0 0\n" * 2 and r.stderr == b""
    r = subprocess.run([exe, "3", "A" * 257], input=b"\n", capture_output=True, timeout=60)
    assert r.returncode == 3 and b"the length must be in [3, 256]" in r.stderr


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Monomer) == 72 and [n for n, _ in capi.Monomer._fields_] == ["k", "reserved", "unit"]
    assert C.sizeof(capi.Alignment) == 40 and C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Satellite) == 104
    assert capi.MONOMER_MAX == R.MAX == 256 and capi.MONOMERS_MAX == 8
    hdr = open(os.path.join(ROOT, "include", "trew_hip.h")).read()
    assert "#define TREW_HIP_ABI_VERSION 4" in hdr and "#define TREW_MONOMER_MAX 256" in hdr
    for sym in ("trew_monomer_parse", "trew_hip_monomers", "trew_hip_monomers_results", "trew_monomers_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None and "int %s(" % sym in hdr
    import trew_amd

    assert trew_amd.monomers is capi.monomers


def test_monomer_parse():
    for k in (3, 256):
        text = MC.unit_of(k, 6)
        m = capi.monomer(text)
        assert m.k == k and m.reserved == 0
        got = "".join("TGCA"[(m.unit[j >> 4] >> (2 * (j & 15))) & 3] for j in range(k))
        assert got == text
        assert all((m.unit[j >> 4] >> (2 * (j & 15))) & 3 == 0 for j in range(k, 256))  # zero bits at and above base k
        lower = capi.monomer(text.lower().encode())
        assert bytes(lower) == bytes(m)
    for text in ("AC", "A" * 257, ""):
        with pytest.raises(capi.TrewHipError, match=r"the length must be in \[3, 256\]"):
            capi.monomer(text)
    for text in ("ACGN", "ACG T", "A" * 100 + "x"):
        with pytest.raises(capi.TrewHipError, match="only A, C, G and T are allowed"):
            capi.monomer(text)
    assert capi.load().trew_monomer_parse(None, None) != 0
    # the packing is trew_hip_satellite.unit's
    assert capi.satellite_unit_text(np.array(list(capi.monomer(TEL).unit), dtype=np.uint32), 6) == TEL


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.monomers_host(reads, ["AAT"], penalty)
    for units in (["AAT"] * 9, []):
        with pytest.raises(capi.TrewHipError, match=r"n_monomers must be in \[1, 8\]"):
            capi.monomers_host(reads, units)
    zero = (C.c_uint32 * 16)()
    for k in (2, 257, 0, -3):
        with pytest.raises(capi.TrewHipError, match=r"monomer: k must be in \[3, 256\]"):
            capi.monomers_host(reads, [capi.Monomer(k, 0, zero)])
    high = (C.c_uint32 * 16)()
    high[0] = 1 << 6  # base 3 of a unit of 3 bases
    with pytest.raises(capi.TrewHipError, match="bits at or above base k"):
        capi.monomers_host(reads, [capi.Monomer(3, 0, high)])
    high = (C.c_uint32 * 16)()
    high[15] = 1 << 30  # base 255 of a unit of 255 bases
    with pytest.raises(capi.TrewHipError, match="bits at or above base k"):
        capi.monomers_host(reads, [capi.Monomer(255, 0, high)])
    lib = capi.load()
    arr, nm = capi._monomer_array(["AAT"])
    assert lib.trew_monomers_host(None, None, None, 1, arr, nm, 3, None) != 0
    assert b"trew_monomers_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_monomers_host(None, None, None, 1, None, 1, 3, None) != 0
    assert b"monomers is NULL" in lib.trew_hip_last_error(None)
    assert lib.trew_monomers_host(None, None, None, 0, arr, nm, 3, None) == 0  # no reads: nothing is read or written
    # the 33-base error of align stays what it was
    with pytest.raises(capi.TrewHipError, match=r"the length must be in \[3, 32\]"):
        capi.align_host(reads, ["A" * 33])


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched"""
    lib = capi.load()
    arr, nm = capi._monomer_array([MC.unit_of(171, 1)])
    n = C.c_uint64(7)
    assert lib.trew_hip_monomers(None, None, 0, arr, nm, 3) == -1
    assert lib.trew_hip_monomers_results(None, 0, None, 0, C.byref(n), None) == -1 and n.value == 7


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_monomers.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.monomers([b"TTAGGGTTAGGG"], [MC.unit_of(171, 1)])
    r = subprocess.run([TREW, "monomers", MC.unit_of(171, 1), FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.fixture(scope="module")
def fastas(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta")
    u = MC.unit_of(171, 1)
    files = {
        "empty": "",
        "no_records": "\n\n",
        "nine": "".join(">m%d\nACGTTGCA\n" % i for i in range(9)),
        "multi_line_bad": ">alpha the first\n" + u[:60] + "\n" + u[60:120] + "\nNN\n",
        "too_long": ">long\n" + "\n".join(["ACGTTGCA" * 8] * 5) + "\n",  # 320 bases over five lines
        "short": ">s\nAC\n",
        "headless": "ACGT\n>x\nACGT\n",
        "good": ">alpha the first\n" + u[:60] + "\n" + u[60:] + "\n>beta\r\n" + TEL + "\r\n",
    }
    out = {}
    for name, text in files.items():
        out[name] = str(d / (name + ".fa"))
        with open(out[name], "w") as f:
            f.write(text)
    return out


U40 = "ACGTTGCAAC" * 4
CLI_ERRORS = [
    (["monomers"], "MONOMER or --fasta FILE is required."),
    (["monomers", U40], "FASTQ is required."),
    (["monomers", FQ], "MONOMER or --fasta FILE is required."),  # neither source
    (["monomers", "--fasta", "@good", U40, FQ], "MONOMER and --fasta cannot both be given."),  # both
    (["monomers", "--fasta", "@good"], "FASTQ is required."),
    (["monomers", "TTAGGN", FQ], "must consist of A, C, G and T."),
    (["monomers", "TTAGGG,", FQ], "the length must be in range 3 to 256."),
    (["monomers", "AC", FQ], "the length must be in range 3 to 256."),
    (["monomers", "A" * 257, FQ], "the length must be in range 3 to 256."),
    (["monomers", ",".join(["AAT"] * 9), FQ], "At most 8 monomers can be given."),
    (["monomers", "--fasta", "@empty", FQ], "no FASTA records"),
    (["monomers", "--fasta", "@no_records", FQ], "no FASTA records"),
    (["monomers", "--fasta", "/nonexistent.fa", FQ], "/nonexistent.fa : file not found"),
    (["monomers", "--fasta", "@nine", FQ], "At most 8 monomers can be given."),
    (["monomers", "--fasta", "@multi_line_bad", FQ], "MONOMER 'alpha' must consist of A, C, G and T."),
    (["monomers", "--fasta", "@too_long", FQ], "MONOMER 'long': the length must be in range 3 to 256."),
    (["monomers", "--fasta", "@short", FQ], "MONOMER 's': the length must be in range 3 to 256."),
    (["monomers", "--fasta", "@headless", FQ], "sequence in front of the first header"),
    (["monomers", "--fasta"], "--fasta: expected 1 argument(s). 0 provided."),
    (["monomers", U40, FQ, "--penalty", "x"], "PENALTY must be a number."),
    (["monomers", U40, FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
    (["monomers", U40, FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
    (["monomers", U40, FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
    (["monomers", U40, FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
    (["monomers", U40, FQ, "-t", "0"], "number of threads must be positive."),
    (["monomers", U40, FQ, "--bogus"], "Unknown argument: --bogus"),
    (["monomers", U40, "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
    (["monomers", "--fasta", "@good", FQ, "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(fastas, args, msg):
    args = [fastas[a[1:]] if a.startswith("@") else a for a in args]
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: monomers" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_monomers_and_align_keeps_its_limit():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "monomers" in r.stderr and "align" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  monomers " in r.stderr
    r = subprocess.run([TREW, "monomers", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: monomers" in r.stderr and "--fasta" in r.stderr and "--penalty" in r.stderr and r.stdout == ""
    r = subprocess.run([TREW, "align", "A" * 33, FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "the length must be in range 3 to 32." in r.stderr and r.stdout == ""
