"""Error-tolerant terminal motif tracts, the parts that need no GPU: the brute-force reference against hand-worked vectors
and against itself, the host implementation (trew_tracts_host) against the reference, the property that makes the measure
useful (a noisy telomere tail is recovered), the additive ABI, the argument errors of `trew tracts`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as A
import tract_ref as R
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
LONG_N = 300  # generator reads that hold >= 5 tails and >= 5 reverse-complemented tails of >= 1500 bases (9 and 9)
Z = (0, 0, 0, 0, 0)


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, motif) %s: got %s, want %s" % (
            f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


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


def long_reads(n=LONG_N):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


def planted_tail_reads(n=12, seed=5):
    """(read, planted tail length): a random body and a (TTAGGG)n 3' tail of 2-6 kb with 5 % substitutions"""
    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        body = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(500, 3000)))
        tlen = rnd.randint(2000, 6000)
        tail = list(("TTAGGG" * (tlen // 6 + 1))[:tlen])
        for i in range(tlen):
            if rnd.random() < 0.05:
                tail[i] = rnd.choice([c for c in "ACGT" if c != tail[i]])
        out.append((body + "".join(tail), tlen))
    return out


HAND = [
    (b"TTAGGG" * 5, "TTAGGG", 3, (30, 30, 30, 30, 30), Z),
    (b"TTAGGGTTAGGGTCAGGGTTAGGGACGTACGTACGT", "TTAGGG", 3, (23, 24, 23, 0, 0), Z),
    (b"ACGTACGTACTTAGGGTTAGGG", "TTAGGG", 3, (12, 0, 0, 12, 12), Z),
    (b"TTAGGGTTAGGGACGACGACGATTAGGGTTAGGG", "TTAGGG", 1, (24, 34, 24, 34, 24), Z),
    (b"TTAGGGTTAGGGACGACGACGATTAGGGTTAGGG", "TTAGGG", 3, (24, 12, 12, 12, 12), Z),
    (b"TTAGGGACACACTTAGGG", "TTAGGG", 1, (12, 6, 6, 6, 6), Z),  # tie: S(6) = S(18) = 6
    (b"TTAGGGTTAGGGTTAGGGNTTAGGGTTAGGG", "TTAGGG", 3, (30, 31, 30, 31, 30), Z),
    (b"CCCTAACCCTAACCCTAAGATTACAGATTACA", "TTAGGG", 3, Z, (18, 18, 18, 0, 0)),
    (b"GATTACATTAGGGTTAGGGTTACGGTTAGGGTTAGGG", "TTAGGG", 7, (29, 0, 0, 30, 29), Z),
    (b"ACGT" * 4, "ACGT", 3, (16, 16, 16, 16, 16), (16, 16, 16, 16, 16)),
    (b"TTAGG", "TTAGGG", 3, Z, Z),
    (b"ttagggTTAGGGttaggg", "TTAGGG", 3, (18, 18, 18, 18, 18), Z),  # lower-case bases are bases
]


@pytest.mark.parametrize("read,motif,penalty,fwd,rev", HAND)
def test_hand_worked_vectors(read, motif, penalty, fwd, rev):
    want = fwd + rev
    assert R.tracts_read(read, motif, penalty) == want
    assert tuple(int(x) for x in R.tracts([read], [motif], penalty)[0, 0]) == want
    assert tuple(int(x) for x in capi.tracts_host([read], [motif], penalty)[0, 0]) == want


def test_reference_forms_agree():
    rnd = random.Random(1)
    reads = [bytes(rnd.choice(b"ACGTACGTNa") for _ in range(rnd.randint(0, 80))) for _ in range(150)]
    reads += [b"TTAGGG" * 9, b"AATAATAATAATCCCTAACCCTAACCCTAA", b"TTAGGGTTAGGcTTAGGGTTnGGGTTAGGGACGTTTAGGGTTAGGG"]
    motifs = ["AAT", "TTAGGG", "TGTG", "AAAA"]
    for penalty in (1, 3, 64):
        got = R.tracts(reads, motifs, penalty)
        for r, read in enumerate(reads):
            for m, motif in enumerate(motifs):
                assert tuple(int(x) for x in got[r, m]) == R.tracts_read(read, motif, penalty)


@pytest.mark.parametrize("penalty", [1, 3, 7, 64])
def test_host_ragged_with_n_and_lower_case(penalty):
    reads = ragged_reads()
    motifs = ["AAT", "TGTG", "ACGTT", "TTAGGG"]  # k = 3, 4, 5, 6
    want = R.tracts(reads, motifs, penalty)
    for mi in range(len(motifs)):
        assert (want["head_len_fwd"][:, mi] >= 100).sum() >= 20 and (want["tail_len_fwd"][:, mi] >= 100).sum() >= 20
    same(capi.tracts_host(reads, motifs, penalty), want)


def test_generator_long_reads():
    reads = long_reads()
    want = R.tracts(reads, ["TTAGGG"], 3)
    # not vacuous, by the reference alone: the generator's 2-6 kb tails with 5 % substitutions are there on both strands ...
    tails = want["tail_len_fwd"][:, 0] >= 1500
    heads = want["head_len_rev"][:, 0] >= 1500
    assert tails.sum() >= 5 and heads.sum() >= 5
    # ... and the longest uninterrupted tract of those reads says next to nothing about them: the point of the feature
    annot = A.annotate(reads, ["TTAGGG"])
    assert annot["tract_len_fwd"][tails, 0].max() < 500 and annot["tract_len_rev"][heads, 0].max() < 500
    same(capi.tracts_host(reads, ["TTAGGG"], 3), want)


def test_noisy_tail_is_recovered():
    """The property that makes the measure useful, on the reference alone: a planted 2-6 kb tail with 5 % substitutions comes
    back within 5 % of its length at penalty 3, and as the head tract of the other strand on the reverse complement."""
    planted = planted_tail_reads()
    reads = [r for r, _ in planted]
    fwd = R.tracts(reads, ["TTAGGG"], 3)
    rc = R.tracts([A.revcomp(r) for r in reads], ["TTAGGG"], 3)
    for i, (read, tlen) in enumerate(planted):
        got = int(fwd["tail_len_fwd"][i, 0])
        assert abs(got - tlen) <= 0.05 * tlen, (tlen, got)
        assert int(rc["head_len_rev"][i, 0]) == got and int(rc["head_cov_rev"][i, 0]) == int(fwd["tail_cov_fwd"][i, 0])
        assert int(A.annotate([read], ["TTAGGG"])["tract_len_fwd"][0, 0]) < 500
    same(capi.tracts_host(reads, ["TTAGGG"], 3), fwd)


def test_host_accepts_packed_planes():
    reads = ragged_reads(300)
    packed = capi.pack_reads(reads)
    same(capi.tracts_host(packed, ["TTAGGG"], 3), capi.tracts_host(reads, ["TTAGGG"], 3))


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.tracts_host(reads, ["AAT"], penalty)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.tracts_host(reads, ["AAT"] * 9)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.tracts_host(reads, [])
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.tracts_host(reads, [capi.Motif(33, 0, 0)])
    with pytest.raises(capi.TrewHipError, match="bits above 2k"):
        capi.tracts_host(reads, [capi.Motif(3, 0, 64)])


def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Tract) == 40 and capi.TRACT_DTYPE.itemsize == 40
    assert tuple(capi.TRACT_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.Tract._fields_)
    assert C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Annot) == 24
    for sym in ("trew_hip_tracts", "trew_hip_tracts_results", "trew_tracts_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_tracts.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.tracts([b"TTAGGGTTAGGG"], ["TTAGGG"])
    r = subprocess.run([TREW, "tracts", "TTAGGG", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["tracts"], "MOTIF is required."),
        (["tracts", "TTAGGG"], "FASTQ is required."),
        (["tracts", "TTAGGN", FQ], "must consist of A, C, G and T."),
        (["tracts", "TTAGGG,", FQ], "the length must be in range 3 to 32."),
        (["tracts", "AC", FQ], "the length must be in range 3 to 32."),
        (["tracts", "A" * 33, FQ], "the length must be in range 3 to 32."),
        (["tracts", ",".join(["AAT"] * 9), FQ], "At most 8 motifs can be given."),
        (["tracts", "TTAGGG", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["tracts", "TTAGGG", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["tracts", "TTAGGG", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["tracts", "TTAGGG", FQ, "--min_tract", "0"], "MIN_TRACT must be greater than or equal to 1."),
        (["tracts", "TTAGGG", FQ, "--min_tract", "x"], "MIN_TRACT must be a number."),
        (["tracts", "TTAGGG", FQ, "-t", "0"], "number of threads must be positive."),
        (["tracts", "TTAGGG", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["tracts", "TTAGGG", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["tracts", "TTAGGG", FQ, "--devices", "0,x"], "Usage: tracts"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: tracts" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_tracts():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "tracts" in r.stderr and "annotate" in r.stderr and "short" in r.stderr and "long" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "tracts" in r.stderr
    r = subprocess.run([TREW, "tracts", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: tracts" in r.stderr and "--penalty" in r.stderr and r.stdout == ""
