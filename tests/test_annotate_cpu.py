"""Per-read motif annotation, the parts that need no GPU: the brute-force reference against hand-worked vectors, the host
implementation (trew_annotate_host) against the reference, motif parsing, the argument errors of `trew annotate`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as R
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, motif) %s: got %s, want %s" % (
            f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def short_reads(n=20000):
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, 150)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


HAND = [
    (b"TTAGGG" * 5, "TTAGGG", (25, 0, 0, 30, 0, 0)),
    (b"CCCTAA" * 5 + b"N" + b"TTAGGG" * 3, "TTAGGG", (13, 25, 31, 18, 0, 30)),
    (b"ACGT" * 4, "ACGT", (13, 13, 0, 16, 0, 16)),
    (b"TTAGG", "TTAGGG", (0, 0, 0, 0, 0, 0)),
    (b"GGTTAG", "TTAGGG", (1, 0, 0, 6, 0, 0)),
    (b"", "TTAGGG", (0, 0, 0, 0, 0, 0)),
    # two tracts of 9 bases: the earlier one is reported; a lower-case base is a base, an N is not
    (b"GGGTTAGGGACGGGTTAGGG", "TTAGGG", (8, 0, 0, 9, 0, 0)),
    (b"ttagggTTAGGGnTTAGGGTTAGGGT", "TTAGGG", (15, 0, 13, 13, 0, 0)),
    # non-primitive motif and homopolymer
    (b"TGTGTGTGA", "TGTG", (5, 0, 0, 8, 0, 0)),
    (b"CAAAAAC", "AAA", (3, 0, 1, 5, 0, 0)),
]


@pytest.mark.parametrize("read,motif,want", HAND)
def test_hand_worked_vectors(read, motif, want):
    assert R.annotate_read(read, motif) == want
    assert tuple(R.annotate([read], [motif])[0, 0]) == want
    assert tuple(capi.annotate_host([read], [motif])[0, 0]) == want


def test_reference_forms_agree():
    rnd = random.Random(1)
    reads = [bytes(rnd.choice(b"ACGTACGTNa") for _ in range(rnd.randint(0, 80))) for _ in range(150)]
    reads += [b"TTAGGG" * 9, b"AATAATAATAATCCCTAACCCTAACCCTAA"]
    motifs = ["AAT", "TTAGGG", "TGTG", "AAAA"]
    got = R.annotate(reads, motifs)
    for r, read in enumerate(reads):
        for m, motif in enumerate(motifs):
            assert tuple(got[r, m]) == R.annotate_read(read, motif)


def test_host_short_one_motif():
    reads = short_reads()
    want = R.annotate(reads, ["TTAGGG"])
    # not vacuous: the generator makes 1.5 % telomeric or junction reads, half of them reverse-complemented
    assert (want["tract_len_fwd"] >= 24).sum() >= 50
    assert (want["tract_len_rev"] >= 24).sum() >= 50
    same(capi.annotate_host(reads, ["TTAGGG"]), want)


def test_host_short_eight_motifs():
    reads = short_reads()

    def cut(k, which):
        s = reads[which][5:5 + k].decode().upper()
        assert set(s) <= set("ACGT")
        return s

    motifs = ["AAT", "tgtg", "CCCTA", "TTAGGG", "GGGTTAG", cut(12, 7), cut(31, 0), cut(32, 100)]
    assert [len(m) for m in motifs] == [3, 4, 5, 6, 7, 12, 31, 32]
    want = R.annotate(reads, motifs)
    for mi in range(len(motifs)):
        assert want["windows_fwd"][:, mi].sum() > 0
    same(capi.annotate_host(reads, motifs), want)


def test_host_ragged_with_n_and_lower_case():
    rnd = random.Random(77)
    reads = []
    for i in range(2000):
        ln = rnd.randint(0, 1000)
        if i % 3 == 0:
            unit = rnd.choice(["TTAGGG", "CCCTAA", "AAT", "TGTG", "ACGTT"])
            s = (unit * (ln // len(unit) + 2))[rnd.randint(0, 5):][:ln]
            s = "".join(rnd.choice("ACGTNacgtn") if rnd.random() < 0.02 else c for c in s)
        else:
            s = "".join(rnd.choice("ACGTACGTACGTACGTNacgtnR") for _ in range(ln))
        reads.append(s.encode())
    motifs = ["TTAGGG", "AAT", "TGTG", "AAAA", "ACGTT"]
    same(capi.annotate_host(reads, motifs), R.annotate(reads, motifs))


def test_host_long_reads():
    buf, st, nd = capi.synth_long_ascii(20250218, 0, 200)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    motifs = ["TTAGGG", "AAT"]
    want = R.annotate(reads, motifs)
    assert want["tract_len_fwd"][:, 0].max() >= 24 and want["tract_len_rev"][:, 0].max() >= 24
    same(capi.annotate_host(reads, motifs), want)


def test_host_accepts_packed_planes():
    reads = short_reads(500)
    packed = capi.pack_reads(reads)
    same(capi.annotate_host(packed, ["TTAGGG"]), capi.annotate_host(reads, ["TTAGGG"]))


def test_motif_parse_round_trips_and_rejections():
    for text in ("TTAGGG", "ttaggg", "AAT", "ACGT" * 8, "TtAgGgC"):
        m = capi.motif(text)
        assert m.k == len(text) and m.reserved == 0
        assert m.word == R.word_of(text.upper())
        back = "".join("TGCA"[(m.word >> (2 * (m.k - 1 - i))) & 3] for i in range(m.k))
        assert back == text.upper()
    for text in ("", "AC", "A" * 33, "TTAGGN", "TTA GGG", "TTAGGG\n", "UUAGGG"):
        with pytest.raises(capi.TrewHipError):
            capi.motif(text)


def test_host_rejects_bad_motifs():
    reads = [b"ACGTACGT"]
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.annotate_host(reads, ["AAT"] * 9)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.annotate_host(reads, [])
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.annotate_host(reads, [capi.Motif(33, 0, 0)])
    with pytest.raises(capi.TrewHipError, match="bits above 2k"):
        capi.annotate_host(reads, [capi.Motif(3, 0, 64)])


def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Annot) == 24
    assert capi.FLAG_DEBUG_ANNOT_GENERAL == 8192


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_annotate.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.annotate([b"TTAGGGTTAGGG"], ["TTAGGG"])
    r = subprocess.run([TREW, "annotate", "TTAGGG", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["annotate"], "MOTIF is required."),
        (["annotate", "TTAGGG"], "FASTQ is required."),
        (["annotate", "TTAGGN", FQ], "must consist of A, C, G and T."),
        (["annotate", "TTAGGG,", FQ], "the length must be in range 3 to 32."),
        (["annotate", "AC", FQ], "the length must be in range 3 to 32."),
        (["annotate", "A" * 33, FQ], "the length must be in range 3 to 32."),
        (["annotate", ",".join(["AAT"] * 9), FQ], "At most 8 motifs can be given."),
        (["annotate", "TTAGGG", FQ, "--min_tract", "0"], "MIN_TRACT must be greater than or equal to 1."),
        (["annotate", "TTAGGG", FQ, "--min_tract", "x"], "MIN_TRACT must be a number."),
        (["annotate", "TTAGGG", FQ, "-t", "0"], "number of threads must be positive."),
        (["annotate", "TTAGGG", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["annotate", "TTAGGG", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["annotate", "TTAGGG", FQ, "--devices", "0,x"], "Usage: annotate"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_annotate():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "annotate" in r.stderr and "short" in r.stderr and "long" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "annotate" in r.stderr
    r = subprocess.run([TREW, "annotate", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: annotate" in r.stderr and r.stdout == ""
