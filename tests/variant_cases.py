"""Inputs and comparisons shared by test_variants_cpu.py and test_gpu_variants.py."""
import random

import numpy as np

import variant_ref as R

# k = 3, 5, 6, 6 (its own reverse complement), 7, 16, 31, 32
MOTIFS = ["AAT", "ACGTT", "TTAGGG", "AAATTT", "TTAGGGC", "TTAGGGTTAGGGTCAG", "ACGTTGCATGCCATGGTTAACCGATCGATTA", "ACGTTGCATGCCATGGTTAACCGATCGATTAG"]
assert [len(m) for m in MOTIFS] == [3, 5, 6, 6, 7, 16, 31, 32] and R.revcomp("AAATTT") == "AAATTT"


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.argwhere(got[f] != want[f])
        assert len(bad) == 0, "%s differs at (read, motif) %s: got %s, want %s" % (
            f, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def rc_read(read):
    """reverse complement of a read that may hold N and lower-case letters"""
    tr = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    return bytes(read).translate(tr)[::-1]


def swapped(rec):
    out = np.zeros_like(rec)
    for f in R.FIELDS:
        out[f] = rec[f.replace("_fwd", "_x").replace("_rev", "_fwd").replace("_x", "_rev")]
    return out


def noisy_reads(n=400, seed=11, max_len=900):
    """ragged reads: random sequence, or flanks around a tract of one of MOTIFS (either strand) with substitutions, a few N,
    lower-case letters and now and then an inserted or deleted base"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        ln = rnd.randint(0, max_len)
        if i % 4 == 3:
            out.append("".join(rnd.choice("ACGTACGTACGTACGTNacgtnR") for _ in range(ln)).encode())
            continue
        unit = rnd.choice(MOTIFS)
        if rnd.random() < 0.5:
            unit = R.revcomp(unit)
        rate = rnd.choice([0.0, 0.01, 0.05, 0.1])
        tract = []
        for c in unit * (ln // len(unit) + 1):
            x = rnd.random()
            if x < rate:
                c = rnd.choice("ACGT")
            elif x < rate + 0.002:
                c = rnd.choice(["N", "", c + rnd.choice("ACGT"), c.lower()])
            tract.append(c)
        flank = "".join(rnd.choice("ACGT") for _ in range(rnd.randint(0, 60)))
        out.append((flank + "".join(tract) + flank[::-1])[:ln + 60].encode())
    return out
