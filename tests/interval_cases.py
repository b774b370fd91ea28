"""Inputs shared by test_intervals_cpu.py and test_gpu_intervals.py: the ragged-read recipe of test_gpu_tracts.py, the
generator's long reads, the rule sets, and comparison helpers.  No test of its own."""
import random

import numpy as np

import interval_ref as R
from trew_amd import capi

LONG_N = 300
TEL = "TTAGGG"
RAGGED_MOTIFS = ["AAT", "TGTG", "ACGTT", TEL]  # k = 3, 4, 5, 6
# (max_gap, min_len): an int, or a factor of k as text
RULES = [(0, 1), (1, 1), ("k", "4k"), ("3k", "4k"), (40, 1), (5000, 1)]


def rule_values(rule, motifs):
    def val(v, k):
        return int(v[:-1] or 1) * k if isinstance(v, str) else v
    return [val(rule[0], len(m)) for m in motifs], [val(rule[1], len(m)) for m in motifs]


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


def same(got, want):
    """(records, counts) pairs: every record and every count, integer for integer"""
    grec, gcnt = got[0], got[1]
    wrec, wcnt = want[0], want[1]
    assert gcnt.shape == wcnt.shape
    bad = np.argwhere(gcnt != wcnt)
    assert len(bad) == 0, "count differs at (read, motif, strand) %s: got %d, want %d" % (bad[0].tolist(), gcnt[tuple(bad[0])], wcnt[tuple(bad[0])])
    assert len(grec) == len(wrec), "%d records, want %d" % (len(grec), len(wrec))
    for f in R.FIELDS:
        bad = np.flatnonzero(grec[f] != wrec[f])
        assert len(bad) == 0, "%s differs at record %d: got %s, want %s" % (f, bad[0], grec[bad[0]], wrec[bad[0]])


def triples(recs, read=0, motif=0, strand=0):
    sel = recs[(recs["read"] == read) & (recs["motif"] == motif) & (recs["strand"] == strand)]
    return [(int(x["start"]), int(x["end"]), int(x["covered"])) for x in sel]
