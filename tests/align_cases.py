"""Reads shared by tests/test_align_cpu.py and tests/test_gpu_align.py: hand vectors, the fuzz set with substitutions, indels
and N (period_cases.noisy), and the builders of reads with errors at chosen places."""
import random

from period_cases import junk, noisy, rep

TEL = "TTAGGG"
# one unit per motif length the GPU tests use: the cyclic wrap at the half-row (15, 16, 17), row (31, 32) and small ends
UNITS = {3: "AAT", 5: "CCCTA", 6: TEL, 15: "GATTACAGGCTTAAC", 16: "GATTACAGGCTTAACG", 17: "GATTACAGGCTTAACGT",
         31: "GATTACAGGCTTAACGGTCATTGCAAGCTAG", 32: "GATTACAGGCTTAACGGTCATTGCAAGCTAGG"}
assert all(len(u) == k for k, u in UNITS.items())
GPU_KS = (3, 5, 6, 15, 16, 17, 31, 32)

_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s.upper()))


def rotations(unit):
    return [unit[i:] + unit[:i] for i in range(len(unit))]


# (read, motif, penalty, fwd record, rev record): score, start, end, consumed, matches
Z = (0, 0, 0, 0, 0)
T10 = TEL * 10
HAND = [
    (T10, TEL, 3, (60, 0, 60, 60, 60), (2, 1, 3, 2, 2)),
    (T10[:27] + T10[28:], TEL, 3, (56, 0, 59, 60, 59), (2, 1, 3, 2, 2)),             # one base removed: one deletion
    (T10[:27] + "C" + T10[27:], TEL, 3, (57, 0, 61, 60, 60), (2, 1, 3, 2, 2)),       # one base added: one insertion
    (T10[:27] + "C" + T10[28:], TEL, 3, (56, 0, 60, 60, 59), (2, 1, 3, 2, 2)),       # one base replaced: one mismatch
    (T10[:27] + "N" + T10[28:], TEL, 3, (56, 0, 60, 60, 59), (2, 1, 3, 2, 2)),       # an N matches nothing
    ("ACGTACGT" + T10 + "ACGTACGT", "GGGTTA", 3, (60, 8, 68, 60, 60), (2, 0, 2, 2, 2)),  # a rotation; rev: AC of TAACCC
    (revcomp(T10), TEL, 3, (2, 3, 5, 2, 2), (60, 0, 60, 60, 60)),
    ("", TEL, 3, Z, Z),
    ("AAAAAAAA", "GGC", 1, Z, Z),
    ("ACACACAC", "GGT", 1, Z, (5, 1, 8, 9, 7)),  # P = 1 against ACC: C AC(C)AC(C)AC, two deleted bases
]


def fuzz_sets(seed=20250601, per_k=7, lo=150, hi=320):
    """[(motif, reads)] for k = 3 .. 32: tracts of a random unit with substitutions at 0.03 and indels at 0.06 (half
    insertions, half deletions), some with N, between random flanks; every third read reverse-complemented."""
    rnd = random.Random(seed)
    out = []
    for k in range(3, 33):
        unit = junk(rnd, k)
        while len(set(rotations(unit))) < k:  # primitive: no shorter period
            unit = junk(rnd, k)
        reads = []
        for i in range(per_k):
            t = noisy(rnd, unit, rnd.randint(lo, hi), 0.03, 0.06, 0.005 if i % 4 == 0 else 0.0)
            s = junk(rnd, rnd.randint(0, 40)) + t + junk(rnd, rnd.randint(0, 40))
            reads.append(revcomp(s) if i % 3 == 2 else s)
        out.append((unit, reads))
    return out


def with_deletion(read, at, d=1):
    return read[:at] + read[at + d:]


def with_insertion(read, at, text="C"):
    return read[:at] + text + read[at:]
