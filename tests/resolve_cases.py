"""Reads shared by tests/test_resolve_cpu.py and tests/test_gpu_resolve.py: the hand vectors, the reads whose candidates tie or
share a seed, the committed search for a short read that `resolve` repairs, and the shapes of the GPU test."""
import random

import period_ref
import refine_ref
import resolve_ref
from period_cases import junk, noisy, rep
from refine_cases import SEED_KEPT, T10, TEL, UNITS as REFINE_UNITS, rotations, with_deletion, with_insertion

ARGS = (1, 32, 3, 24)
FLANK = "ACGTACGT"
N_IN_SEED = T10[:14] + "N" + T10[15:]
# (ACG) x 11 and (ACGTT) x 7 both score 30 (k = 3 and k = 5) and nothing scores more: the smaller k is the earlier candidate
SCORE_TIE = "ACG" * 11 + "TTTTGTTGTG" + "ACGTT" * 7
# one primitive unit per unit length the GPU test uses
UNITS = dict(REFINE_UNITS)
UNITS.update({1: "A", 2: "TG"})
GPU_KS = (1, 2, 3, 6, 16, 17, 31, 32)
assert all(k in UNITS and len(UNITS[k]) == k for k in GPU_KS)

# (read, (min_period, max_period, penalty, min_score), candidates, the record in the order of resolve_ref.FIELDS)
HAND = [
    ("", ARGS, 3, (0,) * 18),
    ("A", ARGS, 3, (0,) * 18),
    ("AA", ARGS, 3, (0,) * 18),
    ("AAA", (1, 32, 3, 1), 4, (1, 1, 1, 0, 3, 0, 3, 3, 3, 3, 3, 0, 3, 3, 2, 0, 1, 3)),  # two admissible k, fewer than C
    ("A" * 40, ARGS, 3, (1, 1, 1, 0, 40, 0, 40, 40, 40, 40, 40, 0, 3, 3, 3, 0, 1, 40)),
    (T10, ARGS, 3, (6, 6, 6, 0, 60, 0, 60, 60, 60, 60, 60, 0, 213, 213, 3, 0, 6, 60)),
    (FLANK + T10 + FLANK, ARGS, 3, (6, 6, 6, 0, 60, 8, 68, 60, 60, 60, 60, 0, 213, 213, 3, 0, 6, 60)),
    (N_IN_SEED, ARGS, 3, (6, 6, 6, 0, 56, 0, 60, 60, 59, 56, 59, 0, 1347, 1347, 3, 0, 6, 56)),
    ("ACGTTGCATGCA", ARGS, 3, (0,) * 18),  # no candidate reaches min_score
]

# candidate 1 (k = 8) has the seed of candidate 0 (k = 4) rotated by two bases: it is aligned, not skipped
ROTATED_SEED = "TAGCTAGCTAGCTAGCTAGCAAGCTAGCTAGCTAGCTAGCTAGACTAGCTAGCTAGCTACTAGCTAGCTAGCTAGCTAGCTAGC"
# the shortest read that short_repaired finds: the winner is candidate 1
SHORT_SEED = 20250722
SHORT_REPAIRED = ("GTCGTGGGCTACTGGGCTACATGGGCACATGGGCTACTGGGCTACATGGGTACATGGGCTACATGGGCTACATGGCTACATGGGCTACATGGAGCTACATTGGCATGCATGGGCGTATCAAGGGCTATGGCCT"
                  "ACAATGGGCTACATGGGCATGGAGTAGCCAAGGCGGT")


def seeds_of(read, candidates=4, args=ARGS):
    """the primitive seeds of a read's candidates, as code lists, by the reference"""
    c = period_ref.codes(read)
    return [refine_ref.seed(c, R) for R in resolve_ref.candidate_records(c, *args, candidates)]


def short_repaired(seed=SHORT_SEED, tries=400):
    """the shortest of `tries` noisy reads under 400 bases (a unit of 5 .. 20 bases, substitutions 0.03, indels 0.06, flanks of
    0 .. 20) whose winner is not candidate 0, by the reference; the smallest text among the shortest"""
    rnd = random.Random(seed)
    reads = []
    for _ in range(tries):
        unit = junk(rnd, rnd.randint(5, 20))
        reads.append(junk(rnd, rnd.randint(0, 20)) + noisy(rnd, unit, rnd.randint(120, 360), 0.03, 0.06) + junk(rnd, rnd.randint(0, 20)))
    got = resolve_ref.resolve(reads)
    return min((r for r, x in zip(reads, got) if x["rank"] > 0), key=lambda r: (len(r), r))


def shape_reads(k, rnd):
    """(short, long): perfect, one-deletion, one-insertion and noisy reads of the unit of k bases for every listed length"""
    unit = UNITS[k]
    short, long_ = [], []
    for n in (0, 1, 2, 3, k, 2 * k - 1, 2 * k, 33, 2047, 2049):
        into = short if n <= 64 else long_
        perfect = rep(unit, n)
        into.append(perfect)
        into.append(with_deletion(perfect, n // 2) if n else perfect)
        into.append(with_insertion(perfect, n // 2, "C"))
        into.append(noisy(rnd, unit, n, 0.03, 0.06, 0.004))
    return short, long_


def mixed_reads(seed, n):
    """n short reads with different candidate counts next to each other: no repeat, one clean unit, noisy tracts of long units"""
    rnd = random.Random(seed)
    out = []
    for i in range(n):
        kind = i % 4
        if kind == 0:
            out.append(junk(rnd, rnd.randint(0, 90), "ACGTN"))
        elif kind == 1:
            out.append(junk(rnd, rnd.randint(0, 9)) + rep(junk(rnd, rnd.randint(1, 9)), rnd.randint(30, 120)))
        else:
            out.append(junk(rnd, rnd.randint(0, 9)) + noisy(rnd, junk(rnd, rnd.randint(5, 32)), rnd.randint(60, 260), 0.03, 0.06, 0.002) + junk(rnd, rnd.randint(0, 9)))
    return out


__all__ = ["ARGS", "FLANK", "GPU_KS", "HAND", "N_IN_SEED", "ROTATED_SEED", "SCORE_TIE", "SEED_KEPT", "SHORT_REPAIRED", "SHORT_SEED", "T10", "TEL", "UNITS",
           "mixed_reads", "rotations", "seeds_of", "shape_reads", "short_repaired"]
