"""Reads shared by tests/test_refine_cpu.py and tests/test_gpu_refine.py: the hand vectors, the fuzz set of noisy long tracts
(period_cases.noisy: substitutions and indels) and the builders of reads whose longest run of eq_k lies at a chosen place."""
import random

from align_cases import UNITS as ALIGN_UNITS, rotations, with_deletion, with_insertion  # noqa: F401
from period_cases import junk, noisy, rep

TEL = "TTAGGG"
T10 = TEL * 10
# one primitive unit per unit length the GPU tests use
UNITS = dict(ALIGN_UNITS)
UNITS.update({1: "A", 2: "TG"})
GPU_KS = (1, 2, 3, 5, 6, 15, 16, 17, 31, 32)
FUZZ_SEED = 20250721


def fuzz_set(seed=FUZZ_SEED, per_k=3):
    """[(unit, read)] for k = 2 .. 32, per_k reads each: a tract of 600 .. 1500 bases of a random primitive unit with
    substitutions at 0.03 and indels at 0.06 (half insertions, half deletions) between random flanks of 0 .. 60 bases"""
    rnd = random.Random(seed)
    out = []
    for k in range(2, 33):
        for _ in range(per_k):
            unit = junk(rnd, k)
            while len(set(rotations(unit))) < k:  # primitive: no shorter period
                unit = junk(rnd, k)
            t = noisy(rnd, unit, rnd.randint(600, 1500), 0.03, 0.06)
            out.append((unit, junk(rnd, rnd.randint(0, 60)) + t + junk(rnd, rnd.randint(0, 60))))
    return out


def replaced(read, at):
    """the read with the base at `at` replaced by the next letter"""
    return read[:at] + "ACGT"[("ACGT".index(read[at]) + 1) % 4] + read[at + 1:]


def run_at(unit, lead, run, tail, rnd):
    """`lead` background bases, then a perfect repeat of `unit` whose eq_k run has `run` positions (run + k bases), then `tail`
    background bases.  The background is drawn so that its bases next to the repeat break the run."""
    k = len(unit)
    body = rep(unit, run + k)

    def other(c):
        return rnd.choice([y for y in "ACGT" if y != c])

    left = junk(rnd, lead)
    if lead:
        left = left[:-1] + other(body[k - 1])  # position lead - 1 is compared with body[k - 1]
    right = junk(rnd, tail)
    if tail:
        right = other(body[run]) + right[1:]  # position lead + run is compared with the first base behind the repeat
    return left + body + right


# a read whose re-voted unit (CCCA A -> AAAAC to AAAAA C: one phase changes) aligns with a lower score than the seed: the seed is kept
SEED_KEPT = ("GACAACCAAAACCAAAACAAAACCAAACCAAACCTAAAACCAAAACCATAAACTTACAAAACCAAAACCAAAACAAAACAAAGAACTAAACCAAAACCATAACCAGAACCAAATCGCAATTT")
FLANK = "ACGTACGT"
# (read, (min_period, max_period, penalty, min_score), the record in the order of refine_ref.FIELDS)
HAND = [
    (FLANK + T10 + FLANK, (1, 32, 3, 24), (6, 6, 6, 0, 60, 8, 68, 60, 60, 60, 60, 0, 213, 213)),   # a perfect repeat with flanks
    (T10, (1, 32, 3, 24), (6, 6, 6, 0, 60, 0, 60, 60, 60, 60, 60, 0, 213, 213)),
    ("A" * 40, (1, 32, 3, 24), (1, 1, 1, 0, 40, 0, 40, 40, 40, 40, 40, 0, 3, 3)),                    # unit length 1
    ("TG" * 30, (1, 32, 3, 24), (2, 2, 2, 0, 60, 0, 60, 60, 60, 60, 60, 0, 1, 1)),                   # unit length 2
    (T10[:14] + "N" + T10[15:], (1, 32, 3, 24), (6, 6, 6, 0, 56, 0, 60, 60, 59, 56, 59, 0, 1347, 1347)),  # an N inside the seed window
    ("", (1, 32, 3, 24), (0,) * 14),
    ("ACGTTGCATGCA", (1, 32, 3, 24), (0,) * 14),                                                     # no periods record
]
