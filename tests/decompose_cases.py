"""Reads shared by tests/test_decompose_cpu.py and tests/test_gpu_decompose.py: a small fuzz set the plain reference can walk,
the reads at the lengths where a wave-per-read kernel goes wrong, every rotation offset of a unit, the tracts cut to the walk's
block of rows, and the generator of the test of what the measure is for (planted variant units among indels)."""
import random

from align_cases import rotations, with_deletion, with_insertion
from period_cases import junk, noisy, rep
from refine_cases import GPU_KS, UNITS  # noqa: F401

ROW_BLOCK = 64  # kernels/trace.inc, kTraceBlock: the walk fetches the rows of a tract 64 at a time, counted down from its end
PLANTED_SEED = 20251019
PLANTED_NEIGHBOURS = tuple(PLANTED_SEED + d for d in (-4, -3, -2, -1, 1, 2, 3, 4))
# A read in which two phases of row `end` hold the record's tuple (rule 3 decides: the smaller phase), found by a search of 50 000
# short noisy reads with the reference; (read, penalty, min_score, the tied phases).  Repeating a unit cannot provoke the tie:
# refine reduces every unit to its primitive root.
END_TIE = ("TGTGATACACACCACAATCACACAACACACACACACCACCCGGAAGG", 1, 6, [2, 4])


def primitive_unit(rnd, k):
    unit = junk(rnd, k)
    while len(set(rotations(unit))) < k:
        unit = junk(rnd, k)
    return unit


def small_set(seed=7, per_k=2):
    """[(unit, read)] for k = 1 .. 32: a tract of 60 .. 260 bases of a random primitive unit with substitutions at 0.03, indels at
    0.06 and, in every fourth read, N, between random flanks of 0 .. 30 bases: short enough for the plain reference"""
    rnd = random.Random(seed)
    out = []
    for k in range(1, 33):
        for i in range(per_k):
            unit = primitive_unit(rnd, k)
            t = noisy(rnd, unit, rnd.randint(60, 260), 0.03, 0.06, 0.01 if (k + i) % 4 == 0 else 0.0)
            out.append((unit, junk(rnd, rnd.randint(0, 30)) + t + junk(rnd, rnd.randint(0, 30))))
    return out


def shape_reads(unit, seed):
    """trace_cases.shape_reads for a unit of any length >= 1: the read lengths 0, 1, k, 2k - 1, 2k, 31, 32, 33, 2047, 2048, 2049
    as perfect, shifted, noisy and random reads, and one deleted / one inserted base at bits 31 and 0 of a word and at the
    64-word seam (base 2047 / 2048)"""
    rnd = random.Random(seed)
    k = len(unit)
    reads = []
    for n in (0, 1, k, 2 * k - 1, 2 * k, 31, 32, 33, 2047, 2048, 2049):
        reads.append(rep(unit, n))
        reads.append(rep(unit, n, 1 % k))
        reads.append(noisy(rnd, unit, n, 0.03, 0.06, 0.005))
        reads.append(junk(rnd, n, "ACGTN"))
    base = rep(unit, 2200)
    for at in (31, 32, 63, 64, 2047, 2048):
        reads.append(with_deletion(base, at))
        reads.append(with_insertion(base, at, "ACGT"[(at + 1) % 4]))
        reads.append(with_insertion(with_deletion(base, at), at + 40, "A"))
    return reads


def rotation_reads(unit, copies=12):
    """a perfect repeat of `unit` begun at each of its k rotations"""
    k = len(unit)
    return [rep(unit, copies * k, q) for q in range(k)]


def block_reads(unit, seed=5):
    """Tracts of ROW_BLOCK q - 1, ROW_BLOCK q and ROW_BLOCK q + 1 bases for q = 1, 2, 3 -- the walk's last block holds all but
    one of its rows, all of them, and a single row -- perfect and with an indel next to the seam, at several offsets into the
    read.  The flank is drawn from N and the letters that the unit does not hold."""
    rnd = random.Random(seed)
    reads = []
    spare = [c for c in "ACGT" if c not in unit]
    for q in (1, 2, 3):
        for n in (ROW_BLOCK * q - 1, ROW_BLOCK * q, ROW_BLOCK * q + 1):
            for lead in (0, 1, 31, ROW_BLOCK - 1, ROW_BLOCK):
                t = rep(unit, n, rnd.randrange(len(unit)))
                flank = junk(rnd, lead, "".join(spare) + "N")
                reads.append(flank + t)
                reads.append(flank + with_deletion(t, n - ROW_BLOCK + 1) + "N")
                reads.append(flank + with_insertion(t, max(n - ROW_BLOCK - 1, 2), "N"))
    return reads


def planted(seed=PLANTED_SEED, n_reads=60, indel=0.04):
    """The reads of the test of what the measure is for: [(unit, read, [(copy, read position, j, base)])].  A read is (unit) x m
    with k = 3 .. 12 and m = 40 .. 60.  Three copies, at least four copies from either end and from each other, carry one
    substituted base each (phase j, the new base) and are otherwise exact; every base of the other copies is, with probability
    `indel`, followed by an inserted base or deleted (half each).  The read position is that of the substituted base."""
    rnd = random.Random(seed)
    out = []
    for i in range(n_reads):
        k = 3 + i % 10
        unit = primitive_unit(rnd, k)
        m = rnd.randint(40, 60)
        while True:
            at = sorted(rnd.sample(range(4, m - 4), 3))
            if at[1] - at[0] >= 4 and at[2] - at[1] >= 4:
                break
        parts, plants, n = [], [], 0
        for c in range(m):
            if c in at:
                j = rnd.randrange(k)
                base = rnd.choice([y for y in "ACGT" if y != unit[j]])
                s = unit[:j] + base + unit[j + 1:]
                plants.append((c, n + j, j, base))
            else:
                s = ""
                for ch in unit:
                    x = rnd.random()
                    if x < indel / 2:
                        s += ch + rnd.choice("ACGT")
                    elif x >= indel:
                        s += ch
            parts.append(s)
            n += len(s)
        out.append((unit, "".join(parts), plants))
    return out
