"""Reads shared by tests/test_trace_cpu.py and tests/test_gpu_trace.py: the hand vectors of the traceback, the reads at the
lengths where a wave-per-read kernel goes wrong, and the tracts cut to the block of rows the kernel's walk fetches at a time."""
import random

from align_cases import T10, TEL, revcomp, with_deletion, with_insertion
from period_cases import junk, noisy, rep

# kernels/trace.inc, kTraceBlock: the walk fetches the rows of a tract 64 at a time, counted down from the tract's end
ROW_BLOCK = 64

# (read, motif, penalty, min_score, strand, items as (start, bases, count, phase, consumed, mismatches, insertions, deletions))
HAND = [
    (T10, TEL, 3, 24, 0, [(0, 60, 10, 0, 60, 0, 0, 0)]),
    (T10[:27] + T10[28:], TEL, 3, 24, 0, [(0, 24, 4, 0, 24, 0, 0, 0), (24, 5, 1, 0, 6, 0, 0, 1), (29, 30, 5, 0, 30, 0, 0, 0)]),
    (T10[:27] + "C" + T10[27:], TEL, 3, 24, 0, [(0, 24, 4, 0, 24, 0, 0, 0), (24, 7, 1, 0, 6, 0, 1, 0), (31, 30, 5, 0, 30, 0, 0, 0)]),
    (T10[:27] + "C" + T10[28:], TEL, 3, 24, 0, [(0, 24, 4, 0, 24, 0, 0, 0), (24, 6, 1, 0, 6, 1, 0, 0), (30, 30, 5, 0, 30, 0, 0, 0)]),
    ("ACGTACGT" + T10 + "ACGTACGT", "GGGTTA", 3, 24, 0, [(8, 3, 1, 3, 3, 0, 0, 0), (11, 54, 9, 0, 54, 0, 0, 0), (65, 3, 1, 0, 3, 0, 0, 0)]),
    ("ACACACAC", "GGT", 1, 1, 1, [(1, 1, 1, 2, 1, 0, 0, 0), (2, 2, 1, 0, 3, 0, 0, 1), (4, 2, 1, 0, 3, 0, 0, 1), (6, 2, 1, 0, 2, 0, 0, 0)]),
]


def shape_reads(unit, seed):
    """The read lengths at which a wave-per-read kernel goes wrong (word and 64-word seams, reads shorter than the motif), as
    perfect, shifted, noisy and random reads, and one deleted / one inserted base at bits 31 and 0 of a word and at base
    2047 / 2048"""
    rnd = random.Random(seed)
    k = len(unit)
    reads = []
    for n in (0, 1, k - 1, k, 31, 32, 33, 2047, 2048, 2049):
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


def block_reads(unit=TEL, seed=5):
    """Tracts of ROW_BLOCK q - 1, ROW_BLOCK q and ROW_BLOCK q + 1 bases for q = 1, 2, 3 -- the walk's last block holds all but
    one of its rows, all of them, and a single row: a tract that ends at a block's first row and one that starts at a block's
    last -- perfect and with an indel next to the seam, at several offsets into the read, on both strands"""
    rnd = random.Random(seed)
    reads = []
    for q in (1, 2, 3):
        for n in (ROW_BLOCK * q - 1, ROW_BLOCK * q, ROW_BLOCK * q + 1):
            for lead in (0, 1, 31, ROW_BLOCK - 1, ROW_BLOCK):
                t = rep(unit, n, rnd.randrange(len(unit)))
                flank = "C" * lead if "C" not in unit else "A" * lead
                reads.append(flank + t)
                reads.append(flank + with_deletion(t, n - ROW_BLOCK + 1) + "AC")
                reads.append(revcomp(flank + with_insertion(t, max(n - ROW_BLOCK - 1, 2), "C")))
    return reads


def two_strand_reads(seed=11, n=12):
    """a noisy tract of TTAGGG and, behind a spacer, one of CCCTAA: both strands reach min_score, with different ranges; every
    third read has only one of them"""
    rnd = random.Random(seed)
    reads = []
    for i in range(n):
        a = noisy(rnd, TEL, rnd.randint(80, 400), 0.03, 0.06)
        b = revcomp(noisy(rnd, TEL, rnd.randint(80, 400), 0.03, 0.06))
        if i % 3 == 2:
            b = junk(rnd, len(b))
        parts = [junk(rnd, rnd.randint(0, 70)), a, junk(rnd, rnd.randint(20, 90)), b, junk(rnd, rnd.randint(0, 70))]
        if i % 2:
            parts[1], parts[3] = parts[3], parts[1]
        reads.append("".join(parts))
    return reads
