"""Reads shared by tests/test_dissect_cpu.py and tests/test_gpu_dissect.py, built from the helpers of the measures dissect is
composed of (tandem_cases, decompose_cases, period_cases, refine_cases): the smallest shapes at which a kernel that traces every
tract of a read, as opposed to its two parents, can go wrong -- a traced tract in a child piece, whose rows restart at a start
that is not the read's; the walk's row block counted down from the end of a tract that is not the read's first; rule 3 decided
in a child; the stack holding an entry while a trace runs."""
import random

from decompose_cases import END_TIE, ROW_BLOCK, block_reads  # noqa: F401
from period_cases import junk, noisy, rep
from refine_cases import GPU_KS, UNITS  # noqa: F401
from repeat_cases import SAT
from tandem_cases import HAND, piece_bound_reads, piece_hi_reads, primitive_unit, two_tract_set  # noqa: F401

SPACER = "ACGTTGCAAGCT"
HAND_READS = [read for read, _ in HAND]
BLOCK_UNIT = "TTAGGC"
LONG_SEED = 20251021


def bound_reads():
    """tandem_cases.piece_bound_reads and piece_hi_reads for every unit length of the GPU tests: a traced tract in a child piece
    whose lo or hi sits at bit 31, 0 and 1 of a word and on either side of the 64-word seam"""
    reads = []
    for k in GPU_KS:
        reads += piece_bound_reads(k)[0] + piece_hi_reads(k)[0]
    return reads


def behind_first(read, n=200):
    """`read` behind a tract of n bases of AATGG and a spacer: what `read` holds lies in a child piece"""
    return rep(SAT, n) + SPACER + read


def child_block_reads():
    """decompose_cases.block_reads (tracts of 64 q - 1, 64 q and 64 q + 1 bases, q = 1, 2, 3) behind a depth-0 tract of 200 bases
    of AATGG: the walk's row block is counted down from the end of a tract that is not the read's first"""
    return [behind_first(r) for r in block_reads(BLOCK_UNIT)]


def end_tie_child():
    """(read, penalty, min_score, the tied phases, the first base of END_TIE's read): decompose_cases.END_TIE's read directly
    behind a stronger depth-0 tract of AATGG, so that rule 3 is decided in a child piece.  At END_TIE's penalty of 1 the depth-0
    tract takes five bases of the read along; the child piece [105, n) has the record of END_TIE's read, shifted, and by the
    reference (tests/test_dissect_cpu.py) the same two phases of its row `end` hold the record's tuple."""
    read, penalty, min_score, phases = END_TIE
    head = rep(SAT, 100)
    return head + read, penalty, min_score, phases, len(head)


def short_unit_reads():
    """units of length 1 and 2 as the second tract, behind a longer tract of AATGG, and as the first with TTAGGG behind"""
    return [behind_first("A" * 60 + "CGT"), behind_first("TG" * 40 + "CCA"), behind_first("C" + "GT" * 31 + "A" + "GT" * 20),
            "A" * 90 + SPACER + "TTAGGG" * 10, "TG" * 50 + SPACER + "A" * 40 + "CGCG"]


def three_tract_reads(seed=3):
    """Three tracts in one read: the middle one the strongest, so both children of the depth-0 piece hold a tract and the longer
    one waits on the stack while the shorter is traced; perfect and noisy, with the longer child on either side"""
    rnd = random.Random(seed)
    reads = []
    for a, b, c in ((60, 200, 90), (90, 200, 60), (120, 260, 121)):
        reads.append(junk(rnd, 7) + rep("TTAGGG", a) + SPACER + rep(SAT, b) + "GATC" + rep("ACCTG", c, 2) + junk(rnd, 5))
        reads.append(junk(rnd, 3) + noisy(rnd, "TTAGGG", a, 0.02, 0.04) + SPACER + noisy(rnd, SAT, b, 0.02, 0.04) + "GATCGATC"
                     + noisy(rnd, "ACCTGCA", c, 0.02, 0.04) + junk(rnd, 9))
    return reads


def long_read(seed=LONG_SEED):
    """one read of at most 20 000 bases with three noisy tracts of more than 2 048 bases each, random bases around them"""
    rnd = random.Random(seed)
    read = junk(rnd, 150)
    for unit, n in (("TTAGGG", 5200), (SAT, 6100), ("ACCTGCATG", 4300)):
        read += noisy(rnd, unit, n, 0.03, 0.06) + junk(rnd, rnd.randint(200, 400))
    assert len(read) <= 20000
    return read


def cli_reads(seed=11, n_plain=12):
    """the reads of the command-line test: the two-tract reads among reads without a tract and short reads"""
    rnd = random.Random(seed)
    reads = []
    for read, _ in two_tract_set():
        reads.append(read)
        if rnd.random() < 0.4:
            reads.append(junk(rnd, rnd.randint(1, 200)))
    reads += [junk(rnd, rnd.randint(30, 300)) for _ in range(n_plain)] + HAND_READS[:4] + three_tract_reads()
    return [r for r in reads if r]
