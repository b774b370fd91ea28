"""Reads and units shared by tests/test_copies_cpu.py and tests/test_gpu_copies.py: the fuzz set of the host definition, the
end-phase tie read for k > 32, one deleted and one inserted base at every position of four copies, tracts around the walk's
block, and runs of deleted and inserted bases across phase k - 1 -> 0 and across a lane seam."""
import random

import monomer_cases as MC
from align_cases import revcomp  # noqa: F401
from period_cases import junk, noisy, rep

# both ends of each Q (phases a lane: 1 up to 64, 2 up to 128, 4 up to 256) and every k mod Q
GPU_KS = (3, 33, 63, 64, 65, 127, 128, 129, 130, 131, 171, 255, 256)
HOST_KS = (33, 47, 64, 65, 100, 128, 129, 171, 193, 255, 256)
FUZZ_SEED = 20251021  # chosen with the reference: more than half of the keys carry a D/I tie or a d tie on the traced path

q_of = MC.q_of
unit_of = MC.unit_of


def block_of(k):
    """the rows of the walk's LDS block in a call whose largest unit has k bases: 4 KB a wave, 64 Q bytes a row"""
    return 64 // q_of(k)


def host_fuzz(seed=FUZZ_SEED, per_k=2):
    """[(unit, reads)] for HOST_KS: tracts of about two copies of a random primitive unit with substitutions at 0.03 and
    indels at 0.06, one read in two with N, between random flanks of 0 .. 20 bases; the second read of a unit is the reverse
    complement of such a read, so that strand rev is traced"""
    rnd = random.Random(seed)
    out = []
    for k in HOST_KS:
        unit = unit_of(k, 7)
        reads = []
        for i in range(per_k):
            t = noisy(rnd, unit, 2 * k + rnd.randint(20, 60), 0.03, 0.06, 0.005 if i % 2 == 0 else 0.0)
            read = junk(rnd, rnd.randint(0, 20)) + t + junk(rnd, rnd.randint(0, 20))
            reads.append(revcomp(read) if i % 2 else read)
        out.append((unit, reads))
    return out


# (AAT) x 40 against the unit (AAT) x 22: every third phase of the last row holds the end cell's tuple
TIE_UNIT, TIE_READ = "AAT" * 22, "AAT" * 40

EDIT_K = 65


def edit_unit():
    """a primitive 65-base unit whose first and last base differ: no run of equal bases spans a copy boundary"""
    for seed in range(100):
        u = unit_of(EDIT_K, 40 + seed)
        if u[0] != u[-1]:
            return u
    raise AssertionError


def edit_reads(unit):
    """[(read, kind, copy, offset)]: six copies of the unit with the base at every position p of the four inner copies deleted,
    and with one base inserted in front of it that differs from both its neighbours.  copy: the index of the copy the edit
    lands in (an inserted base belongs to the segment of the base before it), offset: p within the read"""
    k = len(unit)
    whole = unit * 6
    out = []
    for p in range(k, 5 * k):
        out.append((whole[:p] + whole[p + 1:], "del", p // k, p))
        x = next(b for b in "ACGT" if b != whole[p - 1] and b != whole[p])
        out.append((whole[:p] + x + whole[p:], "ins", (p - 1) // k, p))
    return out


def block_reads(k, seed=5):
    """tracts of B - 1, B, B + 1 and 2 B + 1 bases around the walk's block of B rows, perfect and with an indel next to the
    seam, at several offsets into the read, on both strands.  (A tract shorter than min_score gives no items: the caller picks
    min_score below B - 1.)"""
    rnd = random.Random(seed + k)
    unit = unit_of(k, 11)
    B = block_of(k)
    reads = []
    for n in (B - 1, B, B + 1, 2 * B + 1):
        for phase in (0, k - 1):
            t = rep(unit, n, phase)
            lead = junk(rnd, rnd.choice((0, 1, 31, 33)))
            reads.append(lead + t + junk(rnd, 5))
            reads.append(revcomp(lead + t + junk(rnd, 5)))
            if n > 12:
                reads.append(lead + t[:n - 6] + t[n - 5:] + junk(rnd, 3))     # a deleted base next to the seam
                reads.append(lead + t[:6] + "ACGT"[rnd.randrange(4)] + t[6:])  # an inserted base next to the other end
    return unit, reads


def run_reads(k):
    """runs of d deleted and d inserted bases across phase k - 1 -> 0 and across a lane seam (phase Q * 17), d in {1, Q, 63,
    64, k - 1} where d < k, behind and in front of two copies (monomer_cases.with_deleted_run / with_inserted_run)"""
    unit = unit_of(k, 13)
    Q = q_of(k)
    rnd = random.Random(900 + k)
    reads = []
    for d in sorted({1, Q, 63, 64, k - 1}):
        if d >= k:
            continue
        for phase in (k - 1, (k - d // 2) % k, (Q * 17) % k, (Q * 17 - 1) % k):
            reads.append(MC.with_deleted_run(unit, phase, d, copies=2, lead=junk(rnd, 7), tail=junk(rnd, 7)))
            reads.append(MC.with_inserted_run(unit, phase, junk(rnd, d), copies=2, lead=junk(rnd, 7), tail=junk(rnd, 7)))
    return unit, reads


def shape_reads(k, seed=3):
    """reads of n in {0, 1, k - 1, k, k + 1, 2 k + 1} bases and around a 32-base word and the 64-word seam (2048 bases): perfect,
    shifted, noisy and random"""
    rnd = random.Random(seed * 1000 + k)
    unit = unit_of(k, 17)
    reads = ["", "A"]
    for n in (k - 1, k, k + 1, 2 * k + 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049):
        reads.append(rep(unit, n, 0))
        reads.append(rep(unit, n, rnd.randrange(k)))
        reads.append(noisy(rnd, unit, n, 0.03, 0.06, 0.005))
        reads.append(junk(rnd, n, "ACGTN"))
    return unit, reads
