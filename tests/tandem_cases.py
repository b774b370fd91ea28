"""Reads shared by tests/test_tandems_cpu.py and tests/test_gpu_tandems.py: the hand vectors, the weak read (a periods record
that no single unit aligns to with min_score), the two-tract set of noisy long reads, and the builders of reads whose pieces
start and end where the tests want them."""
import random

from period_cases import TEL, junk, noisy, rep
from refine_cases import UNITS, rotations
from repeat_cases import SAT, fenced

FLANK = "ACGTACGT"
# a drifting unit: AAAC -> AAAG -> AACG.  periods scores 48 at k = 4 over [0, 60); the refined record scores 23 at the defaults
WEAK = "AAAC" * 5 + "AAAG" * 5 + "AACG" * 5
# the weak tract is the depth-0 piece (48 against the 30 of six telomere units): the strong tract is found below it, at depth 1
WEAK_FIRST = WEAK + "GATC" + TEL * 6 + "CATG"
# the strong tract is the depth-0 piece; the weak one lies in the piece behind it and gives no record
STRONG_FIRST = FLANK + TEL * 12 + "GTGT" + WEAK
TWO_PERFECT = FLANK + TEL * 10 + "ACGTTGCA" + SAT * 12 + "ACGT"
# (read, [(depth,) + the record in the order of refine_ref.FIELDS, start and end in read coordinates], in the order of start)
HAND = [
    (TWO_PERFECT, [(1, 6, 6, 6, 0, 60, 8, 68, 60, 60, 60, 60, 0, 213, 213), (0, 5, 5, 5, 0, 61, 76, 137, 61, 61, 61, 61, 0, 965, 965)]),
    (WEAK, []),
    (WEAK_FIRST, [(1, 6, 6, 6, 0, 36, 64, 100, 36, 36, 36, 36, 0, 213, 213)]),
    (STRONG_FIRST, [(0, 6, 6, 6, 0, 72, 8, 80, 72, 72, 72, 72, 0, 213, 213)]),
    ("", []),
    ("ACGTTGCATGCA", []),
]
TWO_TRACT_SEED = 20251015


def primitive_unit(rnd, k):
    unit = junk(rnd, k)
    while len(set(rotations(unit))) < k:  # primitive: no shorter period
        unit = junk(rnd, k)
    return unit


def two_tract_set(seed=TWO_TRACT_SEED, n=30):
    """[(read, [(unit, start, end), (unit, start, end)])]: two tracts of 300 .. 700 bases of random primitive units of 2 .. 12
    bases (two different canonical units a read) with substitutions at 0.03 and indels at 0.06, 40 .. 120 random bases between
    them and 0 .. 40 at each end"""
    import period_ref as P

    def canon(u):
        return P.canonical(P.pack_unit([P.CODE[c] for c in u]), len(u))

    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        u1 = primitive_unit(rnd, rnd.randint(2, 12))
        u2 = primitive_unit(rnd, rnd.randint(2, 12))
        while len(u1) == len(u2) and canon(u1) == canon(u2):
            u2 = primitive_unit(rnd, rnd.randint(2, 12))
        read, planted = junk(rnd, rnd.randint(0, 40)), []
        for i, u in enumerate((u1, u2)):
            t = noisy(rnd, u, rnd.randint(300, 700), 0.03, 0.06)
            planted.append((u, len(read), len(read) + len(t)))
            read += t + junk(rnd, rnd.randint(40, 120) if i == 0 else rnd.randint(0, 40))
        out.append((read, planted))
    return out


EXTENT_UNIT = "TAGTTGTGCCGCA"


def extent_read():
    """A tract whose refined extent is wider than its periods tract: twelve copies of a unit of 13 bases with one base deleted
    (at 76 of the tract) and one inserted (at 103).  A slipped phase costs the fixed-phase score of `periods` about a whole
    unit, more than the copies behind the first slip bring back, so the periods tract ends at the first slip; the alignment
    pays one penalty a slip and bridges both.  Around the periods tract the copies behind the slip would be a tract of their
    own; around the refined tract nothing of the unit is left.  Behind it a spacer and a tract of AATGG."""
    t = EXTENT_UNIT * 12
    t = t[:76] + t[77:103] + "C" + t[103:]
    return "GATCGATC" + t + "ACGTTGCAAGCT" + SAT * 10 + "ACGT"


def piece_bound_reads(k, seed=0):
    """A depth-0 tract of 200 bases of AATGG that ends at `lo`, then the child piece [lo, n) with one tract of UNITS[k] that starts
    at the piece's first base or ends at its last, for lo at bit 31, 0 and 1 of a word and, with a long lead, on either side of
    the 64-word seam (2047, 2048, 2049).  The child's longest run and its seed window then lie at the piece's first (or last)
    bases.  The tract that begins at lo does so with a base that does not continue AATGG, and an N sits five bases in front of
    lo, inside the depth-0 tract: just outside the piece.  Returns (reads, wanted): wanted[i] = (lo, True when the child's
    tract starts at lo, False when it ends at n)."""
    rnd = random.Random(7000 + 10 * k + seed)
    unit, small = UNITS[k], max(6 * k, 48)
    big = rep(SAT, 200, 2)  # the base that would continue it is SAT[(2 + 200) % 5] = T
    reads, wanted = [], []
    for lo in (255, 256, 257, 2047, 2048, 2049):
        for at_start in (True, False):
            head = fenced(rnd, lo - 200, right=big[0])
            t = next(rep(unit, small, ph) for ph in range(k, -1, -1) if rep(unit, small, ph)[0] != "T")
            if at_start:
                read = head + big[:195] + "N" + big[196:] + t + fenced(rnd, 30, left=t[len(t) - k])
            else:
                read = head + big + fenced(rnd, 37, left="T", right=t[k - 1]) + t
            reads.append(read)
            wanted.append((lo, at_start))
    return reads, wanted


def piece_hi_reads(k, seed=0):
    """The mirror of piece_bound_reads: a depth-0 tract of 300 bases of AATGG that STARTS at `hi`, so that the piece in front of it
    ends there, for hi at bit 31, 0 and 1 of a word and on either side of the 64-word seam.  Two shapes.  'end': the piece is
    [0, hi) and its tract of UNITS[k] ends at the piece's last base (hi in 255 .. 257 and 2047 .. 2049: the seam of the piece's own
    grid).  'both': a depth-1 tract of 230 bases of AC ends at lo, and the tract of UNITS[k] fills the depth-2 piece [lo, hi) from
    its first base to its last, both mid-word (hi in 543 .. 545 and 2047 .. 2049).  The child's longest run and seed window then
    lie at the piece's last bases.  Where the unit allows it the first base behind hi goes on with the child's unit (a look one
    base past hi would lengthen the tract), otherwise it differs; the base in front of hi does not go on backwards with AATGG,
    so the depth-0 tract starts at hi; an N sits four bases behind hi, inside the depth-0 tract: at a penalty of 3 a tract
    does not begin within four bases in front of an N, so that is the nearest an N outside the piece can lie.  Returns (reads,
    wanted): wanted[i] = (lo, hi, shape), lo = 0 for 'end'."""
    rnd = random.Random(9000 + 10 * k + seed)
    unit, small = UNITS[k], max(6 * k, 48)
    big = rep(SAT, 300)  # starts with A; the base that would go on backwards is SAT[4] = G
    big = big[:4] + "N" + big[5:]
    reads, wanted = [], []
    for shape, his in (("end", (255, 256, 257, 2047, 2048, 2049)), ("both", (543, 544, 545, 2047, 2048, 2049))):
        for hi in his:
            # the phases whose last base is not G; first those whose next base would be the A behind hi
            phases = [ph for ph in range(k) if rep(unit, small, ph)[-1] != "G"]
            phases.sort(key=lambda ph: rep(unit, small + 1, ph)[-1] != "A")
            t = rep(unit, small, phases[0])
            tail = fenced(rnd, 30, left=SAT[300 % 5])
            if shape == "end":
                read = fenced(rnd, hi - small, right=t[k - 1]) + t + big + tail
                lo = 0
            else:
                lo = hi - small
                mid = next(rep("AC", 230, ph) for ph in (0, 1) if rep("AC", 231, ph)[-1] != t[0])  # AC does not go on into the child
                read = fenced(rnd, lo - 230, right=mid[1]) + mid + t + big + tail
            reads.append(read)
            wanted.append((lo, hi, shape))
    return reads, wanted
