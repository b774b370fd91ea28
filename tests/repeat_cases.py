"""Reads shared by tests/test_repeats_cpu.py and tests/test_gpu_repeats.py: reads with several tracts, built so that the
pieces of the recursion start and end where the tests want them."""
import random

from period_cases import TEL, UNITS, junk, noisy, rep

SAT = "AATGG"


def other(c, rnd):
    return rnd.choice([y for y in "ACGT" if y != c])


def fenced(rnd, n, left=None, right=None):
    """n bases of background whose first base is not `left` and whose last is not `right`: a tract next to it is not
    lengthened by a chance match at its very end"""
    s = list(junk(rnd, n))
    if n and left:
        s[0] = other(left, rnd)
    if n and right:
        s[-1] = other(right, rnd) if n > 1 or not left else rnd.choice([y for y in "ACGT" if y not in (left, right)])
    return "".join(s)


def two_satellites(rnd, sub=0.0):
    """junk(300) + (AATGG)n x 900 b + junk(500) + (TTAGGG)n x 600 b + junk(10)"""
    return junk(rnd, 300) + noisy(rnd, SAT, 900, sub) + junk(rnd, 500) + noisy(rnd, TEL, 600, sub) + junk(rnd, 10)


def tract_len(k):
    return max(3 * k, 30)


def edge_reads(k, seed=0):
    """junk(o) + rep(U1, L1) + gap(g) + rep(U2, L2) + junk(9) for o = 0 .. 63, g in {0, 1, k - 1, k, 40}, L1 > L2 and L1 < L2,
    with (U1, U2) = (UNITS[k], partner), (partner, UNITS[k]) and (UNITS[k], UNITS[k]).  The child piece behind or in front of
    the longer tract then starts or ends at every bit of a word.  With equal units the second tract goes on in the phase of
    the first and every gap base differs from the base the phase asks for: for g < k the bases on either side of the piece
    boundary match at period k.  Returns (reads, equal): equal[i] = (g, k) for the reads of equal units, else None."""
    rnd = random.Random(1000 * k + seed)
    u, p = UNITS[k], UNITS[6 if k != 6 else 2]
    reads, equal = [], []
    for u1, u2 in ((u, p), (p, u), (u, u)):
        for g in sorted({0, 1, k - 1, k, 40}):
            for longer_first in (True, False):
                for o in range(64):
                    l1, l2 = tract_len(len(u1)), tract_len(len(u2))
                    if longer_first:
                        l1 = max(l1, l2) + 17
                    else:
                        l2 = max(l1, l2) + 17
                    if u1 == u2:
                        whole = rep(u1, l1 + g + l2)
                        gap = "".join(other(c, rnd) for c in whole[l1:l1 + g])
                        body = whole[:l1] + gap + whole[l1 + g:]
                    else:
                        body = rep(u1, l1) + junk(rnd, g) + rep(u2, l2)
                    reads.append(junk(rnd, o) + body + junk(rnd, 9))
                    equal.append((g, k) if u1 == u2 else None)
    return reads, equal


def seam_reads(k, seed=0):
    """A parent tract of 400 bases of AATGG that ends at `lo`, then a child piece of more than 2048 bases with one tract of
    UNITS[k] whose start (or end) lies at bit 30, 31, 0 or 1 around the start of the piece's own words 63, 64, 65, 127 and 128
    -- the words of the piece's iteration grid, which starts at word lo >> 5 -- for lo at bit 31, bit 0 and bit 13 of its
    word.  Returns (reads, wanted): wanted[i] = (lo, the position asked for, 'start' or 'end')."""
    rnd = random.Random(2000 * k + seed)
    unit, small = UNITS[k], max(5 * k, 40)
    reads, wanted = [], []
    for lo_bit in (31, 0, 13):
        for w in (63, 64, 65, 127, 128):
            for d in (-2, -1, 0, 1):
                for side in ("start", "end"):
                    lead = 64 + (lo_bit - 400) % 32  # lo = lead + 400 has the wanted bit
                    lo = lead + 400
                    assert lo % 32 == lo_bit
                    at = 32 * ((lo >> 5) + w) + d
                    begin = at if side == "start" else at - small
                    t = rep(unit, small, rnd.randrange(k))
                    big = rep(SAT, 400)
                    # the background next to a tract does not lengthen it: base begin - 1 differs from base begin - 1 + k = t[k - 1]
                    read = fenced(rnd, lead, right=big[0]) + big + fenced(rnd, begin - lo, left=SAT[400 % 5], right=t[k - 1]) + t
                    read += fenced(rnd, 60, left=t[len(t) - k]) + junk(rnd, 40)
                    reads.append(read)
                    wanted.append((lo, at, side))
    return reads, wanted


def k32_seam_reads(seed=0):
    """k = 32 in a child piece: eq positions in the piece's own word 63, their partner bases in its word 64"""
    rnd = random.Random(3200 + seed)
    reads = []
    for lo_bit in (31, 0):
        lead = 64 + (lo_bit - 400) % 32
        lo = lead + 400
        for rel in (2016, 2017, 2040, 2047, 2048):
            for ln in (64, 65, 96):
                for tail in (0, 1, 50):
                    at = 32 * (lo >> 5) + rel
                    reads.append(junk(rnd, lead) + rep(SAT, 400) + junk(rnd, at - lo) + rep(UNITS[32], ln) + junk(rnd, tail))
    return reads


def stack_reads(seed=0):
    """six tracts of decreasing length in three orders: a right-deep chain (the longest first), a left-deep chain (the longest
    last) and a balanced tree; and one read with 64 short tracts.  No period of 1 .. 32 fits two neighbouring tracts (the least
    common multiple of any two of the units' lengths is above 32), so no segment bridges the background between them."""
    rnd = random.Random(64 + seed)
    units = [junk(rnd, k) for k in (32, 31, 29, 27, 25, 23)]
    lens = [420, 340, 270, 200, 140, 90]
    tracts = [rep(u, n) for u, n in zip(units, lens)]

    def build(order):
        return junk(rnd, 37) + "".join(tracts[i] + junk(rnd, 45) for i in order)

    short = [junk(rnd, k) for k in (7, 9, 11, 13)]
    many = "".join(junk(rnd, 40) + rep(short[i % 4], 48) for i in range(64)) + junk(rnd, 40)
    return [build([0, 1, 2, 3, 4, 5]), build([5, 4, 3, 2, 1, 0]), build([3, 1, 4, 0, 5, 2]), many]
