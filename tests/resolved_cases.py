"""Reads shared by tests/test_resolved_cpu.py and tests/test_gpu_resolved.py: the long-unit two-tract set on which the period
choice per piece shows, and the builder that puts a read behind a depth-0 tract as its child piece."""
import random

from period_cases import junk, noisy, rep
from repeat_cases import SAT, fenced
from tandem_cases import primitive_unit

ARGS = (1, 32, 3, 24)
LONG_UNIT_SEED = 20251020
CHILD_LOS = (255, 256, 257, 2047, 2048, 2049)


def long_unit_set(seed=LONG_UNIT_SEED, n=30):
    """tandem_cases.two_tract_set with units of 13 .. 32 bases and tracts of 400 .. 900: [(read, [(unit, start, end)] * 2)], two
    tracts of random primitive units (two different canonical units a read) with substitutions at 0.03 and indels at 0.06,
    40 .. 120 random bases between them and 0 .. 40 at each end.  At these unit lengths the fixed-phase score often prefers a
    multiple or a neighbour of the planted period."""
    import period_ref as P

    def canon(u):
        return P.canonical(P.pack_unit([P.CODE[c] for c in u]), len(u))

    rnd = random.Random(seed)
    out = []
    for _ in range(n):
        u1 = primitive_unit(rnd, rnd.randint(13, 32))
        u2 = primitive_unit(rnd, rnd.randint(13, 32))
        while len(u1) == len(u2) and canon(u1) == canon(u2):
            u2 = primitive_unit(rnd, rnd.randint(13, 32))
        read, planted = junk(rnd, rnd.randint(0, 40)), []
        for i, u in enumerate((u1, u2)):
            t = noisy(rnd, u, rnd.randint(400, 900), 0.03, 0.06)
            planted.append((u, len(read), len(read) + len(t)))
            read += t + junk(rnd, rnd.randint(40, 120) if i == 0 else rnd.randint(0, 40))
        out.append((read, planted))
    return out


def child_read(child, lo, seed=0):
    """`child` as the child piece [lo, n) of a read, as tandem_cases.piece_bound_reads builds one: random bases, then a depth-0
    tract of 200 bases of AATGG that ends at lo with an N five bases in front of lo, then `child`.  The tract's phase is the
    first of 2, 3, 4, 0, 1 at which the child's first base does not continue AATGG (2 unless the child begins with T)."""
    assert lo >= 200
    rnd = random.Random(11000 + lo + seed)
    big = next(rep(SAT, 200, ph) for ph in (2, 3, 4, 0, 1) if SAT[(ph + 200) % 5] != child[0])
    return fenced(rnd, lo - 200, right=big[0]) + big[:195] + "N" + big[196:] + child


def child_reads(child, los=CHILD_LOS):
    return [child_read(child, lo) for lo in los]
