"""Reads and units shared by tests/test_monomers_cpu.py and tests/test_gpu_monomers.py: random primitive units of 3 to 256
bases, the fuzz set of the host definition, arrays of diverged monomers, and reads with runs of deleted and inserted unit
bases at chosen phases."""
import random

from align_cases import revcomp, rotations  # noqa: F401
from period_cases import junk, noisy, rep

# every k at which the kernel takes another path: both ends of each Q (phases a lane: 1 up to 64, 2 up to 128, 4 up to 256),
# k mod 4 = 0, 1, 2, 3 at Q = 4, and a last lane with one live slot
GPU_KS = (3, 4, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 130, 171, 253, 254, 255, 256)
HOST_KS = (33, 47, 63, 64, 65, 100, 127, 128, 129, 171, 192, 193, 255, 256)


def q_of(k):
    return 1 if k <= 64 else 2 if k <= 128 else 4


def unit_of(k, seed=0):
    """a random primitive unit of k bases, the same for the same (k, seed)"""
    rnd = random.Random(1000003 * seed + k)
    unit = junk(rnd, k)
    while len(set(rotations(unit))) < k:
        unit = junk(rnd, k)
    return unit


def host_fuzz(seed=20250917, per_k=3):
    """[(unit, reads)] for HOST_KS: tracts of 2k + 20 .. 60 bases of a random primitive unit with substitutions at 0.03 and
    indels at 0.06, one read in three with N, between random flanks of 0 .. 20 bases (all on the forward strand: the mirror
    is a test of its own)"""
    rnd = random.Random(seed)
    out = []
    for k in HOST_KS:
        unit = unit_of(k, 7)
        reads = []
        for i in range(per_k):
            t = noisy(rnd, unit, 2 * k + rnd.randint(20, 60), 0.03, 0.06, 0.005 if i % 3 == 0 else 0.0)
            reads.append(junk(rnd, rnd.randint(0, 20)) + t + junk(rnd, rnd.randint(0, 20)))
        out.append((unit, reads))
    return out


def diverged(rnd, unit, sub, indel):
    """one copy of the unit, every base substituted at rate `sub`, and at rate `indel` deleted or followed by an extra base"""
    out = []
    for c in unit:
        x = rnd.random()
        if x < sub:
            out.append(rnd.choice([b for b in "ACGT" if b != c]))
        elif x < sub + indel / 2:
            continue
        elif x < sub + indel:
            out.append(c + rnd.choice("ACGT"))
        else:
            out.append(c)
    return "".join(out)


ARRAY_SEED = 1  # chosen with the reference: the tract at P = 2 begins and ends one base from the plant
ARRAY_K, ARRAY_COPIES, ARRAY_FLANK = 171, 6, 150


def diverged_array(seed=ARRAY_SEED):
    """(consensus, read, plant begin, plant end, a random read of the same length): six copies of a random 171-base consensus,
    each independently diverged by 18 % substitutions and 2 % indels, between random flanks of 150 bases"""
    rnd = random.Random(seed)
    consensus = unit_of(ARRAY_K, 3)
    array = "".join(diverged(rnd, consensus, 0.18, 0.02) for _ in range(ARRAY_COPIES))
    read = junk(rnd, ARRAY_FLANK) + array + junk(rnd, ARRAY_FLANK)
    return consensus, read, ARRAY_FLANK, ARRAY_FLANK + len(array), junk(rnd, len(read))


def with_deleted_run(unit, phase, d, copies=3, lead="", tail=""):
    """`copies` whole units from phase 0, then the unit's next d bases from `phase` on left out, then `copies` more units'
    worth of bases: a run of d deleted unit bases that starts at `phase` (d = k leaves no trace)"""
    k = len(unit)
    head = rep(unit, copies * k + phase, 0)
    rest = rep(unit, copies * k, (phase + d) % k)
    return lead + head + rest + tail


def with_inserted_run(unit, phase, text, copies=3, lead="", tail=""):
    k = len(unit)
    return lead + rep(unit, copies * k + phase, 0) + text + rep(unit, copies * k, phase % k) + tail
