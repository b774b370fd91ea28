"""Reads shared by tests/test_satellites_cpu.py and tests/test_gpu_satellites.py: tracts of units of up to 256 bases, built so
that the wide eq word, the pieces of the recursion, the 1024 consensus bins, the primitive root over 256 phases and the
sixteen unit words are met where the tests want them."""
import random

from period_cases import TEL, junk, noisy, rep
from repeat_cases import SAT, fenced, other

WIDE = [33, 40, 63, 64, 65, 68, 96, 100, 127, 128, 129, 155, 171, 178, 200, 234, 255, 256]
SHORT = [1, 2, 3, 5, 6, 7, 12, 19, 31, 32]
# sat_fuzz_reads(seed, FUZZ_N): seeds at which 30 reads or more have three tracts or more at (1, 256, 3, 8) and some tract has depth 3
FUZZ_SEEDS, FUZZ_N = (6, 7), 90


def monomer(k, seed=0):
    """a unit of k bases that is not a repeat of a shorter one (k >= 2: its first two bases differ from its last two)"""
    rnd = random.Random(7919 * k + seed)
    while True:
        u = junk(rnd, k)
        if k == 1 or all(u != rep(u[:d], k) for d in range(1, k) if k % d == 0):
            return u


def sat_fuzz_reads(seed, n=120, max_len=900):
    """ragged reads in the manner of period_cases.fuzz_reads: background with N and lower case; two reads of three carry one to
    five tracts one behind the other, each of a wide unit (33 .. 256 bases, two to four copies) or of a short one, with
    substitutions, indels and N, until the read has max_len bases"""
    rnd = random.Random(seed)
    alphabet = "ACGTACGTACGTACGTNacgtn"
    reads = []
    for i in range(n):
        if i % 3 == 0:
            reads.append(junk(rnd, rnd.randint(0, max_len), alphabet).encode())
            continue
        s = junk(rnd, rnd.randint(0, 80), alphabet)
        for _ in range(rnd.randint(1, 5)):
            k = rnd.choice(WIDE if rnd.random() < 0.4 else SHORT)
            want = rnd.randint(20, 120) if k <= 32 else rnd.randint(2 * k, 4 * k)
            if len(s) + want > max_len:
                continue
            s += noisy(rnd, junk(rnd, k), want, rnd.choice([0, 0.02, 0.05]), rnd.choice([0, 0, 0.005]), rnd.choice([0, 0.01]))
            s += junk(rnd, rnd.randint(0, 60), alphabet)
        reads.append(s.encode())
    return reads


# ---- the eq word
def eq_edge_reads(k, seed=0):
    """one exact tract of monomer(k) whose start (or end) lies at bit 30, 31, 0 or 1 around the start of word 1, 2, 63, 64,
    126 and 128; a tract that starts in the words 56 .. 63 has its partner bases in the next iteration's words.  Returns
    (reads, wanted): wanted[i] = (the position asked for, 'start' or 'end')."""
    rnd = random.Random(3000 * k + seed)
    unit, ln = monomer(k), 2 * k + max(k // 2, 40)
    reads, wanted = [], []
    for w in (1, 2, 63, 64, 126, 128):
        for d in (-2, -1, 0, 1):
            for side in ("start", "end"):
                at = 32 * w + d
                begin = at if side == "start" else at - ln
                if begin < 0:
                    continue
                t = rep(unit, ln, rnd.randrange(k))
                # the background next to the tract does not lengthen it
                reads.append(fenced(rnd, begin, right=t[k - 1]) + t + fenced(rnd, 45, left=t[len(t) - k]))
                wanted.append((at, side))
    return reads, wanted


def end_reads(k, seed=0):
    """tracts that end at or near the end of the read: the partner word of a position is then the read's last word, or a word
    that does not exist; every read length modulo 32 around a word boundary"""
    rnd = random.Random(3100 * k + seed)
    unit = monomer(k)
    return [junk(rnd, lead) + rep(unit, 2 * k + extra) + junk(rnd, tail) for lead in (0, 7, 32) for extra in (1, 17, 31, 32, 33)
            for tail in (0, 1, 5, 31, 32, 33)]


# ---- pieces
def tract_len(k):
    return max(3 * k, 30)


def wide_edge_reads(k, seed=0):
    """repeat_cases.edge_reads for a wide k: junk(o) + rep(U1, L1) + gap(g) + rep(U2, L2) + junk(9) for o = 0 .. 63,
    g in {0, 1, k - 1, k, 40}, L1 > L2 and L1 < L2, with (U1, U2) two different units of k bases in both orders and one unit
    twice.  The child piece behind or in front of the longer tract then starts or ends at every bit of a word.  Returns
    (reads, equal) as edge_reads does."""
    rnd = random.Random(1000 * k + seed)
    u, p = monomer(k), monomer(k, 1)
    reads, equal = [], []
    for u1, u2 in ((u, p), (p, u), (u, u)):
        for g in sorted({0, 1, k - 1, k, 40}):
            for longer_first in (True, False):
                for o in range(64):
                    l1 = l2 = tract_len(k)
                    if longer_first:
                        l1 += 17
                    else:
                        l2 += 17
                    if u1 == u2:
                        whole = rep(u1, l1 + g + l2)
                        gap = "".join(other(c, rnd) for c in whole[l1:l1 + g])
                        body = whole[:l1] + gap + whole[l1 + g:]
                    else:
                        body = rep(u1, l1) + junk(rnd, g) + rep(u2, l2)
                    reads.append(junk(rnd, o) + body + junk(rnd, 9))
                    equal.append((g, k) if u1 == u2 else None)
    return reads, equal


def wide_stack_reads(seed=0):
    """six tracts of wide units, of decreasing score, as a right-deep chain (the longest first), a left-deep chain (the longest
    last) and a balanced tree"""
    rnd = random.Random(640 + seed)
    ks = (171, 128, 97, 65, 41, 33)
    lens = [171 * 4, 128 * 4, 97 * 4, 65 * 4, 41 * 4 + 20, 33 * 4]
    tracts = [rep(monomer(k), n) for k, n in zip(ks, lens)]

    def build(order):
        return junk(rnd, 37) + "".join(tracts[i] + junk(rnd, 45) for i in order)

    return [build([0, 1, 2, 3, 4, 5]), build([5, 4, 3, 2, 1, 0]), build([3, 1, 4, 0, 5, 2])]


# ---- the consensus
def rotate_codes(text, r):
    """every base replaced by the base whose code is r larger (mod 4): T G C A in code order"""
    return "".join("TGCA"[("TGCA".index(c) + r) % 4] for c in text)


def majority_reads(k, seed=0):
    """five noisy copies of a unit, four times, the codes rotated by 0 .. 3: every base is the majority of every phase once"""
    rnd = random.Random(4000 * k + seed)
    body = noisy(rnd, monomer(k), 5 * k, 0.03)
    lead, tail = junk(rnd, 40), junk(rnd, 40)
    return [rotate_codes(lead + body + tail, r) for r in range(4)]


def tie_read(k):
    """two copies that differ at phases 5 and k - 1 and a third that ends in front of phase 5: both phases tie one to one.
    Returns (read, the two units)"""
    a = monomer(k)
    b = list(a)
    for j in (5, k - 1):
        b[j] = "TGCA"[("TGCA".index(a[j]) + 1 + (j & 1)) % 4]
    b = "".join(b)
    return a + b + a[:3], (a, b)


def n_phase_read(k):
    """three copies with N at phase 7 of every copy: no valid base there, code 0"""
    a = monomer(k)
    a = a[:7] + "N" + a[8:]
    return a * 3


def long_span_read(k=171, copies=15):
    """a tract longer than one iteration of 2048 bases"""
    rnd = random.Random(15)
    return junk(rnd, 70) + noisy(rnd, monomer(k), copies * k, 0.02) + junk(rnd, 50)


def root_vectors():
    """(read, K, period): scored at min_period = max_period = K, the consensus unit of K phases has the primitive root `period`"""
    out = []
    for K, d in ((256, 1), (256, 2), (256, 128), (252, 6), (127, 127), (171, 19), (255, 85), (256, 256), (192, 64)):
        out.append((rep(monomer(d), 3 * K + 11), K, d))
    return out


BOUNDARY_PERIODS = (15, 16, 17, 18, 31, 32, 33, 255, 256)  # the last base of the unit is base 14 .. 17, 30 .. 32, 254, 255


def boundary_reads():
    """(read, period): exact tracts whose unit ends at, one short of and one past a unit-word boundary; the unit ends with A
    (code 3), so both bits of the last base are set and everything above it must be zero"""
    out = []
    for d in BOUNDARY_PERIODS:
        u = monomer(d, 3)
        u = u[:-1] + ("A" if u[-2:-1] != "A" else "C")
        out.append((rep(u, 3 * d + 40), d))
    return out


def three_kinds(rnd, sub=0.0):
    """junk + (AATGG)n + junk + a 171-mer array + junk + (TTAGGG)n + junk: three tracts"""
    return (junk(rnd, 300) + noisy(rnd, SAT, 500, sub) + junk(rnd, 400) + noisy(rnd, monomer(171), 171 * 6, sub) + junk(rnd, 400) +
            noisy(rnd, TEL, 600, sub) + junk(rnd, 50))
