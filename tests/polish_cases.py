"""Reads shared by tests/test_polish_cpu.py and tests/test_gpu_polish.py: the fuzz set of noisy arrays of long units, the
low-indel set of short units, one error at every 7th position of a 68-base unit, and the hand-made reads above 32 bases (an N
in the seed window, a seed that is kept, a seed whose root is a proper divisor of the scored period)."""
import random

from monomer_cases import q_of, unit_of  # noqa: F401
from period_cases import junk, noisy, rep
from refine_cases import replaced, run_at  # noqa: F401

FUZZ_KS = (33, 40, 48, 64, 65, 68, 100, 128, 129, 171, 200, 234, 256)
FUZZ_SEED = 20251021   # chosen with the reference: the three conditions of test_polish_cpu.py hold (the counts stand there)
SHORT_SEED = 20251022  # chosen with the reference: at least three quarters of the reads keep their scored period at 64, 128, 256
COPIES = 20


def planted_set(ks, seed, per_k, sub, indel):
    """[(unit, read, begin, end)]: per_k reads for every k, COPIES copies of a random primitive unit with substitutions at a
    rate drawn from `sub` and indels from `indel` (half insertions, half deletions), between random flanks of 0 .. 60 bases;
    [begin, end) is the planted array"""
    rnd = random.Random(seed)
    out = []
    for k in ks:
        for i in range(per_k):
            unit = unit_of(k, seed % 1000 + i)
            t = noisy(rnd, unit, COPIES * k, rnd.uniform(*sub), rnd.uniform(*indel))
            lead = junk(rnd, rnd.randint(0, 60))
            out.append((unit, lead + t + junk(rnd, rnd.randint(0, 60)), len(lead), len(lead) + len(t)))
    return out


def fuzz_set(seed=FUZZ_SEED):
    """k in FUZZ_KS, three reads each, substitutions 0.02 .. 0.03, indels 0.003 .. 0.01"""
    return planted_set(FUZZ_KS, seed, 3, (0.02, 0.03), (0.003, 0.01))


def short_set(seed=SHORT_SEED):
    """k = 2 .. 32, three reads each, substitutions 0.02 .. 0.03, indels 0.01"""
    return planted_set(range(2, 33), seed, 3, (0.02, 0.03), (0.01, 0.01))


U68 = unit_of(68, 11)


def one_error_reads():
    """[(kind, at, read)]: (U68) x 8 with one deleted, one inserted and one replaced base at every 7th position"""
    body = U68 * 8
    out = []
    for at in range(0, len(body), 7):
        extra = "ACGT"[("ACGT".index(body[at]) + 2) % 4]  # differs from the base it stands in front of
        out += [("del", at, body[:at] + body[at + 1:]), ("ins", at, body[:at] + extra + body[at:]), ("sub", at, replaced(body, at))]
    return out


def n_in_seed_window(k=100, at=80, lead=0, tail=0):
    """Two copies and twenty bases of a 100-base unit with an N at `at`, between `lead` and `tail` N: the runs of eq_k are
    [0, at) and [at + 1, k + 20), the first is the longest, so the seed window is the first copy, the N lies in it at phase
    `at` >= 64 and the consensus supplies the base (from position k + at).  Asserted here with the reference."""
    import period_ref
    import refine_ref

    unit = unit_of(k, 12)
    body = unit * 2 + unit[:20]
    read = "N" * lead + body[:at] + "N" + body[at + 1:] + "N" * tail
    c = period_ref.codes(read)
    R = period_ref.period_read(read, 1, 256, 3, 24)
    start, end = int(R[3]), int(R[4])
    rs = refine_ref.longest_run(period_ref.eq_k(c, k), start, end - k)
    assert int(R[1]) == k and rs == start == lead and "N" in read[rs:rs + k] and (lead + at - start) % k == at >= 64
    assert refine_ref.seed(c, R) == [period_ref.CODE[b] for b in unit]  # the N took the unit's base
    return read


def divisor_read(k=17, copies=12):
    """a perfect repeat of a 17-base unit: with min_period = 34 the scored period is 34 and the seed's root 17"""
    return "ACGTTGCA" + unit_of(k, 13) * copies + "TGCATGCA"


# a read whose re-voted unit aligns with a lower score than the seed, with a period above 32: found by search with the
# reference (polish_ref.polish_read, P = 3, min_score 24); SEED_KEPT_ARGS are the arguments of the search
SEED_KEPT_ARGS = (1, 256, 3, 24)
SEED_KEPT = ("TGATACTCGGAGGACCCGTCAACGCTCCTCCATGGGATTCCGGAGGACCCGTCAACGCTCCTCCATGGGGTCCCCGGAGGACCCGTACAACGCTCAGCATGGGATACCCGGAGGACACGTCAACGCTCCTCCAATTGGGATTCCCGGAGGACCCGTCTACGCTCCTATTCCA")


# ---- the longest run of eq_k at chosen places (the builders of tests/test_gpu_refine.py for any unit length)
def with_subs(read, subs):
    for at in subs:
        read = replaced(read, at)
    return read


def runs_of(read, k):
    """[(start, length)] of the runs of eq_k of a read of A, C, G and T"""
    eq = [read[i] == read[i + k] for i in range(len(read) - k)] + [False]
    out, i = [], 0
    while i < len(eq):
        if eq[i]:
            j = i
            while eq[j]:
                j += 1
            out.append((i, j - i))
            i = j
        else:
            i += 1
    return out


def runs_read(unit, start, length, count=1):
    """A perfect repeat with replaced bases: a replaced base at p clears eq_k at p - k and at p, so the runs lie between them.
    `count` runs of `length` positions, the first at `start`, one replaced base between two of them; every other run has 39."""
    k = len(unit)
    ends = [start + (i + 1) * (length + k + 1) - 1 for i in range(count)]
    n = ends[-1] + 100 + k
    read = with_subs(rep(unit, n), list(range(start - 1, -1, -(40 + k))) + ends + list(range(ends[-1] + 40 + k, n, 40 + k)))
    longest = sorted(runs_of(read, k), key=lambda r: (-r[1], r[0]))
    assert longest[:count] == [(start + i * (length + k + 1), length) for i in range(count)] and longest[count][1] < length
    return read


def with_deletion(read, at):
    return read[:at] + read[at + 1:]


def with_insertion(read, at, base):
    return read[:at] + base + read[at:]


# every planted unit length at which the kernel takes another path: both ends of each Q and every k mod Q
GPU_KS = (1, 2, 3, 6, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 171, 253, 254, 255, 256)


# Reads at whose tied votes the record depends on the smallest phase winning (polish_ref.tie_matters: with the vote given to another
# tied phase the re-vote gives another unit, support or number of changed phases), found by search with the reference, P = 3:
# (max_period of the call, Q of its layout, read, whether such a tie lies in two slots of one lane, whether one lies in two lanes)
TIE_READS = [
    (64, 1, "ATGCACTGACGGGAGAGACAGGATAACCCGTAAGGCACGAACCCTTTGGGCGGGACAGACGGCTAACACGTAAGGCACGAACCCTTTGGGCGGGAGAGACGGATAACATGAAGGCAAGGAACCCTTTGTGCGGGAGTGACGGATAATACGTAGGGCACGAACCCTTTGCGCGGGAGCTA", False, True),
    (128, 2, "CAGTAGAGGGAGAGCGATGGCTTTGCAACGCTTTAACGCTCTCTTGAGCCGTGATCAGAGGTGCGTGTAGGCCCAGTCGTCTAGGCCCTACTCGTTATCTCTGTAGAAGGAGAGATATGGCTTGGCAACGCTTTAGCGGTTTCTTGAGCCTGGATCAGGGGGTCGTGTAGGCCCAGTCGTACTTGGTGCTACACGTCATTCTGTAGAAGGAGAGCTATGGCTTTGCAACGCTTTAGCGGTTGCTTGTCCCTGGATCAGAGGTACGTGTAGGCACAGTCGAACTAGGCGCTCCTCGTTATTCTGTAGATAGAGAGCTACGGCTTTGCAACGCATTAGCGCTTGCTTGAGCCTACGTC", False, True),
    (128, 2, "CTCCTAGCCCGTTGAATGTAACGTAACCAGTCAATGAATGTTTATGGATCAAGTTGTGTTATCACAAGAGATACTTGACCCCCAAAGTCACCATACTTAGCCTCTCCACCGCGCTGAATGTAACGTAACCATTCCAGGTTTGTTCATGGTTCAAGTTGTGTTATCTCAAGTAAACTTACCCCCCAAGTCACCGTACTACGCTCTCCAGCACGTGGGAATGTATCGTAACCAGTCAATGGTTGTTCATGGATCAAGTTGTGTTATCTCAAATAAACTTTACCCCCCAAGTCACCGTCCTACCCTCTCCAGCGAGTTGGATGTAACGTACCCAGTCAATGTTTGCTCATGGATCAAGATGTGTTATCTCAAGTAAACTCTACCCCCCAGTCTCACGTACTATAA", True, False),
    (256, 4, "TGTTAGTTTGCCCGCATCATGTATATTTCAGACGCCGTTCTTCAAGGTCTGGCCCCGGCGCGCGGCTGGTGACTTAAGCCAAACGTTGTTCGACAGTCCGTCCGCCCCGTGAGCCGACGCCGGCCAGCAGGCTCCGCAGAAACGTCCGCAGCCCGGAGACAAGGTCCTAACAAAGTTGTTTAGCCCGGATCATGTATCTTTCAGACGCCGTCCTTCAACGTCTGGGCCGGTGTCGGCTGGTGACTGAAGCCCAACGCGGTTCGACAGTCCGTCCGCCCAGAAACACGCGGCGGCCAGAAGATTTCGCAGAAACGCCCGAACCCAGGACACAAGGTCCGATCAAAGTCGTTTTGCCCGCATTATGTATATATCATACGCCGTTCTTCAACGTCTAGGCCGGTGCGCGGCTGGTGACTTAAGCCCAACGCTGTTCTACAGTCACGTCCGCCCAGAAATAGCCTCCGGCCACCAGGTTCGCAGTAACACCCGCACCCCGGTCACAAGGTCCTAAGAAAGTTTTTTTGCCCGCACCATGTATATTTCAGACGCCGTTCTTCAACGTCTGGGCCGGTGCGCGGCTGGTGACTTAAGCCCAACGCTGTTCGACAGTCCTGTA", True, True),
]
