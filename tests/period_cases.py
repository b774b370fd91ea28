"""Reads shared by tests/test_periods_cpu.py and tests/test_gpu_periods.py: the hand vectors, the tie vectors, and the
builders of tracts in an aperiodic background."""
import random

TEL = "TTAGGG"
# the four k <= 32 motifs of the reference's known-answer test (test.cpp:172-214)
KAT32 = ["TTGCATCACACCCTCGCCG", "TTAGGG", "TTAGAGCCCACA", "TTTTGCCCTCATCACACCCTCGCCTCCTTCGC"]
# one primitive unit per period the word- and iteration-boundary tests use
UNITS = {1: "A", 2: "TG", 3: "AAT", 6: TEL, 31: "GATTACAGGCTTAACGGTCATTGCAAGCTAG", 32: "GATTACAGGCTTAACGGTCATTGCAAGCTAGG"}
assert all(len(u) == k for k, u in UNITS.items())


def rep(unit, n, phase=0):
    return (unit * (n // len(unit) + 3))[phase:phase + n]


def junk(rnd, n, alphabet="ACGT"):
    return "".join(rnd.choice(alphabet) for _ in range(n))


def _scores(read):
    import period_ref as R

    c = R.codes(read)
    return [R.segment_prefix(R.eq_k(c, k), 3)[0] for k in range(1, min(32, len(c) - 1) + 1)]


def tie_reads(gap, lead=33):
    """(TG)x10 and (TTAGGG)x4 both score 18 (k = 2 and k = 6), `gap` bases of spacer apart, in both orders: k* = 2 each time.
    Then two identical (TTAGGG)x8 tracts (score 42) `gap` apart: the earlier one is reported.  The spacers are random
    sequence, drawn again until no period bridges them or lengthens a tract: the two scores are exact and the largest."""
    a, b = "TG" * 10, TEL * 4
    out = []
    for first, second, score in ((a, b, 18), (b, a, 18), (TEL * 8, TEL * 8, 42)):
        for seed in range(1000):
            rnd = random.Random(seed)
            read = junk(rnd, lead) + first + junk(rnd, gap) + second + junk(rnd, 9)
            mid = lead + len(first) + gap // 2
            k1, k2 = (2 if first == a else 6), (2 if second == a else 6)
            if max(_scores(read)) == score and _scores(read[:mid])[k1 - 1] == score and _scores(read[mid:])[k2 - 1] == score:
                break
        else:
            raise AssertionError("no spacer found")
        out.append(read)
    return out


def noisy(rnd, unit, n, sub=0.0, indel=0.0, n_rate=0.0):
    """n bases of `unit` from a random phase with substitutions, single-base insertions / deletions and N"""
    out = []
    for c in rep(unit, n, rnd.randrange(len(unit))):
        x = rnd.random()
        if x < sub:
            out.append(rnd.choice([y for y in "ACGT" if y != c]))
        elif x < sub + indel / 2:
            out.append(c + rnd.choice("ACGT"))
        elif x < sub + indel:
            pass
        elif x < sub + indel + n_rate:
            out.append("N")
        else:
            out.append(c)
    return "".join(out)[:n]


def fuzz_reads(seed, n=400, max_len=700):
    """ragged reads of 0 .. max_len bases: background with N and lower case, and in two reads of three one or two tracts of a
    random unit of 1 .. 32 bases with substitutions, indels and N"""
    rnd = random.Random(seed)
    reads = []
    for i in range(n):
        ln = rnd.randint(0, max_len)
        s = junk(rnd, ln, "ACGTACGTACGTACGTNacgtn")
        if i % 3:
            for _ in range(rnd.randint(1, 2)):
                unit = junk(rnd, rnd.choice([1, 2, 3, 4, 5, 6, 7, 12, 16, 19, 31, 32]))
                t = noisy(rnd, unit, rnd.randint(0, ln), rnd.choice([0, 0.02, 0.1]), rnd.choice([0, 0.01]), rnd.choice([0, 0.01]))
                at = rnd.randint(0, ln - len(t))
                s = s[:at] + t + s[at + len(t):]
        reads.append(s.encode())
    return reads
