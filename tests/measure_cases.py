"""The read set of tests/test_gpu_measure_state.py and tests/test_measures_host_cpu.py: ragged reads of telomere units with
planted substitutions and a few N, at the lengths where the per-read motif measures change path."""
import random

K32 = "TTAGGGTTAGGCTTAGGGTCAGGGTTAGGGTA"  # a motif of 32 bases
assert len(K32) == 32
# 0, 1, k - 1 and k for k = 3, 6 and 32; either side of one and two words; either side of the 63-word and 64-word iteration
# seams of variants and tracts
LENGTHS = [0, 1, 2, 3, 5, 6, 31, 32, 33, 63, 64, 65, 2015, 2016, 2017, 2049]
_RC = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def _repeat(rnd, unit, n, sub_every, n_every):
    """n bases of `unit` back to back from a random phase, one base in ~sub_every substituted, one in ~n_every an N"""
    phase = rnd.randrange(len(unit))
    s = list((unit * (n // len(unit) + 2))[phase:phase + n])
    for i in range(n):
        if rnd.randrange(sub_every) == 0:
            s[i] = rnd.choice([c for c in "ACGT" if c != s[i]])
        elif n_every and rnd.randrange(n_every) == 0:
            s[i] = "N"
    return "".join(s)


def make_reads():
    """40 reads (bytes): every length as forward units with substitutions and as reverse-strand units with N, then eight long
    reads that string together tracts of the k = 3, 6 and 32 motifs and random bases"""
    rnd = random.Random(20250611)
    reads = []
    for n in LENGTHS:
        reads.append(_repeat(rnd, "TTAGGG", n, 23, 0))
        reads.append("".join(_RC[c] for c in reversed(_repeat(rnd, "TTAGGG", n, 37, 150))))
    for n in LENGTHS[-4:] * 2:
        s = ""
        while len(s) < n:
            unit = rnd.choice(["TTAGGG", "TTG", K32, None])
            m = rnd.choice([7, 40, 200, 500])
            s += "".join(rnd.choice("ACGT") for _ in range(m)) if unit is None else _repeat(rnd, unit, m, 29, 400)
        reads.append(s[:n])
    return [r.encode() for r in reads]
