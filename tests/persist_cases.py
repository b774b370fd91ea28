"""Reads and schedule shared by tests/test_persist_cpu.py and tests/test_gpu_persist.py: twelve kinds of read, each with a
property that makes a wave-per-read kernel leave something behind (bins in use, a block of direction bytes, a piece stack, a
strand flag) or find nothing at all, and a schedule that puts every ordered pair of kinds (previous read, next read) into the
sequence of reads one persistent wave works through: wave w of `waves` takes the reads w, w + waves, w + 2 waves, ..."""
import functools
import random

import align_cases
from period_cases import TEL, junk, noisy, rep
from tandem_cases import primitive_unit

SEED = 20260218
K = 12  # kinds
U32 = align_cases.UNITS[32]
MOTIFS = [TEL, "CCCTA", U32]  # the motif list of the motif measures
PENALTY, MIN_SCORE = 3, 24
TEL_RC = align_cases.revcomp(TEL)  # CCCTAA
# kind 10: eight exact tracts of units of up to six bases (a tract of n bases of a unit of k scores n - k, and 24 are needed), the
# second one the longest and the others shorter from the third on: the best tract of the read has pieces with tracts on both
# sides, and behind it every further tract lies one piece deeper
TRACT_UNITS = ["AATGG", TEL, "AC", "CCG", "AAAG", "GAT", "CTTGA", "TCGG"]
TRACT_BASES = [40, 44, 42, 38, 36, 34, 32, 31]


def _built():
    """{kind: text} of the ten kinds that are built outright; kinds 3 and 8 are drawn until their property holds (kinds)"""
    rnd = random.Random(SEED)
    fixed = {}
    fixed[0] = ""
    fixed[1] = "A"
    fixed[2] = "N" * 70
    fixed[4] = junk(rnd, 50) + rep(TEL, 42) + junk(rnd, 50)
    fixed[5] = junk(rnd, 40) + U32 * 6 + junk(rnd, 40)
    fixed[6] = rep(TEL_RC, 130)
    fixed[7] = TEL * 8 + junk(rnd, 30) + TEL_RC * 8
    fixed[9] = "AATGG" * 30 + junk(rnd, 40) + TEL * 25
    fixed[10] = junk(rnd, 12).join(rep(u, n) for u, n in zip(TRACT_UNITS, TRACT_BASES))
    mono = primitive_unit(rnd, 171)
    fixed[11] = mono * 3
    return fixed


def _records_anywhere(read):
    """True when a measure of the suite says anything of `read` at the defaults of this file (see has_record)"""
    from trew_amd import capi

    packed = capi.pack_reads([read.encode()])
    return any(has_record(name, host(name, packed), 0) for name in MEASURES)


def _kind8_ok(read):
    from trew_amd import capi

    packed = capi.pack_reads([read.encode()])
    if not capi.refine_host(packed)[0]["changed"] > 0:
        return False
    for items in (capi.trace_host(packed, MOTIFS, PENALTY, MIN_SCORE)[0], capi.decompose_host(packed)[0]):
        if not ((items["insertions"] > 0).any() and (items["deletions"] > 0).any()):
            return False
    return True


@functools.lru_cache(maxsize=None)
def kinds():
    """the K reads, as bytes; the same bytes on every call and in every process"""
    fixed = _built()
    for seed in range(SEED, SEED + 1000):  # kind 3: 150 random bases of which no measure says anything
        text = junk(random.Random(seed), 150)
        if not _records_anywhere(text):
            fixed[3] = text
            break
    for seed in range(SEED, SEED + 1000):  # kind 8: noisy TTAGGG with the unit re-voted, an insertion and a deletion
        rnd = random.Random(seed)
        text = junk(rnd, 20) + noisy(rnd, TEL, 200, 0.03, 0.06) + junk(rnd, 20)
        if _kind8_ok(text):
            fixed[8] = text
            break
    assert sorted(fixed) == list(range(K)), sorted(fixed)
    return tuple(fixed[i].encode() for i in range(K))


# ---------------------------------------------------------------- the fourteen measures at this file's parameters
MEASURES = ["annotate", "tracts", "intervals", "variants", "periods", "chain", "repeats", "satellites", "align", "refine", "tandems", "trace",
            "decompose", "dissect"]


def host(name, packed):
    """the host definition of measure `name` over a packed batch: penalty 3, min_score 24, periods 1 to 32 (satellites: to 256)"""
    from trew_amd import capi

    f = getattr(capi, name + "_host")
    if name in ("annotate", "intervals", "variants", "chain"):
        return f(packed, MOTIFS)
    if name in ("tracts", "align"):
        return f(packed, MOTIFS, PENALTY)
    if name == "trace":
        return f(packed, MOTIFS, PENALTY, MIN_SCORE)
    return f(packed, 1, 256 if name == "satellites" else 32, PENALTY, MIN_SCORE)


def has_record(name, result, r):
    """whether measure `name` says anything of read r in `result`, the value of host(name, ...): a record, an item or a
    non-zero count for the logged measures; a record with a period for periods and refine; a non-zero record for annotate
    and tracts and one with units or variants for variants, which write one for every read; for align, where a single base
    already scores 1, a strand that reaches min_score (what trace would trace)"""
    if name == "variants":  # a record without units says `top` = VARIANT_NONE
        return any(result[0][r][f].any() for f in ("units_fwd", "variants_fwd", "units_rev", "variants_rev"))
    if name in ("annotate", "tracts"):
        return any(result[r][f].any() for f in result.dtype.names)
    if name == "align":
        return bool((result[r]["score_fwd"] >= MIN_SCORE).any() or (result[r]["score_rev"] >= MIN_SCORE).any())
    if name in ("periods", "refine"):
        return bool(result[r]["period"] > 0)
    if name == "decompose":
        return bool(result[1][r] > 0 or result[2][r]["period"] > 0)
    if name == "dissect":
        return bool(result[2][r].any())
    return bool(result[1][r].any())  # intervals, chain, repeats, satellites, tandems, trace: the counts of the read


# ---------------------------------------------------------------- the schedule
def debruijn(k):
    """A cyclic sequence of length k * k over range(k) in which every ordered pair (a, b), a = b included, occurs as neighbours
    exactly once: B(k, 2), the concatenation of the Lyndon words over range(k) whose length divides 2, in lexicographic order."""
    a = [0] * 3  # a[1], a[2]: the word at hand
    out = []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                out.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)

    db(1, 1)
    return out


def check_debruijn(seq, k):
    assert len(seq) == k * k and set(seq) == set(range(k))
    pairs = [(seq[i], seq[(i + 1) % len(seq)]) for i in range(len(seq))]
    assert len(set(pairs)) == k * k == len(pairs)


def schedule(waves, trips, k=K):
    """the kind of every read of a batch of waves * trips reads: read t * waves + w, the one wave w of `waves` takes on its trip
    t, is of kind S[(t + w) % k^2], S = debruijn(k).  With trips = k^2 + 1 every wave sees every ordered pair of kinds."""
    s = debruijn(k)
    return [s[(t + w) % len(s)] for t in range(trips) for w in range(waves)]


def pairs_per_wave(kinds_of_reads, waves):
    """[set of (previous kind, next kind)] per wave for a batch whose read r is of kind kinds_of_reads[r]"""
    out = []
    for w in range(waves):
        mine = kinds_of_reads[w::waves]
        out.append(set(zip(mine, mine[1:])))
    return out


def batch(waves, trips, cut=0):
    """(reads, kinds of the reads): the schedule for `waves` waves and `trips` trips without the last `cut` reads"""
    sched = schedule(waves, trips)
    sched = sched[:len(sched) - cut]
    ks = kinds()
    return [ks[i] for i in sched], sched
