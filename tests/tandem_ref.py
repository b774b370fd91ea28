"""Reference of the de novo repeats under indels, every tract of a read (trew_hip_tandem), written from the
definition on top of refine_ref and period_ref and independent of the C++ and HIP implementations.

A piece [lo, hi) of a read has the refined record of read[lo:hi] taken as a read of its own, start and end shifted by lo, and
the periods tract of step 1 of that computation, shifted likewise.  tandems(piece): no periods record, nothing; a refined
record X with score >= min_score, X, then the pieces in front of X and behind it; otherwise (a weak piece) no record, then the
pieces in front of the periods tract and behind it.

Two forms that must agree: `tandems_read` depth-first as the definition states it, with refine_ref.refine_read on read[lo:hi]
(O(n k^2) per piece: short reads), and `tandems_rounds` round by round over many reads, with the vectorised refine_ref.refine
over all pieces of one depth."""
import os

import numpy as np

import period_ref as P
import refine_ref as R

FIELDS = ("read", "depth") + R.FIELDS
DTYPE = np.dtype([(f, "<u8" if f in ("unit", "seed_unit") else "<u4") for f in FIELDS])
assert DTYPE.itemsize == 72
SCORE, START, END = R.FIELDS.index("score"), R.FIELDS.index("start"), R.FIELDS.index("end")
P_START, P_END = P.FIELDS.index("start"), P.FIELDS.index("end")


def _split(x, per, lo, min_score):
    """(the record in read coordinates or None, the tract the children lie around) of a piece that starts at lo, from its
    refined record x and its periods record per (tuples)"""
    if x[SCORE] >= min_score:
        x = x[:START] + (x[START] + lo, x[END] + lo) + x[END + 1:]
        return x, (x[START], x[END])
    return None, (per[P_START] + lo, per[P_END] + lo)


def tandems_read(read, min_period=1, max_period=32, penalty=3, min_score=24):
    """[(depth,) + record] of one read, in the order of the definition"""
    args = (min_period, max_period, penalty, min_score)
    out = []

    def go(lo, hi, depth):
        per = P.period_read(read[lo:hi], *args)
        if per == P.ZERO:
            return
        x, (a, b) = _split(R.refine_read(read[lo:hi], *args), per, lo, min_score)
        if x is not None:
            out.append((depth,) + x)
        assert lo <= a < b <= hi  # the recursion shrinks
        go(lo, a, depth + 1)
        go(b, hi, depth + 1)

    go(0, len(read), 0)
    return out


def tandems_rounds(reads, min_period=1, max_period=32, penalty=3, min_score=24):
    """[[(depth,) + record] per read], found round by round: every piece of depth d of every read, then depth d + 1"""
    args = (min_period, max_period, penalty, min_score)
    out = [[] for _ in reads]
    pieces, depth = [(i, 0, len(r)) for i, r in enumerate(reads)], 0
    while pieces:
        texts = [reads[i][lo:hi] for i, lo, hi in pieces]
        recs = R.refine(texts, *args)
        nxt = []
        for (i, lo, hi), text, x in zip(pieces, texts, recs):
            x = tuple(int(v) for v in x)
            if x == R.ZERO:  # no periods record: refine gives a zero record then, and only then
                continue
            x, (a, b) = _split(x, P.period_read(text, *args), lo, min_score)
            if x is not None:
                out[i].append((depth,) + x)
            assert lo <= a < b <= hi
            # a piece that cannot have a periods record (score_k <= length - k) is dropped here already: it changes nothing
            nxt += [(i, l, h) for l, h in ((lo, a), (b, hi)) if h - l > min_period and h - l - min_period >= min_score]
        pieces, depth = nxt, depth + 1
    return out


def tandems(reads, min_period=1, max_period=32, penalty=3, min_score=24, shape=None):
    """(DTYPE records sorted by (read, start), counts per read): the order every interface returns.  shape: tandems_read for
    the depth-first form, default the round-by-round form"""
    args = (min_period, max_period, penalty, min_score)
    reads = [r.decode() if isinstance(r, bytes) else r for r in reads]
    per_read = [shape(r, *args) for r in reads] if shape else tandems_rounds(reads, *args)
    rows, counts = [], np.zeros(len(reads), dtype=np.uint32)
    for i, mine in enumerate(per_read):
        mine = sorted(mine, key=lambda x: x[1 + START])
        counts[i] = len(mine)
        rows += [(i,) + x for x in mine]
    return np.array(rows, dtype=DTYPE) if rows else np.zeros(0, dtype=DTYPE), counts


HEADER = "read,length,depth," + R.HEADER.split(",", 2)[2]


def cli_lines(path, reads, recs, penalty):
    """stdout of `trew tandems` for one file: (the file's section, the >Summary section), formatted from records"""
    rows = [">" + os.path.realpath(path), HEADER]
    summary = {}
    for x in recs:
        i, d = int(x["read"]), int(x["period"])
        c = R.columns(tuple(int(x[f]) for f in R.FIELDS), penalty)
        canon = P.canonical(x["unit"], d)
        sp = int(x["seed_period"])
        rows.append("%d,%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%s,%d,%d,%d" % (
            i, len(reads[i]), x["depth"], d, P.unit_text(x["unit"], d), P.unit_text(canon, d), x["start"], x["end"], x["score"], c["copies"],
            x["consumed"], x["matches"], c["mismatches"], c["insertions"], c["deletions"], sp, P.unit_text(x["seed_unit"], sp),
            x["seed_score"], x["changed"], x["scored_period"]))
        who, tracts, bases, copies = summary.get((d, canon), (set(), 0, 0, 0))
        summary[(d, canon)] = (who | {i}, tracts + 1, bases + int(x["end"]) - int(x["start"]), copies + c["copies"])
    tail = [">Summary", "period,canonical,reads,tracts,bases,copies"]
    for (d, canon), (who, tracts, bases, copies) in sorted(summary.items(), key=lambda kv: (-len(kv[1][0]), kv[0])):
        tail.append("%d,%s,%d,%d,%d,%d" % (d, P.unit_text(canon, d), len(who), tracts, bases, copies))
    return rows, tail
