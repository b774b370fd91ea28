"""Brute-force reference of the de novo repeats of a read, every tract (trew_hip_repeat), written from the
definition on top of period_ref.period_read and independent of the C++ and HIP implementations.

A piece [lo, hi) of a read has the record of read[lo:hi] taken as a read of its own, start and end shifted by lo.  The
recursion is written in two shapes: `repeats_read` depth-first as the definition states it (the record, then the piece in
front of it, then the piece behind it) and `repeats_read_rounds` breadth-first (all pieces of one depth, then the next)."""
import numpy as np

import period_ref as R

FIELDS = ("read", "depth") + R.FIELDS
DTYPE = np.dtype([(f, "<u8" if f == "unit" else "<u4") for f in FIELDS])
START, END = R.FIELDS.index("start"), R.FIELDS.index("end")


def piece_record(read, lo, hi, **kw):
    """the record of the piece [lo, hi) in read coordinates, or None"""
    x = R.period_read(read[lo:hi], **kw)
    if x == R.ZERO:
        return None
    return x[:START] + (x[START] + lo, x[END] + lo) + x[END + 1:]


def repeats_read(read, min_period=1, max_period=32, penalty=3, min_score=24):
    """[(depth,) + record] of one read, in the order of the definition"""
    kw = dict(min_period=min_period, max_period=max_period, penalty=penalty, min_score=min_score)
    out = []

    def go(lo, hi, depth):
        x = piece_record(read, lo, hi, **kw)
        if x is None:
            return
        out.append((depth,) + x)
        go(lo, x[START], depth + 1)
        go(x[END], hi, depth + 1)

    go(0, len(read), 0)
    return out


def repeats_read_rounds(read, min_period=1, max_period=32, penalty=3, min_score=24):
    """the same records, found round by round: every piece of depth d, then every piece of depth d + 1"""
    kw = dict(min_period=min_period, max_period=max_period, penalty=penalty, min_score=min_score)
    out, pieces, depth = [], [(0, len(read))], 0
    while pieces:
        nxt = []
        for lo, hi in pieces:
            x = piece_record(read, lo, hi, **kw)
            if x is not None:
                out.append((depth,) + x)
                nxt += [(lo, x[START]), (x[END], hi)]
        pieces, depth = nxt, depth + 1
    return out


def repeats(reads, min_period=1, max_period=32, penalty=3, min_score=24, shape=repeats_read):
    """(DTYPE records sorted by (read, start), counts per read): the order every interface returns"""
    rows, counts = [], np.zeros(len(reads), dtype=np.uint32)
    for i, r in enumerate(reads):
        mine = sorted(shape(r, min_period, max_period, penalty, min_score), key=lambda x: x[1 + START])
        counts[i] = len(mine)
        rows += [(i,) + x for x in mine]
    return np.array(rows, dtype=DTYPE) if rows else np.zeros(0, dtype=DTYPE), counts


def cli_lines(path, reads, recs):
    """stdout of `trew repeats` for one file: (the file's section, the >Summary section), formatted from records"""
    rows = [">" + path, "read,length,depth,period,unit,canonical,start,end,score,matches,support,scored_period"]
    summary = {}
    for x in recs:
        i, d = int(x["read"]), int(x["period"])
        canon = R.canonical(x["unit"], d)
        rows.append("%d,%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d" % (i, len(reads[i]), x["depth"], d, R.unit_text(x["unit"], d), R.unit_text(canon, d), x["start"],
                                                        x["end"], x["score"], x["matches"], x["support"], x["scored_period"]))
        who, tracts, bases = summary.get((d, canon), (set(), 0, 0))
        summary[(d, canon)] = (who | {i}, tracts + 1, bases + int(x["end"]) - int(x["start"]))
    tail = [">Summary", "period,canonical,reads,tracts,bases"]
    for (d, canon), (who, tracts, bases) in sorted(summary.items(), key=lambda kv: (-len(kv[1][0]), kv[0])):
        tail.append("%d,%s,%d,%d,%d" % (d, R.unit_text(canon, d), len(who), tracts, bases))
    return rows, tail
