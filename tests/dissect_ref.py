"""Reference of units in place for every tract of a read, no motif given (trew_hip_dissect), composed from the
references of its two halves and independent of the library and of oracle/: the recursion of tandem_ref over the pieces of a
read, and for every piece that gives a record decompose_ref on the piece's bases taken as a read of their own, offset by the
piece's first base.

  1. The pieces, their depths and their records are tandem_ref's: a piece [lo, hi) without a periods record ends its branch; with a
     refined record X of score >= min_score it yields X and splits around X; otherwise (weak) it yields nothing and splits
     around its periods tract.
  2. A piece with a record X yields X with reserved = the anchor of X.unit (decompose_ref.anchor) and the items of
     decompose_ref for read[lo:hi], with lo added to start.
  3. The records of a read are sorted by start; an item's motif is the index of its tract among them, its strand 0.

Two forms that must agree: dissect_read (plain Python, depth first as the definition states it: period_ref.period_read,
refine_ref.refine_read and decompose_ref.decompose_read on read[lo:hi]; short reads) and dissect_rounds (round by round over
many reads: refine_ref.refine and decompose_ref.decompose, both vectorised, over all pieces of one depth)."""
import os

import numpy as np

import decompose_ref as D
import period_ref as P
import refine_ref as R
import tandem_ref as T
import trace_ref

DTYPE = T.DTYPE
ITEM_DTYPE = trace_ref.ITEM_DTYPE
ANCHOR = D.ANCHOR
START, END = T.START, T.END


def dissect_read(read, min_period=1, max_period=32, penalty=3, min_score=24):
    """[((depth,) + record with reserved = anchor, [items as trace_ref.items_of gives them, start in read coordinates])] of one
    read, in the order of the definition"""
    args = (min_period, max_period, penalty, min_score)
    out = []

    def go(lo, hi, depth):
        piece = read[lo:hi]
        per = P.period_read(piece, *args)
        if per == P.ZERO:
            return
        x, (a, b) = T._split(R.refine_read(piece, *args), per, lo, min_score)
        if x is not None:
            rec, items = D.decompose_read(piece, *args)
            assert rec[:ANCHOR] + (0,) + rec[ANCHOR + 1:] == x[:START] + (x[START] - lo, x[END] - lo) + x[END + 1:]
            out.append(((depth,) + x[:ANCHOR] + (rec[ANCHOR],) + x[ANCHOR + 1:], [(it[0] + lo,) + it[1:] for it in items]))
        assert lo <= a < b <= hi  # the recursion shrinks
        go(lo, a, depth + 1)
        go(b, hi, depth + 1)

    go(0, len(read), 0)
    return out


def dissect_rounds(reads, min_period=1, max_period=32, penalty=3, min_score=24):
    """[the same per read], found round by round: every piece of depth d of every read, then depth d + 1"""
    args = (min_period, max_period, penalty, min_score)
    out = [[] for _ in reads]
    pieces, depth = [(i, 0, len(r)) for i, r in enumerate(reads)], 0
    while pieces:
        texts = [reads[i][lo:hi] for i, lo, hi in pieces]
        recs = R.refine(texts, *args)
        items, counts, anchored = D.decompose(texts, *args, recs=recs)
        first = [0] + [int(v) for v in np.cumsum(counts, dtype=np.int64)]
        nxt = []
        for q, ((i, lo, hi), text, x) in enumerate(zip(pieces, texts, recs)):
            x = tuple(int(v) for v in x)
            if x == R.ZERO:  # no periods record: refine gives a zero record then, and only then
                continue
            x, (a, b) = T._split(x, P.period_read(text, *args), lo, min_score)
            if x is not None:
                mine = [tuple(int(v) for v in it)[3:11] for it in items[first[q]:first[q + 1]]]
                assert all(int(it["read"]) == q for it in items[first[q]:first[q + 1]])
                out[i].append(((depth,) + x[:ANCHOR] + (int(anchored["reserved"][q]),) + x[ANCHOR + 1:], [(it[0] + lo,) + it[1:] for it in mine]))
            else:
                assert counts[q] == 0  # a weak piece is not traced
            assert lo <= a < b <= hi
            nxt += [(i, l, h) for l, h in ((lo, a), (b, hi)) if h - l > min_period and h - l - min_period >= min_score]
        pieces, depth = nxt, depth + 1
    return out


def dissect(reads, min_period=1, max_period=32, penalty=3, min_score=24, shape=None):
    """(DTYPE records sorted by (read, start) with reserved = anchor, ITEM_DTYPE items sorted by (read, start) with motif = the
    index of the item's tract in its read, counts (n_reads, 2) = (tracts, items), rows = the sum of end - start over the
    records): the order every interface returns.  shape: dissect_read for the depth-first form, default the round-by-round form"""
    args = (min_period, max_period, penalty, min_score)
    reads = [r.decode() if isinstance(r, bytes) else r for r in reads]
    per_read = [shape(r, *args) for r in reads] if shape else dissect_rounds(reads, *args)
    rows, items, counts, n_rows = [], [], np.zeros((len(reads), 2), dtype=np.uint32), 0
    for i, mine in enumerate(per_read):
        mine = sorted(mine, key=lambda x: x[0][1 + START])
        counts[i, 0] = len(mine)
        for t, (x, its) in enumerate(mine):
            rows.append((i,) + x)
            n_rows += x[1 + END] - x[1 + START]
            items += [(i, t, 0) + it + (0,) for it in its]
            counts[i, 1] += len(its)
    return (np.array(rows, dtype=DTYPE) if rows else np.zeros(0, dtype=DTYPE), np.array(items, dtype=ITEM_DTYPE).reshape(-1), counts, n_rows)


HEADER = T.HEADER + ",anchor,strand,units,edited,signature"
ITEM_HEADER = "read,length,tract,period,anchor,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit"


def cli_lines(path, reads, result, penalty, per_item=False):
    """stdout of `trew dissect` (with --items: per_item) for one file: (the file's section, the >Summary section), formatted
    from result = (records, items, ...) of these reads"""
    recs, items = result[:2]
    texts = [r.decode("latin-1") if isinstance(r, (bytes, bytearray)) else r for r in reads]
    by_tract = {}
    for it in items:
        by_tract.setdefault((int(it["read"]), int(it["motif"])), []).append(tuple(int(v) for v in it)[3:11])
    rows = [">" + os.path.realpath(path), ITEM_HEADER if per_item else HEADER]
    summary, tract = {}, {}
    for x in recs:
        i, d = int(x["read"]), int(x["period"])
        t = tract[i] = tract.get(i, -1) + 1
        read = texts[i]
        c = R.columns(tuple(int(x[f]) for f in R.FIELDS), penalty)
        canon = P.canonical(x["unit"], d)
        u = D.unit_codes(x["unit"], d)
        m = P.pack_unit(u[int(x["reserved"]):] + u[:int(x["reserved"])])
        assert m == P.pack_unit(D.anchor(u)[1])
        its = by_tract[(i, t)]
        units, edited, sig = trace_ref.signature(read, d, 0, its)
        sp = int(x["seed_period"])
        if per_item:
            for it in its:
                unit = trace_ref.signature(read, d, 0, [it])[2]
                rows.append("%d,%d,%d,%d,%s,%s,%s" % (i, len(read), t, d, P.unit_text(m, d), ",".join(str(v) for v in it), "=" if unit[0] == "=" else unit))
        else:
            rows.append("%d,%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%s,%d,%d,%d,%s,%s,%d,%d,%s" % (
                i, len(read), x["depth"], d, P.unit_text(x["unit"], d), P.unit_text(canon, d), x["start"], x["end"], x["score"], c["copies"],
                x["consumed"], x["matches"], c["mismatches"], c["insertions"], c["deletions"], sp, P.unit_text(x["seed_unit"], sp),
                x["seed_score"], x["changed"], x["scored_period"], P.unit_text(m, d), "+" if canon == m else "-", units, edited, sig))
        who, sums = summary.get((d, canon), (set(), (0,) * 6))
        add = (1, int(x["end"]) - int(x["start"]), c["copies"], units, edited, len(its))
        summary[(d, canon)] = (who | {i}, tuple(a + b for a, b in zip(sums, add)))
    tail = [">Summary", "period,canonical,reads,tracts,bases,copies,units,edited,items"]
    for (d, canon), (who, sums) in sorted(summary.items(), key=lambda kv: (-len(kv[1][0]), kv[0])):
        tail.append("%d,%s,%d,%s" % (d, P.unit_text(canon, d), len(who), ",".join(str(a) for a in sums)))
    return rows, tail
