"""Reference of tandems, decompose and dissect with resolve's period choice per piece (trew_hip_tandems_resolved,
trew_hip_decompose_resolved, trew_hip_dissect_resolved), composed from the references of their parts and
independent of the library and of oracle/.

resolved(piece, C) of a piece [lo, hi) is what resolve_ref gives read[lo:hi] taken as a read of its own: the number of candidates
m, the winner's sixteen words W (start and end shifted by lo) and the periods tract T0 of candidate 0 (shifted likewise).

  tandems    m = 0: nothing.  W.score >= min_score: W, then the pieces in front of W and behind it.  Otherwise (weak): no record,
             then the pieces in front of T0 and behind it.  That is tandem_ref._split with (W, candidate 0) for (X, R).
  decompose  decompose_ref with W of the whole read in the place of refine_ref's record.
  dissect    dissect_ref over those pieces and records: decompose_ref on the piece with its W.

Two forms of each that must agree: depth first and cell by cell (resolve_ref.resolve_read, trace_ref.trace_strand; short reads)
and round by round over many reads (resolve_ref.resolve and decompose_ref.decompose, both vectorised, over all pieces of one
depth).  With C = 1 every result is tandem_ref's, decompose_ref's and dissect_ref's."""
import numpy as np

import align_ref
import decompose_ref as D
import dissect_ref
import period_ref as P
import refine_ref as R
import resolve_ref as V
import tandem_ref as T
import trace_ref

DTYPE = T.DTYPE
ITEM_DTYPE = trace_ref.ITEM_DTYPE
ANCHOR = D.ANCHOR
START, END = T.START, T.END
NW = len(R.FIELDS)  # the sixteen words, as fields


def resolved_read(text, min_period, max_period, penalty, min_score, candidates):
    """(m, W, candidate 0 as a periods record) of `text` taken as a read of its own, cell by cell; W = R.ZERO when m = 0"""
    cands = V.candidate_records(P.codes(text), min_period, max_period, penalty, min_score, candidates)
    rec = V.resolve_read(text, min_period, max_period, penalty, min_score, candidates)
    assert rec[NW] == len(cands) and (rec == V.ZERO) == (not cands)
    return len(cands), rec[:NW], cands[0] if cands else P.ZERO


def resolved_many(texts, min_period, max_period, penalty, min_score, candidates):
    """[(m, W, candidate 0)] of many texts, W by the vectorised form"""
    recs = V.resolve(texts, min_period, max_period, penalty, min_score, candidates)
    out = []
    for text, x in zip(texts, recs):
        cands = V.candidate_records(P.codes(text), min_period, max_period, penalty, min_score, candidates) if int(x["candidates"]) else []
        assert int(x["candidates"]) == len(cands)
        out.append((len(cands), tuple(int(x[f]) for f in R.FIELDS), cands[0] if cands else P.ZERO))
    return out


def worth(lo, hi, min_period, min_score):
    """a piece that can have a periods record at all (score_k <= length - k): dropping the others changes nothing"""
    return hi - lo > min_period and hi - lo - min_period >= min_score


# ---------------------------------------------------------------- tandems
def tandems_read(read, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """[(depth,) + record] of one read, in the order of the definition"""
    out = []

    def go(lo, hi, depth):
        m, w, first = resolved_read(read[lo:hi], min_period, max_period, penalty, min_score, candidates)
        if m == 0:
            return
        x, (a, b) = T._split(w, first, lo, min_score)
        if x is not None:
            out.append((depth,) + x)
        assert lo <= a < b <= hi  # the recursion shrinks
        go(lo, a, depth + 1)
        go(b, hi, depth + 1)

    go(0, len(read), 0)
    return out


def tandems_rounds(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3, where=None):
    """[[(depth,) + record] per read], found round by round: every piece of depth d of every read, then depth d + 1.  where: a list
    that receives (read, lo, hi, record) for every piece that gives a record"""
    out = [[] for _ in reads]
    pieces, depth = [(i, 0, len(r)) for i, r in enumerate(reads)], 0
    while pieces:
        got = resolved_many([reads[i][lo:hi] for i, lo, hi in pieces], min_period, max_period, penalty, min_score, candidates)
        nxt = []
        for (i, lo, hi), (m, w, first) in zip(pieces, got):
            if m == 0:
                continue
            x, (a, b) = T._split(w, first, lo, min_score)
            if x is not None:
                out[i].append((depth,) + x)
                if where is not None:
                    where.append((i, lo, hi, x))
            assert lo <= a < b <= hi
            nxt += [(i, l, h) for l, h in ((lo, a), (b, hi)) if worth(l, h, min_period, min_score)]
        pieces, depth = nxt, depth + 1
    return out


def _texts(reads):
    return [r.decode() if isinstance(r, bytes) else r for r in reads]


def tandems(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3, depth_first=False):
    """(tandem_ref.DTYPE records sorted by (read, start), counts per read): tandem_ref.tandems' order and assembly"""
    reads = _texts(reads)
    args = (min_period, max_period, penalty, min_score, candidates)
    per_read = iter([tandems_read(r, *args) for r in reads] if depth_first else tandems_rounds(reads, *args))
    return T.tandems(reads, min_period, max_period, penalty, min_score, shape=lambda *_: next(per_read))


# ---------------------------------------------------------------- decompose
def decompose_read(read, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """(the record in the order of refine_ref.FIELDS with reserved = anchor, [items]): decompose_ref.decompose_read with W"""
    rec = resolved_read(read, min_period, max_period, penalty, min_score, candidates)[1]
    if not D.traced(rec, min_score):
        return rec, []
    k = rec[0]
    rho, M = D.anchor(D.unit_codes(rec[12], k))
    arec, _, cols = trace_ref.trace_strand(align_ref.codes(read), M, penalty)
    assert arec == rec[4:9], "W's alignment fields are the alignment of the read against W.unit"
    return rec[:ANCHOR] + (rho,) + rec[ANCHOR + 1:], trace_ref.items_of(cols, k)


def decompose(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3, depth_first=False):
    """(items, counts, records) as decompose_ref.decompose returns them"""
    reads = _texts(reads)
    if not depth_first:
        recs = V.refined(V.resolve(reads, min_period, max_period, penalty, min_score, candidates))
        return D.decompose(reads, min_period, max_period, penalty, min_score, recs=recs)
    recs, counts, rows = np.zeros(len(reads), dtype=D.DTYPE), np.zeros(len(reads), dtype=np.uint32), []
    for i, read in enumerate(reads):
        rec, its = decompose_read(read, min_period, max_period, penalty, min_score, candidates)
        recs[i] = rec
        counts[i] = len(its)
        rows += [(i, 0, 0) + it + (0,) for it in its]
    return np.array(rows, dtype=ITEM_DTYPE).reshape(-1), counts, recs


# ---------------------------------------------------------------- dissect
def dissect_read(read, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """[((depth,) + record with reserved = anchor, [items, start in read coordinates])] of one read, in the order of the definition"""
    args = (min_period, max_period, penalty, min_score, candidates)
    out = []

    def go(lo, hi, depth):
        piece = read[lo:hi]
        m, w, first = resolved_read(piece, *args)
        if m == 0:
            return
        x, (a, b) = T._split(w, first, lo, min_score)
        if x is not None:
            rec, items = decompose_read(piece, *args)
            assert rec[:ANCHOR] + (0,) + rec[ANCHOR + 1:] == w
            out.append(((depth,) + x[:ANCHOR] + (rec[ANCHOR],) + x[ANCHOR + 1:], [(it[0] + lo,) + it[1:] for it in items]))
        assert lo <= a < b <= hi
        go(lo, a, depth + 1)
        go(b, hi, depth + 1)

    go(0, len(read), 0)
    return out


def dissect_rounds(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """[the same per read], found round by round"""
    out = [[] for _ in reads]
    pieces, depth = [(i, 0, len(r)) for i, r in enumerate(reads)], 0
    while pieces:
        texts = [reads[i][lo:hi] for i, lo, hi in pieces]
        got = resolved_many(texts, min_period, max_period, penalty, min_score, candidates)
        recs = np.array([w for _, w, _ in got], dtype=R.DTYPE)
        items, counts, anchored = D.decompose(texts, min_period, max_period, penalty, min_score, recs=recs)
        first_item = [0] + [int(v) for v in np.cumsum(counts, dtype=np.int64)]
        nxt = []
        for q, ((i, lo, hi), (m, w, first)) in enumerate(zip(pieces, got)):
            if m == 0:
                continue
            x, (a, b) = T._split(w, first, lo, min_score)
            if x is not None:
                mine = [tuple(int(v) for v in it)[3:11] for it in items[first_item[q]:first_item[q + 1]]]
                out[i].append(((depth,) + x[:ANCHOR] + (int(anchored["reserved"][q]),) + x[ANCHOR + 1:], [(it[0] + lo,) + it[1:] for it in mine]))
            else:
                assert counts[q] == 0  # a weak piece is not traced
            assert lo <= a < b <= hi
            nxt += [(i, l, h) for l, h in ((lo, a), (b, hi)) if worth(l, h, min_period, min_score)]
        pieces, depth = nxt, depth + 1
    return out


def dissect(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3, depth_first=False):
    """(records, items, counts (n_reads, 2), rows) as dissect_ref.dissect returns them"""
    reads = _texts(reads)
    args = (min_period, max_period, penalty, min_score, candidates)
    per_read = iter([dissect_read(r, *args) for r in reads] if depth_first else dissect_rounds(reads, *args))
    return dissect_ref.dissect(reads, min_period, max_period, penalty, min_score, shape=lambda *_: next(per_read))


# the commands print the columns of their plain forms: tandem_ref.cli_lines, decompose_ref.cli_lines and dissect_ref.cli_lines
# format these records as they are
