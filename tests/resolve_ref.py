"""Reference of `resolve` (trew_hip_resolved), written from the definition on top of period_ref and refine_ref and
independent of the library and of oracle/: the C best-scoring periods of `periods`' fixed-phase score are the candidates, steps
2 to 6 of `refine` run for each with its own segment, and the record with the largest final score is kept.

Two forms that must agree: resolve_read (plain Python, refine_ref's cell-by-cell pieces; short reads) and resolve (refine_ref's
vectorised passes over every (read, candidate) pair at once)."""
import os

import numpy as np

import align_ref
import period_ref
import refine_ref

MAX_CANDIDATES = 4
EXTRA_FIELDS = ("candidates", "rank", "first_period", "first_score")
FIELDS = refine_ref.FIELDS + EXTRA_FIELDS
DTYPE = np.dtype([(f, "<u4") for f in refine_ref.U32_FIELDS] + [("unit", "<u8"), ("seed_unit", "<u8")] + [(f, "<u4") for f in EXTRA_FIELDS])
assert DTYPE.itemsize == 80
ZERO = (0,) * len(FIELDS)


def period_scores(c, min_period, max_period, penalty):
    """[(score, k, b, e)] for every admissible k, in the order (score descending, k ascending)"""
    out = []
    for k in range(min_period, min(max_period, len(c) - 1) + 1):
        score, b, e = period_ref.segment_prefix(period_ref.eq_k(c, k), penalty)
        out.append((score, k, b, e))
    return sorted(out, key=lambda t: (-t[0], t[1]))


def candidate_records(c, min_period, max_period, penalty, min_score, candidates):
    """the candidates of step 1 as tuples in the order of period_ref.FIELDS with what refine_ref.seed reads of them:
    scored_period, score, start and end (the other fields zero)"""
    assert 1 <= candidates <= MAX_CANDIDATES
    best = [t for t in period_scores(c, min_period, max_period, penalty) if t[0] >= min_score][:candidates]
    return [(0, k, score, b, e + k, 0, 0, 0, 0) for score, k, b, e in best]


def choose(recs):
    """(the winner's sixteen fields, its rank): the largest score, then the smallest period, then the smallest c"""
    rank = min(range(len(recs)), key=lambda i: (-recs[i][4], recs[i][0], i))
    return recs[rank], rank


def _record(recs):
    if not recs:
        return ZERO
    win, rank = choose(recs)
    return tuple(win) + (len(recs), rank, recs[0][0], recs[0][4])


def resolve_read(read, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """the record of one read as a tuple in the order of FIELDS, step by step from the definition"""
    c = period_ref.codes(read)
    x = [int(v) for v in c]
    recs = []
    for R in candidate_records(c, min_period, max_period, penalty, min_score, candidates):
        S = refine_ref.seed(c, R)
        a1 = align_ref.align_strand(x, S, penalty)
        cnt = refine_ref.vote_plain(x[a1[1]:a1[2]], S, penalty)
        recs.append(refine_ref._finish(R, S, a1, cnt, lambda U: align_ref.align_strand(x, U, penalty)))
    return _record(recs)


def candidate_table(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """per read the refined records of all its candidates, as tuples in the order of refine_ref.FIELDS: the vectorised passes
    of refine_ref over every (read, candidate) pair"""
    cs = [period_ref.codes(r) for r in reads]
    pairs = [(i, R) for i, c in enumerate(cs) for R in candidate_records(c, min_period, max_period, penalty, min_score, candidates)]
    table = [[] for _ in reads]
    if not pairs:
        return table
    xs = [[int(v) for v in cs[i]] for i, _ in pairs]
    Ss = [refine_ref.seed(cs[i], R) for i, R in pairs]
    X, lens = refine_ref._plane(xs)
    T, ks = refine_ref._units(Ss)
    a1, _ = refine_ref._pass_many(X, lens, T, ks, penalty)
    X2, lens2 = refine_ref._plane([x[int(a[1]):int(a[2])] for x, a in zip(xs, a1)])
    _, cnt = refine_ref._pass_many(X2, lens2, T, ks, penalty, vote=True)
    Us = []
    for r, S in enumerate(Ss):
        u0 = refine_ref.revote(S, cnt[r].tolist())[0]
        Us.append(u0[:period_ref.primitive(u0)])
    T3, ks3 = refine_ref._units(Us)
    a3, _ = refine_ref._pass_many(X, lens, T3, ks3, penalty)
    for r, (i, R) in enumerate(pairs):
        table[i].append(refine_ref._finish(R, Ss[r], tuple(int(v) for v in a1[r]), cnt[r].tolist(), lambda U, r=r: tuple(int(v) for v in a3[r])))
    return table


def resolve(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """DTYPE records of shape (n_reads,), the vectorised form"""
    out = np.zeros(len(reads), dtype=DTYPE)
    for i, recs in enumerate(candidate_table(reads, min_period, max_period, penalty, min_score, candidates)):
        out[i] = _record(recs)
    return out


def refined(recs):
    """the first sixteen words of DTYPE records as refine_ref.DTYPE records"""
    out = np.zeros(len(recs), dtype=refine_ref.DTYPE)
    for f in refine_ref.FIELDS:
        out[f] = recs[f]
    return out


HEADER = refine_ref.HEADER + ",candidates,rank,first_period,first_score"


def cli_lines(path, reads, recs, penalty, min_score=24):
    """stdout of `trew resolve` for one file: (the file's section, the >Summary section), formatted from records"""
    rows = [">" + os.path.realpath(path), HEADER]
    summary = {}
    for i, (read, x) in enumerate(zip(reads, recs)):
        d = int(x["period"])
        if d == 0 or int(x["score"]) < min_score:
            continue
        c = refine_ref.columns(tuple(int(x[f]) for f in refine_ref.FIELDS), penalty)
        canon = period_ref.canonical(x["unit"], d)
        sp = int(x["seed_period"])
        rows.append("%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%s,%d,%d,%d,%d,%d,%d,%d" % (
            i, len(read), d, period_ref.unit_text(x["unit"], d), period_ref.unit_text(canon, d), x["start"], x["end"], x["score"], c["copies"],
            x["consumed"], x["matches"], c["mismatches"], c["insertions"], c["deletions"], sp, period_ref.unit_text(x["seed_unit"], sp),
            x["seed_score"], x["changed"], x["scored_period"], x["candidates"], x["rank"], x["first_period"], x["first_score"]))
        n, bases, copies, repaired = summary.get((d, canon), (0, 0, 0, 0))
        summary[(d, canon)] = (n + 1, bases + int(x["end"]) - int(x["start"]), copies + c["copies"], repaired + (int(x["rank"]) > 0))
    tail = [">Summary", "period,canonical,reads,bases,copies,repaired"]
    for (d, canon), (n, bases, copies, repaired) in sorted(summary.items(), key=lambda kv: (-kv[1][0], kv[0])):
        tail.append("%d,%s,%d,%d,%d,%d" % (d, period_ref.unit_text(canon, d), n, bases, copies, repaired))
    return rows, tail
