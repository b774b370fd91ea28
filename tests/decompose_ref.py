"""Reference of units in place with no motif given (trew_hip_decompose), composed from the references of its two
halves and independent of the library and of oracle/: the refined record of the read (refine_ref), the rotations of its unit
written out one by one, and the traceback of the read's forward strand against the smallest of them (trace_ref).

  1. R = refine_ref's record.  Zero, or R.score < min_score: no items, anchor 0.
  2. The k rotations of U = R.unit, rotation q with base j = U[(j + q) mod k], packed first base most significant; M is the one
     with the smallest word, anchor its q.  (U is primitive: the words are distinct.)  No reverse complement.
  3. The items of trace_ref for the codes of the read against M, for every k >= 1.

Two forms that must agree: decompose_read (plain Python: refine_ref.refine_read and trace_ref.trace_strand, the full table;
O(n k^2), short reads) and decompose (refine_ref.refine and dirs_units, trace_ref.dirs_many's doubling form vectorised with
numpy over the phases and over many reads, each with a unit of its own)."""
import os

import numpy as np

import align_ref
import period_ref
import refine_ref
import trace_ref

F, D, I = trace_ref.F, trace_ref.D, trace_ref.I
ITEM_DTYPE = trace_ref.ITEM_DTYPE
DTYPE = refine_ref.DTYPE
ANCHOR = refine_ref.FIELDS.index("reserved")


def unit_codes(word, k):
    return [(int(word) >> (2 * (k - 1 - j))) & 3 for j in range(k)]


def anchor(u):
    """(rho, M) of the unit codes u: every rotation written out, the smallest packed word wins"""
    k = len(u)
    rots = [[u[(j + q) % k] for j in range(k)] for q in range(k)]
    words = [period_ref.pack_unit(r) for r in rots]
    assert len(set(words)) == k, "a primitive unit has k distinct rotations"
    rho = min(range(k), key=lambda q: words[q])
    return rho, rots[rho]


def traced(rec, min_score):
    return int(rec[0]) > 0 and int(rec[4]) >= min_score


def decompose_read(read, min_period=1, max_period=32, penalty=3, min_score=24, doubling=False, restarted=False):
    """(the record as a tuple in the order of refine_ref.FIELDS with reserved = anchor, [items as trace_ref.items_of gives them])"""
    rec = refine_ref.refine_read(read, min_period, max_period, penalty, min_score)
    if not traced(rec, min_score):
        return rec, []
    k = rec[0]
    rho, M = anchor(unit_codes(rec[12], k))
    arec, _, cols = trace_ref.trace_strand(align_ref.codes(read), M, penalty, doubling=doubling, restarted=restarted)
    assert arec == rec[4:9], "the alignment record does not depend on the rotation"
    return rec[:ANCHOR] + (rho,) + rec[ANCHOR + 1:], trace_ref.items_of(cols, k)


def dirs_units(X, lens, T, ks, P):
    """trace_ref.dirs_many with a unit per read.  X: (R, n_max) codes, lens: (R,), T: (R, 32) unit codes (anything >= 8 past a
    read's unit length), ks: (R,) -> (records (R, 5), j* (R,), dirs (R, n_max + 1, 32) uint8 = op | d << 2).  Phase j of read r is
    live for j < ks[r], as in refine_ref._pass_many."""
    Rn, n_max = X.shape
    rows = np.arange(Rn)[:, None]
    j = np.arange(32, dtype=np.int64)[None, :]
    kk = ks.astype(np.int64)[:, None]
    live_j = j < kk
    src = {s: np.where(live_j, (j - s) % kk, j) for s in (1, 2, 4, 8, 16)}
    A = np.zeros((Rn, 32), dtype=np.int64)
    B = np.zeros((Rn, 32), dtype=np.int64)
    b_score, b_end, b_A, b_B = (np.zeros((Rn, 32), dtype=np.int64) for _ in range(4))
    dirs = np.zeros((Rn, n_max + 1, 32), dtype=np.uint8)
    one, pen = np.int64(1) << 32, np.int64(P) << 32
    better = align_ref._better
    for i in range(1, n_max + 1):
        live = (lens >= i)[:, None]
        hit = X[:, i - 1][:, None] == T
        dA, dB = A[rows, src[1]], B[rows, src[1]]
        dA = np.where(hit, dA + one, dA - pen)
        dB = np.where(hit, dB + one + 1, dB + one)
        VA = np.full((Rn, 32), i, dtype=np.int64)
        VB = np.zeros((Rn, 32), dtype=np.int64)
        op = np.full((Rn, 32), F, dtype=np.int64)
        for cA, cB, name in ((dA, dB, D), (A - pen, B, I)):
            take = (cA >= 0) & better((cA, cB), (VA, VB))
            VA, VB, op = np.where(take, cA, VA), np.where(take, cB, VB), np.where(take, name, op)
        dd = np.zeros((Rn, 32), dtype=np.int64)
        for s in (1, 2, 4, 8, 16):
            cA = VA[rows, src[s]] - np.int64(P * s) * one
            cB = VB[rows, src[s]] + np.int64(s) * one
            cd = dd[rows, src[s]] + s
            same = (cA == VA) & (cB == VB)
            take = (s < kk) & (cA >= 0) & (better((cA, cB), (VA, VB)) | (same & (cd < dd)))
            VA, VB, dd = np.where(take, cA, VA), np.where(take, cB, VB), np.where(take, cd, dd)
        dirs[:, i, :] = (op | (dd << 2)).astype(np.uint8)
        A, B = np.where(live, VA, A), np.where(live, VB, B)
        up = live & live_j & ((VA >> 32) > b_score)
        b_score = np.where(up, VA >> 32, b_score)
        b_end = np.where(up, i, b_end)
        b_A, b_B = np.where(up, VA, b_A), np.where(up, VB, b_B)
    rec = np.zeros((Rn, 5), dtype=np.int64)
    jstar = np.zeros(Rn, dtype=np.int64)
    for r in range(Rn):
        key = max((int(b_score[r, q]), -int(b_end[r, q]), int(b_A[r, q]) & 0xFFFFFFFF, int(b_B[r, q]) >> 32, int(b_B[r, q]) & 0xFFFFFFFF, -q)
                  for q in range(int(ks[r])))
        if key[0] > 0:
            rec[r] = (key[0], key[2], -key[1], key[3], key[4])
            jstar[r] = -key[5]
    return rec, jstar, dirs


def decompose(reads, min_period=1, max_period=32, penalty=3, min_score=24, recs=None, columns=None):
    """(items: ITEM_DTYPE array sorted by (read, start), motif = strand = 0; counts (n_reads,); records: DTYPE (n_reads,) with
    reserved = anchor), the vectorised form; `recs`: refine_ref.refine's records of these reads computed before; `columns`: a
    dict that receives the columns of trace_ref.walk of every read with items"""
    recs = (refine_ref.refine(reads, min_period, max_period, penalty, min_score) if recs is None else recs).copy()
    counts = np.zeros(len(reads), dtype=np.uint32)
    idx = [i for i in range(len(reads)) if traced(tuple(int(v) for v in recs[i]), min_score)]
    rows = []
    if idx:
        xs = [align_ref.codes(reads[i]) for i in idx]
        anchored = [anchor(unit_codes(recs["unit"][i], int(recs["period"][i]))) for i in idx]
        X, lens = refine_ref._plane(xs)
        T, ks = refine_ref._units([M for _, M in anchored])
        arec, jstar, dirs = dirs_units(X, lens, T, ks, penalty)
        for r, i in enumerate(idx):
            k = int(ks[r])
            rr = tuple(int(v) for v in arec[r])
            assert rr == tuple(int(recs[f][i]) for f in ("score", "start", "end", "consumed", "matches")), "the alignment record does not depend on the rotation"
            cols = trace_ref.walk_bytes(xs[r], anchored[r][1], rr, int(jstar[r]), dirs[r][:, :k])
            its = trace_ref.items_of(cols, k)
            if columns is not None:
                columns[i] = cols
            recs["reserved"][i] = anchored[r][0]
            counts[i] = len(its)
            rows += [(i, 0, 0) + it + (0,) for it in its]
    return np.array(rows, dtype=ITEM_DTYPE).reshape(-1), counts, recs


def anchor_word(rec):
    """M of a record (a DTYPE element) as a packed word"""
    k = int(rec["period"])
    return period_ref.pack_unit(anchor(unit_codes(rec["unit"], k))[1])


HEADER = refine_ref.HEADER + ",anchor,strand,units,edited,signature"
ITEM_HEADER = "read,length,period,anchor,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit"


def cli_lines(path, reads, result, penalty, min_score=24, per_item=False):
    """stdout of `trew decompose` (with --items: per_item) for one file: (the file's section, the >Summary section), formatted
    from result = (items, counts, records) of these reads"""
    items, _, recs = result[:3]
    texts = [r.decode("latin-1") if isinstance(r, (bytes, bytearray)) else r for r in reads]
    by_read = {}
    for it in items:
        by_read.setdefault(int(it["read"]), []).append(tuple(int(v) for v in it)[3:11])
    rows = [">" + os.path.realpath(path), ITEM_HEADER if per_item else HEADER]
    summary = {}
    for i, (read, x) in enumerate(zip(texts, recs)):
        d = int(x["period"])
        if d == 0 or int(x["score"]) < min_score:
            continue
        c = refine_ref.columns(x, penalty)
        canon = period_ref.canonical(x["unit"], d)
        m = anchor_word(x)
        assert m == period_ref.pack_unit(unit_codes(x["unit"], d)[int(x["reserved"]):] + unit_codes(x["unit"], d)[:int(x["reserved"])])
        its = by_read[i]
        units, edited, sig = trace_ref.signature(read, d, 0, its)
        sp = int(x["seed_period"])
        if per_item:
            for it in its:
                unit = trace_ref.signature(read, d, 0, [it])[2]
                rows.append("%d,%d,%d,%s,%s,%s" % (i, len(read), d, period_ref.unit_text(m, d), ",".join(str(v) for v in it), "=" if unit[0] == "=" else unit))
        else:
            rows.append("%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%s,%d,%d,%d,%s,%s,%d,%d,%s" % (
                i, len(read), d, period_ref.unit_text(x["unit"], d), period_ref.unit_text(canon, d), x["start"], x["end"], x["score"], c["copies"],
                x["consumed"], x["matches"], c["mismatches"], c["insertions"], c["deletions"], sp, period_ref.unit_text(x["seed_unit"], sp),
                x["seed_score"], x["changed"], x["scored_period"], period_ref.unit_text(m, d), "+" if canon == m else "-", units, edited, sig))
        add = (1, int(x["end"]) - int(x["start"]), c["copies"], units, edited, len(its))
        summary[(d, canon)] = tuple(a + b for a, b in zip(summary.get((d, canon), (0,) * 6), add))
    tail = [">Summary", "period,canonical,reads,bases,copies,units,edited,items"]
    for (d, canon), v in sorted(summary.items(), key=lambda kv: (-kv[1][0], kv[0])):
        tail.append("%d,%s,%s" % (d, period_ref.unit_text(canon, d), ",".join(str(a) for a in v)))
    return rows, tail
