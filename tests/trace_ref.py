"""Brute-force reference of the traceback of the wraparound alignment (trew_hip_trace): the alignment of align_ref.py with
three tie rules, walked back from its end cell and cut into copies of the motif.  Independent of the library and of oracle/.

Everything is align_ref.py's: the codes, M_s, P, the tuples (score, start, consumed, matches), V, H and the record.  Added:

  1. V[i][j]: among candidates with equal tuples the fresh start comes first, then the diagonal, then the inserted read base;
     op in {F, D, I} names the winner.
  2. H[i][j]: d is the smallest d < k that attains the largest tuple.
  3. The end cell is (end, j*) of the record; on equal (score, -i, start, consumed, matches) the smallest j wins.

The walk starts at the end cell.  At H[i][j] it emits d columns `del` for the phases j, j - 1, ..., j - d + 1, sets
j <- (j - d) mod k and looks at op of V[i][j]: F ends the walk (i = start); D emits `eq` or `sub` for (read base i - 1, phase j)
and goes to H[i-1][(j-1) mod k]; I emits `ins` (read base i - 1, no phase) and goes to H[i-1][j].  Reversed, the columns are
the alignment in read order.  A segment begins at the first column and in front of every column whose phase is 0; an `ins`
stays in the running segment.  A segment is one item (start, bases, count = 1, phase, consumed, mismatches, insertions,
deletions); consecutive complete exact copies (phase 0, consumed k, no error) merge into one item with count = r.

Three forms that must agree: table(..., doubling=False) is the definition cell by cell, max over d included; table(...,
doubling=True) replaces the max over d by the steps 1, 2, 4, 8, 16 with d carried beside the tuple; dirs_many is the second
form vectorised with numpy over j and over many reads.  table(..., row0=start) is the table restarted at the tract's start."""
import os

import numpy as np

import align_ref as R

F, D, I = 0, 1, 2
ITEM_FIELDS = ("read", "motif", "strand", "start", "bases", "count", "phase", "consumed", "mismatches", "insertions", "deletions", "reserved")
ITEM_DTYPE = np.dtype([(f, "<u4") for f in ITEM_FIELDS])


def table(x, t, P, row0=0, row_end=None, doubling=False, ties=None):
    """rows row0 + 1 .. row_end of the table that has H[row0][j] = (0, row0, 0, 0) -> (record, j*, op, d); op[i][j] and d[i][j]
    are dicts of lists by row.  row0 = 0 is the full table.  ties: a dict that receives "end", the phases whose cell in row
    `end` equals the end cell."""
    k = len(t)
    n = len(x) if row_end is None else row_end
    H = [(0, row0, 0, 0)] * k
    op, dd = {row0: [F] * k}, {row0: [0] * k}
    best = (0, 0, 0, 0, 0, 0)  # (score, -end, start, consumed, matches, -j)
    rows_H = {}
    for i in range(row0 + 1, n + 1):
        c = x[i - 1]
        V, o = [], []
        for j in range(k):
            s, b, C, m = H[(j - 1) % k]
            diag = (s + 1, b, C + 1, m + 1) if c == t[j] else (s - P, b, C + 1, m)
            s, b, C, m = H[j]
            cell, w = (0, i, 0, 0), F
            if diag > cell:
                cell, w = diag, D
            if (s - P, b, C, m) > cell:
                cell, w = (s - P, b, C, m), I
            V.append(cell)
            o.append(w)
        if not doubling:
            H, dl = [], []
            for j in range(k):
                cell, w = V[j], 0
                for d in range(1, k):
                    s, b, C, m = V[(j - d) % k]
                    if (s - P * d, b, C + d, m) > cell:
                        cell, w = (s - P * d, b, C + d, m), d
                H.append(cell)
                dl.append(w)
        else:
            H, dl = list(V), [0] * k
            for st in (1, 2, 4, 8, 16):
                if st >= k:
                    break
                nH, nd = list(H), list(dl)
                for j in range(k):
                    s, b, C, m = H[(j - st) % k]
                    cand, cd = (s - P * st, b, C + st, m), dl[(j - st) % k] + st
                    if cand > H[j] or (cand == H[j] and cd < dl[j]):
                        nH[j], nd[j] = cand, cd
                H, dl = nH, nd
        op[i], dd[i] = o, dl
        for j, (s, b, C, m) in enumerate(H):
            best = max(best, (s, -i, b, C, m, -j))
        rows_H[i] = H
    if best[0] == 0:
        return (0, 0, 0, 0, 0), 0, op, dd
    if ties is not None:
        ties["end"] = [j for j, cell in enumerate(rows_H[-best[1]]) if cell == (best[0], best[2], best[3], best[4])]
    return (best[0], best[2], -best[1], best[3], best[4]), -best[5], op, dd


def walk(x, t, rec, jstar, op, dd):
    """the columns (kind, read base or None, phase or None) in read order"""
    k = len(t)
    i, j = rec[2], jstar
    cols = []
    while True:
        d = dd[i][j]
        for q in range(d):
            cols.append(("del", None, (j - q) % k))
        j = (j - d) % k
        o = op[i][j]
        if o == F:
            assert i == rec[1], "the walk ends at the record's start"
            break
        if o == D:
            cols.append(("eq" if x[i - 1] == t[j] else "sub", i - 1, j))
            j = (j - 1) % k
        else:
            cols.append(("ins", i - 1, None))
        i -= 1
    cols.reverse()
    return cols


def items_of(cols, k):
    """[(start, bases, count, phase, consumed, mismatches, insertions, deletions)] of one key's columns, runs merged"""
    segs, cur = [], None
    for kind, base, phase in cols:
        if cur is None or phase == 0:
            cur = dict(start=None, bases=0, phase=None, consumed=0, sub=0, ins=0, dele=0)
            segs.append(cur)
        if phase is not None:
            cur["consumed"] += 1
            if cur["phase"] is None:
                cur["phase"] = phase
        if base is not None:
            cur["bases"] += 1
            if cur["start"] is None:
                cur["start"] = base
        cur["sub"] += kind == "sub"
        cur["ins"] += kind == "ins"
        cur["dele"] += kind == "del"
    # a segment of deleted bases alone (no read base) starts where the next read base lies
    nxt = None
    for sg in reversed(segs):
        if sg["start"] is None:
            sg["start"] = nxt
        nxt = sg["start"]
    out = []
    for sg in segs:
        exact = sg["phase"] == 0 and sg["consumed"] == k and not (sg["sub"] or sg["ins"] or sg["dele"])
        if exact and out and out[-1][-1]:
            p = out[-1][0]
            out[-1] = ((p[0], p[1] + k, p[2] + 1, 0, p[4] + k, 0, 0, 0), True)
        else:
            out.append(((sg["start"], sg["bases"], 1, sg["phase"], sg["consumed"], sg["sub"], sg["ins"], sg["dele"]), exact))
    return [it for it, _ in out]


def trace_strand(x, t, P, doubling=False, restarted=False):
    """(record, j*, columns) of one strand from the single-read forms"""
    rec, jstar, op, dd = table(x, t, P, doubling=doubling)
    if rec[0] == 0:
        return rec, 0, []
    if restarted:
        rec2, j2, op, dd = table(x, t, P, row0=rec[1], row_end=rec[2], doubling=doubling)
        assert rec2 == rec and j2 == jstar, "the restarted table has the same record and end phase"
    return rec, jstar, walk(x, t, rec, jstar, op, dd)


def dirs_many(X, lens, t, P):
    """X: (R, n_max) codes, lens: (R,) -> (records (R, 5), j* (R,), dirs (R, n_max + 1, k) uint8 = op | d << 2, ties (R, n_max + 1,
    k) uint8): the doubling form of align_ref._strand_many with (op, d) beside the tuple.  ties: bit 0, the diagonal and the
    inserted read base both give the cell's V; bit 1, more than one d gives the cell's H (a tie rule decided there)."""
    Rn, n_max = X.shape
    k = len(t)
    tt = np.asarray(t, dtype=np.int64)[None, :]
    A = np.zeros((Rn, k), dtype=np.int64)
    B = np.zeros((Rn, k), dtype=np.int64)
    b_score = np.zeros((Rn, k), dtype=np.int64)
    b_end = np.zeros((Rn, k), dtype=np.int64)
    b_A = np.zeros((Rn, k), dtype=np.int64)
    b_B = np.zeros((Rn, k), dtype=np.int64)
    dirs = np.zeros((Rn, n_max + 1, k), dtype=np.uint8)
    ties = np.zeros((Rn, n_max + 1, k), dtype=np.uint8)
    one, pen = np.int64(1) << 32, np.int64(P) << 32
    better = R._better
    for i in range(1, n_max + 1):
        live = (lens >= i)[:, None]
        hit = X[:, i - 1][:, None] == tt
        dA, dB = np.roll(A, 1, axis=1), np.roll(B, 1, axis=1)
        dA = np.where(hit, dA + one, dA - pen)
        dB = np.where(hit, dB + one + 1, dB + one)
        VA = np.full((Rn, k), i, dtype=np.int64)
        VB = np.zeros((Rn, k), dtype=np.int64)
        op = np.full((Rn, k), F, dtype=np.int64)
        for cA, cB, name in ((dA, dB, D), (A - pen, B, I)):
            take = (cA >= 0) & better((cA, cB), (VA, VB))
            VA, VB, op = np.where(take, cA, VA), np.where(take, cB, VB), np.where(take, name, op)
        tie_v = (op != F) & (dA == A - pen) & (dB == B) & (dA == VA) & (dB == VB)
        dd = np.zeros((Rn, k), dtype=np.int64)
        tie_h = np.zeros((Rn, k), dtype=bool)
        for s in (1, 2, 4, 8, 16):
            if s >= k:
                break
            cA = np.roll(VA, s, axis=1) - np.int64(P * s) * one
            cB = np.roll(VB, s, axis=1) + np.int64(s) * one
            cd = np.roll(dd, s, axis=1) + s
            same = (cA == VA) & (cB == VB)
            take = (cA >= 0) & (better((cA, cB), (VA, VB)) | (same & (cd < dd)))
            tie_h = np.where(take, np.roll(tie_h, s, axis=1) | same, tie_h | same)
            VA, VB, dd = np.where(take, cA, VA), np.where(take, cB, VB), np.where(take, cd, dd)
        dirs[:, i, :] = (op | (dd << 2)).astype(np.uint8)
        ties[:, i, :] = tie_v.astype(np.uint8) | (tie_h.astype(np.uint8) << 1)
        A, B = np.where(live, VA, A), np.where(live, VB, B)
        up = live & ((VA >> 32) > b_score)
        b_score = np.where(up, VA >> 32, b_score)
        b_end = np.where(up, i, b_end)
        b_A, b_B = np.where(up, VA, b_A), np.where(up, VB, b_B)
    rec = np.zeros((Rn, 5), dtype=np.int64)
    jstar = np.zeros(Rn, dtype=np.int64)
    for r in range(Rn):
        key = max((int(b_score[r, j]), -int(b_end[r, j]), int(b_A[r, j]) & 0xFFFFFFFF, int(b_B[r, j]) >> 32, int(b_B[r, j]) & 0xFFFFFFFF, -j)
                  for j in range(k))
        if key[0] > 0:
            rec[r] = (key[0], key[2], -key[1], key[3], key[4])
            jstar[r] = -key[5]
    return rec, jstar, dirs, ties


def path_ties(t, rec, jstar, dirs, ties):
    """(a D/I tie, a d tie) on the traced path of one read's byte tables"""
    k = len(t)
    i, j = rec[2], jstar
    di = dt = False
    while True:
        dt |= bool(ties[i][j] & 2)
        j = (j - (int(dirs[i][j]) >> 2)) % k
        o = int(dirs[i][j]) & 3
        if o == F:
            return di, dt
        di |= bool(ties[i][j] & 1)
        if o == D:
            j = (j - 1) % k
        i -= 1


def walk_bytes(x, t, rec, jstar, dirs):
    """walk() on the byte table of dirs_many (one read's (n + 1, k) slice)"""
    d = dirs.astype(np.int64)
    return walk(x, t, rec, jstar, d & 3, d >> 2)


def trace_keys(reads, motifs, penalty=3):
    """{(read, motif, strand): (record, j*, columns, (D/I tie on the path, d tie on the path))} for every key with a positive
    score, by dirs_many"""
    out = {}
    if not len(reads):
        return out
    cs = [R.codes(r) for r in reads]
    lens = np.array([len(c) for c in cs], dtype=np.int64)
    X = np.full((len(cs), max(int(lens.max()), 1)), 4, dtype=np.int64)
    for r, c in enumerate(cs):
        X[r, :len(c)] = c
    for m, motif in enumerate(motifs):
        for s in range(2):
            t = R.strand_codes(motif, s)
            rec, jstar, dirs, ties = dirs_many(X, lens, t, penalty)
            for r in range(len(cs)):
                if rec[r, 0] > 0:
                    rr = tuple(int(v) for v in rec[r])
                    out[(r, m, s)] = (rr, int(jstar[r]), walk_bytes(cs[r], t, rr, int(jstar[r]), dirs[r]), path_ties(t, rr, int(jstar[r]), dirs[r], ties[r]))
    return out


def trace(reads, motifs, penalty=3, min_score=24, keys=None):
    """(items: ITEM_DTYPE array sorted by (read, motif, strand, start), counts (n_reads, n_motifs, 2), records: align_ref.DTYPE
    (n_reads, n_motifs)); `keys`: a trace_keys result computed before"""
    keys = trace_keys(reads, motifs, penalty) if keys is None else keys
    rows = []
    counts = np.zeros((len(reads), len(motifs), 2), dtype=np.uint32)
    recs = np.zeros((len(reads), len(motifs)), dtype=R.DTYPE)
    for (r, m, s), (rec, _, cols, _) in sorted(keys.items()):
        for f, name in enumerate(("score", "start", "end", "consumed", "matches")):
            recs[name + ("_fwd", "_rev")[s]][r, m] = rec[f]
        if rec[0] < min_score:
            continue
        its = items_of(cols, len(motifs[m]))
        counts[r, m, s] = len(its)
        rows += [(r, m, s) + it + (0,) for it in its]
    return np.array(rows, dtype=ITEM_DTYPE).reshape(-1), counts, recs


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def signature(read, k, strand, items):
    """(units, edited, signature text) of one key's items (tuples start, bases, count, phase, consumed, sub, ins, del) as
    `trew trace` prints them"""
    units = edited = 0
    parts = []
    for start, bases, count, phase, consumed, sub, ins, dele in items:
        if consumed == k * count:
            units += count
        err = sub + ins + dele
        edited += err > 0
        if count > 1 or (consumed == k and phase == 0 and not err):
            parts.append("=%d" % count)
            continue
        text = read[start:start + bases].upper()
        if strand:
            text = "".join(_COMP.get(c, "N") for c in reversed(text))
        parts.append(text if consumed == k else text.lower())
    return units, edited, " ".join(parts)


def cli_lines(path, reads, motifs, traced, penalty, min_score=24, per_item=False):
    """stdout of `trew trace` (with --items: per_item), formatted from traced = (items, counts, records) of these reads"""
    items, _, a = traced[:3]
    texts = [r.decode("latin-1") if isinstance(r, (bytes, bytearray)) else r for r in reads]
    by_key = {}
    for it in items:
        by_key.setdefault((int(it["read"]), int(it["motif"]), int(it["strand"])), []).append(tuple(int(v) for v in it)[3:11])
    lines = [">" + os.path.realpath(path)]
    lines.append("read,length,motif,strand,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit" if per_item else
                 "read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,signature")
    sums = {(m, s): [0] * 12 for m in range(len(motifs)) for s in range(2)}
    for r, read in enumerate(texts):
        for m, motif in enumerate(motifs):
            for s, sfx in enumerate(("_fwd", "_rev")):
                score, start, end, consumed, matches = (int(a[f + sfx][r, m]) for f in ("score", "start", "end", "consumed", "matches"))
                if score < min_score:
                    continue
                its = by_key[(r, m, s)]
                c = R.columns(score, start, end, consumed, matches, len(motif), penalty)
                units, edited, sig = signature(read, len(motif), s, its)
                row = (start, end, score, c["copies"], consumed, matches, c["mismatches"], c["insertions"], c["deletions"])
                if per_item:
                    for it in its:
                        unit = signature(read, len(motif), s, [it])[2]
                        lines.append("%d,%d,%s,%s,%s,%s" % (r, len(read), motif, "+-"[s], ",".join(str(x) for x in it), "=" if unit[0] == "=" else unit))
                else:
                    lines.append("%d,%d,%s,%s,%s,%d,%d,%s" % (r, len(read), motif, "+-"[s], ",".join(str(x) for x in row), units, edited, sig))
                add = (1, end - start) + row[2:] + (units, edited, len(its))
                sums[(m, s)] = [x + y for x, y in zip(sums[(m, s)], add)]
    lines += [">Summary", "motif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,items"]
    for m, motif in enumerate(motifs):
        for s in range(2):
            lines.append("%s,%s,%d,%s" % (motif, "+-"[s], len(reads), ",".join(str(x) for x in sums[(m, s)])))
    return lines
