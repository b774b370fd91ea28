"""Brute-force reference of the traceback of the wraparound alignment for units of up to 256 bases (trew_hip_copies):
trace_ref.py's definition, word for word, with 3 <= k <= 256.  Independent of the library and of oracle/.

Three forms that must agree:

  trace_ref.table(x, t, P)   the definition cell by cell in plain Python, generic in k: O(n k^2) tuple compares
  table(x, t, P)             the same definition -- every d of every cell tried, the smallest d that attains the largest tuple
                             kept -- with numpy over (d, j): O(n k^2) still, fast enough for k = 256
  del_table(x, t, P)         the linear-plus-wrap closure of monomer_ref.py with one bit a cell in the place of d:
                             del = "H[j] is strictly larger than V[j] was before the closure".  d is recovered by following the
                             bits: while del[j]: j <- (j - 1) mod k.

table() also says where a tie rule decided: the diagonal and the inserted read base both give V (rule 1), more than one d gives
H (rule 2)."""
import numpy as np

import align_ref as A
import monomer_ref as M
import trace_ref as T

F, D, I = T.F, T.D, T.I
ITEM_DTYPE = T.ITEM_DTYPE


def table(x, t, P, row0=0, row_end=None):
    """rows row0 + 1 .. row_end of the table that has H[row0][j] = (0, row0, 0, 0) -> (record, j*, op, d, tie_v, tie_h); op, d,
    tie_v, tie_h are (n + 1, k) arrays indexed by the row"""
    k = len(t)
    n = len(x) if row_end is None else row_end
    tt = np.asarray(t, dtype=np.int64)
    one = np.int64(1) << 32
    j = np.arange(k)
    dcol = np.arange(k, dtype=np.int64)[:, None]
    src = (j[None, :] - dcol) % k  # src[d][j] = (j - d) mod k
    HA = np.full(k, row0, dtype=np.int64)
    HB = np.zeros(k, dtype=np.int64)
    op = np.zeros((n + 1, k), dtype=np.int64)
    dd = np.zeros((n + 1, k), dtype=np.int64)
    tie_v = np.zeros((n + 1, k), dtype=bool)
    tie_h = np.zeros((n + 1, k), dtype=bool)
    best = (0, 0, 0, 0, 0, 0)  # (score, -end, start, consumed, matches, -j)
    for i in range(row0 + 1, n + 1):
        hit = x[i - 1] == tt
        dA, dB = np.roll(HA, 1), np.roll(HB, 1)
        dA = np.where(hit, dA + one, dA - P * one)
        dB = np.where(hit, dB + one + 1, dB + one)
        iA, iB = HA - P * one, HB
        VA = np.full(k, i, dtype=np.int64)
        VB = np.zeros(k, dtype=np.int64)
        o = np.full(k, F, dtype=np.int64)
        for cA, cB, name in ((dA, dB, D), (iA, iB, I)):  # rule 1: F, D, I on equal tuples
            take = (cA >= 0) & A._better((cA, cB), (VA, VB))
            VA, VB, o = np.where(take, cA, VA), np.where(take, cB, VB), np.where(take, name, o)
        tie_v[i] = (o != F) & (dA == iA) & (dB == iB) & (dA == VA) & (dB == VB)
        cA = VA[src] - (np.int64(P) * dcol) * one  # every d of every cell
        cB = VB[src] + dcol * one
        ok = cA >= 0
        mA = np.where(ok, cA, -1).max(axis=0)
        m1 = ok & (cA == mA[None, :])
        mB = np.where(m1, cB, -1).max(axis=0)
        m2 = m1 & (cB == mB[None, :])
        op[i], dd[i], tie_h[i] = o, m2.argmax(axis=0), m2.sum(axis=0) > 1  # rule 2: the smallest d
        HA, HB = mA, mB
        for jj in range(k):
            best = max(best, (int(HA[jj]) >> 32, -i, int(HA[jj]) & 0xFFFFFFFF, int(HB[jj]) >> 32, int(HB[jj]) & 0xFFFFFFFF, -jj))
    if best[0] == 0:
        return (0, 0, 0, 0, 0), 0, op, dd, tie_v, tie_h
    return (best[0], best[2], -best[1], best[3], best[4]), -best[5], op, dd, tie_v, tie_h


def del_table(x, t, P, row0=0, row_end=None):
    """the same rows in the linear-plus-wrap form -> (record, j*, op, dl): dl[i][j] is the cell's one bit"""
    k = len(t)
    n = len(x) if row_end is None else row_end
    H = [(0, row0, 0, 0)] * k
    op, dl = {row0: [F] * k}, {row0: [False] * k}
    best = (0, 0, 0, 0, 0, 0)

    def shifted(c, d):
        return (c[0] - P * d, c[1], c[2] + d, c[3])

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
        L = list(V)
        for j in range(1, k):
            L[j] = max(L[j], shifted(L[j - 1], 1))
        W = L[k - 1]
        H = [max(L[j], shifted(W, j + 1)) for j in range(k)]
        op[i], dl[i] = o, [H[j] > V[j] for j in range(k)]
        for j, (s, b, C, m) in enumerate(H):
            best = max(best, (s, -i, b, C, m, -j))
    if best[0] == 0:
        return (0, 0, 0, 0, 0), 0, op, dl
    return (best[0], best[2], -best[1], best[3], best[4]), -best[5], op, dl


def d_of_bits(bits, j):
    """the d of cell j recovered from a row of bits: the steps down while the bit is set"""
    k, d = len(bits), 0
    while bits[j]:
        j, d = (j - 1) % k, d + 1
        assert d < k
    return d


def path_ties(rec, jstar, op, dd, tie_v, tie_h):
    """(a D/I tie, a d tie) on the traced path of one key's table()"""
    k = op.shape[1]
    i, j = rec[2], jstar
    di = dt = False
    while True:
        dt |= bool(tie_h[i][j])
        j = (j - int(dd[i][j])) % k
        o = int(op[i][j])
        if o == F:
            return di, dt
        di |= bool(tie_v[i][j])
        if o == D:
            j = (j - 1) % k
        i -= 1


def copies_keys(reads, units, penalty=3, min_score=24):
    """{(read, unit, strand): (record, j*, columns, (D/I tie on the path, d tie on the path))} for every key whose score (by
    monomer_ref's O(n k) form) reaches min_score, the table by table(): the full one, from row 0"""
    out = {}
    recs = M.monomers(reads, units, penalty)
    for r, read in enumerate(reads):
        x = A.codes(read)
        for m, unit in enumerate(units):
            for s, sfx in enumerate(("_fwd", "_rev")):
                if int(recs["score" + sfx][r, m]) < min_score:
                    continue
                t = M.strand_codes(unit, s)
                rec, jstar, op, dd, tie_v, tie_h = table(x, t, penalty)
                assert rec == tuple(int(recs[f + sfx][r, m]) for f in ("score", "start", "end", "consumed", "matches"))
                out[(r, m, s)] = (rec, jstar, T.walk(x, t, rec, jstar, op, dd), path_ties(rec, jstar, op, dd, tie_v, tie_h))
    return out, recs


def copies(reads, units, penalty=3, min_score=24, keys=None):
    """(items: ITEM_DTYPE array sorted by (read, unit, strand, start), counts (n_reads, n_units, 2), records: align_ref.DTYPE
    (n_reads, n_units), n_rows); `keys`: a copies_keys result computed before"""
    keys, recs = copies_keys(reads, units, penalty, min_score) if keys is None else keys
    rows, n_rows = [], 0
    counts = np.zeros((len(reads), len(units), 2), dtype=np.uint32)
    for (r, m, s), (rec, _, cols, _) in sorted(keys.items()):
        its = T.items_of(cols, len(units[m]))
        counts[r, m, s] = len(its)
        n_rows += rec[2] - rec[1]
        rows += [(r, m, s) + it + (0,) for it in its]
    return np.array(rows, dtype=ITEM_DTYPE).reshape(-1), counts, recs, n_rows


def signature(read, k, strand, items, bases=False):
    """(units, edited, signature text) of one key's items (tuples start, bases, count, phase, consumed, sub, ins, del) as `trew
    copies` prints them: trace_ref.signature for k <= 32 or with bases, else bases:mismatches.insertions.deletions for an item
    that is no run, an end piece in parentheses"""
    if k <= 32 or bases:
        return T.signature(read, k, strand, items)
    units = edited = 0
    parts = []
    for start, nb, count, phase, consumed, sub, ins, dele in items:
        if consumed == k * count:
            units += count
        err = sub + ins + dele
        edited += err > 0
        if count > 1 or (consumed == k and phase == 0 and not err):
            parts.append("=%d" % count)
            continue
        text = "%d:%d.%d.%d" % (nb, sub, ins, dele)
        parts.append(text if consumed == k else "(" + text + ")")
    return units, edited, " ".join(parts)


def cli_lines(path, reads, names, units, traced, penalty, min_score=24, per_item=False, bases=False):
    """stdout of `trew copies` (with --items: per_item; with --bases: bases), formatted from traced = (items, counts, records) of
    these reads; names: the typed texts or the FASTA names"""
    import os

    items, _, a = traced[:3]
    texts = [r.decode("latin-1") if isinstance(r, (bytes, bytearray)) else r for r in reads]
    by_key = {}
    for it in items:
        by_key.setdefault((int(it["read"]), int(it["motif"]), int(it["strand"])), []).append(tuple(int(v) for v in it)[3:11])
    lines = [">" + os.path.realpath(path)]
    lines.append("read,length,motif,strand,start,bases,count,phase,consumed,mismatches,insertions,deletions,unit" if per_item else
                 "read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,signature")
    sums = {(m, s): [0] * 12 for m in range(len(units)) for s in range(2)}
    for r, read in enumerate(texts):
        for m, unit in enumerate(units):
            k = len(unit)
            for s, sfx in enumerate(("_fwd", "_rev")):
                score, start, end, consumed, matches = (int(a[f + sfx][r, m]) for f in ("score", "start", "end", "consumed", "matches"))
                if score < min_score:
                    continue
                its = by_key[(r, m, s)]
                c = A.columns(score, start, end, consumed, matches, k, penalty)
                n_units, edited, sig = signature(read, k, s, its, bases)
                row = (start, end, score, c["copies"], consumed, matches, c["mismatches"], c["insertions"], c["deletions"])
                if per_item:
                    for it in its:
                        text = T.signature(read, k, s, [it])[2]
                        unit_col = "=" if text[0] == "=" else text if k <= 32 or bases else ""
                        lines.append("%d,%d,%s,%s,%s,%s" % (r, len(read), names[m], "+-"[s], ",".join(str(x) for x in it), unit_col))
                else:
                    lines.append("%d,%d,%s,%s,%s,%d,%d,%s" % (r, len(read), names[m], "+-"[s], ",".join(str(x) for x in row), n_units, edited, sig))
                add = (1, end - start) + row[2:] + (n_units, edited, len(its))
                sums[(m, s)] = [x + y for x, y in zip(sums[(m, s)], add)]
    lines += [">Summary", "motif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions,units,edited,items"]
    for m in range(len(units)):
        for s in range(2):
            lines.append("%s,%s,%d,%s" % (names[m], "+-"[s], len(reads), ",".join(str(x) for x in sums[(m, s)])))
    return lines
