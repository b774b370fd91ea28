"""Brute-force reference of the indel-aware motif tract per read (trew_hip_align): a local alignment of the read against
the motif repeated without end (wraparound dynamic programming).  Independent of the library and of oracle/.

A cell holds a tuple (score, start, consumed, matches), compared lexicographically, the larger one wins.  With the text
T[j] = M_s[j mod k] (strand 1: the reverse complement of the motif), H[0][j] = (0, 0, 0, 0) and for i = 1 .. n

  V[i][j] = max( (0, i, 0, 0),                                                            a fresh start
                 H[i-1][(j-1) mod k] + (+1, ., +1, +1) if x[i-1] == M_s[j] else (-P, ., +1, 0),  the diagonal (N matches nothing)
                 H[i-1][j] + (-P, ., 0, 0) )                                               an inserted read base
  H[i][j] = max over d = 0 .. k-1 of V[i][(j-d) mod k] + (-P d, ., +d, 0)                 d deleted motif bases

The record of a strand is the cell with the largest (score, -i, start, consumed, matches): (score, start, end = i, consumed,
matches), all zero when the largest score is 0.

Two forms that must agree: align_read (the definition above in plain Python tuples, O(n k^2)) and align (the max over d
replaced by the five doubling steps 1, 2, 4, 8, 16 on the cyclic order, vectorised over j and over many reads with numpy)."""
import os

import numpy as np

FIELDS = tuple(name + sfx for sfx in ("_fwd", "_rev") for name in ("score", "start", "end", "consumed", "matches"))
DTYPE = np.dtype([(f, "<u4") for f in FIELDS])
COLUMNS = ("copies", "mismatches", "insertions", "deletions")
_CODE = {"T": 0, "G": 1, "C": 2, "A": 3}


def codes(read):
    if isinstance(read, (bytes, bytearray)):
        read = read.decode("latin-1")
    return [_CODE.get(c.upper(), 4) for c in read]


def strand_codes(motif, strand):
    c = codes(motif)
    assert 3 <= len(c) <= 32 and max(c) < 4
    return [3 - x for x in reversed(c)] if strand else c


def align_strand(x, t, P):
    """x: the codes of the read, t: the codes of the strand's target -> (score, start, end, consumed, matches)"""
    k = len(t)
    H = [(0, 0, 0, 0)] * k
    best = (0, 0, 0, 0, 0)  # (score, -end, start, consumed, matches)
    for i in range(1, len(x) + 1):
        c = x[i - 1]
        V = []
        for j in range(k):
            s, b, C, m = H[(j - 1) % k]
            diag = (s + 1, b, C + 1, m + 1) if c == t[j] else (s - P, b, C + 1, m)
            s, b, C, m = H[j]
            V.append(max((0, i, 0, 0), diag, (s - P, b, C, m)))
        H = []
        for j in range(k):
            cands = []
            for d in range(k):
                s, b, C, m = V[(j - d) % k]
                cands.append((s - P * d, b, C + d, m))
            H.append(max(cands))
        for s, b, C, m in H:
            best = max(best, (s, -i, b, C, m))
    if best[0] == 0:
        return (0, 0, 0, 0, 0)
    return (best[0], best[2], -best[1], best[3], best[4])


def align_read(read, motif, penalty=3):
    """the ten fields of one (read, motif) from the definition"""
    x = codes(read)
    return align_strand(x, strand_codes(motif, 0), penalty) + align_strand(x, strand_codes(motif, 1), penalty)


def _better(a, b):
    """a, b: pairs of int64 key arrays (score << 32 | start, consumed << 32 | matches) -> where a is the larger tuple"""
    return (a[0] > b[0]) | ((a[0] == b[0]) & (a[1] > b[1]))


def _strand_many(X, lens, t, P):
    """X: (R, n_max) codes, lens: (R,), t: target codes -> (R, 5) int64 records.  Scores in H are never negative (the fresh
    start is always a candidate), so a tuple is the two keys A = score << 32 | start and B = consumed << 32 | matches."""
    R, n_max = X.shape
    k = len(t)
    t = np.asarray(t, dtype=np.int64)[None, :]
    A = np.zeros((R, k), dtype=np.int64)
    B = np.zeros((R, k), dtype=np.int64)
    b_score = np.zeros((R, k), dtype=np.int64)
    b_end = np.zeros((R, k), dtype=np.int64)
    b_A = np.zeros((R, k), dtype=np.int64)
    b_B = np.zeros((R, k), dtype=np.int64)
    one, pen = np.int64(1) << 32, np.int64(P) << 32
    for i in range(1, n_max + 1):
        live = (lens >= i)[:, None]
        c = X[:, i - 1][:, None]
        hit = c == t
        dA, dB = np.roll(A, 1, axis=1), np.roll(B, 1, axis=1)
        dA = np.where(hit, dA + one, dA - pen)
        dB = np.where(hit, dB + one + 1, dB + one)
        iA, iB = A - pen, B
        VA = np.full((R, k), i, dtype=np.int64)
        VB = np.zeros((R, k), dtype=np.int64)
        for cA, cB in ((dA, dB), (iA, iB)):
            take = (cA >= 0) & _better((cA, cB), (VA, VB))  # a negative score loses to the fresh start
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        for s in (1, 2, 4, 8, 16):
            cA = np.roll(VA, s, axis=1) - np.int64(P * s) * one
            cB = np.roll(VB, s, axis=1) + np.int64(s) * one
            take = (cA >= 0) & _better((cA, cB), (VA, VB))
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        A, B = np.where(live, VA, A), np.where(live, VB, B)
        up = live & ((VA >> 32) > b_score)  # strictly: the earliest end stays
        b_score = np.where(up, VA >> 32, b_score)
        b_end = np.where(up, i, b_end)
        b_A, b_B = np.where(up, VA, b_A), np.where(up, VB, b_B)
    out = np.zeros((R, 5), dtype=np.int64)
    for r in range(R):
        key = max((int(b_score[r, j]), -int(b_end[r, j]), int(b_A[r, j]) & 0xFFFFFFFF, int(b_B[r, j]) >> 32, int(b_B[r, j]) & 0xFFFFFFFF)
                  for j in range(k))
        if key[0] > 0:
            out[r] = (key[0], key[2], -key[1], key[3], key[4])
    return out


def align(reads, motifs, penalty=3):
    """DTYPE records of shape (n_reads, n_motifs), the O(n k) form"""
    out = np.zeros((len(reads), len(motifs)), dtype=DTYPE)
    if not len(reads):
        return out
    cs = [codes(r) for r in reads]
    lens = np.array([len(c) for c in cs], dtype=np.int64)
    X = np.full((len(cs), max(int(lens.max()), 1)), 4, dtype=np.int64)
    for r, c in enumerate(cs):
        X[r, :len(c)] = c
    for m, motif in enumerate(motifs):
        for s, sfx in enumerate(("_fwd", "_rev")):
            rec = _strand_many(X, lens, strand_codes(motif, s), penalty)
            for f, name in enumerate(("score", "start", "end", "consumed", "matches")):
                out[name + sfx][:, m] = rec[:, f]
    return out


def columns(score, start, end, consumed, matches, k, penalty):
    """the derived columns of one strand's record: dict of copies, mismatches, insertions, deletions (all exact)"""
    L = end - start
    assert (matches - score) % penalty == 0
    E = (matches - score) // penalty
    deletions = E - (L - matches)
    insertions = E - (consumed - matches)
    return dict(copies=consumed // k, mismatches=L - matches - insertions, insertions=insertions, deletions=deletions)


def cli_lines(path, reads, motifs, a, penalty, min_score=24):
    """stdout of `trew align`, formatted from the records a"""
    lines = [">" + os.path.realpath(path), "read,length,motif,strand,start,end,score,copies,consumed,matches,mismatches,insertions,deletions"]
    sums = {(m, s): [0] * 9 for m in range(len(motifs)) for s in range(2)}
    for r, read in enumerate(reads):
        for m, motif in enumerate(motifs):
            for s, sfx in enumerate(("_fwd", "_rev")):
                score, start, end, consumed, matches = (int(a[f + sfx][r, m]) for f in ("score", "start", "end", "consumed", "matches"))
                if score < min_score:
                    continue
                c = columns(score, start, end, consumed, matches, len(motif), penalty)
                row = (start, end, score, c["copies"], consumed, matches, c["mismatches"], c["insertions"], c["deletions"])
                lines.append("%d,%d,%s,%s,%s" % (r, len(read), motif, "+-"[s], ",".join(str(x) for x in row)))
                add = (1, end - start) + row[2:]
                sums[(m, s)] = [x + y for x, y in zip(sums[(m, s)], add)]
    lines += [">Summary", "motif,strand,reads,reads_reported,bases,score,copies,consumed,matches,mismatches,insertions,deletions"]
    for m, motif in enumerate(motifs):
        for s in range(2):
            lines.append("%s,%s,%d,%s" % (motif, "+-"[s], len(reads), ",".join(str(x) for x in sums[(m, s)])))
    return lines
