"""Reference of the refined de novo repeat per read (trew_hip_refined), written from the definition and
independent of the library and of oracle/: the record of `periods` (period_ref), a literal seed unit from the longest run of
eq_k, the wraparound alignment of the read against it (align_ref's recurrence), a forward-decoded vote per phase, and the
alignment against the re-voted unit.

Two forms that must agree: refine_read (plain Python tuples, align_ref.align_strand and a vote written cell by cell from the
definition; O(n k^2), short reads) and refine (the recurrence with the five doubling steps, vectorised with numpy over the
phases and over many reads, each with a unit length of its own)."""
import os

import numpy as np

import align_ref
import period_ref

U32_FIELDS = ("period", "seed_period", "scored_period", "changed", "score", "start", "end", "consumed", "matches", "seed_score", "support", "reserved")
FIELDS = U32_FIELDS + ("unit", "seed_unit")
DTYPE = np.dtype([(f, "<u4") for f in U32_FIELDS] + [("unit", "<u8"), ("seed_unit", "<u8")])
assert DTYPE.itemsize == 64
ZERO = (0,) * len(FIELDS)


def longest_run(eq, b, e):
    """the start of the longest run of true values among eq[b:e], the first of the longest; b without one"""
    best, rs, i = 0, b, b
    while i < e:
        if not eq[i]:
            i += 1
            continue
        j = i
        while j < e and eq[j]:
            j += 1
        if j - i > best:
            best, rs = j - i, i
        i = j
    return rs


def seed(c, R):
    """the codes of the seed unit S (primitive) of a read with the codes c and the non-zero periods record R (a tuple in the
    order of period_ref.FIELDS)"""
    k, start, end = int(R[1]), int(R[3]), int(R[4])
    b, e = start, end - k
    rs = longest_run(period_ref.eq_k(c, k), b, e)
    cons, _ = period_ref.consensus(c, start, end, k)
    s0 = [int(c[rs + j]) if c[rs + j] < 4 else cons[(rs + j - start) % k] for j in range(k)]
    return s0[:period_ref.primitive(s0)]


def vote_plain(x, t, P):
    """cnt[j][code] of the forward decode over the codes x (a read of its own) against the unit t"""
    k = len(t)
    H = [(0, 0, 0, 0)] * k
    cnt = [[0] * 4 for _ in range(k)]
    for i in range(1, len(x) + 1):
        c = x[i - 1]
        V, D = [], []
        for j in range(k):
            s, b, C, m = H[(j - 1) % k]
            diag = (s + 1, b, C + 1, m + 1) if c == t[j] else (s - P, b, C + 1, m)
            s, b, C, m = H[j]
            V.append(max((0, i, 0, 0), diag, (s - P, b, C, m)))
            D.append(diag)
        js = max(range(k), key=lambda j: (V[j], -j))
        if c < 4 and D[js] == V[js]:
            cnt[js][c] += 1
        H = [max((V[(j - d) % k][0] - P * d, V[(j - d) % k][1], V[(j - d) % k][2] + d, V[(j - d) % k][3]) for d in range(k)) for j in range(k)]
    return cnt


def revote(S, cnt):
    """(U0, support, changed)"""
    u0 = []
    for j, s in enumerate(S):
        top = max(cnt[j])
        u0.append(s if cnt[j][s] == top else min(x for x in range(4) if cnt[j][x] == top))
    return u0, sum(cnt[j][u0[j]] for j in range(len(S))), sum(1 for j in range(len(S)) if u0[j] != S[j])


def _finish(R, S, a1, cnt, align_fn):
    u0, support, changed = revote(S, cnt)
    U = u0[:period_ref.primitive(u0)]
    a2 = a1
    if U != S:
        a2 = align_fn(U)
        if a2[0] < a1[0]:
            U, a2, changed = S, a1, 0
    return (len(U), len(S), int(R[1]), changed) + tuple(int(v) for v in a2) + (int(a1[0]), support, 0, period_ref.pack_unit(U), period_ref.pack_unit(S))


def refine_read(read, min_period=1, max_period=32, penalty=3, min_score=24):
    """the record of one read as a tuple in the order of FIELDS, step by step from the definition"""
    R = period_ref.period_read(read, min_period, max_period, penalty, min_score)
    if R == period_ref.ZERO:
        return ZERO
    c = period_ref.codes(read)
    x = [int(v) for v in c]
    S = seed(c, R)
    a1 = align_ref.align_strand(x, S, penalty)
    cnt = vote_plain(x[a1[1]:a1[2]], S, penalty)
    return _finish(R, S, a1, cnt, lambda U: align_ref.align_strand(x, U, penalty))


def _better(a, b):
    return (a[0] > b[0]) | ((a[0] == b[0]) & (a[1] > b[1]))


def _pass_many(X, lens, T, ks, P, vote=False):
    """X: (R, n_max) codes, lens: (R,), T: (R, 32) unit codes (anything >= 8 past a read's unit length), ks: (R,) unit lengths
    -> ((R, 5) records, (R, 32, 4) vote counts).  Phase j of read r is live for j < ks[r]; the other phases hold fresh starts,
    are read by no live phase and take no part in the best cell or the vote."""
    R, n_max = X.shape
    rows = np.arange(R)[:, None]
    j = np.arange(32, dtype=np.int64)[None, :]
    kk = ks.astype(np.int64)[:, None]
    live_j = j < kk
    src = {s: np.where(live_j, (j - s) % kk, j) for s in (1, 2, 4, 8, 16)}
    A = np.zeros((R, 32), dtype=np.int64)
    B = np.zeros((R, 32), dtype=np.int64)
    b_score, b_end, b_A, b_B = (np.zeros((R, 32), dtype=np.int64) for _ in range(4))
    cnt = np.zeros((R, 32, 4), dtype=np.int64)
    one, pen = np.int64(1) << 32, np.int64(P) << 32
    for i in range(1, n_max + 1):
        live = (lens >= i)[:, None]
        c = X[:, i - 1][:, None]
        hit = c == T
        dA, dB = A[rows, src[1]], B[rows, src[1]]
        dA = np.where(hit, dA + one, dA - pen)
        dB = np.where(hit, dB + one + 1, dB + one)
        iA, iB = A - pen, B
        VA = np.full((R, 32), i, dtype=np.int64)
        VB = np.zeros((R, 32), dtype=np.int64)
        for cA, cB in ((dA, dB), (iA, iB)):
            take = (cA >= 0) & _better((cA, cB), (VA, VB))  # a negative score loses to the fresh start
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        if vote:
            mA = np.where(live_j, VA, -1)
            topA = mA.max(axis=1, keepdims=True)
            mB = np.where(mA == topA, VB, -1)
            js = np.argmax((mA == topA) & (mB == mB.max(axis=1, keepdims=True)), axis=1)  # the first of the largest
            r = np.arange(R)
            ok = live[:, 0] & (c[:, 0] < 4) & (dA[r, js] == VA[r, js]) & (dB[r, js] == VB[r, js])
            np.add.at(cnt, (r[ok], js[ok], c[ok, 0]), 1)
        for s in (1, 2, 4, 8, 16):
            cA = VA[rows, src[s]] - np.int64(P * s) * one
            cB = VB[rows, src[s]] + np.int64(s) * one
            take = (s < kk) & (cA >= 0) & _better((cA, cB), (VA, VB))
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        A, B = np.where(live, VA, A), np.where(live, VB, B)
        up = live & live_j & ((VA >> 32) > b_score)  # strictly: the earliest end stays
        b_score = np.where(up, VA >> 32, b_score)
        b_end = np.where(up, i, b_end)
        b_A, b_B = np.where(up, VA, b_A), np.where(up, VB, b_B)
    out = np.zeros((R, 5), dtype=np.int64)
    for r in range(R):
        key = max((int(b_score[r, q]), -int(b_end[r, q]), int(b_A[r, q]) & 0xFFFFFFFF, int(b_B[r, q]) >> 32, int(b_B[r, q]) & 0xFFFFFFFF)
                  for q in range(int(ks[r])))
        if key[0] > 0:
            out[r] = (key[0], key[2], -key[1], key[3], key[4])
    return out, cnt


def _plane(cs):
    lens = np.array([len(c) for c in cs], dtype=np.int64)
    X = np.full((len(cs), max(int(lens.max()), 1)), 4, dtype=np.int64)
    for r, c in enumerate(cs):
        X[r, :len(c)] = c
    return X, lens


def _units(us):
    T = np.full((len(us), 32), 9, dtype=np.int64)
    for r, u in enumerate(us):
        T[r, :len(u)] = u
    return T, np.array([len(u) for u in us], dtype=np.int64)


def align_units(reads, units, penalty=3):
    """(R, 5) forward records (score, start, end, consumed, matches) of reads[r] against units[r] (code lists of 1 .. 32)"""
    X, lens = _plane([[int(v) for v in period_ref.codes(r)] for r in reads])
    T, ks = _units(units)
    return _pass_many(X, lens, T, ks, penalty)[0]


def refine(reads, min_period=1, max_period=32, penalty=3, min_score=24):
    """DTYPE records of shape (n_reads,), the vectorised form"""
    out = np.zeros(len(reads), dtype=DTYPE)
    Rs = [period_ref.period_read(r, min_period, max_period, penalty, min_score) for r in reads]
    idx = [i for i, R in enumerate(Rs) if R != period_ref.ZERO]
    if not idx:
        return out
    cs = [period_ref.codes(reads[i]) for i in idx]
    xs = [[int(v) for v in c] for c in cs]
    Ss = [seed(c, Rs[i]) for c, i in zip(cs, idx)]
    X, lens = _plane(xs)
    T, ks = _units(Ss)
    a1, _ = _pass_many(X, lens, T, ks, penalty)
    X2, lens2 = _plane([x[int(a[1]):int(a[2])] for x, a in zip(xs, a1)])
    _, cnt = _pass_many(X2, lens2, T, ks, penalty, vote=True)
    u0s = [revote(S, cnt[r].tolist())[0] for r, S in enumerate(Ss)]
    Us = [u0[:period_ref.primitive(u0)] for u0 in u0s]
    T3, ks3 = _units(Us)
    a3, _ = _pass_many(X, lens, T3, ks3, penalty)
    for r, i in enumerate(idx):
        rec = _finish(Rs[i], Ss[r], tuple(int(v) for v in a1[r]), cnt[r].tolist(), lambda U, r=r: tuple(int(v) for v in a3[r]))
        out[i] = rec
    return out


def columns(rec, penalty):
    """the derived columns of a record (a DTYPE element or a tuple in the order of FIELDS): align_ref.columns with k = period"""
    rec = tuple(int(v) for v in rec)
    if rec[0] == 0:
        return dict(copies=0, mismatches=0, insertions=0, deletions=0)
    return align_ref.columns(rec[4], rec[5], rec[6], rec[7], rec[8], rec[0], penalty)


HEADER = "read,length,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,seed_score,changed,scored_period"


def cli_lines(path, reads, recs, penalty, min_score=24):
    """stdout of `trew refine` for one file: (the file's section, the >Summary section), formatted from records"""
    rows = [">" + os.path.realpath(path), HEADER]
    summary = {}
    for i, (read, x) in enumerate(zip(reads, recs)):
        d = int(x["period"])
        if d == 0 or int(x["score"]) < min_score:
            continue
        c = columns(x, penalty)
        canon = period_ref.canonical(x["unit"], d)
        sp = int(x["seed_period"])
        rows.append("%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%s,%d,%d,%d" % (
            i, len(read), d, period_ref.unit_text(x["unit"], d), period_ref.unit_text(canon, d), x["start"], x["end"], x["score"], c["copies"],
            x["consumed"], x["matches"], c["mismatches"], c["insertions"], c["deletions"], sp, period_ref.unit_text(x["seed_unit"], sp),
            x["seed_score"], x["changed"], x["scored_period"]))
        n, bases, copies = summary.get((d, canon), (0, 0, 0))
        summary[(d, canon)] = (n + 1, bases + int(x["end"]) - int(x["start"]), copies + c["copies"])
    tail = [">Summary", "period,canonical,reads,bases,copies"]
    for (d, canon), (n, bases, copies) in sorted(summary.items(), key=lambda kv: (-kv[1][0], kv[0])):
        tail.append("%d,%s,%d,%d,%d" % (d, period_ref.unit_text(canon, d), n, bases, copies))
    return rows, tail
