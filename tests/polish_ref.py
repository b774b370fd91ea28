"""Reference of the refined de novo repeat per read for periods up to 256 (trew_hip_polished), written from the
definition and independent of the library and of oracle/: the depth-0 record of `satellites` (period_ref.period_read, which
accepts any max_period), refine_ref's seed and re-vote, and the recurrence of monomer_ref for every unit length 1 .. 256.

Two forms that must agree: polish_read (plain Python tuples: align_ref.align_strand and refine_ref.vote_plain, O(n k^2), short
reads) and polish (monomer_ref._strand_many's linear-plus-wrap closure with the vote, vectorised with numpy over the phases
and over many reads, each with a unit length of its own)."""
import os

import numpy as np

import align_ref
import period_ref
import refine_ref
import satellite_ref

MAX_PERIOD = 256
U32_FIELDS = refine_ref.U32_FIELDS
FIELDS = U32_FIELDS + ("unit", "seed_unit")
DTYPE = np.dtype([(f, "<u4") for f in U32_FIELDS] + [("unit", "<u4", (16,)), ("seed_unit", "<u4", (16,))])
assert DTYPE.itemsize == 176
ZERO = (0,) * len(U32_FIELDS) + ((), ())  # a record as a tuple: the twelve words, then the codes of U and of S


def _finish(R, S, a1, cnt, align_fn):
    u0, support, changed = refine_ref.revote(S, cnt)
    U = u0[:period_ref.primitive(u0)]
    a2 = a1
    if U != S:
        a2 = align_fn(U)
        if a2[0] < a1[0]:
            U, a2, changed = S, a1, 0
    return (len(U), len(S), int(R[1]), changed) + tuple(int(v) for v in a2) + (int(a1[0]), support, 0, tuple(U), tuple(S))


def polish_read(read, min_period=1, max_period=MAX_PERIOD, penalty=3, min_score=24):
    """the record of one read as a tuple (ZERO's shape), step by step from the definition"""
    R = period_ref.period_read(read, min_period, max_period, penalty, min_score)
    if R == period_ref.ZERO:
        return ZERO
    c = period_ref.codes(read)
    x = [int(v) for v in c]
    S = refine_ref.seed(c, R)
    a1 = align_ref.align_strand(x, S, penalty)
    cnt = refine_ref.vote_plain(x[a1[1]:a1[2]], S, penalty)
    return _finish(R, S, a1, cnt, lambda U: align_ref.align_strand(x, U, penalty))


def vote_trace(x, t, P):
    """The forward decode over the codes x (a read of its own) against the unit t, row by row: [(the phases whose V is the
    largest, ascending -- the first one is j*; whether the row votes; the base)].  Plain tuples, the maximum over d in
    monomer_ref's linear-plus-wrap form, O(n k)."""
    k = len(t)
    H = [(0, 0, 0, 0)] * k
    out = []

    def shifted(cell, d):
        return (cell[0] - P * d, cell[1], cell[2] + d, cell[3])

    for i in range(1, len(x) + 1):
        c = x[i - 1]
        V, D = [], []
        for j in range(k):
            s, b, C, m = H[(j - 1) % k]
            diag = (s + 1, b, C + 1, m + 1) if c == t[j] else (s - P, b, C + 1, m)
            s, b, C, m = H[j]
            V.append(max((0, i, 0, 0), diag, (s - P, b, C, m)))
            D.append(diag)
        top = max(V)
        tied = [j for j in range(k) if V[j] == top]
        out.append((tied, c < 4 and D[tied[0]] == V[tied[0]], c))
        L = list(V)
        for j in range(1, k):
            L[j] = max(L[j], shifted(L[j - 1], 1))
        H = [max(L[j], shifted(L[k - 1], j + 1)) for j in range(k)]  # a candidate that does not score never wins: V holds the fresh start
    return out


def trace_counts(trace, k):
    """cnt[j][code] of a vote_trace"""
    cnt = [[0] * 4 for _ in range(k)]
    for tied, voted, c in trace:
        if voted:
            cnt[tied[0]][c] += 1
    return cnt


def seed_and_trace(read, min_period=1, max_period=MAX_PERIOD, penalty=3, min_score=24):
    """(R, rs, S, A1, vote_trace over A1's tract) of a read with a step-1 record"""
    R = period_ref.period_read(read, min_period, max_period, penalty, min_score)
    assert R != period_ref.ZERO
    c = period_ref.codes(read)
    x = [int(v) for v in c]
    k, start, end = int(R[1]), int(R[3]), int(R[4])
    rs = refine_ref.longest_run(period_ref.eq_k(c, k), start, end - k)
    S = refine_ref.seed(c, R)
    a1 = tuple(int(v) for v in align_units([read], [S], penalty)[0])
    return R, rs, S, a1, vote_trace(x[a1[1]:a1[2]], S, penalty)


def tie_matters(S, trace):
    """[(row, j*, another tied phase)] of the voting rows of a trace at which the record depends on the smallest phase winning the
    tie: with the vote given to the other phase the re-vote gives another unit, support or number of changed phases"""
    cnt = trace_counts(trace, len(S))
    want = refine_ref.revote(S, cnt)
    out = []
    for row, (tied, voted, c) in enumerate(trace):
        if not voted:
            continue
        for p in tied[1:]:
            cnt[tied[0]][c] -= 1
            cnt[p][c] += 1
            if refine_ref.revote(S, cnt) != want:
                out.append((row, tied[0], p))
            cnt[p][c] -= 1
            cnt[tied[0]][c] += 1
    return out


def _pass_many(X, lens, T, ks, P, vote=False):
    """X: (R, n_max) codes, lens: (R,), T: (R, K) unit codes (anything >= 8 past a read's unit length), ks: (R,) unit lengths
    -> ((R, 5) records, (R, K, 4) vote counts).  Phase j of read r is live for j < ks[r]; a live phase reads lower phases and
    phase ks[r] - 1 only, so the dead ones take no part in a cell, in the best cell or in the vote."""
    R, n_max = X.shape
    K = T.shape[1]
    r = np.arange(R)
    j = np.arange(K, dtype=np.int64)[None, :]
    live_j = j < ks.astype(np.int64)[:, None]
    last = ks.astype(np.int64) - 1
    A = np.zeros((R, K), dtype=np.int64)
    B = np.zeros((R, K), dtype=np.int64)
    b_score, b_end, b_A, b_B = (np.zeros((R, K), dtype=np.int64) for _ in range(4))
    cnt = np.zeros((R, K, 4), dtype=np.int64)
    one, pen = np.int64(1) << 32, np.int64(P) << 32
    wrap_d = j + 1  # phase j takes W shifted by j + 1
    better = align_ref._better
    for i in range(1, n_max + 1):
        live = (lens >= i)[:, None]
        c = X[:, i - 1][:, None]
        hit = c == T
        dA, dB = np.roll(A, 1, axis=1), np.roll(B, 1, axis=1)
        dA[:, 0], dB[:, 0] = A[r, last], B[r, last]
        dA = np.where(hit, dA + one, dA - pen)
        dB = np.where(hit, dB + one + 1, dB + one)
        VA = np.full((R, K), i, dtype=np.int64)
        VB = np.zeros((R, K), dtype=np.int64)
        for cA, cB in ((dA, dB), (A - pen, B)):
            take = (cA >= 0) & better((cA, cB), (VA, VB))  # a negative score loses to the fresh start
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        if vote:
            mA = np.where(live_j, VA, -1)
            topA = mA.max(axis=1, keepdims=True)
            mB = np.where(mA == topA, VB, -1)
            js = np.argmax((mA == topA) & (mB == mB.max(axis=1, keepdims=True)), axis=1)  # the first of the largest
            ok = live[:, 0] & (c[:, 0] < 4) & (dA[r, js] == VA[r, js]) & (dB[r, js] == VB[r, js])
            np.add.at(cnt, (r[ok], js[ok], c[ok, 0]), 1)
        s = 1
        while s < K:  # the prefix closure: no wrap, a phase below s has no source; a step at or above a read's k changes nothing
            cA = np.full((R, K), -1, dtype=np.int64)
            cB = np.zeros((R, K), dtype=np.int64)
            cA[:, s:] = VA[:, :-s] - np.int64(P * s) * one
            cB[:, s:] = VB[:, :-s] + np.int64(s) * one
            take = (cA >= 0) & better((cA, cB), (VA, VB))
            VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
            s *= 2
        cA = VA[r, last][:, None] - (np.int64(P) * wrap_d) * one
        cB = VB[r, last][:, None] + wrap_d * one
        take = (cA >= 0) & better((cA, cB), (VA, VB))
        VA, VB = np.where(take, cA, VA), np.where(take, cB, VB)
        A, B = np.where(live, VA, A), np.where(live, VB, B)
        up = live & live_j & ((VA >> 32) > b_score)  # strictly: the earliest end stays
        b_score = np.where(up, VA >> 32, b_score)
        b_end = np.where(up, i, b_end)
        b_A, b_B = np.where(up, VA, b_A), np.where(up, VB, b_B)
    out = np.zeros((R, 5), dtype=np.int64)
    for q in range(R):
        key = max((int(b_score[q, p]), -int(b_end[q, p]), int(b_A[q, p]) & 0xFFFFFFFF, int(b_B[q, p]) >> 32, int(b_B[q, p]) & 0xFFFFFFFF)
                  for p in range(int(ks[q])))
        if key[0] > 0:
            out[q] = (key[0], key[2], -key[1], key[3], key[4])
    return out, cnt


def _units(us):
    T = np.full((len(us), max(len(u) for u in us)), 9, dtype=np.int64)
    for r, u in enumerate(us):
        T[r, :len(u)] = u
    return T, np.array([len(u) for u in us], dtype=np.int64)


def align_units(reads, units, penalty=3):
    """(R, 5) forward records (score, start, end, consumed, matches) of reads[r] against units[r] (code lists of 1 .. 256)"""
    X, lens = refine_ref._plane([[int(v) for v in period_ref.codes(r)] for r in reads])
    T, ks = _units(units)
    return _pass_many(X, lens, T, ks, penalty)[0]


def polish_tuples(reads, min_period=1, max_period=MAX_PERIOD, penalty=3, min_score=24):
    """the records as tuples (ZERO's shape), the vectorised form"""
    out = [ZERO] * len(reads)
    Rs = [period_ref.period_read(r, min_period, max_period, penalty, min_score) for r in reads]
    idx = [i for i, R in enumerate(Rs) if R != period_ref.ZERO]
    if not idx:
        return out
    cs = [period_ref.codes(reads[i]) for i in idx]
    xs = [[int(v) for v in c] for c in cs]
    Ss = [refine_ref.seed(c, Rs[i]) for c, i in zip(cs, idx)]
    X, lens = refine_ref._plane(xs)
    T, ks = _units(Ss)
    a1, _ = _pass_many(X, lens, T, ks, penalty)
    X2, lens2 = refine_ref._plane([x[int(a[1]):int(a[2])] for x, a in zip(xs, a1)])
    _, cnt = _pass_many(X2, lens2, T, ks, penalty, vote=True)
    u0s = [refine_ref.revote(S, cnt[r].tolist())[0] for r, S in enumerate(Ss)]
    Us = [u0[:period_ref.primitive(u0)] for u0 in u0s]
    a3 = a1
    if any(U != S for U, S in zip(Us, Ss)):
        T3, ks3 = _units(Us)
        a3, _ = _pass_many(X, lens, T3, ks3, penalty)
    for r, i in enumerate(idx):
        out[i] = _finish(Rs[i], Ss[r], tuple(int(v) for v in a1[r]), cnt[r].tolist(), lambda U, r=r: tuple(int(v) for v in a3[r]))
    return out


def records(tuples):
    """DTYPE records of tuples in ZERO's shape"""
    out = np.zeros(len(tuples), dtype=DTYPE)
    for o, t in zip(out, tuples):
        for f, v in zip(U32_FIELDS, t[:12]):
            o[f] = v
        o["unit"] = satellite_ref.unit_words(t[12])
        o["seed_unit"] = satellite_ref.unit_words(t[13])
    return out


def polish(reads, min_period=1, max_period=MAX_PERIOD, penalty=3, min_score=24):
    """DTYPE records of shape (n_reads,), the vectorised form"""
    return records(polish_tuples(reads, min_period, max_period, penalty, min_score))


def as_tuple(x):
    """a DTYPE record (the library's or this file's) in ZERO's shape"""
    return tuple(int(x[f]) for f in U32_FIELDS) + (tuple(satellite_ref.unit_codes(x["unit"], x["period"])),
                                                   tuple(satellite_ref.unit_codes(x["seed_unit"], x["seed_period"])))


def columns(rec, penalty):
    """the derived columns of a record (a DTYPE element or a tuple in ZERO's shape): align_ref.columns with k = period"""
    rec = tuple(int(rec[i]) for i in range(12)) if isinstance(rec, tuple) else tuple(int(rec[f]) for f in U32_FIELDS)
    if rec[0] == 0:
        return dict(copies=0, mismatches=0, insertions=0, deletions=0)
    return align_ref.columns(rec[4], rec[5], rec[6], rec[7], rec[8], rec[0], penalty)


def text(codes):
    return "".join(period_ref.LETTER[c] for c in codes)


HEADER = refine_ref.HEADER


def cli_lines(path, reads, recs, penalty, min_score=24):
    """stdout of `trew polish` for one file: (the file's section, the >Summary section), formatted from records"""
    rows = [">" + os.path.realpath(path), HEADER]
    summary = {}
    for i, (read, x) in enumerate(zip(reads, recs)):
        d = int(x["period"])
        if d == 0 or int(x["score"]) < min_score:
            continue
        c = columns(x, penalty)
        t = as_tuple(x)
        canon = satellite_ref.canonical_codes(t[12])
        rows.append("%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%s,%d,%d,%d" % (
            i, len(read), d, text(t[12]), text(canon), x["start"], x["end"], x["score"], c["copies"], x["consumed"], x["matches"], c["mismatches"],
            c["insertions"], c["deletions"], x["seed_period"], text(t[13]), x["seed_score"], x["changed"], x["scored_period"]))
        n, bases, copies = summary.get((d, canon), (0, 0, 0))
        summary[(d, canon)] = (n + 1, bases + int(x["end"]) - int(x["start"]), copies + c["copies"])
    tail = [">Summary", "period,canonical,reads,bases,copies"]
    for (d, canon), (n, bases, copies) in sorted(summary.items(), key=lambda kv: (-kv[1][0], kv[0])):
        tail.append("%d,%s,%d,%d,%d" % (d, text(canon), n, bases, copies))
    return rows, tail
