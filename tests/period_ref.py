"""Brute-force reference of the de novo repeat period and unit per read (trew_hip_period), written from the
definition and independent of the C++ and HIP implementations.

Two forms of the best-scoring segment of eq_k: `segment_prefix` (S, its running minimum, V = S - min: the definition as it
is stated) and `segment_direct` (the maximum over all (b, e) with the tie rules spelled out; quadratic, short reads only).
The consensus and the primitive root are written from the definition as well."""
import numpy as np

FIELDS = ("period", "scored_period", "score", "start", "end", "matches", "support", "reserved", "unit")
DTYPE = np.dtype([(f, "<u8" if f == "unit" else "<u4") for f in FIELDS])
CODE = {"T": 0, "G": 1, "C": 2, "A": 3}
LETTER = "TGCA"
ZERO = (0,) * len(FIELDS)


def codes(read):
    """per base: T 0, G 1, C 2, A 3 (either case), 4 for anything else"""
    if isinstance(read, bytes):
        read = read.decode()
    return np.array([CODE.get(c, 4) for c in read.upper()], dtype=np.int64)


def eq_k(c, k):
    """eq_k[i], 0 <= i < n - k: bases i and i + k are both valid and equal"""
    return (c[:-k] == c[k:]) & (c[:-k] < 4)


def segment_prefix(eq, P):
    """(score, b, e) from S(e), min over b <= e of S(b) and V(e); the smallest e, then the largest b"""
    S = np.concatenate([[0], np.cumsum(np.where(eq, 1, -P))])
    low = np.minimum.accumulate(S)
    V = S - low
    e = int(np.argmax(V))  # the first of the largest
    b = int(np.flatnonzero(S[: e + 1] == low[e])[-1])
    return int(V[e]), b, e


def segment_direct(eq, P):
    """(score, b, e): the largest sum over all segments [b, e), b <= e; the earliest end wins a tie, then the shortest segment"""
    sc = [1 if x else -P for x in eq]
    best = (0, 0, 0)
    for e in range(len(sc) + 1):
        for b in range(e, -1, -1):  # the shortest segment of this end first
            s = sum(sc[b:e])
            if s > best[0]:
                best = (s, b, e)
    return best


def consensus(c, start, end, k):
    """(u, support): per phase the code with the largest count among the valid bases, the smallest code on a tie (0 without
    a valid base); support = the sum of those counts"""
    cnt = [[0] * 4 for _ in range(k)]
    for p in range(start, end):
        if c[p] < 4:
            cnt[(p - start) % k][int(c[p])] += 1
    u = [max(range(4), key=lambda x: (cnt[j][x], -x)) for j in range(k)]
    return u, sum(cnt[j][u[j]] for j in range(k))


def primitive(u):
    """the smallest divisor d of len(u) with u[j] == u[(j + d) % len(u)] for all j"""
    k = len(u)
    for d in range(1, k + 1):
        if k % d == 0 and all(u[j] == u[(j + d) % k] for j in range(k)):
            return d


def pack_unit(u):
    w = 0
    for x in u:
        w = (w << 2) | x
    return w


def period_read(read, min_period=1, max_period=32, penalty=3, min_score=24, segment=segment_prefix):
    """the record of one read as a tuple in the order of FIELDS"""
    c = codes(read)
    n = len(c)
    best = None
    for k in range(min_period, min(max_period, n - 1) + 1):
        score, b, e = segment(eq_k(c, k), penalty)
        if best is None or score > best[0]:  # strictly: the smallest k keeps a tie
            best = (score, k, b, e)
    if best is None or best[0] < min_score:
        return ZERO
    score, k, b, e = best
    start, end = b, e + k
    matches = int(eq_k(c, k)[b:e].sum())
    assert matches * (1 + penalty) == score + penalty * (e - b)
    u, support = consensus(c, start, end, k)
    d = primitive(u)
    return (d, k, score, start, end, matches, support, 0, pack_unit(u[:d]))


def periods(reads, min_period=1, max_period=32, penalty=3, min_score=24):
    out = np.zeros(len(reads), dtype=DTYPE)
    for i, r in enumerate(reads):
        out[i] = period_read(r, min_period, max_period, penalty, min_score)
    return out


def unit_text(word, k):
    return "".join(LETTER[(int(word) >> (2 * (k - 1 - j))) & 3] for j in range(k))


def revcomp_word(word, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (word & 3))
        word >>= 2
    return r


def canonical(word, k):
    """the smaller of the smallest rotations of the unit and of its reverse complement: the form of the scan's rows"""
    word = int(word)
    mask = (1 << (2 * k)) - 1
    best = None
    for w in (word, revcomp_word(word, k)):
        for _ in range(k):
            best = w if best is None or w < best else best
            w = ((w << 2) | (w >> (2 * (k - 1)))) & mask
    return best


def revcomp(read):
    if isinstance(read, bytes):
        read = read.decode()
    return read.upper().translate(str.maketrans("ACGT", "TGCA"))[::-1]


def cli_lines(path, reads, recs):
    """stdout of `trew periods` for one file: (the file's section, the >Summary section), formatted from records"""
    rows = [">" + path, "read,length,period,unit,canonical,start,end,score,matches,support,scored_period"]
    summary = {}
    for i, (read, x) in enumerate(zip(reads, recs)):
        d = int(x["period"])
        if d == 0:
            continue
        canon = canonical(x["unit"], d)
        rows.append("%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d" % (i, len(read), d, unit_text(x["unit"], d), unit_text(canon, d), x["start"], x["end"],
                                                     x["score"], x["matches"], x["support"], x["scored_period"]))
        n, bases = summary.get((d, canon), (0, 0))
        summary[(d, canon)] = (n + 1, bases + int(x["end"]) - int(x["start"]))
    tail = [">Summary", "period,canonical,reads,bases"]
    for (d, canon), (n, bases) in sorted(summary.items(), key=lambda kv: (-kv[1][0], kv[0])):
        tail.append("%d,%s,%d,%d" % (d, unit_text(canon, d), n, bases))
    return rows, tail
