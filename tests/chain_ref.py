"""Brute-force reference of the ordered unit chain, written from the definition alone.

Base codes T = 0, G = 1, C = 2, A = 3; the complement of code c is 3 - c.  A read has n bases, a motif M has k bases and is
taken as typed.  Targets: T_fwd = M, T_rev = revcomp(M).  Window i (0 <= i <= n - k) is valid when all of its k bytes are
one of ACGT in either case.  Per strand s: exact_s[i] = window i is valid and equals T_s; var_s[i] = it is valid and differs
from T_s in exactly one position j, where the read has base c; its bin is 4 j + c on the forward strand and
4 (k-1-j) + (3-c) on the reverse strand.  A variant window is anchored when (i >= k and exact_s[i-k]) or (i + k <= n - k and
exact_s[i+k]).  Items of a (read, motif, strand): a run {start i, count r, NONE} for every maximal sequence of exact windows
i, i + k, ..., i + (r-1) k, and {start i, 1, bin} for every anchored variant window; sorted by start.

Two independent shapes of the same definition (they share only the window classification), independent of the library and of
oracle/:
  chain_read_marks   marks every run start (exact, window i - k not exact) and every run end (exact, window i + k not exact)
                     and pairs them inside their residue class
  chain_read_walk    walks every residue class c, c + k, c + 2 k, ... once and keeps the open run
"""
import numpy as np

CODE = {"T": 0, "G": 1, "C": 2, "A": 3, "t": 0, "g": 1, "c": 2, "a": 3}
BASES = "TGCA"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
NONE = 0xFFFFFFFF
FIELDS = ("read", "motif", "strand", "start", "count", "bin")
CHAIN_DTYPE = np.dtype([(f, "<u4") for f in FIELDS])


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s.upper()))


def bin_text(motif, b):
    """the variant unit of a bin in motif orientation: the motif with base b // 4 replaced"""
    m = list(motif.upper())
    m[b // 4] = BASES[b & 3]
    return "".join(m)


_LUT = np.full(256, 4, dtype=np.uint8)
for _c, _v in CODE.items():
    _LUT[ord(_c)] = _v


def classify(read, target, strand):
    """per window: 'E' exact, a bin (int) for a window with exactly one mismatch, None otherwise (one mismatch matrix of
    windows x k)"""
    k, n = len(target), len(read)
    if n < k:
        return []
    codes = _LUT[np.frombuffer(read.encode("latin-1"), dtype=np.uint8)]
    win = np.lib.stride_tricks.sliding_window_view(codes, k)
    valid = (win != 4).all(axis=1)
    diff = win != np.array([CODE[c] for c in target], dtype=np.uint8)[None, :]
    nd = diff.sum(axis=1)
    out = [None] * (n - k + 1)
    for i in np.flatnonzero(valid & (nd == 0)).tolist():
        out[i] = "E"
    for i in np.flatnonzero(valid & (nd == 1)).tolist():
        j = int(diff[i].argmax())
        c = int(win[i, j])
        out[i] = 4 * j + c if strand == 0 else 4 * (k - 1 - j) + (3 - c)
    return out


def _text(read):
    return read.decode("latin-1") if isinstance(read, (bytes, bytearray)) else read


def chain_read_marks(read, motif):
    """One read, one motif: [items of fwd, items of rev], an item = (start, count, bin), sorted by start."""
    read, motif = _text(read), motif.upper()
    k = len(motif)
    out = []
    for s, target in enumerate((motif, revcomp(motif))):
        w = classify(read, target, s)
        nwin = len(w)
        ex = lambda i: 0 <= i < nwin and w[i] == "E"  # noqa: E731
        starts = [i for i in range(nwin) if ex(i) and not ex(i - k)]
        ends = [i for i in range(nwin) if ex(i) and not ex(i + k)]
        items = []
        for c in range(k):
            ss = [i for i in starts if i % k == c]
            ee = [i for i in ends if i % k == c]
            assert len(ss) == len(ee)
            for a, b in zip(ss, ee):
                assert a <= b and (b - a) % k == 0
                items.append((a, (b - a) // k + 1, NONE))
        items += [(i, 1, w[i]) for i in range(nwin) if isinstance(w[i], int) and (ex(i - k) or ex(i + k))]
        out.append(sorted(items))
    return out


def chain_read_walk(read, motif):
    """The same by walking each residue class."""
    read, motif = _text(read), motif.upper()
    k = len(motif)
    out = []
    for s, target in enumerate((motif, revcomp(motif))):
        w = classify(read, target, s)
        items = []
        for c in range(k):
            cls = w[c::k]  # windows c, c + k, ...
            open_at = None
            for q, x in enumerate(cls):
                if x == "E":
                    if open_at is None:
                        open_at = q
                    continue
                if open_at is not None:
                    items.append((c + open_at * k, q - open_at, NONE))
                    open_at = None
                if isinstance(x, int):
                    before = q > 0 and cls[q - 1] == "E"
                    after = q + 1 < len(cls) and cls[q + 1] == "E"
                    if before or after:
                        items.append((c + q * k, 1, x))
            if open_at is not None:
                items.append((c + open_at * k, len(cls) - open_at, NONE))
        out.append(sorted(items))
    return out


def chain(reads, motifs, form=chain_read_marks):
    """(CHAIN_DTYPE items sorted by (read, motif, strand, start), counts of shape (len(reads), len(motifs), 2, 2) =
    [read][motif][strand]{runs, variants})"""
    rows = []
    counts = np.zeros((len(reads), len(motifs), 2, 2), dtype=np.uint32)
    for r, read in enumerate(reads):
        for m, motif in enumerate(motifs):
            for s, items in enumerate(form(read, motif)):
                for start, count, b in items:
                    rows.append((r, m, s, start, count, b))
                    counts[r, m, s, 0 if b == NONE else 1] += 1
    return np.array(rows, dtype=CHAIN_DTYPE) if rows else np.zeros(0, dtype=CHAIN_DTYPE), counts


def signature(items, motif):
    """`trew chain`'s signature of the items (start, count, bin) of one key, in start order"""
    k = len(motif)
    tokens, at = [], None
    for start, count, b in items:
        if at is not None and start != at:
            tokens.append(("+%d" if start > at else "-%d") % abs(start - at))
        tokens.append("=%d" % count if b == NONE else bin_text(motif, b))
        at = start + count * k
    return " ".join(tokens)
