"""Brute-force reference of the per-read motif annotation, written from the definition alone.

For a read of n bases and a motif M of k bases: window i (0 <= i <= n - k) is valid when all of its k bytes are one of
ACGT in either case (the bytes the packed format gives a code; every other byte sets its nmask bit); canon(x) is the
smallest rotation of x as a 2k-bit word, first base most significant, T=0 G=1 C=2 A=3.  match_s[i] = window i is valid and
canon(window i) == target_s with target_fwd = canon(M), target_rev = canon(revcomp(M)).  windows_s counts the matches; the longest run of consecutive
matching windows (the earliest on a tie) gives tract_start_s = its first window and tract_len_s = windows + k - 1 bases.

Independent of the library and of oracle/: plain Python for single reads (annotate_read), numpy over all windows of many
reads at once (annotate) -- every window still gets its validity, its smallest rotation and one comparison.
"""
import os

import numpy as np

CODE = {"T": 0, "G": 1, "C": 2, "A": 3, "t": 0, "g": 1, "c": 2, "a": 3}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
FIELDS = ("windows_fwd", "windows_rev", "tract_start_fwd", "tract_len_fwd", "tract_start_rev", "tract_len_rev")
ANNOT_DTYPE = np.dtype([(f, "<u4") for f in FIELDS])


def word_of(s):
    w = 0
    for ch in s:
        w = (w << 2) | CODE[ch]
    return w


def canon_word(w, k):
    mask = (1 << (2 * k)) - 1
    best = w
    for _ in range(k - 1):
        w = ((w << 2) | (w >> (2 * (k - 1)))) & mask
        best = min(best, w)
    return best


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def targets(motif):
    motif = motif.upper()
    k = len(motif)
    return canon_word(word_of(motif), k), canon_word(word_of(revcomp(motif)), k)


def _longest(match, k):
    best_len = best_start = run = 0
    for i, m in enumerate(match):
        run = run + 1 if m else 0
        if run > best_len:
            best_len, best_start = run, i - run + 1
    return (best_start, best_len + k - 1) if best_len else (0, 0)


def annotate_read(read, motif):
    """One read (bytes or str), one motif, window by window in plain Python: the six numbers in FIELDS order."""
    if isinstance(read, bytes):
        read = read.decode("latin-1")
    k = len(motif)
    tf, tr = targets(motif)
    mf, mr = [], []
    for i in range(len(read) - k + 1):
        win = read[i:i + k]
        valid = all(c in CODE for c in win)
        c = canon_word(word_of(win), k) if valid else None
        mf.append(valid and c == tf)
        mr.append(valid and c == tr)
    sf, lf = _longest(mf, k)
    sr, lr = _longest(mr, k)
    return (sum(mf), sum(mr), sf, lf, sr, lr)


_LUT = np.full(256, 255, dtype=np.uint8)
for _c, _v in CODE.items():
    _LUT[ord(_c)] = _v


def annotate(reads, motifs):
    """Structured array of shape (len(reads), len(motifs)).  All reads are laid end to end with one invalid byte between
    them, so no window that crosses from one read into the next is valid; every window of that text is then canonicalised
    (minimum over its k rotations) and compared."""
    reads = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
    n_reads = len(reads)
    out = np.zeros((n_reads, len(motifs)), dtype=ANNOT_DTYPE)
    if n_reads == 0:
        return out
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    starts = np.zeros(n_reads, dtype=np.int64)
    starts[1:] = np.cumsum(lens[:-1] + 1)
    text = np.frombuffer(b"N".join(reads) + b"N", dtype=np.uint8)
    codes = _LUT[text]
    bad = codes == 255
    c64 = np.where(bad, 0, codes).astype(np.uint64)
    total = len(text)
    canon_by_k = {}
    for mi, motif in enumerate(motifs):
        k = len(motif)
        if total < k:
            continue
        if k not in canon_by_k:
            nwin = total - k + 1
            word = np.zeros(nwin, dtype=np.uint64)
            nbad = np.zeros(nwin, dtype=np.int64)
            for j in range(k):
                word = (word << np.uint64(2)) | c64[j:j + nwin]
                nbad += bad[j:j + nwin]
            mask = np.uint64((1 << (2 * k)) - 1)
            best = word.copy()
            rot = word
            for _ in range(k - 1):
                rot = ((rot << np.uint64(2)) | (rot >> np.uint64(2 * (k - 1)))) & mask
                best = np.minimum(best, rot)
            canon_by_k[k] = (best, nbad == 0)
        canon, valid = canon_by_k[k]
        nwin = len(canon)
        win_read = np.searchsorted(starts, np.arange(nwin), side="right") - 1  # the read a window starts in
        for strand, target in enumerate(targets(motif)):
            match = valid & (canon == np.uint64(target))
            sfx = "fwd" if strand == 0 else "rev"
            out["windows_" + sfx][:, mi] = np.bincount(win_read[match], minlength=n_reads)
            # maximal runs of consecutive matching windows
            d = np.diff(np.concatenate(([0], match.astype(np.int8), [0])))
            rs = np.flatnonzero(d == 1)
            re_ = np.flatnonzero(d == -1)
            if len(rs) == 0:
                continue
            rlen = re_ - rs
            rread = win_read[rs]
            order = np.lexsort((rs, -rlen, rread))  # by read, longest first, earliest first
            first = np.concatenate(([True], rread[order][1:] != rread[order][:-1]))
            pick = order[first]
            out["tract_start_" + sfx][rread[pick], mi] = rs[pick] - starts[rread[pick]]
            out["tract_len_" + sfx][rread[pick], mi] = rlen[pick] + k - 1
    return out


def cli_lines(path, reads, motifs, a, min_tract=None):
    """stdout of `trew annotate` for one file, formatted from the records a of shape (reads, motifs)"""
    lines = [">" + os.path.realpath(path),
             "read,length,motif,windows_fwd,windows_rev,tract_start_fwd,tract_len_fwd,tract_start_rev,tract_len_rev"]
    reported = [0] * len(motifs)
    for r, read in enumerate(reads):
        for m, motif in enumerate(motifs):
            x = a[r, m]
            if max(int(x["tract_len_fwd"]), int(x["tract_len_rev"])) >= (min_tract if min_tract is not None else 4 * len(motif)):
                reported[m] += 1
                lines.append("%d,%d,%s,%s" % (r, len(read), motif, ",".join(str(int(x[f])) for f in FIELDS)))
    lines += [">Summary", "motif,reads,reads_reported,bases,windows_fwd,windows_rev,longest_tract"]
    bases = sum(len(r) for r in reads)
    for m, motif in enumerate(motifs):
        longest = max([0] + [max(int(x["tract_len_fwd"]), int(x["tract_len_rev"])) for x in a[:, m]])
        lines.append("%s,%d,%d,%d,%d,%d,%d" % (motif, len(reads), reported[m], bases, int(a["windows_fwd"][:, m].astype(np.uint64).sum()),
                                                int(a["windows_rev"][:, m].astype(np.uint64).sum()), longest))
    return lines
