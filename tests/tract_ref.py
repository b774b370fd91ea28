"""Brute-force reference of the error-tolerant terminal motif tracts, written from the definition alone.

For a read of n bases, a motif M of k bases, a strand s and an integer penalty P (1 <= P <= 64): match_s[i] is annot_ref's
(window i is valid and its smallest rotation equals that of the strand's target); cov_s[p] = 1 when some matching window
contains base p (match_s[i] for an i with i <= p <= i + k - 1); score(p) = +1 if cov_s[p] else -P; S(e) = sum of score(p)
over p < e, S(0) = 0.  head_len = the smallest e in [0, n] at which S is largest, head_cov = covered bases in front of it;
tail_len = n - b with b the largest position at which S is smallest, tail_cov = covered bases from b on; covered = all of
them.  On ties the shorter tract wins at both ends; n < k gives zeros.

Independent of the library and of oracle/: plain Python for single reads (tracts_read: window by window, base by base),
numpy for many reads at once (tracts: every window canonicalised, coverage as a difference array, S as a cumulative sum).
"""
import os

import numpy as np

import annot_ref as A

NAMES = ("covered", "head_len", "head_cov", "tail_len", "tail_cov")
FIELDS = tuple(n + "_fwd" for n in NAMES) + tuple(n + "_rev" for n in NAMES)
TRACT_DTYPE = np.dtype([(f, "<u4") for f in FIELDS])


def _ends(cov, penalty):
    n = len(cov)
    S = [0]
    for p in range(n):
        S.append(S[-1] + (1 if cov[p] else -penalty))
    head = min(e for e in range(n + 1) if S[e] == max(S))
    b = max(e for e in range(n + 1) if S[e] == min(S))
    return (sum(cov), head, sum(cov[:head]), n - b, sum(cov[b:]))


def tracts_read(read, motif, penalty):
    """One read (bytes or str), one motif: the ten numbers in FIELDS order."""
    if isinstance(read, bytes):
        read = read.decode("latin-1")
    k = len(motif)
    n = len(read)
    out = ()
    for target in A.targets(motif):
        cov = [0] * n
        for i in range(n - k + 1):
            win = read[i:i + k]
            if all(c in A.CODE for c in win) and A.canon_word(A.word_of(win), k) == target:
                for p in range(i, i + k):
                    cov[p] = 1
        out += _ends(cov, penalty)
    return out


def tracts(reads, motifs, penalty):
    """Structured array of shape (len(reads), len(motifs)).  The reads are laid end to end with one invalid byte between
    them (annot_ref.annotate's layout), so no window crosses from one read into the next."""
    reads = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
    n_reads = len(reads)
    out = np.zeros((n_reads, len(motifs)), dtype=TRACT_DTYPE)
    if n_reads == 0:
        return out
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    starts = np.zeros(n_reads, dtype=np.int64)
    starts[1:] = np.cumsum(lens[:-1] + 1)
    text = np.frombuffer(b"N".join(reads) + b"N", dtype=np.uint8)
    codes = A._LUT[text]
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
        for strand, target in enumerate(A.targets(motif)):
            sfx = "_fwd" if strand == 0 else "_rev"
            match = np.flatnonzero(valid & (canon == np.uint64(target)))
            # cov[p] = number of matching windows over p > 0 (difference array); the separators stay uncovered
            d = np.zeros(total + 1, dtype=np.int64)
            np.add.at(d, match, 1)
            np.add.at(d, match + k, -1)
            cov = (np.cumsum(d[:total]) > 0).astype(np.int64)
            csum = np.concatenate(([0], np.cumsum(cov)))  # covered bases in front of text position
            for r in range(n_reads):
                a, n = int(starts[r]), int(lens[r])
                c = csum[a:a + n + 1] - csum[a]  # covered among the first e bases, e = 0 .. n
                S = c - penalty * (np.arange(n + 1) - c)
                head = int(np.argmax(S))  # the first largest
                b = n - int(np.argmin(S[::-1]))  # the last smallest
                out["covered" + sfx][r, mi] = c[n]
                out["head_len" + sfx][r, mi] = head
                out["head_cov" + sfx][r, mi] = c[head]
                out["tail_len" + sfx][r, mi] = n - b
                out["tail_cov" + sfx][r, mi] = c[n] - c[b]
    return out


def cli_lines(path, reads, motifs, t, min_tract=None):
    """stdout of `trew tracts`, formatted from the reference records t"""
    lines = [">" + os.path.realpath(path), "read,length,motif," + ",".join(FIELDS)]
    reported = [0] * len(motifs)
    lens = ("head_len_fwd", "head_len_rev", "tail_len_fwd", "tail_len_rev")
    for r, read in enumerate(reads):
        for m, motif in enumerate(motifs):
            x = t[r, m]
            if max(int(x[f]) for f in lens) >= (min_tract if min_tract is not None else 4 * len(motif)):
                reported[m] += 1
                lines.append("%d,%d,%s,%s" % (r, len(read), motif, ",".join(str(int(x[f])) for f in FIELDS)))
    lines += [">Summary", "motif,reads,reads_reported,bases,covered_fwd,covered_rev,longest_head,longest_tail"]
    bases = sum(len(r) for r in reads)
    for m, motif in enumerate(motifs):
        lines.append("%s,%d,%d,%d,%d,%d,%d,%d" % (
            motif, len(reads), reported[m], bases, int(t["covered_fwd"][:, m].astype(np.uint64).sum()),
            int(t["covered_rev"][:, m].astype(np.uint64).sum()),
            max(int(t["head_len_fwd"][:, m].max()), int(t["head_len_rev"][:, m].max())),
            max(int(t["tail_len_fwd"][:, m].max()), int(t["tail_len_rev"][:, m].max()))))
    return lines
