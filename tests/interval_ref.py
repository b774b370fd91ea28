"""Brute-force reference of the gap-tolerant motif intervals, written from the definition alone.

For a read of n bases, a motif M of k bases, a strand s and a rule (max_gap, min_len): match_s[i] is annot_ref's (window i
is valid and its smallest rotation equals that of the strand's target); cov_s[p] = 1 when some matching window contains
base p, as in tract_ref.  With the covered positions p_1 < p_2 < ..., an interval is a maximal group of consecutive covered
positions in which every two neighbours satisfy p_(j+1) - p_j - 1 <= max_gap; its record is (start = first covered position,
end = last covered position + 1, covered = covered bases in [start, end)); it is kept when end - start >= min_len.

Independent of the library and of oracle/: plain Python for single reads (intervals_read: window by window, base by base),
numpy for many reads at once (intervals: every window canonicalised, coverage as a difference array, the groups from the
differences of the covered positions).  Records are (read, motif, strand, start, end, covered), sorted in that order.
"""
import os

import numpy as np

import annot_ref as A

FIELDS = ("read", "motif", "strand", "start", "end", "covered")
INTERVAL_DTYPE = np.dtype([(f, "<u4") for f in FIELDS])


def coverage_read(read, motif):
    """cov_fwd, cov_rev of one read (bytes or str): lists of 0 / 1."""
    if isinstance(read, bytes):
        read = read.decode("latin-1")
    k, n = len(motif), len(read)
    out = []
    for target in A.targets(motif):
        cov = [0] * n
        for i in range(n - k + 1):
            win = read[i:i + k]
            if all(c in A.CODE for c in win) and A.canon_word(A.word_of(win), k) == target:
                for p in range(i, i + k):
                    cov[p] = 1
        out.append(cov)
    return out


def _group(cov, max_gap, min_len):
    out, cur = [], None  # cur = [start, last covered, covered]
    for p, c in enumerate(cov):
        if not c:
            continue
        if cur is not None and p - cur[1] - 1 > max_gap:
            out.append(cur)
            cur = None
        if cur is None:
            cur = [p, p, 0]
        cur[1] = p
        cur[2] += 1
    if cur is not None:
        out.append(cur)
    return [(s, e + 1, c) for s, e, c in out if e + 1 - s >= min_len]


def intervals_read(read, motif, max_gap, min_len):
    """One read, one motif: ([(start, end, covered), ...] of the forward strand, the same of the reverse strand)."""
    return tuple(_group(cov, max_gap, min_len) for cov in coverage_read(read, motif))


def intervals(reads, motifs, max_gap, min_len):
    """max_gap, min_len: an int or one value per motif.  Returns (records, counts): a structured array sorted by (read,
    motif, strand, start) and the number of kept intervals of every key, shape (len(reads), len(motifs), 2).  The reads are
    laid end to end with one invalid byte between them (annot_ref.annotate's layout), so no window crosses from one read
    into the next; a group of covered positions is cut at every read boundary whatever max_gap is."""
    reads = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
    n_reads, nm = len(reads), len(motifs)
    gaps = [int(max_gap)] * nm if isinstance(max_gap, (int, np.integer)) else [int(g) for g in max_gap]
    mins = [int(min_len)] * nm if isinstance(min_len, (int, np.integer)) else [int(g) for g in min_len]
    assert len(gaps) == nm and len(mins) == nm
    counts = np.zeros((n_reads, nm, 2), dtype=np.uint32)
    recs = []
    if n_reads:
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
                match = np.flatnonzero(valid & (canon == np.uint64(target)))
                d = np.zeros(total + 1, dtype=np.int64)
                np.add.at(d, match, 1)
                np.add.at(d, match + k, -1)
                pos = np.flatnonzero(np.cumsum(d[:total]) > 0)  # the covered positions of the whole text
                if len(pos) == 0:
                    continue
                rd = np.searchsorted(starts, pos, side="right") - 1  # the read of every covered position
                new = np.ones(len(pos), dtype=bool)  # does a group begin here?
                new[1:] = (rd[1:] != rd[:-1]) | (pos[1:] - pos[:-1] - 1 > gaps[mi])
                first = np.flatnonzero(new)
                last = np.concatenate((first[1:], [len(pos)])) - 1
                keep = pos[last] + 1 - pos[first] >= mins[mi]
                first, last = first[keep], last[keep]
                r = rd[first]
                np.add.at(counts[:, mi, strand], r, 1)
                g = np.zeros(len(first), dtype=INTERVAL_DTYPE)
                g["read"], g["motif"], g["strand"] = r, mi, strand
                g["start"], g["end"], g["covered"] = pos[first] - starts[r], pos[last] + 1 - starts[r], last - first + 1
                recs.append(g)
    out = np.concatenate(recs) if recs else np.zeros(0, dtype=INTERVAL_DTYPE)
    return out[np.lexsort((out["start"], out["strand"], out["motif"], out["read"]))], counts


def cli_lines(path, reads, motifs, want):
    """stdout of `trew intervals`, rendered from the reference (records, counts)"""
    recs, counts = want
    lines = [">" + os.path.realpath(path), "read,length,motif,strand,start,end,covered"]
    for x in recs:
        lines.append("%d,%d,%s,%s,%d,%d,%d" % (x["read"], len(reads[x["read"]]), motifs[x["motif"]], "+-"[x["strand"]], x["start"], x["end"], x["covered"]))
    lines += [">Summary", "motif,reads,reads_with_interval,bases,intervals_fwd,intervals_rev,longest_fwd,longest_rev,terminal_fwd,terminal_rev"]
    bases = sum(len(r) for r in reads)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    for m, motif in enumerate(motifs):
        row = [motif, len(reads), int((counts[:, m].sum(axis=1) > 0).sum()), bases]
        per = [recs[(recs["motif"] == m) & (recs["strand"] == s)] for s in (0, 1)]
        row += [len(p) for p in per]
        row += [int((p["end"].astype(np.int64) - p["start"]).max()) if len(p) else 0 for p in per]
        row += [int(((p["start"] == 0) | (p["end"] == lens[p["read"]])).sum()) for p in per]
        lines.append(",".join(str(v) for v in row))
    return lines
