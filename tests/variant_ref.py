"""Brute-force reference of the telomere variant repeats, written from the definition alone.

Base codes T = 0, G = 1, C = 2, A = 3; the complement of code c is 3 - c.  A read has n bases, a motif M has k bases and is
taken as typed.  Targets: T_fwd = M, T_rev = revcomp(M).  Window i (0 <= i <= n - k) is valid when all of its k bytes are
one of ACGT in either case.  Per strand s: exact_s[i] = window i is valid and equals T_s; var_s[i] = it is valid and differs
from T_s in exactly one position j, where the read has base c.  A variant window is anchored when (i >= k and exact_s[i-k])
or (i + k <= n - k and exact_s[i+k]).  Its bin is 4 j + c on the forward strand and 4 (k-1-j) + (3-c) on the reverse strand.
Record per (read, motif), fwd then rev: units (exact windows), variants (anchored variant windows), distinct (non-zero
bins), top (largest bin count, smallest bin on a tie, NONE without variants), top_count.  Per batch: hist[m][s][bin] = sum of
the reads' bin counts, reads_with[m][s][bin] = reads whose bin count is non-zero.

Independent of the library and of oracle/: plain Python for single reads (variants_read: window by window, base by base),
numpy for many reads at once (variants: one mismatch matrix of windows x k per read and strand).
"""
import os

import numpy as np

CODE = {"T": 0, "G": 1, "C": 2, "A": 3, "t": 0, "g": 1, "c": 2, "a": 3}
BASES = "TGCA"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
NONE = 0xFFFFFFFF
BINS = 128
FIELDS = tuple(name + s for s in ("_fwd", "_rev") for name in ("units", "variants", "distinct", "top", "top_count"))
VARIANT_DTYPE = np.dtype([(f, "<u4") for f in FIELDS])


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s.upper()))


def bin_of(pos, base):
    """bin of `base` (a letter) at 0-based position `pos` of the motif"""
    return 4 * pos + CODE[base]


def bin_text(motif, b):
    """the variant unit of a bin in motif orientation: the motif with base b // 4 replaced; '-' for NONE"""
    if b == NONE:
        return "-"
    m = list(motif.upper())
    m[b // 4] = BASES[b & 3]
    return "".join(m)


def _summary(bins):
    nz = [(c, b) for b, c in enumerate(bins) if c]
    if not nz:
        return 0, NONE, 0
    top_count = max(c for c, _ in nz)
    return len(nz), min(b for c, b in nz if c == top_count), top_count


def variants_read(read, motif):
    """One read (bytes or str), one motif: (the ten numbers in FIELDS order, [bins of fwd, bins of rev])."""
    if isinstance(read, bytes):
        read = read.decode("latin-1")
    motif = motif.upper()
    k, n = len(motif), len(read)
    rec, hists = [], []
    for s, target in enumerate((motif, revcomp(motif))):
        tcode = [CODE[c] for c in target]
        exact, var = [], []
        for i in range(n - k + 1):
            win = read[i:i + k]
            if not all(c in CODE for c in win):
                exact.append(False)
                var.append(None)
                continue
            diff = [(j, CODE[c]) for j, c in enumerate(win) if CODE[c] != tcode[j]]
            exact.append(len(diff) == 0)
            var.append(diff[0] if len(diff) == 1 else None)
        bins = [0] * BINS
        nvar = 0
        for i, v in enumerate(var):
            if v is None:
                continue
            if (i >= k and exact[i - k]) or (i + k <= n - k and exact[i + k]):
                j, c = v
                bins[4 * j + c if s == 0 else 4 * (k - 1 - j) + (3 - c)] += 1
                nvar += 1
        rec += [sum(exact), nvar, *_summary(bins)]
        hists.append(bins)
    return tuple(rec), hists


_LUT = np.full(256, 4, dtype=np.uint8)
for _c, _v in CODE.items():
    _LUT[ord(_c)] = _v


def variants(reads, motifs):
    """(records of shape (len(reads), len(motifs)), hist, reads_with of shape (len(motifs), 2, BINS), per_read of shape
    (len(reads), len(motifs), 2, BINS))."""
    reads = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in reads]
    out = np.zeros((len(reads), len(motifs)), dtype=VARIANT_DTYPE)
    out["top_fwd"] = NONE
    out["top_rev"] = NONE
    per_read = np.zeros((len(reads), len(motifs), 2, BINS), dtype=np.uint64)
    for r, read in enumerate(reads):
        codes = _LUT[np.frombuffer(read, dtype=np.uint8)]
        n = len(codes)
        for m, motif in enumerate(motifs):
            motif = motif.upper()
            k = len(motif)
            if n < k:
                continue
            nwin = n - k + 1
            win = np.lib.stride_tricks.sliding_window_view(codes, k)  # (nwin, k)
            valid = (win != 4).all(axis=1)
            for s, target in enumerate((motif, revcomp(motif))):
                t = np.array([CODE[c] for c in target], dtype=np.uint8)
                diff = win != t[None, :]
                nd = diff.sum(axis=1)
                exact = valid & (nd == 0)
                var = valid & (nd == 1)
                back = np.zeros(nwin, dtype=bool)
                fwd = np.zeros(nwin, dtype=bool)
                if nwin > k:
                    back[k:] = exact[:-k]
                    fwd[:-k] = exact[k:]
                idx = np.flatnonzero(var & (back | fwd))
                j = diff[idx].argmax(axis=1)
                c = win[idx, j].astype(np.int64)
                b = 4 * j + c if s == 0 else 4 * (k - 1 - j) + (3 - c)
                bins = np.bincount(b, minlength=BINS)
                per_read[r, m, s] = bins
                sfx = "_fwd" if s == 0 else "_rev"
                out["units" + sfx][r, m] = exact.sum()
                out["variants" + sfx][r, m] = len(idx)
                out["distinct" + sfx][r, m] = (bins != 0).sum()
                if len(idx):
                    out["top" + sfx][r, m] = bins.argmax()  # the first, i.e. smallest, bin with the largest count
                    out["top_count" + sfx][r, m] = bins.max()
    return out, per_read.sum(axis=0), (per_read != 0).sum(axis=0).astype(np.uint64), per_read


def cli_lines(files, motifs, min_units=4, results=None):
    """stdout of `trew variants`; files = [(path, reads)], formatted from results = [(records, hist, reads_with)], one per file
    (default: the reference's)"""
    lines = []
    nm = len(motifs)
    tot = dict(reads=0, bases=0, rep=[0] * nm, uf=[0] * nm, ur=[0] * nm, vf=[0] * nm, vr=[0] * nm)
    hist = np.zeros((nm, 2, BINS), dtype=np.uint64)
    rw = np.zeros_like(hist)
    for i, (path, reads) in enumerate(files):
        rec, h, w = results[i] if results is not None else variants(reads, motifs)[:3]
        hist += h
        rw += w
        lines += [">" + os.path.realpath(path), "read,length,motif," + ",".join(FIELDS)]
        for r, read in enumerate(reads):
            for m, motif in enumerate(motifs):
                x = {f: int(rec[f][r, m]) for f in FIELDS}
                if max(x["units_fwd"] + x["variants_fwd"], x["units_rev"] + x["variants_rev"]) >= min_units:
                    tot["rep"][m] += 1
                    x["top_fwd"], x["top_rev"] = bin_text(motif, x["top_fwd"]), bin_text(motif, x["top_rev"])
                    lines.append("%d,%d,%s,%s" % (r, len(read), motif, ",".join(str(x[f]) for f in FIELDS)))
        tot["reads"] += len(reads)
        tot["bases"] += sum(len(r) for r in reads)
        for m in range(nm):
            for key, f in (("uf", "units_fwd"), ("ur", "units_rev"), ("vf", "variants_fwd"), ("vr", "variants_rev")):
                tot[key][m] += int(rec[f][:, m].astype(np.uint64).sum())
    lines += [">Summary", "motif,reads,reads_reported,bases,units_fwd,units_rev,variants_fwd,variants_rev"]
    for m, motif in enumerate(motifs):
        lines.append("%s,%d,%d,%d,%d,%d,%d,%d" % (motif, tot["reads"], tot["rep"][m], tot["bases"], tot["uf"][m], tot["ur"][m], tot["vf"][m], tot["vr"][m]))
    lines += [">Variants", "motif,variant,pos,base,count_fwd,reads_fwd,count_rev,reads_rev"]
    for m, motif in enumerate(motifs):
        both = hist[m, 0] + hist[m, 1]
        for b in sorted(np.flatnonzero(both).tolist(), key=lambda b: (-int(both[b]), b)):
            lines.append("%s,%s,%d,%s,%d,%d,%d,%d" % (motif, bin_text(motif, b), b // 4, BASES[b & 3], hist[m, 0, b], rw[m, 0, b], hist[m, 1, b], rw[m, 1, b]))
    return lines
