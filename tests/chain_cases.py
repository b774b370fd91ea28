"""Inputs and comparisons shared by test_chain_cpu.py and test_gpu_chain.py."""
import os

import numpy as np

import chain_ref as R
from trew_amd import capi
from variant_cases import MOTIFS, noisy_reads, rc_read  # noqa: F401

TEL, RTEL = "TTAGGG", "CCCTAA"
K31, K32 = MOTIFS[6], MOTIFS[7]
NONE = R.NONE
# the placements the kernel's seams ask for: bits 30, 31, 0, 1 of a word in front of, at and behind the 63-word iteration's
# seams (words 62 | 63, 125 | 126) and the seams a 64-word iteration would have (63 | 64)
EDGE_WORDS = (1, 2, 62, 63, 64, 125, 126)
EDGE_BITS = (30, 31, 0, 1)
EDGE_MOTIFS = ["AAT", TEL, K31, K32]


def same(got, want):
    """got, want = (items, counts [, ...]): item for item in the order of (read, motif, strand, start), count for count"""
    gi, gc = got[0], got[1]
    wi, wc = want[0], want[1]
    assert gc.shape == wc.shape
    bad = np.argwhere(gc != wc)
    assert len(bad) == 0, "counts differ at (read, motif, strand, kind) %s: got %s, want %s" % (bad[0].tolist(), gc[tuple(bad[0])], wc[tuple(bad[0])])
    assert len(gi) == len(wi), "%d items, want %d" % (len(gi), len(wi))
    for f in R.FIELDS:
        bad = np.flatnonzero(gi[f] != wi[f])
        assert len(bad) == 0, "%s differs at item %d: got %s, want %s" % (f, bad[0], gi[bad[0]], wi[bad[0]])


def key_items(items, r, m, s):
    """the (start, count, bin) of one key, in start order"""
    x = items[(items["read"] == r) & (items["motif"] == m) & (items["strand"] == s)]
    return [(int(a), int(b), int(c)) for a, b, c in zip(x["start"], x["count"], x["bin"])]


def subst(unit, j, c):
    return unit[:j] + c + unit[j + 1:]


def other_base(c):
    return "C" if c != "C" else "A"


def filler(unit, n):
    """n bases of a homopolymer, or of two alternating bases, none of whose windows is a unit of `unit` or one substitution
    away from one, on either strand (so a filler next to a tract neither extends a run nor anchors anything)"""
    for pat in ("C", "A", "G", "T", "CG", "AT", "AC", "GT", "AG", "CT"):
        probe = (pat * (len(unit) + 2))[:2 * len(unit) + 2]
        if all(x is None for s, t in enumerate((unit, R.revcomp(unit))) for x in R.classify(probe, t, s)):
            return (pat * n)[:n]
    raise AssertionError("no filler for " + unit)


def run_start_read(unit, p, r=3):
    """a run of r units whose first window is p"""
    return filler(unit, p) + unit * r + filler(unit, 40)


def run_end_read(unit, p):
    """a run whose last window is p (as many units as fit in front, four at the most)"""
    k = len(unit)
    r = 1 + min(3, p // k)
    return filler(unit, p - (r - 1) * k) + unit * r + filler(unit, 40), r


def variant_fwd_anchor_read(unit, p):
    """a variant unit at window p whose only anchor is the exact unit at p + k"""
    k = len(unit)
    return filler(unit, p) + subst(unit, k // 2, other_base(unit[k // 2])) + unit + filler(unit, 40)


def variant_back_anchor_read(unit, p):
    """a variant unit at window p whose only anchor is the exact unit at p - k"""
    k = len(unit)
    return filler(unit, p - k) + unit + subst(unit, k // 2, other_base(unit[k // 2])) + filler(unit, 40)


def dirty_planes(words, offsets, lengths, rnd):
    """the packed planes with their nmask bits set past every read's end and anything in the two planes there"""
    dirty = np.array(words, dtype=np.uint32)
    for o, n in zip(offsets.tolist(), lengths.tolist()):
        if n % 32:
            last = o + 3 * (n // 32)
            hi = np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
            dirty[last + 2] |= hi
            dirty[last] |= np.uint32(rnd.getrandbits(32)) & hi
            dirty[last + 1] |= np.uint32(rnd.getrandbits(32)) & hi
    return dirty


def mirrored(items, counts, lengths, ks):
    """what the definition promises for the reverse complements of the reads: strands swapped, start -> n - k - start for a
    variant and n - k - (start + (count - 1) k) for a run, the bin unchanged; sorted again"""
    out = items.copy()
    n = np.asarray(lengths, dtype=np.int64)[items["read"]]
    k = np.asarray(ks, dtype=np.int64)[items["motif"]]
    out["strand"] = 1 - items["strand"]
    out["start"] = (n - k - (items["start"].astype(np.int64) + (items["count"].astype(np.int64) - 1) * k)).astype(np.uint32)
    order = np.lexsort((out["start"], out["strand"], out["motif"], out["read"]))
    return out[order], counts[:, :, ::-1, :]


def cli_lines(files, motifs, min_units=4, per_item=False, results=None):
    """stdout of `trew chain`; files = [(path, reads)], formatted from results = [(items, counts, n_items)], one per file (default:
    trew_chain_host's)"""
    lines = []
    nm = len(motifs)
    tot = np.zeros((nm, 2, 5), dtype=np.int64)  # reads, units, variants, runs, longest run
    for i, (path, reads) in enumerate(files):
        items, counts, _ = results[i] if results is not None else capi.chain_host(reads, motifs)
        lines += [">" + os.path.realpath(path), "read,length,motif,strand,start,count,unit" if per_item else "read,length,motif,strand,start,end,units,variants,runs,signature"]
        keys = np.stack([items["read"], items["motif"], items["strand"]], axis=1)
        cuts = np.flatnonzero(np.any(np.diff(keys, axis=0) != 0, axis=1)) + 1 if len(items) else np.zeros(0, dtype=np.int64)
        for grp in (np.split(items, cuts) if len(items) else []):
            r, m, s = int(grp["read"][0]), int(grp["motif"][0]), int(grp["strand"][0])
            k = len(motifs[m])
            is_run = grp["bin"] == NONE
            units, nvar, runs = int(grp["count"][is_run].sum()), int((~is_run).sum()), int(is_run.sum())
            tot[m, s, 1:4] += (units, nvar, runs)
            tot[m, s, 4] = max(tot[m, s, 4], int(grp["count"][is_run].max()) if runs else 0)
            if units + nvar < min_units:
                continue
            tot[m, s, 0] += 1
            head = "%d,%d,%s,%s" % (r, len(reads[r]), motifs[m], "-" if s else "+")
            if per_item:
                lines += ["%s,%d,%d,%s" % (head, x["start"], x["count"], "=" if x["bin"] == NONE else capi.chain_unit_text(motifs[m], int(x["bin"]))) for x in grp]
            else:
                end = int((grp["start"].astype(np.int64) + grp["count"].astype(np.int64) * k).max())
                lines.append("%s,%d,%d,%d,%d,%d,%s" % (head, grp["start"][0], end, units, nvar, runs, capi.chain_signature(grp, motifs[m])))
    lines += [">Summary", "motif,strand,reads,units,variants,runs,longest_run"]
    for m, motif in enumerate(motifs):
        for s in (0, 1):
            lines.append("%s,%s,%d,%d,%d,%d,%d" % ((motif, "-" if s else "+") + tuple(tot[m, s].tolist())))
    return lines
