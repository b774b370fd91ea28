"""Brute-force reference of the de novo repeats with periods up to 256 (trew_hip_satellite).  The definition is
that of period_ref.period_read and repeat_ref.repeats_read / repeats_read_rounds, which accept any max_period and return the
unit as a Python integer (first base most significant); what is added here is the record's unit of sixteen words, the text
forms, and the stdout of `trew satellites`."""
import numpy as np

import period_ref as R
import repeat_ref as RR

MAX_PERIOD = 256
FIELDS = RR.FIELDS
DTYPE = np.dtype([(f, "<u4", (16,)) if f == "unit" else (f, "<u4") for f in FIELDS])
assert DTYPE.itemsize == 104
SCALARS = tuple(f for f in FIELDS if f != "unit")


def unit_codes_of_int(word, d):
    """the codes of a unit that period_ref packed into an integer, first base first"""
    return [(int(word) >> (2 * (d - 1 - j))) & 3 for j in range(d)]


def unit_words(codes):
    """unit[16]: base j in bits [2 (j & 15), 2 (j & 15) + 2) of word j >> 4; nothing above"""
    w = [0] * 16
    for j, c in enumerate(codes):
        w[j >> 4] |= c << (2 * (j & 15))
    return w


def unit_codes(words, d):
    return [(int(words[j >> 4]) >> (2 * (j & 15))) & 3 for j in range(int(d))]


def unit_text(words, d):
    return "".join(R.LETTER[c] for c in unit_codes(words, d))


def canonical_codes(codes):
    """the smaller of the smallest rotation of the unit and the smallest rotation of its reverse complement, compared base by
    base in code order, first base first"""
    codes = list(codes)
    rc = [3 - c for c in reversed(codes)]
    return min(tuple(x[i:] + x[:i]) for x in (codes, rc) for i in range(len(codes)))


def satellites(reads, min_period=1, max_period=MAX_PERIOD, penalty=3, min_score=24, shape=RR.repeats_read):
    """(DTYPE records sorted by (read, start), counts per read): the order every interface returns"""
    rows, counts = [], np.zeros(len(reads), dtype=np.uint32)
    for i, r in enumerate(reads):
        mine = sorted(shape(r, min_period, max_period, penalty, min_score), key=lambda x: x[1 + RR.START])
        counts[i] = len(mine)
        rows += [(i,) + x for x in mine]
    out = np.zeros(len(rows), dtype=DTYPE)
    for o, x in zip(out, rows):
        for f, v in zip(FIELDS, x):
            o[f] = unit_words(unit_codes_of_int(v, x[FIELDS.index("period")])) if f == "unit" else v
    return out, counts


def cli_lines(path, reads, recs):
    """stdout of `trew satellites` for one file: (the file's section, the >Summary section), formatted from records"""
    rows = [">" + path, "read,length,depth,period,unit,canonical,start,end,score,matches,support,scored_period"]
    summary = {}
    for x in recs:
        i, d = int(x["read"]), int(x["period"])
        codes = unit_codes(x["unit"], d)
        canon = canonical_codes(codes)
        text = "".join(R.LETTER[c] for c in canon)
        rows.append("%d,%d,%d,%d,%s,%s,%d,%d,%d,%d,%d,%d" % (i, len(reads[i]), x["depth"], d, unit_text(x["unit"], d), text, x["start"], x["end"], x["score"],
                                                        x["matches"], x["support"], x["scored_period"]))
        who, tracts, bases = summary.get((d, canon), (set(), 0, 0))
        summary[(d, canon)] = (who | {i}, tracts + 1, bases + int(x["end"]) - int(x["start"]))
    tail = [">Summary", "period,canonical,reads,tracts,bases"]
    for (d, canon), (who, tracts, bases) in sorted(summary.items(), key=lambda kv: (-len(kv[1][0]), kv[0])):
        tail.append("%d,%s,%d,%d,%d" % (d, "".join(R.LETTER[c] for c in canon), len(who), tracts, bases))
    return rows, tail
