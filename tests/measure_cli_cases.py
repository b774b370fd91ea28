"""The file of tests/test_gpu_measure_cli.py -- one generated FASTQ of a few hundred KB that is cut into many chunks by a small
TREW_MEASURE_CHUNK_BYTES -- and what the fourteen measure commands must print for it, formatted from the CPU definitions
(capi.*_host) over the whole file, with file-wide ordinals, by the formatters of the measures' own tests; and a second, small
file of many short tracts a read (make_tract_file), which fills dissect's record log as well."""
import os
import random

import numpy as np

import align_ref
import annot_ref
import decompose_ref
import dissect_ref
import interval_ref
import period_ref
import refine_ref
import repeat_ref
import satellite_ref
import tandem_ref
import trace_ref
import tract_ref
import variant_ref
from chain_cases import cli_lines as chain_cli_lines
from test_fastq_chunks_cpu import chunk_spans
from test_fastq_blocks_cpu import reference_rule
from trew_amd import capi

SEED = 20260117
CHUNK = 4096
MOTIFS = ["TTAGGG", "AATGG"]
SAT_MAX_PERIOD = 180  # keeps satellites_host short; the planted 171-mer is within it
COMMANDS = ["annotate", "tracts", "intervals", "variants", "periods", "chain", "repeats", "satellites", "align", "refine", "tandems", "trace",
            "decompose", "dissect"]
LOGGED = ["intervals", "chain", "repeats", "satellites", "tandems", "trace", "decompose", "dissect"]  # the eight with an append log that can overflow
ITEMIZED = ["decompose", "dissect"]  # the two whose --items form is run beside their rows form
_RC = str.maketrans("ACGTacgt", "TGCAtgca")


def command_line(name, paths, per_item=False):
    """arguments of `trew` for one command at its defaults; per_item: decompose and dissect with --items"""
    if name in ITEMIZED:  # in their rows form a row per tract, with the signature printed from the chunk's text
        return [name, *(["--items"] if per_item else []), *paths]
    if name in ("periods", "repeats", "refine", "tandems"):
        return [name, *paths]
    if name == "trace":  # a row per item: the log's records themselves, in place
        return [name, "--items", ",".join(MOTIFS), *paths]
    if name == "satellites":
        return [name, "--max_period", str(SAT_MAX_PERIOD), *paths]
    return [name, ",".join(MOTIFS), *paths]


def _junk(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _noisy_tract(rnd, unit, n, variants=()):
    """about n bases of `unit` back to back: one unit in 8 replaced by one of `variants`, one base in 60 substituted, one in
    150 deleted, one in 150 followed by an inserted base"""
    out = []
    while sum(len(u) for u in out) < n:
        u = rnd.choice(variants) if variants and rnd.randrange(8) == 0 else unit
        s = ""
        for c in u:
            x = rnd.randrange(300)
            if x < 5:
                c = rnd.choice([b for b in "ACGT" if b != c])
            elif x < 7:
                continue
            elif x < 9:
                c += rnd.choice("ACGT")
            s += c
        out.append(s)
    return "".join(out)


def _planted(rnd, j):
    """planted read number j: a noisy (TTAGGG)n tract of at least 300 bases at the head of the read, in three stretches with
    some twenty random bases between them (several intervals and tracts a read); every second one an (AATGG)n tract, every
    fifth four copies of a 171-mer beside it; every fourth reverse-complemented"""
    s = ""
    for piece in range(3):
        s += _noisy_tract(rnd, "TTAGGG", rnd.randint(100, 220), ("TCAGGG", "TGAGGG"))
        s += _junk(rnd, rnd.randint(22, 30))
    s += _junk(rnd, rnd.randint(0, 150))
    if j % 2 == 1:
        s += _noisy_tract(rnd, "AATGG", rnd.randint(80, 400)) + _junk(rnd, rnd.randint(0, 60))
    if j % 5 == 2:
        s += _junk(rnd, 171) * 4 + _junk(rnd, rnd.randint(0, 60))
    s = s[:1500]
    if j % 4 == 3:
        s = s.translate(_RC)[::-1]
    return s


def make_records(seed=SEED):
    """[header, sequence, quality] (str, no newlines) of about 600 reads of 0 to 1500 bases.  A third of the reads are planted
    ones, and they come in runs of 1 to 20 with twice as many plain reads behind each run: some chunks hold many tracts, others
    none.  Header lengths vary; some quality lines start with '@'; a few reads are empty, some have a lowercase stretch, and
    every seventh plain read holds a (CA)n microsatellite."""
    rnd = random.Random(seed)
    recs, j, plain = [], 0, 0
    runs = [1, 2, 5, 1, 3, 8, 2, 1, 20, 4, 1, 2, 6, 3, 1, 12, 2, 5, 1, 3, 9, 2, 4, 1, 7, 3, 2, 15, 1, 4, 6, 2, 3, 1, 5, 8, 2, 1, 10, 3, 4, 6, 9, 4, 5]
    for run in runs:
        for is_planted in [True] * run + [False] * (2 * run):
            if is_planted:
                seq = _planted(rnd, j)
                j += 1
            else:
                n = rnd.choice([0, 1, 5, 36, 150, 151, 400, rnd.randint(0, 700)])
                seq = _junk(rnd, n)
                if plain % 7 == 3 and n >= 100:
                    seq = seq[:20] + "CA" * 30 + seq[80:]
                plain += 1
            i = len(recs)
            if i % 11 == 5 and len(seq) > 40:  # a lowercase stretch
                a = rnd.randrange(len(seq) - 30)
                seq = seq[:a] + seq[a:a + 30].lower() + seq[a + 30:]
            header = "@r%d%s" % (i, " " + "x" * rnd.randint(0, 40) if i % 3 else "")
            qual = ("@" if i % 5 == 1 and seq else "") + "I" * (len(seq) - (1 if i % 5 == 1 and seq else 0))
            recs.append([header, seq, qual])
    return recs


def render(recs, eol="\n"):
    return "".join(h + eol + s + eol + "+" + eol + q + eol for h, s, q in recs).encode()


def borders(data, chunk):
    """the file offsets at which a chunk's new bytes begin (the first chunk's 0 left out)"""
    return [off + carried for off, carried, _, _ in chunk_spans(data, chunk)[1:]]


def place_borders(recs, chunk=CHUNK):
    """Pads two headers so that, at this chunk length, one border falls exactly behind a header's newline and a later one
    exactly in front of a sequence line's newline.  A border that falls d bytes behind such a place is met by d more header
    bytes in the same record: the border itself is decided by the bytes in front of the record."""
    first = 0
    for kind in ("behind_header", "at_sequence_newline"):
        data = render(recs)
        starts, pos = [], 0
        for h, s, q in recs:
            starts.append(pos)
            pos += len(h) + len(s) + len(q) + 5
        best = None
        for b in borders(data, chunk):
            r = max(i for i, p in enumerate(starts) if p <= b)
            h, s, q = recs[r]
            target = starts[r] + len(h) + 1 + (0 if kind == "behind_header" else len(s))
            d = b - target
            inside = d <= len(s) if kind == "behind_header" else d <= len(q) + 2
            if r >= first and 0 <= d and inside and (best is None or d < best[0]):
                best = (d, r)
        d, r = best
        recs[r][0] += "p" * d
        first = r + 1
    return recs


def make_file(seed=SEED):
    return render(place_borders(make_records(seed)))


def reads_of(data):
    """the sequence lines of the file as the reference's newline counter sees them (a '\\r' stays part of its line)"""
    return [data[s:s + n] for s, n in reference_rule(data)]


def host_results(reads):
    """the CPU definitions of the fourteen commands over the whole file, at the commands' defaults"""
    p = capi.pack_reads(reads)
    return {
        "annotate": capi.annotate_host(p, MOTIFS),
        "tracts": capi.tracts_host(p, MOTIFS, 3),
        "intervals": capi.intervals_host(p, MOTIFS),
        "variants": capi.variants_host(p, MOTIFS),
        "periods": capi.periods_host(p),
        "chain": capi.chain_host(p, MOTIFS),
        "repeats": capi.repeats_host(p),
        "satellites": capi.satellites_host(p, max_period=SAT_MAX_PERIOD),
        "align": capi.align_host(p, MOTIFS, 3),
        "refine": capi.refine_host(p),
        "tandems": capi.tandems_host(p),
        "trace": capi.trace_host(p, MOTIFS, 3, 24),
        "decompose": capi.decompose_host(p),
        "dissect": capi.dissect_host(p),
    }


def _shifted(recs, n):
    out = recs.copy()
    out["read"] += n
    return np.concatenate([recs, out])


def _one_file(name, path, reads, res, per_item=False):
    """(the file's section, the summary section) of a one-file run"""
    real = os.path.realpath(path)
    if name == "annotate":
        lines = annot_ref.cli_lines(path, reads, MOTIFS, res)
    elif name == "tracts":
        lines = tract_ref.cli_lines(path, reads, MOTIFS, res)
    elif name == "intervals":
        lines = interval_ref.cli_lines(path, reads, MOTIFS, res[:2])
    elif name == "align":
        lines = align_ref.cli_lines(path, reads, MOTIFS, res, 3)
    elif name == "periods":
        return period_ref.cli_lines(real, reads, res)
    elif name == "repeats":
        return repeat_ref.cli_lines(real, reads, res[0])
    elif name == "satellites":
        return satellite_ref.cli_lines(real, reads, res[0])
    elif name == "refine":
        return refine_ref.cli_lines(path, reads, res, 3)
    elif name == "tandems":
        return tandem_ref.cli_lines(path, reads, res[0], 3)
    elif name == "trace":
        lines = trace_ref.cli_lines(path, reads, MOTIFS, res, 3, per_item=True)
    elif name == "decompose":
        return decompose_ref.cli_lines(path, reads, res, 3, per_item=per_item)
    elif name == "dissect":
        return dissect_ref.cli_lines(path, reads, res, 3, per_item=per_item)
    at = lines.index(">Summary")
    return lines[:at], lines[at:]


def expected(name, paths, reads, res, per_item=False):
    """stdout of `trew <name>` for the same reads under every path of `paths`: a section per path, with ordinals that start
    at 0 in each, and one summary over all of them; per_item: the --items form of decompose and dissect"""
    if name == "variants":
        return variant_ref.cli_lines([(p, reads) for p in paths], MOTIFS, results=[res] * len(paths))
    if name == "chain":
        return chain_cli_lines([(p, reads) for p in paths], MOTIFS, results=[res] * len(paths))
    sections = [_one_file(name, p, reads, res, per_item) for p in paths]
    if len(paths) == 1:
        return sections[0][0] + sections[0][1]
    assert len(paths) == 2
    n = len(reads)
    if name in ("annotate", "tracts", "align", "periods", "refine"):
        both = np.concatenate([res, res])
    elif name == "trace":
        both = (_shifted(res[0], n), np.concatenate([res[1], res[1]]), np.concatenate([res[2], res[2]]))
    elif name == "decompose":  # items, counts, records: the records are one per read, the items name theirs
        both = (_shifted(res[0], n), np.concatenate([res[1], res[1]]), np.concatenate([res[2], res[2]]))
    elif name == "dissect":  # records and items both name their read
        both = (_shifted(res[0], n), _shifted(res[1], n))
    elif name == "intervals":
        both = (_shifted(res[0], n), np.concatenate([res[1], res[1]]))
    else:
        both = (_shifted(res[0], n),)
    return sections[0][0] + sections[1][0] + _one_file(name, paths[0], reads + reads, both, per_item)[1]


def reported_reads(name, lines):
    """ordinals of the reads with a row in the one-file output `lines`, in order"""
    stop = lines.index(">Summary")
    return [int(ln.split(",")[0]) for ln in lines[2:stop]]


def summary_keys(name, lines):
    """(period, canonical) -> ordinals of the reads with such a row, from the rows of periods, refine, decompose (a row per
    read: the period is column 2), repeats, satellites, tandems or dissect (a row per tract, with its depth: column 3)"""
    col = 2 if name in ("periods", "refine", "decompose") else 3
    out = {}
    for ln in lines[2:lines.index(">Summary")]:
        f = ln.split(",")
        out.setdefault((f[col], f[col + 2]), set()).add(int(f[0]))
    return out


def tract_rows(name, lines):
    """(read, start, end, strand, signature) of every row of decompose or dissect in their rows form"""
    col = 5 if name == "decompose" else 6
    out = []
    for ln in lines[2:lines.index(">Summary")]:
        f = ln.split(",")
        out.append((int(f[0]), int(f[col]), int(f[col + 1]), f[-4], f[-1]))
    return out


def log_overflows(name, res, chunk_reads):
    """(chunks whose items exceed the first item log of fold_decompose / fold_dissect, sixteen a read; chunks whose records
    exceed dissect's first record log, four a read and sixteen more), from the host definition's result `res`"""
    n_reads = 1 + max(i for c in chunk_reads for i in c)
    items, tracts = [0] * n_reads, [0] * n_reads
    for r in res[0 if name == "decompose" else 1]["read"]:
        items[int(r)] += 1
    if name == "dissect":
        for r in res[0]["read"]:
            tracts[int(r)] += 1
    over_items = [n for n, c in enumerate(chunk_reads) if sum(items[i] for i in c) > 16 * len(c)]
    over_tracts = [n for n, c in enumerate(chunk_reads) if c and sum(tracts[i] for i in c) > 4 * len(c) + 16]
    return over_items, over_tracts


# The second file: about 40 KB of reads with many short tracts each, for the one capacity the first file never fills.  A read
# of the first file has two tracts at the most, so at any chunk length fold_dissect's record log (4 n + 16 records for n reads)
# holds every batch.  Here every third read holds 26 exact tracts and the others 10, each of 36 bases of a unit of 2 to 6 bases
# with 18 random bases in front of it: at chunk 4096 a batch is two or three reads, and its 20 to 46 tracts fall on either side
# of the 24 or 28 records its log starts with.  A read's recursion splits around one tract at a time, so its depth grows with
# its tracts.  In front of them stand two reads of 14 tracts that are one item each (whole copies of the unit's anchored
# rotation, the bases beside them no match): the first chunk is these two, 28 records for a log of 24 and about as many items
# for a log of 32 -- the one batch that is resubmitted for its records alone.
TRACT_SEED = 20260330
TRACT_READS = 2 + 24
TRACT_BASES, TRACT_GAP = 36, 18
CLEAN_TRACTS, CLEAN_BASES = 14, 30


def _unit(rnd, k, avoid):
    """a unit of k bases that is no repetition of a shorter one and shares no rotation with `avoid`"""
    while True:
        u = _junk(rnd, k)
        if all(u != u[:d] * (k // d) for d in range(1, k) if k % d == 0) and (avoid is None or len(avoid) != k or u not in avoid + avoid):
            return u


def _anchored(unit):
    """the rotation of `unit` that decompose traces against: the one with the smallest packed word"""
    word = period_ref.pack_unit(decompose_ref.anchor(list(align_ref.codes(unit)))[1])
    return period_ref.unit_text(word, len(unit))


def _clean_read(rnd):
    """CLEAN_TRACTS tracts of CLEAN_BASES bases, whole copies of an anchored unit of 2, 3, 5 or 6 bases, between random bases
    of which the two beside a tract do not continue it"""
    seq, unit = "", None
    for _ in range(CLEAN_TRACTS):
        unit = _anchored(_unit(rnd, rnd.choice([2, 3, 5, 6]), unit))
        seq += _junk(rnd, TRACT_GAP - 2) + rnd.choice([c for c in "ACGT" if c != unit[-1]]) + unit * (CLEAN_BASES // len(unit))
        seq += rnd.choice([c for c in "ACGT" if c != unit[0]])
    return seq + _junk(rnd, TRACT_GAP)


def make_tract_records(seed=TRACT_SEED):
    rnd = random.Random(seed + 1)
    recs = [["@c%d" % i, seq, "I" * len(seq)] for i, seq in enumerate(_clean_read(rnd) for _ in range(2))]
    rnd = random.Random(seed)
    for i in range(TRACT_READS - 2):
        seq, unit = "", None
        for _ in range(26 if i % 3 == 0 else 10):
            unit = _unit(rnd, rnd.randint(2, 6), unit)
            phase = rnd.randrange(len(unit))
            seq += _junk(rnd, TRACT_GAP) + (unit * (TRACT_BASES // len(unit) + 2))[phase:phase + TRACT_BASES]
        seq += _junk(rnd, TRACT_GAP)
        recs.append(["@m%d" % i, seq, "I" * len(seq)])
    return recs


def make_tract_file(seed=TRACT_SEED):
    return render(make_tract_records(seed))
