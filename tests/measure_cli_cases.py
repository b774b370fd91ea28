"""The file of tests/test_gpu_measure_cli.py -- one generated FASTQ of a few hundred KB that is cut into many chunks by a small
TREW_MEASURE_CHUNK_BYTES -- and what the twelve measure commands must print for it, formatted from the CPU definitions
(capi.*_host) over the whole file, with file-wide ordinals, by the formatters of the measures' own tests."""
import os
import random

import numpy as np

import align_ref
import annot_ref
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
COMMANDS = ["annotate", "tracts", "intervals", "variants", "periods", "chain", "repeats", "satellites", "align", "refine", "tandems", "trace"]
LOGGED = ["intervals", "chain", "repeats", "satellites", "tandems", "trace"]  # the six with an append log that can overflow
_RC = str.maketrans("ACGTacgt", "TGCAtgca")


def command_line(name, paths):
    """arguments of `trew` for one command at its defaults"""
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
    """the CPU definitions of the twelve commands over the whole file, at the commands' defaults"""
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
    }


def _shifted(recs, n):
    out = recs.copy()
    out["read"] += n
    return np.concatenate([recs, out])


def _one_file(name, path, reads, res):
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
    at = lines.index(">Summary")
    return lines[:at], lines[at:]


def expected(name, paths, reads, res):
    """stdout of `trew <name>` for the same reads under every path of `paths`: a section per path, with ordinals that start
    at 0 in each, and one summary over all of them"""
    if name == "variants":
        return variant_ref.cli_lines([(p, reads) for p in paths], MOTIFS, results=[res] * len(paths))
    if name == "chain":
        return chain_cli_lines([(p, reads) for p in paths], MOTIFS, results=[res] * len(paths))
    sections = [_one_file(name, p, reads, res) for p in paths]
    if len(paths) == 1:
        return sections[0][0] + sections[0][1]
    assert len(paths) == 2
    n = len(reads)
    if name in ("annotate", "tracts", "align", "periods", "refine"):
        both = np.concatenate([res, res])
    elif name == "trace":
        both = (_shifted(res[0], n), np.concatenate([res[1], res[1]]), np.concatenate([res[2], res[2]]))
    elif name == "intervals":
        both = (_shifted(res[0], n), np.concatenate([res[1], res[1]]))
    else:
        both = (_shifted(res[0], n),)
    return sections[0][0] + sections[1][0] + _one_file(name, paths[0], reads + reads, both)[1]


def reported_reads(name, lines):
    """ordinals of the reads with a row in the one-file output `lines`, in order"""
    stop = lines.index(">Summary")
    return [int(ln.split(",")[0]) for ln in lines[2:stop]]


def summary_keys(name, lines):
    """(period, canonical) -> ordinals of the reads with such a row, from the rows of periods, refine, repeats, satellites or
    tandems"""
    col = 2 if name in ("periods", "refine") else 3
    out = {}
    for ln in lines[2:lines.index(">Summary")]:
        f = ln.split(",")
        out.setdefault((f[col], f[col + 2]), set()).add(int(f[0]))
    return out
