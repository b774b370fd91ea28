"""Units in place under indels (the traceback of the wraparound alignment), the parts that need no GPU: the forms of
trace_ref.py against each other cell by cell and against hand-worked vectors, the consequences of the definition on the fuzz
set, the restarted table against the full one, the host definition (trew_trace_host) against the reference, the signature
formatter, the stand-alone sanitizer harness, the additive ABI, the argument errors of the C ABI and of `trew trace`.

The end-phase tie (rule 3) does not occur in any key of the fuzz set, whose motifs are primitive; a read built for it is
(AAT)x10 against the motif AATAAT, where the phases j and j + 3 hold equal cells in every row (test_end_phase_tie)."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_ref as R
import trace_ref as T
from align_cases import T10, TEL, fuzz_sets, revcomp, with_deletion, with_insertion
from period_cases import junk, noisy
from trace_cases import HAND, block_reads, two_strand_reads
from trew_amd import capi

assert tuple(capi.TRACE_DTYPE.names) == T.ITEM_FIELDS  # the reference and the record name their fields alike, in the same order
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")


def same(got, want):
    gi, gc, gr = got[:3]
    wi, wc, wr = want[:3]
    assert gr.shape == wr.shape and gc.shape == wc.shape
    for f in wr.dtype.names:
        assert (gr[f] == wr[f]).all(), f
    assert (gc == wc).all()
    assert len(gi) == len(wi)
    bad = np.flatnonzero(gi != wi)
    assert len(bad) == 0, "item %d differs: got %s, want %s" % (bad[0], gi[bad[0]], wi[bad[0]])


def tup(it):
    return tuple(int(v) for v in it)[3:11]


@pytest.fixture(scope="module")
def fuzz():
    """[(motif, reads, {penalty: trace_keys})], the reference computed once"""
    return [(unit, reads, {p: T.trace_keys(reads, [unit], p) for p in (1, 3, 64)}) for unit, reads in fuzz_sets()]


def test_reference_forms_agree_on_every_cell():
    """the full table (max over d, smallest d) against the doubling steps with d carried, and against the numpy form, on (op, d)
    of every cell, the record and the end phase: every k, all three penalties"""
    rnd = random.Random(9)
    for k in range(3, 33):
        unit = junk(rnd, k)
        reads = [junk(rnd, rnd.randint(0, 6), "ACGTN") + noisy(rnd, unit, rnd.randint(0, 50), 0.04, 0.1, 0.01) + junk(rnd, rnd.randint(0, 6))
                 for _ in range(2)]
        cs = [R.codes(r) for r in reads]
        lens = np.array([len(c) for c in cs], dtype=np.int64)
        X = np.full((len(cs), max(int(lens.max()), 1)), 4, dtype=np.int64)
        for r, c in enumerate(cs):
            X[r, :len(c)] = c
        for penalty in (1, 3, 64):
            for s in range(2):
                t = R.strand_codes(unit, s)
                recs, jstar, dirs, _ = T.dirs_many(X, lens, t, penalty)
                for r, x in enumerate(cs):
                    full = T.table(x, t, penalty)
                    dbl = T.table(x, t, penalty, doubling=True)
                    assert full == dbl, (reads[r], unit, penalty, s)
                    assert full[0] == tuple(int(v) for v in recs[r]) == R.align_strand(x, t, penalty)
                    if full[0][0]:
                        assert full[1] == int(jstar[r])
                    for i in range(1, len(x) + 1):
                        assert [o | (d << 2) for o, d in zip(full[2][i], full[3][i])] == dirs[r, i].tolist(), (reads[r], unit, penalty, s, i)


@pytest.mark.parametrize("read,motif,penalty,min_score,strand,items", HAND)
def test_hand_worked_vectors(read, motif, penalty, min_score, strand, items):
    x, t = R.codes(read), R.strand_codes(motif, strand)
    for doubling in (False, True):
        for restarted in (False, True):
            rec, _, cols = T.trace_strand(x, t, penalty, doubling=doubling, restarted=restarted)
            assert T.items_of(cols, len(motif)) == items
    got = T.trace([read], [motif], penalty, min_score)
    assert [tup(it) for it in got[0] if it["strand"] == strand] == items
    same(capi.trace_host([read.encode()], [motif], penalty, min_score), got)


def test_one_deleted_and_one_inserted_base_land_in_their_copy():
    run = lambda a, b: (a, b - a, (b - a) // 6, 0, b - a, 0, 0, 0)
    for at in range(6, 56):
        got = T.trace([with_deletion(T10, at)], [TEL], 3, 24)
        c = 6 * (at // 6)
        want = [run(0, c)] * (c > 0) + [(c, 5, 1, 0, 6, 0, 0, 1)] + [run(c + 5, 59)] * (c + 5 < 59)
        assert [tup(it) for it in got[0] if it["strand"] == 0] == want, at
    for at in range(4, 57):
        got = T.trace([with_insertion(T10, at, "C")], [TEL], 3, 24)
        c = 6 * ((at - 1) // 6)  # an inserted base in front of a copy stays in the copy before it
        want = [run(0, c)] * (c > 0) + [(c, 7, 1, 0, 6, 0, 1, 0)] + [run(c + 7, 61)] * (c + 7 < 61)
        assert [tup(it) for it in got[0] if it["strand"] == 0] == want, at


def test_end_phase_tie():
    """rule 3: (AAT)x10 against AATAAT -- the cells of the phases 2 and 5 are equal in the end row, the smaller phase wins, and the
    tract is a piece of three bases, four copies and a piece of three bases; the larger phase would give five copies from phase 0"""
    read, motif = "AAT" * 10, "AATAAT"
    ties = {}
    rec, jstar, _, _ = T.table(R.codes(read), R.strand_codes(motif, 0), 3, ties=ties)
    assert rec == (30, 0, 30, 30, 30) and ties["end"] == [2, 5] and jstar == 2
    got = T.trace([read], [motif], 3, 24)
    assert [tup(it) for it in got[0]] == [(0, 3, 1, 3, 3, 0, 0, 0), (3, 24, 4, 0, 24, 0, 0, 0), (27, 3, 1, 0, 3, 0, 0, 0)]
    same(capi.trace_host([read], [motif], 3, 24), got)


def test_consequences_on_the_fuzz_set(fuzz):
    """the items of a key tile [start, end); their bases, consumed and errors sum to the record's; every item has bases >= 1; the
    first and the last column are eq; only the first item has a phase, only the first and the last can be short without an
    error.  And the fuzz set is what it is meant to be: by the reference alone at least half of the keys have a D/I tie on the
    traced path and at least half a d tie (206 and 185 of 217 when this was written)."""
    total = di = dt = 0
    for unit, reads, keys in fuzz:
        k = len(unit)
        for penalty in (1, 3, 64):
            for (r, m, s), (rec, jstar, cols, ties) in keys[penalty].items():
                if rec[0] < 24:
                    continue
                score, start, end, consumed, matches = rec
                its = T.items_of(cols, k)
                assert cols[0][0] == "eq" and cols[-1][0] == "eq"
                at = start
                for it in its:
                    assert it[0] == at and it[1] >= 1
                    at += it[1]
                assert at == end and sum(it[1] for it in its) == end - start and sum(it[4] for it in its) == consumed
                c = R.columns(score, start, end, consumed, matches, k, penalty)
                assert [sum(it[q] for it in its) for q in (5, 6, 7)] == [c["mismatches"], c["insertions"], c["deletions"]]
                assert all(it[3] == 0 for it in its[1:])
                for q, it in enumerate(its):
                    if it[4] < k * it[2] and not (it[5] or it[6] or it[7]):
                        assert q in (0, len(its) - 1)
                    assert it[2] == 1 or (it[1] == it[4] == k * it[2] and it[3:] == (0, k * it[2], 0, 0, 0))
                if penalty == 3:
                    total += 1
                    di += ties[0]
                    dt += ties[1]
    print("keys %d, with a D/I tie on the path %d, with a d tie on the path %d" % (total, di, dt))
    assert total >= 200 and 2 * di >= total and 2 * dt >= total


def test_restarted_table_traces_the_same_columns(fuzz):
    """fact (b): the table restarted at the tract's start, over the tract's rows alone, has the record, the end phase and the
    columns of the full table -- on every key of the fuzz set at P = 3 (the tract as a read of its own: every start field
    moves by `start`, which no comparison sees) and, with the rows numbered as in the read, on every seventh key"""
    n = 0
    for unit, reads, keys in fuzz:
        mine = [(key, v) for key, v in sorted(keys[3].items()) if v[0][0] >= 24]
        subs = T.trace_keys([reads[r][v[0][1]:v[0][2]] for (r, m, s), v in mine], [unit], 3)
        for q, ((r, m, s), (rec, jstar, cols, _)) in enumerate(mine):
            score, start, end, consumed, matches = rec
            sub = subs[(q, 0, s)]
            assert sub[0] == (score, 0, end - start, consumed, matches) and sub[1] == jstar
            assert [(kind, None if b is None else b + start, ph) for kind, b, ph in sub[2]] == cols
            if n % 7 == 0:
                x, t = R.codes(reads[r]), R.strand_codes(unit, s)
                rec2, j2, op, dd = T.table(x, t, 3, row0=start, row_end=end, doubling=True)
                assert rec2 == rec and j2 == jstar and T.walk(x, t, rec, jstar, op, dd) == cols
            n += 1
    assert n >= 200


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_host_against_reference_on_the_fuzz_set(fuzz, penalty):
    for unit, reads, keys in fuzz:
        want = T.trace(reads, [unit], penalty, 24, keys=keys[penalty])
        got = capi.trace_host(reads, [unit], penalty, 24)
        same(got, want)
        assert got[3] == len(want[0])
        # the records are align's, field for field
        al = capi.align_host(reads, [unit], penalty)
        assert all((got[2][f] == al[f]).all() for f in al.dtype.names)


def test_host_many_motifs_packed_planes_lower_case_and_n():
    rnd = random.Random(12)
    motifs = ["AAT", "TGTG", "ACGTT", TEL, "GGGTTAG", junk(rnd, 12)]
    reads = [junk(rnd, rnd.randint(0, 60), "ACGTacgtNn") + noisy(rnd, rnd.choice(motifs), rnd.randint(0, 120), 0.03, 0.06, 0.01).lower()
             + junk(rnd, rnd.randint(0, 30)) for _ in range(40)] + ["", "A", "N" * 40, T10[:17] + "N" + T10[18:]]
    want = T.trace(reads, motifs, 3, 12)
    assert len(want[0]) > 100 and [tup(it) for it in want[0] if it["read"] == 43 and it["motif"] == 3 and it["strand"] == 0][1] == (12, 6, 1, 0, 6, 1, 0, 0)
    same(capi.trace_host(reads, motifs, 3, 12), want)
    same(capi.trace_host(capi.pack_reads(reads), motifs, 3, 12), want)
    reads = block_reads() + two_strand_reads()
    same(capi.trace_host(reads, [TEL], 3, 24), T.trace(reads, [TEL], 3, 24))


def test_host_cap_and_count():
    unit, reads = fuzz_sets()[3]
    items, counts, records, n = capi.trace_host(reads, [unit], 3, 24)
    assert n == len(items) == counts.sum() and n > 20
    part, counts2, records2, n2 = capi.trace_host(reads, [unit], 3, 24, cap=5)
    assert n2 == n and len(part) == 5 and (part == items[:5]).all() and (counts2 == counts).all() and (records2 == records).all()
    none, _, _, n3 = capi.trace_host(reads, [unit], 3, 24, cap=0)
    assert n3 == n and len(none) == 0
    # counts and records may be NULL; a min_score above every score gives no items
    lib = capi.load()
    words, offsets, lengths = capi.pack_reads(reads)
    arr, nm = capi._motif_array([unit])
    got = C.c_uint64(0)
    assert lib.trew_trace_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, 3, 24, None, 0, C.byref(got), None, None) == 0
    assert got.value == n
    top = int(max(records["score_fwd"].max(), records["score_rev"].max()))
    assert capi.trace_host(reads, [unit], 3, top + 1)[3] == 0 and capi.trace_host(reads, [unit], 3, top)[3] > 0


def test_signature_formatter():
    read = "ACGTACGT" + T10[:27] + "C" + T10[28:40] + T10[41:] + "ACGT"
    items, _, _, _ = capi.trace_host([read], ["GGGTTA"], 3, 24)
    fwd = items[items["strand"] == 0]
    assert capi.trace_signature(fwd, read, 6) == (9, 2, "tta =4 CGGTTA =1 GGTTA =2 ggg")
    assert T.signature(read, 6, 0, [tup(it) for it in fwd]) == (9, 2, "tta =4 CGGTTA =1 GGTTA =2 ggg")
    # strand rev: the items stay in read order, the bases of each are reverse-complemented
    rc = revcomp(read)
    items, _, _, _ = capi.trace_host([rc.encode()], ["GGGTTA"], 3, 24)
    rev = items[items["strand"] == 1]
    assert capi.trace_signature(rev, rc.encode(), 6) == T.signature(rc, 6, 1, [tup(it) for it in rev])
    assert capi.trace_signature(rev, rc, 6) == (9, 2, "ggg =2 GGTTA =1 CGGTTA =4 tta")
    assert capi.trace_signature(rev[:0], rc, 6) == (0, 0, "")


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path):
    exe = str(tmp_path / "trace_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "trace_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    sets = fuzz_sets()
    reads = [r.upper().encode() for _, rs in sets[::3] for r in rs[:3]] + [b"", b"A", TEL.encode() * 400]
    motifs = [sets[0][0], TEL, sets[-2][0], sets[-1][0]]
    assert [len(m) for m in motifs] == [3, 6, 31, 32]

    def text(items, counts, records):
        return ("".join(" ".join(str(int(v)) for v in it) + "\n" for it in items) + "".join("%d " % c for c in counts.reshape(-1)) + "\n"
                + "".join(" ".join(str(int(x[f])) for f in R.FIELDS) + "\n" for x in records.reshape(-1)))

    for penalty, min_score, cap in ((1, 24, 1 << 20), (3, 24, 1 << 20), (64, 10, 1 << 20), (3, 24, 7), (3, 24, 0)):
        r = subprocess.run([exe, str(penalty), str(min_score), str(cap), ",".join(motifs)], input=b"".join(x + b"\n" for x in reads),
                           capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        items, counts, records, n = capi.trace_host(reads, motifs, penalty, min_score)
        assert n > (100 if penalty < 64 else 5)
        assert r.stdout.decode() == "%d\n" % n + text(items[:cap], counts, records)
    r = subprocess.run([exe, "3", "24", "4", TEL], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0\n0 0 0 0 \n" + b"0 0 0 0 0 0 0 0 0 0\n" * 2 and r.stderr == b""


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.TraceItem) == 48 and capi.TRACE_DTYPE.itemsize == 48
    assert tuple(capi.TRACE_DTYPE.names) == T.ITEM_FIELDS == tuple(n for n, _ in capi.TraceItem._fields_)
    assert C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Alignment) == 40
    for sym in ("trew_hip_trace", "trew_hip_trace_results", "trew_trace_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.trace_host(reads, ["AAT"], penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.trace_host(reads, ["AAT"], 3, 0)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.trace_host(reads, ["AAT"] * 9)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.trace_host(reads, [])
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.trace_host(reads, [capi.Motif(33, 0, 0)])
    with pytest.raises(capi.TrewHipError, match="bits above 2k"):
        capi.trace_host(reads, [capi.Motif(3, 0, 64)])
    lib = capi.load()
    arr, nm = capi._motif_array(["AAT"])
    n = C.c_uint64(0)
    assert lib.trew_trace_host(None, None, None, 1, arr, nm, 3, 24, None, 0, C.byref(n), None, None) != 0
    assert b"trew_trace_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_trace_host(None, None, None, 0, arr, nm, 3, 24, None, 0, None, None, None) != 0
    assert lib.trew_trace_host(None, None, None, 0, arr, nm, 3, 24, None, 4, C.byref(n), None, None) != 0  # a capacity without a buffer
    assert lib.trew_trace_host(None, None, None, 0, arr, nm, 3, 24, None, 0, C.byref(n), None, None) == 0 and n.value == 0  # no reads


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched"""
    lib = capi.load()
    arr, nm = capi._motif_array([TEL])
    n, rows = C.c_uint64(7), C.c_uint64(9)
    assert lib.trew_hip_trace(None, None, 0, arr, nm, 3, 24, 16, 16) == -1
    assert lib.trew_hip_trace_results(None, 0, None, 0, C.byref(n), C.byref(rows), None, None, None) == -1 and (n.value, rows.value) == (7, 9)


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_trace.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.trace([b"TTAGGGTTAGGG"], [TEL])
    r = subprocess.run([TREW, "trace", TEL, FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["trace"], "MOTIF is required."),
        (["trace", "TTAGGG"], "FASTQ is required."),
        (["trace", "TTAGGN", FQ], "must consist of A, C, G and T."),
        (["trace", "TTAGGG,", FQ], "the length must be in range 3 to 32."),
        (["trace", "AC", FQ], "the length must be in range 3 to 32."),
        (["trace", "A" * 33, FQ], "the length must be in range 3 to 32."),
        (["trace", ",".join(["AAT"] * 9), FQ], "At most 8 motifs can be given."),
        (["trace", "TTAGGG", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["trace", "TTAGGG", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["trace", "TTAGGG", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["trace", "TTAGGG", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["trace", "TTAGGG", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["trace", "TTAGGG", FQ, "--items", "3"], "3 : file not found"),
        (["trace", "TTAGGG", FQ, "-t", "0"], "number of threads must be positive."),
        (["trace", "TTAGGG", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["trace", "TTAGGG", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["trace", "TTAGGG", FQ, "--devices", "0,x"], "Usage: trace"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: trace" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_trace():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "trace" in r.stderr and "align" in r.stderr and "short" in r.stderr and "long" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  trace " in r.stderr
    r = subprocess.run([TREW, "trace", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: trace" in r.stderr and "--penalty" in r.stderr and "--min_score" in r.stderr and "--items" in r.stderr and r.stdout == ""
