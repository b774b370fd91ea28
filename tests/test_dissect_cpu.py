"""Units in place for every tract of a read, no motif given (trew_hip_dissect) without a GPU: the two forms of the
reference against each other, trew_dissect_host against the reference on the case sets of dissect_cases.py at penalties 1, 3 and
64, the consequences the header states, the records against trew_tandems_host and the items against trew_decompose_host on
every piece's substring, the capacities and counts of the host call, the stand-alone harness under sanitizers, the ABI and the
argument errors of the library and of the command line."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_ref
import decompose_ref as D
import dissect_cases as DC
import dissect_ref as X
import tandem_ref
import trace_ref as T
from trew_amd import capi

assert tuple(capi.TRACE_DTYPE.names) == T.ITEM_FIELDS and tuple(capi.TANDEM_DTYPE.names) == tandem_ref.FIELDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
PARAMS = ((1, 5), (3, 24), (64, 3))  # (penalty, min_score), those of tests/test_gpu_decompose.py


def same(got, want):
    """(records, items, counts, ..., rows) of a host or device call against dissect_ref.dissect's (records, items, counts, rows)"""
    gr, gi, gc = got[:3]
    wr, wi, wc, rows = want
    assert len(gr) == len(wr), "%d records, want %d" % (len(gr), len(wr))
    for f in wr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert len(bad) == 0, "record field %s differs at %d: got %s, want %s" % (f, bad[0], gr[bad[0]], wr[bad[0]])
    assert gc.shape == wc.shape and (gc == wc).all()
    assert len(gi) == len(wi), "%d items, want %d" % (len(gi), len(wi))
    bad = np.flatnonzero(gi != wi)
    assert len(bad) == 0, "item %d differs: got %s, want %s" % (bad[0], gi[bad[0]], wi[bad[0]])
    assert got[-1] == rows and got[-3] == len(wr) and got[-2] == len(wi)


def sets():
    return {"hand": DC.HAND_READS, "bound": DC.bound_reads(), "blocks": DC.child_block_reads(), "short_units": DC.short_unit_reads(),
            "three": DC.three_tract_reads(), "two_tract": [r for r, _ in DC.two_tract_set()], "long": [DC.long_read()]}


@pytest.fixture(scope="module")
def two_tract():
    reads = [r for r, _ in DC.two_tract_set()]
    return reads, X.dissect(reads)


# ---- the reference
def test_reference_forms_agree():
    """the depth-first plain form against the round-by-round vectorised one on the short reads, at all three penalties"""
    reads = DC.HAND_READS + DC.short_unit_reads() + DC.three_tract_reads()[:2] + [DC.end_tie_child()[0]] + DC.child_block_reads()[::27]
    n = 0
    for penalty, min_score in PARAMS:
        a = X.dissect(reads, penalty=penalty, min_score=min_score, shape=X.dissect_read)
        b = X.dissect(reads, penalty=penalty, min_score=min_score)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and (a[2] == b[2]).all() and a[3] == b[3]
        n += len(a[0])
    assert n > 40


def test_hand_vectors():
    """tandem_cases.HAND: the records are the hand-written ones but for reserved; WEAK_FIRST's only record is at depth 1, below a
    piece with no record, no items and no rows; a read without a repeat and the empty read give nothing"""
    recs, items, counts, rows = X.dissect(DC.HAND_READS)
    got = capi.dissect_host(DC.HAND_READS)
    same(got, (recs, items, counts, rows))
    at = 0
    for i, (_, want) in enumerate(DC.HAND):
        assert counts[i, 0] == len(want)
        for w in want:
            x = tuple(int(v) for v in recs[at])
            assert x[0] == i and x[1:13] == w[:12] and x[14:] == w[13:]
            at += 1
    weak_first = DC.HAND_READS.index(DC.HAND[2][0])
    only = recs[recs["read"] == weak_first]
    assert len(only) == 1 and only["depth"][0] == 1 and rows == int((recs["end"] - recs["start"]).sum())
    assert (items["read"] == weak_first).sum() == counts[weak_first, 1] > 0
    assert (counts[[1, 4, 5]] == 0).all()


# ---- the host definition against the reference
@pytest.mark.parametrize("name", ["hand", "bound", "blocks", "short_units", "three", "two_tract", "long"])
def test_host_definition_equals_the_reference(name):
    reads = sets()[name]
    for penalty, min_score in PARAMS:
        got = capi.dissect_host(reads, 1, 32, penalty, min_score)
        same(got, X.dissect(reads, 1, 32, penalty, min_score))
        assert got[3] > 0 or name == "hand"


def check_against_parents(reads, penalty, min_score):
    """the records are trew_tandems_host's but for reserved; the depth-0 record and its items are trew_decompose_host's of the
    read.  Returns the depth-0 tracts checked."""
    recs, items, counts, n_recs, n_items, n_rows = capi.dissect_host(reads, 1, 32, penalty, min_score)
    t_recs, t_counts, t_found = capi.tandems_host(reads, 1, 32, penalty, min_score)
    assert n_recs == t_found and (counts[:, 0] == t_counts).all()
    for f in recs.dtype.names:
        assert f == "reserved" or (recs[f] == t_recs[f]).all(), f
    assert n_rows == int((recs["end"].astype(np.int64) - recs["start"]).sum()) and n_items == len(items) == int(counts[:, 1].sum())
    # depth-0 tracts: the piece is the read
    d_items, d_counts, d_recs, _ = capi.decompose_host(reads, 1, 32, penalty, min_score)
    checked = 0
    for x in recs[recs["depth"] == 0]:
        i = int(x["read"])
        mine = items[(items["read"] == i) & (items["start"] >= x["start"]) & (items["start"] < x["end"])]
        want = d_items[d_items["read"] == i]
        assert x["reserved"] == d_recs["reserved"][i] and len(mine) == len(want) == d_counts[i]
        for f in ("start", "bases", "count", "phase", "consumed", "mismatches", "insertions", "deletions", "strand"):
            assert (mine[f] == want[f]).all()
        checked += 1
    return checked


def test_consequences(two_tract):
    """what include/trew_hip.h states: the items of a tract tile [start, end) of its record; bases, consumed and errors sum to
    the record's; only the first item of a tract has a phase; motif numbers the read's tracts in start order; strand is 0; rows
    = the sum of end - start; the records equal trew_tandems_host's but for reserved; the depth-0 record and its items equal
    trew_decompose_host's; a read's output does not depend on the batch.  And of the reference alone: 60 records, two in each of
    the 30 reads at depths 0 and 1, 29 359 rows, at least 28 reads with two traced tracts."""
    reads, want = two_tract
    recs, items, counts, rows = want
    assert len(recs) == 60 and (counts[:, 0] == 2).all() and sorted(set(recs["depth"])) == [0, 1] and rows == 29359
    assert sum(1 for i in range(len(reads)) if len(set(items["motif"][items["read"] == i])) == 2) >= 28
    got = capi.dissect_host(reads)
    same(got, want)
    recs, items, counts = got[:3]
    assert (items["strand"] == 0).all() and (items["reserved"] == 0).all() and (items["bases"] >= 1).all()
    cols = capi.tandem_columns(recs, 3)
    at = 0
    for q, x in enumerate(recs):
        i = int(x["read"])
        tract = q - int(np.flatnonzero(recs["read"] == i)[0])
        mine = items[(items["read"] == i) & (items["motif"] == tract)]
        assert len(mine) and (items[at:at + len(mine)] == mine).all()  # sorted by (read, start): a tract's items are consecutive
        at += len(mine)
        assert mine["start"][0] == x["start"] and (mine["start"][1:] == (mine["start"] + mine["bases"])[:-1]).all()
        assert mine["start"][-1] + mine["bases"][-1] == x["end"]
        assert mine["bases"].sum() == x["end"] - x["start"] and mine["consumed"].sum() == x["consumed"]
        assert (mine["phase"][1:] == 0).all()
        for f in ("mismatches", "insertions", "deletions"):
            assert mine[f].sum() == cols[f][q]
        k = int(x["period"])
        m = capi.decompose_anchor(x)
        assert m == min(((int(x["unit"]) << (2 * s)) | (int(x["unit"]) >> (2 * (k - s)))) & ((1 << (2 * k)) - 1) for s in range(k))
        units, edited, sig = capi.trace_signature(mine, reads[i], k)
        assert units == int(mine["count"][mine["consumed"] == k * mine["count"]].sum()) and sig
    assert at == len(items) and got[5] == int((recs["end"] - recs["start"]).sum())
    assert check_against_parents(reads, 3, 24) == 30
    # a read alone and in another batch
    for i in (0, 7, 29):
        alone = capi.dissect_host([reads[i]])
        mine_r, mine_i = recs[recs["read"] == i].copy(), items[items["read"] == i].copy()
        mine_r["read"] = 0
        mine_i["read"] = 0
        assert alone[0].tobytes() == mine_r.tobytes() and alone[1].tobytes() == mine_i.tobytes()


def test_every_tract_equals_decompose_of_its_piece(two_tract):
    """trew_decompose_host on each piece's substring equals the tract's items, offset by the piece's first base: the depth-1
    tract of a two-tract read lies in the piece in front of the depth-0 tract or in the one behind it"""
    reads, (recs, items, counts, _) = two_tract
    n = 0
    for i, read in enumerate(reads):
        mine = recs[recs["read"] == i]
        top = mine[mine["depth"] == 0][0]
        for t, x in enumerate(mine):
            lo, hi = (0, len(read)) if x["depth"] == 0 else (0, int(top["start"])) if x["start"] < top["start"] else (int(top["end"]), len(read))
            d_items, d_counts, d_recs, _ = capi.decompose_host([read[lo:hi]])
            want = items[(items["read"] == i) & (items["motif"] == t)]
            assert d_recs["start"][0] + lo == x["start"] and d_recs["end"][0] + lo == x["end"] and d_recs["reserved"][0] == x["reserved"]
            assert len(d_items) == len(want) and (d_items["start"] + lo == want["start"]).all()
            for f in ("bases", "count", "phase", "consumed", "mismatches", "insertions", "deletions"):
                assert (d_items[f] == want[f]).all()
            n += 1
    assert n == 60


def test_end_phase_tie_in_a_child():
    """rule 3 decided in a child piece: by the reference the child's row `end` holds the record's tuple in the two phases of
    decompose_cases.END_TIE, and the smaller one is the end cell"""
    read, penalty, min_score, phases, first = DC.end_tie_child()
    want = X.dissect([read], 1, 32, penalty, min_score)
    recs = want[0]
    assert len(recs) == 2 and list(recs["depth"]) == [0, 1] and recs["start"][0] == 0
    lo = int(recs["end"][0])  # the child piece is [lo, n)
    assert first <= lo < int(recs["start"][1])
    piece = read[lo:]
    r, its = D.decompose_read(piece, 1, 32, penalty, min_score)
    assert r[5] + lo == recs["start"][1] and r[6] + lo == recs["end"][1] and r[11] == recs["reserved"][1]
    M = D.anchor(D.unit_codes(r[12], r[0]))[1]
    for row0, row_end in ((0, None), (r[5], r[6])):  # the full table of the piece and the restarted one
        ties = {}
        arec, jstar, _, _ = T.table(align_ref.codes(piece), M, penalty, row0=row0, row_end=row_end, ties=ties)
        assert arec == r[4:9] and ties["end"] == phases and jstar == phases[0]
    assert len(its) >= 3
    same(capi.dissect_host([read], 1, 32, penalty, min_score), want)


def test_caps_and_counts_of_the_host_call(two_tract):
    """*n_records, *n_items and *n_rows are exact whatever the capacities, the counts always; the buffers get the first ones of
    the sorted orders and nothing beyond their capacity"""
    reads, want = two_tract
    full = capi.dissect_host(reads)
    for rec_cap, item_cap in ((0, 0), (1, 1), (7, 100), (60, 3263), (59, 4000), (1000, 5000)):
        recs, items, counts, nr, ni, rows = capi.dissect_host(reads, rec_cap=rec_cap, item_cap=item_cap)
        assert (nr, ni, rows) == (60, len(want[1]), want[3]) and (counts == want[2]).all()
        assert len(recs) == min(rec_cap, 60) and len(items) == min(item_cap, ni)
        assert recs.tobytes() == full[0][:rec_cap].tobytes() and items.tobytes() == full[1][:item_cap].tobytes()
    # raw: the words behind the capacity stay as they were
    lib = capi.load()
    words, offsets, lengths = capi._packed(reads)
    recs = np.full(72 * 4, 0xA5, dtype=np.uint8).view(capi.TANDEM_DTYPE)
    items = np.full(48 * 6, 0xA5, dtype=np.uint8).view(capi.TRACE_DTYPE)
    nr, ni = C.c_uint64(0), C.c_uint64(0)
    assert lib.trew_dissect_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), 1, 32, 3, 24, recs.ctypes.data, 3,
                                 items.ctypes.data, 5, C.byref(nr), C.byref(ni), None, None) == 0
    assert (nr.value, ni.value) == (60, len(want[1]))
    assert recs[:3].tobytes() == full[0][:3].tobytes() and recs[3:].tobytes() == b"\xa5" * 72
    assert items[:5].tobytes() == full[1][:5].tobytes() and items[5:].tobytes() == b"\xa5" * 48


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path):
    exe = str(tmp_path / "dissect_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "dissect_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.upper().encode() for r in ([r for r, _ in DC.two_tract_set()][::5] + DC.HAND_READS + DC.short_unit_reads() + DC.three_tract_reads()
                                          + DC.child_block_reads()[::9] + DC.bound_reads()[::17] + ["A", "A" * 50, "TG" * 40, "TTAGGG" * 400])]

    def text(recs, items, counts):
        return ("".join(" ".join(str(int(x[f])) for f in tandem_ref.FIELDS) + "\n" for x in recs)
                + "".join(" ".join(str(int(v)) for v in it) + "\n" for it in items) + "".join("%d " % c for c in counts.reshape(-1)) + "\n")

    for args, rec_cap, item_cap in (((1, 32, 1, 24), 1 << 16, 1 << 20), ((1, 32, 3, 24), 1 << 16, 1 << 20), ((1, 32, 64, 10), 1 << 16, 1 << 20),
                                    ((5, 32, 3, 24), 3, 7), ((1, 32, 3, 24), 0, 0), ((1, 32, 3, 24), 0, 9)):
        r = subprocess.run([exe, *[str(a) for a in args], str(rec_cap), str(item_cap)], input=b"".join(x + b"\n" for x in reads), capture_output=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        recs, items, counts, nr, ni, rows = capi.dissect_host(reads, *args)
        assert nr > (30 if args[2] < 64 else 5) and ni >= nr
        assert r.stdout.decode() == "%d %d %d\n" % (nr, ni, rows) + text(recs[:rec_cap], items[:item_cap], counts)
    r = subprocess.run([exe, "1", "32", "3", "24", "4", "4"], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0 0 0\n0 0 0 0 \n" and r.stderr == b""
    r = subprocess.run([exe, "0", "32", "3", "24", "4", "4"], input=b"ACGT\n", capture_output=True, timeout=60)
    assert r.returncode == 3 and b"min_period" in r.stderr


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.TraceItem) == 48 and capi.TANDEM_DTYPE.itemsize == 72
    for sym in ("trew_hip_dissect", "trew_hip_dissect_results", "trew_dissect_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    hdr = open(os.path.join(ROOT, "include", "trew_hip.h")).read()
    assert "#define TREW_HIP_ABI_VERSION 4" in hdr and "int trew_hip_dissect(" in hdr and "int trew_hip_dissect_results(" in hdr
    import trew_amd

    assert trew_amd.dissect is capi.dissect


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 32), (1, 33), (7, 6)):
        with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
            capi.dissect_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.dissect_host(reads, 1, 32, penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.dissect_host(reads, 1, 32, 3, 0)
    lib = capi.load()
    n, m = C.c_uint64(0), C.c_uint64(0)
    assert lib.trew_dissect_host(None, None, None, 1, 1, 32, 3, 24, None, 0, None, 0, C.byref(n), C.byref(m), None, None) != 0
    assert b"trew_dissect_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_dissect_host(None, None, None, 0, 1, 32, 3, 24, None, 0, None, 0, None, C.byref(m), None, None) != 0
    assert lib.trew_dissect_host(None, None, None, 0, 1, 32, 3, 24, None, 0, None, 0, C.byref(n), None, None, None) != 0
    assert lib.trew_dissect_host(None, None, None, 0, 1, 32, 3, 24, None, 4, None, 0, C.byref(n), C.byref(m), None, None) != 0  # a capacity without a buffer
    assert lib.trew_dissect_host(None, None, None, 0, 1, 32, 3, 24, None, 0, None, 4, C.byref(n), C.byref(m), None, None) != 0
    assert lib.trew_dissect_host(None, None, None, 0, 1, 32, 3, 24, None, 0, None, 0, C.byref(n), C.byref(m), None, None) == 0 and n.value == m.value == 0


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched"""
    lib = capi.load()
    a, b, c = C.c_uint64(7), C.c_uint64(8), C.c_uint64(9)
    assert lib.trew_hip_dissect(None, None, 0, 1, 32, 3, 24, 16, 16, 16) == -1
    assert lib.trew_hip_dissect_results(None, 0, None, 0, None, 0, C.byref(a), C.byref(b), C.byref(c), None, None) == -1
    assert (a.value, b.value, c.value) == (7, 8, 9)


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_dissect.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.dissect([b"TTAGGGTTAGGG"])
    r = subprocess.run([TREW, "dissect", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["dissect"], "FASTQ is required."),
        (["dissect", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["dissect", FQ, "--max_period", "33"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["dissect", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["dissect", FQ, "--min_period", "x"], "MIN_PERIOD must be a number."),
        (["dissect", FQ, "--max_period", "x"], "MAX_PERIOD must be a number."),
        (["dissect", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["dissect", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["dissect", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["dissect", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["dissect", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["dissect", FQ, "--items", "3"], "3 : file not found"),
        (["dissect", FQ, "-t", "0"], "number of threads must be positive."),
        (["dissect", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["dissect", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["dissect", FQ, "--devices", "0,x"], "Usage: dissect"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: dissect" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_dissect():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "dissect" in r.stderr and "decompose" in r.stderr and "tandems" in r.stderr and "short" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  dissect " in r.stderr
    r = subprocess.run([TREW, "dissect", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: dissect" in r.stderr and "--penalty" in r.stderr and "--min_period" in r.stderr and "--items" in r.stderr and r.stdout == ""
