"""tandems, decompose and dissect with resolve's period choice per piece (trew_hip_tandems_resolved, trew_hip_decompose_resolved,
trew_hip_dissect_resolved) without a GPU: the two forms of the reference against each other, the three host
definitions against the reference at penalties 1, 3 and 64 and one to four candidates, one candidate against the plain host
functions word for word, the hand vectors, the purpose (planted long units found that the plain measures cut into copies of a
wrong unit), the consequences the header states, the stand-alone harness under sanitizers, the ABI and the argument errors of
the library and of the three commands."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import dissect_cases as DC
import period_ref as P
import resolve_cases as VC
import resolved_cases as RC
import resolved_ref as X
import tandem_cases as TC
import tandem_ref as T
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
PARAMS = ((1, 24), (3, 24), (64, 10))  # (penalty, min_score)
CS = (1, 2, 3, 4)


def rec(x):
    return tuple(int(v) for v in x)


def same_arrays(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s: %s differs at %d: got %s, want %s" % (what, f, bad[0], got[bad[0]], want[bad[0]])


def same_tandems(got, want):
    """(records, counts, ...) of the library against resolved_ref.tandems' (records, counts)"""
    same_arrays(got[0], want[0], "tandems")
    assert got[1].tolist() == want[1].tolist()


def same_decompose(got, want):
    """(items, counts, records, ...) against resolved_ref.decompose's"""
    same_arrays(got[2], want[2], "decompose records")
    assert got[1].tolist() == want[1].tolist()
    same_arrays(got[0], want[0], "decompose items")


def same_dissect(got, want):
    """(records, items, counts, n_records, n_items, n_rows) against resolved_ref.dissect's (records, items, counts, rows)"""
    same_arrays(got[0], want[0], "dissect records")
    assert got[2].tolist() == want[2].tolist()
    same_arrays(got[1], want[1], "dissect items")
    assert got[3:6] == (len(want[0]), len(want[1]), want[3])


def short_reads():
    """short enough for the cell-by-cell form: the hand vectors of tandems, dissect and resolve, the reads whose candidates tie,
    share a seed or are repaired, and random ones with different candidate counts"""
    return ([r for r, _ in TC.HAND] + DC.HAND_READS + DC.short_unit_reads() + [VC.SHORT_REPAIRED, VC.SCORE_TIE, VC.ROTATED_SEED, VC.N_IN_SEED]
            + [r for r, _, _, _ in VC.HAND] + VC.mixed_reads(31, 24))


@pytest.fixture(scope="module")
def long_units():
    """(planted, reads, {C: resolved_ref.tandems}) of the long-unit two-tract set, computed once"""
    fs = RC.long_unit_set()
    reads = [r for r, _ in fs]
    return [p for _, p in fs], reads, {c: X.tandems(reads, *RC.ARGS, c) for c in (1, 3)}


# ---- the reference's two forms, and the host definitions against them
@pytest.mark.parametrize("penalty,min_score", PARAMS)
def test_reference_forms_agree_and_the_host_definitions_equal_them(penalty, min_score):
    reads = short_reads()
    for c in CS:
        args = (1, 32, penalty, min_score, c)
        want_t, want_d, want_x = X.tandems(reads, *args), X.decompose(reads, *args), X.dissect(reads, *args)
        same_tandems(X.tandems(reads, *args, depth_first=True), want_t)
        same_decompose(X.decompose(reads, *args, depth_first=True), want_d)
        deep = X.dissect(reads, *args, depth_first=True)
        same_dissect(deep[:3] + (len(deep[0]), len(deep[1]), deep[3]), want_x)
        same_tandems(capi.tandems_host(reads, *args[:4], candidates=c), want_t)
        same_decompose(capi.decompose_host(reads, *args[:4], candidates=c), want_d)
        same_dissect(capi.dissect_host(reads, *args[:4], candidates=c), want_x)


def test_one_candidate_is_the_plain_measure_word_for_word():
    """the resolved entry points at C = 1 (called as such: capi takes the plain path for candidates = 1) against the plain host
    functions, on the hand vectors, the two-tract set, the case sets of dissect_cases.py and random reads"""
    rnd = random.Random(5)
    reads = ([r for r, _ in TC.HAND] + [r for r, _ in TC.two_tract_set()][::3] + DC.HAND_READS + DC.short_unit_reads() + DC.three_tract_reads()
             + DC.child_block_reads()[::9] + VC.mixed_reads(7, 40) + ["".join(rnd.choice("ACGTN") for _ in range(rnd.randint(0, 300))) for _ in range(20)])
    lib = capi.load()
    words, offsets, lengths = capi.pack_reads(reads)
    n = len(offsets)
    for penalty, min_score in PARAMS:
        head = (words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, n, 1, 32, penalty, min_score)
        plain_t, plain_d, plain_x = (f(reads, 1, 32, penalty, min_score) for f in (capi.tandems_host, capi.decompose_host, capi.dissect_host))
        out, counts, found = np.zeros(plain_t[2] + 1, dtype=capi.TANDEM_DTYPE), np.zeros(n, dtype=np.uint32), C.c_uint64(0)
        assert lib.trew_tandems_resolved_host(*head, 1, out.ctypes.data, len(out), C.byref(found), counts.ctypes.data) == 0
        assert found.value == plain_t[2] > 0 and out[:found.value].tobytes() == plain_t[0].tobytes() and counts.tobytes() == plain_t[1].tobytes()
        items, refined, n_items = np.zeros(plain_d[3] + 1, dtype=capi.TRACE_DTYPE), np.zeros(n, dtype=capi.REFINE_DTYPE), C.c_uint64(0)
        assert lib.trew_decompose_resolved_host(*head, 1, items.ctypes.data, len(items), C.byref(n_items), counts.ctypes.data, refined.ctypes.data) == 0
        assert n_items.value == plain_d[3] > 0 and items[:n_items.value].tobytes() == plain_d[0].tobytes()
        assert counts.tobytes() == plain_d[1].tobytes() and refined.tobytes() == plain_d[2].tobytes()
        recs, items, counts2 = np.zeros(plain_x[3] + 1, dtype=capi.TANDEM_DTYPE), np.zeros(plain_x[4] + 1, dtype=capi.TRACE_DTYPE), np.zeros((n, 2), dtype=np.uint32)
        nr, ni, nw = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        assert lib.trew_dissect_resolved_host(*head, 1, recs.ctypes.data, len(recs), items.ctypes.data, len(items), C.byref(nr), C.byref(ni), C.byref(nw),
                                              counts2.ctypes.data) == 0
        assert (nr.value, ni.value, nw.value) == plain_x[3:] and recs[:nr.value].tobytes() == plain_x[0].tobytes()
        assert items[:ni.value].tobytes() == plain_x[1].tobytes() and counts2.tobytes() == plain_x[2].tobytes()
        # and the reference at one candidate is the plain reference
        few = reads[:20]
        same_tandems(X.tandems(few, 1, 32, penalty, min_score, 1), T.tandems(few, 1, 32, penalty, min_score))


# ---- hand vectors
def rows_of(read, c):
    got, counts, found = capi.tandems_host([read], candidates=c)
    want = sorted(X.tandems_read(read, *RC.ARGS, c), key=lambda x: x[1 + T.START])
    assert [rec(x)[1:] for x in got] == want and counts.tolist() == [len(want)] == [found]
    return want


def test_hand_vectors():
    tel36 = (6, 6, 6, 0, 36, 64, 100, 36, 36, 36, 36, 0, 213, 213)
    for c in CS:
        assert rows_of(TC.WEAK, c) == []  # three candidates, all scoring 23: no row at any C
        assert rows_of(TC.WEAK_FIRST, c) == [((0,) if c >= 3 else (1,)) + tel36]  # candidate 2 of the whole read wins at depth 0
        assert rows_of(TC.STRONG_FIRST, c) == dict(TC.HAND)[TC.STRONG_FIRST]
        assert rows_of(TC.TWO_PERFECT, c) == dict(TC.HAND)[TC.TWO_PERFECT]  # the multiples tie and candidate 0 keeps it
        for read in ("", "A", "AC", "ACG", "AAA"):
            assert rows_of(read, c) == []
            assert capi.decompose_host([read], candidates=c)[3] == 0 and capi.dissect_host([read], candidates=c)[3:] == (0, 0, 0)
    m, w, first = X.resolved_read(TC.WEAK, *RC.ARGS, 3)
    assert m == 3 and w[T.SCORE] == 23 and (first[T.P_START], first[T.P_END]) == (0, 60)
    assert capi.resolve_host([TC.WEAK_FIRST])[0]["rank"] == 2
    assert rows_of("A" * 40, 3) == [(0, 1, 1, 1, 0, 40, 0, 40, 40, 40, 40, 40, 0, 3, 3)]


# ---- the purpose
def unit_key(text):
    return len(text), P.canonical(P.pack_unit([P.CODE[c] for c in text]), len(text))


def found_units(planted, recs):
    """the (read, planted tract) pairs whose unit is the unit of a record of the read, compared as canonical"""
    out = set()
    for i, pl in enumerate(planted):
        mine = recs[recs["read"] == i]
        keys = {(int(x["period"]), P.canonical(x["unit"], int(x["period"]))) for x in mine}
        out |= {(i, q) for q, (u, _, _) in enumerate(pl) if unit_key(u) in keys}
    return out


def test_planted_long_units_are_gained_and_none_is_lost(long_units):
    """Two noisy tracts a read, units of 13 .. 32 bases (resolved_cases.long_unit_set, seed 20251020, 30 reads = 60 planted units),
    by the reference alone: with one candidate (= tandems) 47 planted units are the unit of a row, with three 50; 3 gained, none
    lost; both units of a read in 18 reads, then 21; 60 rows either way.  Required: none lost, at least 2 gained.  Then the
    library equals the reference record for record."""
    planted, reads, ref = long_units
    one, three = found_units(planted, ref[1][0]), found_units(planted, ref[3][0])
    print("found with 1 candidate: %d, with 3: %d, gained %d, lost %d, rows %d and %d" % (len(one), len(three), len(three - one), len(one - three),
                                                                                        len(ref[1][0]), len(ref[3][0])))
    assert not one - three
    assert len(three - one) >= 2
    both = [sum(1 for i in range(len(reads)) if (i, 0) in s and (i, 1) in s) for s in (one, three)]
    print("both units of a read: %d, then %d" % tuple(both))
    assert both[1] >= both[0]
    same_tandems(T.tandems(reads, *RC.ARGS), ref[1])  # one candidate is tandem_ref, record for record
    for c in (1, 3):
        same_tandems(capi.tandems_host(reads, *RC.ARGS, candidates=c), ref[c])


# ---- consequences
def test_consequences(long_units):
    _, long_reads, _ = long_units
    reads = short_reads() + long_reads[:6] + RC.child_reads(VC.SHORT_REPAIRED)[:2]
    texts = [r.decode() if isinstance(r, bytes) else r for r in reads]
    for c in CS:
        res = capi.resolve_host(reads, *RC.ARGS, c)
        items, counts, recs, n_items = capi.decompose_host(reads, *RC.ARGS, candidates=c)
        tan, t_counts, _ = capi.tandems_host(reads, *RC.ARGS, candidates=c)
        d_recs, d_items, d_counts, nr, ni, rows = capi.dissect_host(reads, *RC.ARGS, candidates=c)
        # decompose's record is resolve's first sixteen words but for reserved
        for f in capi.REFINE_DTYPE.names:
            assert f == "reserved" or (recs[f] == res[f]).all(), f
        # a depth-0 row exactly when resolve's score reaches min_score, and then it is that record
        for i in range(len(reads)):
            top = tan[(tan["read"] == i) & (tan["depth"] == 0)]
            assert len(top) == (1 if res["score"][i] >= RC.ARGS[3] else 0)
            if len(top):
                assert all(top[f][0] == res[f][i] for f in capi.REFINE_DTYPE.names)
        # tracts are disjoint, inside the read and sorted
        for i in range(len(reads)):
            mine = tan[tan["read"] == i]
            assert (mine["start"] < mine["end"]).all() and (mine["end"][:-1] <= mine["start"][1:]).all() and (mine["end"] <= len(reads[i])).all()
        # dissect's records are tandems' with the anchor
        assert len(d_recs) == len(tan) and (d_counts[:, 0] == t_counts).all()
        for f in capi.TANDEM_DTYPE.names:
            assert f == "reserved" or (d_recs[f] == tan[f]).all(), f
        assert (d_recs["reserved"] < d_recs["period"]).all() and rows == int((d_recs["end"] - d_recs["start"]).sum())
        # items tile each tract and their errors add up to the row's columns
        tract = {}
        for x in d_recs:
            i = int(x["read"])
            t = tract[i] = tract.get(i, -1) + 1
            its = d_items[(d_items["read"] == i) & (d_items["motif"] == t)]
            assert len(its) and its["start"][0] == x["start"] and its["start"][-1] + its["bases"][-1] == x["end"]
            assert (its["start"][1:] == its["start"][:-1] + its["bases"][:-1]).all()
            col = capi.refine_columns(x, RC.ARGS[2])
            assert int(its["consumed"].sum()) == x["consumed"] and int(its["mismatches"].sum()) == col["mismatches"]
            assert int(its["insertions"].sum()) == col["insertions"] and int(its["deletions"].sum()) == col["deletions"]
        # every record of period >= 3 (a motif has at least three bases) is the alignment of its piece against its unit
        where = []
        X.tandems_rounds(texts, *RC.ARGS, c, where=where)
        assert len(where) == len(tan)
        checked = 0
        for i, lo, hi, x in where:
            k = x[0]
            if k < 3:
                continue
            a = capi.align_host([texts[i][lo:hi]], [P.unit_text(x[12], k)], RC.ARGS[2])[0, 0]
            assert (a["score_fwd"], a["start_fwd"] + lo, a["end_fwd"] + lo, a["consumed_fwd"], a["matches_fwd"]) == x[4:9]
            checked += 1
        assert checked >= 20


# ---- the stand-alone harness under sanitizers
def test_definitions_run_clean_under_sanitizers_and_agree_with_the_library(tmp_path, long_units):
    exe = str(tmp_path / "resolved_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "resolved_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.upper().encode() for r in short_reads() + long_units[1][:3] + RC.child_reads(VC.SHORT_REPAIRED)[2:4] + ["A" * 50, "TG" * 40, "TTAGGG" * 400]]
    text = b"".join(x + b"\n" for x in reads)

    def lines(arr, fields=None):
        return "".join(" ".join(str(int(x[f])) for f in (fields or arr.dtype.names)) + "\n" for x in arr)

    def tail(counts):
        return "".join("%d " % c for c in counts.reshape(-1)) + "\n"

    for args, c, rec_cap, item_cap in (((1, 32, 1, 24), 2, 1 << 16, 1 << 20), ((1, 32, 3, 24), 3, 1 << 16, 1 << 20), ((1, 32, 64, 10), 4, 1 << 16, 1 << 20),
                                       ((5, 32, 3, 24), 3, 3, 7), ((1, 32, 3, 24), 1, 0, 0), ((1, 32, 3, 24), 4, 0, 9)):
        def run(measure):
            r = subprocess.run([exe, measure, *[str(a) for a in args], str(c), str(rec_cap), str(item_cap)], input=text, capture_output=True, timeout=300)
            assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
            return r.stdout.decode()

        recs, counts, found = capi.tandems_host(reads, *args, candidates=c)
        assert found > 20 and run("tandems") == "%d\n" % found + lines(recs[:rec_cap]) + tail(counts)
        items, counts, refined, n_items = capi.decompose_host(reads, *args, candidates=c)
        assert n_items > 20 and run("decompose") == "%d\n" % n_items + lines(refined) + lines(items[:item_cap]) + tail(counts)
        recs, items, counts, nr, ni, rows = capi.dissect_host(reads, *args, candidates=c)
        assert nr == found and run("dissect") == "%d %d %d\n" % (nr, ni, rows) + lines(recs[:rec_cap]) + lines(items[:item_cap]) + tail(counts)
    r = subprocess.run([exe, "dissect", "1", "32", "3", "24", "3", "4", "4"], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0 0 0\n0 0 0 0 \n" and r.stderr == b""
    for measure in ("tandems", "decompose", "dissect"):
        for c in ("0", "5"):
            r = subprocess.run([exe, measure, "1", "32", "3", "24", c, "4", "4"], input=b"ACGT\n", capture_output=True, timeout=60)
            assert r.returncode == 3 and b"resolve: 1 <= candidates <= 4 is required" in r.stderr


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "trew_hip.h")).read()
    assert "#define TREW_HIP_ABI_VERSION 4" in hdr
    for name in ("tandems", "decompose", "dissect"):
        for sym in ("trew_hip_%s_resolved" % name, "trew_%s_resolved_host" % name):
            assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None and "int %s(" % sym in hdr
    import trew_amd

    assert trew_amd.tandems is capi.tandems and trew_amd.decompose is capi.decompose and trew_amd.dissect is capi.dissect


def test_candidates_out_of_range_are_argument_errors():
    reads = [b"TTAGGG" * 10]
    for c in (0, 5, -1):
        for f in (capi.tandems_host, capi.decompose_host, capi.dissect_host):
            with pytest.raises(capi.TrewHipError, match="resolve: 1 <= candidates <= 4 is required"):
                f(reads, candidates=c)
    # the sibling's checks come first, with its texts
    with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
        capi.tandems_host(reads, 0, 32, candidates=5)
    with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
        capi.dissect_host(reads, 1, 32, 0, candidates=5)
    lib = capi.load()
    n, m = C.c_uint64(0), C.c_uint64(0)
    assert lib.trew_tandems_resolved_host(None, None, None, 1, 1, 32, 3, 24, 3, None, 0, C.byref(n), None) != 0
    assert b"trew_tandems_resolved_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_decompose_resolved_host(None, None, None, 1, 1, 32, 3, 24, 3, None, 0, C.byref(n), None, None) != 0
    assert b"trew_decompose_resolved_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_dissect_resolved_host(None, None, None, 1, 1, 32, 3, 24, 3, None, 0, None, 0, C.byref(n), C.byref(m), None, None) != 0
    assert b"trew_dissect_resolved_host: null argument" in lib.trew_hip_last_error(None)
    # the device calls without a context: status -1, nothing touched
    assert lib.trew_hip_tandems_resolved(None, None, 0, 1, 32, 3, 24, 3, 16) == -1
    assert lib.trew_hip_decompose_resolved(None, None, 0, 1, 32, 3, 24, 3, 16, 16) == -1
    assert lib.trew_hip_dissect_resolved(None, None, 0, 1, 32, 3, 24, 3, 16, 16, 16) == -1


@pytest.mark.parametrize("command", ["tandems", "decompose", "dissect"])
def test_cli_candidates_option(command):
    for c in ("0", "5"):
        r = subprocess.run([TREW, command, FQ, "--candidates", c], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout == "" and "CANDIDATES must be in range 1 to 4." in r.stderr and "Usage: %s" % command in r.stderr
    r = subprocess.run([TREW, command, FQ, "--candidates", "x"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "CANDIDATES must be a number." in r.stderr
    r = subprocess.run([TREW, command, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "[--candidates C]" in r.stderr and "default 1" in r.stderr and r.stdout == ""
    # without a GPU both spellings of the plain command fail alike; with one, tests/test_gpu_resolved.py compares their output
    plain = subprocess.run([TREW, command, FQ], capture_output=True, text=True, timeout=120)
    one = subprocess.run([TREW, command, FQ, "--candidates", "1"], capture_output=True, text=True, timeout=120)
    assert (plain.returncode, plain.stdout) == (one.returncode, one.stdout)


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_resolved.py)
    for f in (trew_amd.tandems, trew_amd.decompose, trew_amd.dissect):
        with pytest.raises(capi.TrewHipError):
            f([b"TTAGGGTTAGGG"], candidates=3)
    r = subprocess.run([TREW, "dissect", FQ, "--candidates", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr
