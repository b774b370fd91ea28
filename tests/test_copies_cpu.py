"""CPU-only checks of the traceback for units of up to 256 bases (trew_hip_copies): the one-bit direction
against (op, d) of the O(n k^2) definition on every cell, the host definition against the brute-force reference on a fuzz set
of k from 33 to 256 and against trew_trace_host and trew_monomers_host, the consequences of the definition at k > 32, the
tie reads, cap and count, both signature forms, the stand-alone sanitizer harness, the additive ABI, and the argument errors
of the C ABI and of `trew copies`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_ref as A
import copies_cases as CC
import copies_ref as R
import monomer_ref as M
import trace_ref as T
from align_cases import TEL, fuzz_sets, revcomp
from period_cases import junk, noisy
from trew_amd import capi

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
    for f in T.ITEM_FIELDS:
        bad = np.flatnonzero(gi[f] != wi[f])
        assert len(bad) == 0, "item %d differs in %s: got %s, want %s" % (bad[0], f, gi[bad[0]], wi[bad[0]])


def tup(it):
    return tuple(int(v) for v in it)[3:11]


@pytest.fixture(scope="module")
def fuzz():
    """[(unit, reads, copies_keys at P = 3 and min_score 24)] of copies_cases.host_fuzz, the O(n k^2) reference computed once"""
    return [(unit, reads, R.copies_keys(reads, [unit], 3, 24)) for unit, reads in CC.host_fuzz()]


# ---- one bit in the place of d
def check_bits(x, t, P, op, dd):
    """(op, d) of the definition against the del-bit form on every cell; returns the cells with d > 1"""
    rec, jstar, op2, dl = R.del_table(x, t, P)
    k, deep = len(t), 0
    for i in range(1, len(x) + 1):
        for j in range(k):
            assert op2[i][j] == op[i][j], (i, j)
            assert R.d_of_bits(dl[i], j) == dd[i][j], (i, j, dd[i][j])
            deep += dd[i][j] > 1
    return rec, jstar, deep


@pytest.mark.parametrize("k", [3, 6, 32, 33, 64, 65])
def test_del_bit_recovers_d_of_the_definition_on_every_cell(k):
    """trace_ref.table is the definition cell by cell in plain Python; copies_ref.table the same with numpy over (d, j); the
    bits of copies_ref.del_table give d back by following them.  Reads of at most 4 k bases, P = 1, 3, 64."""
    rnd = random.Random(300 + k)
    unit = CC.unit_of(k, 1)
    t = M.strand_codes(unit, 0)
    n = 4 * k if k < 32 else 2 * k + k // 2
    reads = [noisy(rnd, unit, n - 8, 0.04, 0.10, 0.01)[:n - 4] + junk(rnd, 4), junk(rnd, 3, "ACGTN") + noisy(rnd, unit, n - 10, 0.02, 0.05)[:n - 3]]
    deep = 0
    for P in (1, 3, 64):
        for read in reads:
            x = A.codes(read)
            assert len(x) <= 4 * k
            rec, jstar, op, dd = T.table(x, t, P)
            rec2, j2, op2, dd2, _, _ = R.table(x, t, P)
            assert (rec2, j2) == (rec, jstar)
            for i in range(1, len(x) + 1):
                assert list(op2[i]) == op[i] and list(dd2[i]) == dd[i], i
            rec3, j3, d = check_bits(x, t, P, op, dd)
            assert (rec3, j3) == (rec, jstar)
            deep += d
    assert deep > 0  # cells whose d needs more than one step


@pytest.mark.parametrize("k", [171, 256])
def test_del_bit_recovers_d_at_the_large_k(k):
    """one read of about k + 60 bases, P = 3, every cell, against copies_ref.table; the host's items are the reference's"""
    rnd = random.Random(400 + k)
    unit = CC.unit_of(k, 2)
    read = junk(rnd, 6) + noisy(rnd, unit, k + 50, 0.03, 0.08, 0.005) + junk(rnd, 6)
    x, t = A.codes(read), M.strand_codes(unit, 0)
    rec, jstar, op, dd, _, _ = R.table(x, t, 3)
    rec2, j2, deep = check_bits(x, t, 3, op, dd)
    assert (rec2, j2) == (rec, jstar) and rec[0] > 24 and deep > 0
    same(capi.copies_host([read], [unit], 3, 24), R.copies([read], [unit], 3, 24))


# ---- the host definition
def test_host_against_reference_on_the_fuzz_set(fuzz):
    """field for field; and the fuzz set is what it is meant to be: by the reference alone more than half of the keys carry a
    D/I tie or a d tie on the traced path, and both strands are traced"""
    assert tuple(len(u) for u, _, _ in fuzz) == CC.HOST_KS
    keys = tied = 0
    strands = set()
    for unit, reads, ref in fuzz:
        want = R.copies(reads, [unit], 3, 24, keys=ref)
        got = capi.copies_host(reads, [unit], 3, 24)
        same(got, want)
        assert got[3] == len(want[0]) and got[4] == want[3]
        for (r, m, s), (_, _, _, (di, dt)) in ref[0].items():
            keys += 1
            tied += di or dt
            strands.add(s)
    assert keys >= 2 * len(CC.HOST_KS) - 2 and strands == {0, 1}
    assert 2 * tied > keys, (tied, keys)


@pytest.mark.parametrize("penalty", [1, 64])
def test_host_against_reference_at_other_penalties(penalty):
    for unit, reads in CC.host_fuzz()[:4]:
        same(capi.copies_host(reads, [unit], penalty, 10), R.copies(reads, [unit], penalty, 10))


def test_host_equals_trace_host_up_to_32_bases():
    """items, counts and records field for field, k = 3 .. 32 on trace's fuzz set, P = 1, 3, 64"""
    sets = fuzz_sets()
    assert sorted({len(u) for u, _ in sets})[0] == 3 and max(len(u) for u, _ in sets) == 32
    total = 0
    for unit, reads in sets:
        for penalty in (1, 3, 64):
            want = capi.trace_host(reads, [unit], penalty, 24)
            got = capi.copies_host(reads, [unit], penalty, 24)
            same(got, want)
            assert got[3] == want[3]
            total += got[3]
    assert total > 1000
    # several units in one call, the typed motif and the monomer side by side
    units = [sets[0][0], TEL, sets[-1][0]]
    reads = sets[5][1] + sets[-1][1]
    same(capi.copies_host(reads, units, 3, 24), capi.trace_host(reads, units, 3, 24))


def test_records_equal_monomers_host(fuzz):
    for unit, reads, _ in fuzz[::3]:
        for penalty in (1, 3):
            got = capi.copies_host(reads, [unit, TEL], penalty, 24)[2]
            want = capi.monomers_host(reads, [unit, TEL], penalty)
            for f in M.FIELDS:
                assert (got[f] == want[f]).all()


# ---- consequences at k > 32
def test_consequences_above_32_bases(fuzz):
    """the items of a key tile [start, end); bases, consumed and the errors sum to the record's; only the first item has phase
    != 0; every item has bases >= 1; n_rows is the sum of end - start over the keys with items"""
    keys = 0
    for unit, reads, _ in fuzz:
        k = len(unit)
        items, counts, recs, n, rows = capi.copies_host(reads, [unit], 3, 24)
        want_rows = 0
        for r in range(len(reads)):
            for s, sfx in enumerate(("_fwd", "_rev")):
                mine = items[(items["read"] == r) & (items["strand"] == s)]
                score, start, end, consumed, matches = (int(recs[f + sfx][r, 0]) for f in ("score", "start", "end", "consumed", "matches"))
                assert counts[r, 0, s] == len(mine) and (len(mine) > 0) == (score >= 24)
                if not len(mine):
                    continue
                keys += 1
                want_rows += end - start
                pos = start
                for it in mine:
                    assert int(it["start"]) == pos and int(it["bases"]) >= 1
                    pos += int(it["bases"])
                assert pos == end
                assert int(mine["consumed"].sum()) == consumed
                assert all(int(p) == 0 for p in mine["phase"][1:])
                c = A.columns(score, start, end, consumed, matches, k, 3)
                assert (int(mine["mismatches"].sum()), int(mine["insertions"].sum()), int(mine["deletions"].sum())) == (c["mismatches"], c["insertions"], c["deletions"])
        assert rows == want_rows
    assert keys > len(CC.HOST_KS)


def test_restarted_table_traces_the_same_columns(fuzz):
    """fact (b) of 4.7h does not depend on k: the table started again from (0, start, 0, 0) in row start has the record, the end
    phase and the columns of the full table, on every key of the fuzz set"""
    n = 0
    for unit, reads, (ref, _) in fuzz:
        for (r, m, s), (rec, jstar, cols, _) in ref.items():
            x, t = A.codes(reads[r]), M.strand_codes(unit, s)
            rec2, j2, op, dd, _, _ = R.table(x, t, 3, row0=rec[1], row_end=rec[2])
            assert (rec2, j2) == (rec, jstar)
            assert T.walk(x, t, rec, jstar, op, dd) == cols
            n += 1
    assert n >= 2 * len(CC.HOST_KS) - 2


# ---- tie reads
def test_end_phase_tie_above_32_bases():
    """(AAT) x 40 against (AAT) x 22: every third phase of the last row holds the end cell's tuple, the smallest one wins"""
    unit, read = CC.TIE_UNIT, CC.TIE_READ
    x, t = A.codes(read), M.strand_codes(unit, 0)
    rec, jstar, op, dd, _, _ = R.table(x, t, 3)
    assert rec == (120, 0, 120, 120, 120) and jstar == 2
    ties = {}
    T.table(x, t, 3, ties=ties)
    assert ties["end"] == list(range(2, 66, 3))
    items, counts, _, n, rows = capi.copies_host([read], [unit], 3, 24)
    # the last base sits at phase 2, so the first at phase (2 - 119) mod 66 = 15: a piece of 51, a whole copy, a piece of 3
    assert n == 3 and rows == 120
    assert [tup(it) for it in items] == [(0, 51, 1, 15, 51, 0, 0, 0), (51, 66, 1, 0, 66, 0, 0, 0), (117, 3, 1, 0, 3, 0, 0, 0)]
    same(capi.copies_host([read], [unit], 3, 24), R.copies([read], [unit], 3, 24))


def test_one_deleted_and_one_inserted_base_land_in_their_copy():
    unit = CC.edit_unit()
    k = CC.EDIT_K
    cases = CC.edit_reads(unit)
    assert len(cases) == 2 * 4 * k
    items, counts, recs, n, _ = capi.copies_host([c[0] for c in cases], [unit], 3, 24)
    for r, (read, kind, copy, p) in enumerate(cases):
        mine = [tup(it) for it in items[(items["read"] == r) & (items["strand"] == 0)]]
        edited = (copy * k, k - 1, 1, 0, k, 0, 0, 1) if kind == "del" else (copy * k, k + 1, 1, 0, k, 0, 1, 0)
        tail = 5 - copy
        want = [(0, copy * k, copy, 0, copy * k, 0, 0, 0)] if copy else []
        want += [edited, (edited[0] + edited[1], tail * k, tail, 0, tail * k, 0, 0, 0)]
        assert mine == want, (kind, p)


# ---- contract and text
def test_host_cap_and_count(fuzz):
    unit, reads, _ = fuzz[3]
    units = [unit, fuzz[4][0]]
    reads = reads + fuzz[4][1]
    items, counts, records, n, rows = capi.copies_host(reads, units, 3, 24)
    assert n == len(items) == counts.sum() and n > 8 and rows > 0
    part, counts2, records2, n2, rows2 = capi.copies_host(reads, units, 3, 24, cap=5)
    assert (n2, rows2) == (n, rows) and len(part) == 5 and (part == items[:5]).all() and (counts2 == counts).all() and (records2 == records).all()
    none, _, _, n3, _ = capi.copies_host(reads, units, 3, 24, cap=0)
    assert n3 == n and len(none) == 0
    order = [(int(it["read"]), int(it["motif"]), int(it["strand"]), int(it["start"])) for it in items]
    assert order == sorted(order)
    # counts, records and n_rows may be NULL; a min_score above every score gives no items and no rows
    lib = capi.load()
    words, offsets, lengths = capi.pack_reads(reads)
    arr, nm = capi._monomer_array(units)
    got = C.c_uint64(0)
    assert lib.trew_copies_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, 3, 24, None, 0, C.byref(got), None, None,
                                None) == 0
    assert got.value == n
    top = int(max(records["score_fwd"].max(), records["score_rev"].max()))
    assert capi.copies_host(reads, units, 3, top + 1)[3:] == (0, 0) and capi.copies_host(reads, units, 3, top)[3] > 0


def test_signature_forms():
    unit = CC.unit_of(40, 5)
    whole = unit * 6
    read = "ACGT" + whole[7:95] + whole[96:140] + "G" + whole[140:230] + "TT"
    items, _, _, _, _ = capi.copies_host([read], [unit], 3, 24)
    fwd = items[items["strand"] == 0]
    units, edited, sig = capi.copies_signature(fwd, read, 40)
    # bases 7 .. 39 of a copy, a copy, one without its base 15, one with a G in front of its base 20, a copy, 30 bases
    assert (units, edited) == (4, 2)
    assert sig == "(33:0.0.0) =1 39:0.0.1 41:0.1.0 =1 (30:0.0.0)"
    # --bases: trace's form at any k, which is also the form of k <= 32
    assert capi.copies_signature(fwd, read, 40, bases=True) == capi.trace_signature(fwd, read, 40)
    assert capi.copies_signature(fwd, read, 40, bases=True)[2].split()[2] == (whole[80:95] + whole[96:120])
    tel = "ACGTACGT" + TEL * 4 + "TTAGG" + TEL * 3
    items, _, _, _, _ = capi.copies_host([tel], [TEL], 3, 24)
    fwd = items[items["strand"] == 0]
    assert capi.copies_signature(fwd, tel, 6) == capi.trace_signature(fwd, tel, 6) == (8, 1, "=4 TTAGG =3")
    # strand rev: the items stay in read order, the counts form needs no bases
    rc = revcomp(read)
    items, _, _, _, _ = capi.copies_host([rc], [unit], 3, 24)
    rev = items[items["strand"] == 1]
    assert capi.copies_signature(rev, rc, 40) == (4, 2, "(30:0.0.0) =1 41:0.1.0 39:0.0.1 =1 (33:0.0.0)")
    assert capi.copies_signature(rev[:0], rc, 40) == (0, 0, "")


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path, fuzz):
    exe = str(tmp_path / "copies_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "copies_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.upper().encode() for _, rs, _ in fuzz[::3] for r in rs] + [b"", b"A", TEL.encode() * 50, CC.TIE_READ.encode()]
    units = [TEL, CC.TIE_UNIT] + [fuzz[i][0] for i in (0, 2, 3, 7, 9, 10)]
    assert [len(u) for u in units] == [6, 66, 33, 64, 65, 171, 255, 256]

    def text(items, counts, records):
        return ("".join(" ".join(str(int(v)) for v in it) + "\n" for it in items) + "".join("%d " % c for c in counts.reshape(-1)) + "\n"
                + "".join(" ".join(str(int(x[f])) for f in M.FIELDS) + "\n" for x in records.reshape(-1)))

    for penalty, min_score, cap in ((1, 24, 1 << 16), (3, 24, 7), (64, 10, 0)):
        r = subprocess.run([exe, str(penalty), str(min_score), str(cap), ",".join(units)], input=b"".join(x + b"\n" for x in reads), capture_output=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        items, counts, records, n, rows = capi.copies_host(reads, units, penalty, min_score)
        assert n > 4
        assert r.stdout.decode() == "%d %d\n" % (n, rows) + text(items[:cap], counts, records)
    r = subprocess.run([exe, "3", "24", "4", "A" * 256], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0 0\n0 0 0 0 \n" + b"0 0 0 0 0 0 0 0 0 0\n" * 2 and r.stderr == b""
    r = subprocess.run([exe, "3", "24", "4", "A" * 257], input=b"\n", capture_output=True, timeout=60)
    assert r.returncode == 3 and b"the length must be in [3, 256]" in r.stderr


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.TraceItem) == 48 and C.sizeof(capi.Monomer) == 72 and C.sizeof(capi.Alignment) == 40
    hdr = open(os.path.join(ROOT, "include", "trew_hip.h")).read()
    assert "#define TREW_HIP_ABI_VERSION 4" in hdr
    for sym in ("trew_hip_copies", "trew_hip_copies_results", "trew_copies_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None and "int %s(" % sym in hdr
    import trew_amd

    assert trew_amd.copies is capi.copies
    assert callable(trew_amd.TrewHip.copies) and callable(trew_amd.TrewHip.copies_results)


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.copies_host(reads, ["AAT"], penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.copies_host(reads, ["AAT"], 3, 0)
    for units in (["AAT"] * 9, []):
        with pytest.raises(capi.TrewHipError, match=r"n_monomers must be in \[1, 8\]"):
            capi.copies_host(reads, units)
    zero = (C.c_uint32 * 16)()
    for k in (2, 257, 0, -3):
        with pytest.raises(capi.TrewHipError, match=r"monomer: k must be in \[3, 256\]"):
            capi.copies_host(reads, [capi.Monomer(k, 0, zero)])
    high = (C.c_uint32 * 16)()
    high[0] = 1 << 6  # base 3 of a unit of 3 bases
    with pytest.raises(capi.TrewHipError, match="bits at or above base k"):
        capi.copies_host(reads, [capi.Monomer(3, 0, high)])
    lib = capi.load()
    arr, nm = capi._monomer_array(["AAT"])
    n = C.c_uint64(0)
    assert lib.trew_copies_host(None, None, None, 1, arr, nm, 3, 24, None, 0, C.byref(n), None, None, None) != 0
    assert b"trew_copies_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_copies_host(None, None, None, 1, None, 1, 3, 24, None, 0, C.byref(n), None, None, None) != 0
    assert b"monomers is NULL" in lib.trew_hip_last_error(None)
    assert lib.trew_copies_host(None, None, None, 0, arr, nm, 3, 24, None, 0, None, None, None, None) != 0
    assert lib.trew_copies_host(None, None, None, 0, arr, nm, 3, 24, None, 4, C.byref(n), None, None, None) != 0  # a capacity without a buffer
    assert lib.trew_copies_host(None, None, None, 0, arr, nm, 3, 24, None, 0, C.byref(n), None, None, None) == 0 and n.value == 0  # no reads


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched"""
    lib = capi.load()
    arr, nm = capi._monomer_array([CC.unit_of(171, 1)])
    n, rows = C.c_uint64(7), C.c_uint64(9)
    assert lib.trew_hip_copies(None, None, 0, arr, nm, 3, 24, 16, 16) == -1
    assert lib.trew_hip_copies_results(None, 0, None, 0, C.byref(n), C.byref(rows), None, None, None) == -1 and (n.value, rows.value) == (7, 9)


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_copies.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.copies([b"TTAGGGTTAGGG"], [CC.unit_of(171, 1)])
    r = subprocess.run([TREW, "copies", CC.unit_of(171, 1), FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.fixture(scope="module")
def fastas(tmp_path_factory):
    d = tmp_path_factory.mktemp("fasta")
    u = CC.unit_of(171, 1)
    files = {
        "empty": "",
        "nine": "".join(">m%d\nACGTTGCA\n" % i for i in range(9)),
        "multi_line_bad": ">alpha the first\n" + u[:60] + "\n" + u[60:120] + "\nNN\n",
        "too_long": ">long\n" + "\n".join(["ACGTTGCA" * 8] * 5) + "\n",  # 320 bases over five lines
        "headless": "ACGT\n>x\nACGT\n",
        "good": ">alpha the first\n" + u[:60] + "\n" + u[60:] + "\n>beta\r\n" + TEL + "\r\n",
    }
    out = {}
    for name, text in files.items():
        out[name] = str(d / (name + ".fa"))
        with open(out[name], "w") as f:
            f.write(text)
    return out


U40 = "ACGTTGCAAC" * 4
CLI_ERRORS = [
    (["copies"], "MONOMER or --fasta FILE is required."),
    (["copies", U40], "FASTQ is required."),
    (["copies", FQ], "MONOMER or --fasta FILE is required."),
    (["copies", "--fasta", "@good", U40, FQ], "MONOMER and --fasta cannot both be given."),
    (["copies", "--fasta", "@good"], "FASTQ is required."),
    (["copies", "TTAGGN", FQ], "must consist of A, C, G and T."),
    (["copies", "AC", FQ], "the length must be in range 3 to 256."),
    (["copies", "A" * 257, FQ], "the length must be in range 3 to 256."),
    (["copies", ",".join(["AAT"] * 9), FQ], "At most 8 monomers can be given."),
    (["copies", "--fasta", "@empty", FQ], "no FASTA records"),
    (["copies", "--fasta", "/nonexistent.fa", FQ], "/nonexistent.fa : file not found"),
    (["copies", "--fasta", "@nine", FQ], "At most 8 monomers can be given."),
    (["copies", "--fasta", "@multi_line_bad", FQ], "MONOMER 'alpha' must consist of A, C, G and T."),
    (["copies", "--fasta", "@too_long", FQ], "MONOMER 'long': the length must be in range 3 to 256."),
    (["copies", "--fasta", "@headless", FQ], "sequence in front of the first header"),
    (["copies", "--fasta"], "--fasta: expected 1 argument(s). 0 provided."),
    (["copies", U40, FQ, "--penalty", "x"], "PENALTY must be a number."),
    (["copies", U40, FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
    (["copies", U40, FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
    (["copies", U40, FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
    (["copies", U40, FQ, "--items", "3"], "3 : file not found"),
    (["copies", U40, FQ, "--bases", "3"], "3 : file not found"),
    (["copies", U40, FQ, "-t", "0"], "number of threads must be positive."),
    (["copies", U40, FQ, "--bogus"], "Unknown argument: --bogus"),
    (["copies", U40, "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
]


@pytest.mark.parametrize("args,msg", CLI_ERRORS, ids=[str(i) for i in range(len(CLI_ERRORS))])
def test_cli_argument_errors(fastas, args, msg):
    args = [fastas[a[1:]] if a.startswith("@") else a for a in args]
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: copies" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_copies():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "copies" in r.stderr and "monomers" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  copies " in r.stderr
    r = subprocess.run([TREW, "copies", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: copies" in r.stderr and "--fasta" in r.stderr and "--items" in r.stderr and "--bases" in r.stderr and r.stdout == ""
