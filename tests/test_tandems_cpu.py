"""De novo repeats under indels, every tract of a read (`tandems`), the parts that need no GPU: the two forms of tandem_ref.py
against hand-worked vectors and against each other, the consequences of the definition, what the measure is for (both planted
tracts of noisy two-tract reads, whole, against `repeats`), the host definition (trew_tandems_host) against the reference, the
stand-alone sanitizer harness, the additive ABI, the argument errors of the C ABI and of `trew tandems`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import period_ref as P
import refine_ref as R
import repeat_ref
import tandem_ref as T
from period_cases import junk, noisy
from tandem_cases import (EXTENT_UNIT, HAND, STRONG_FIRST, TWO_TRACT_SEED, WEAK, WEAK_FIRST, extent_read, piece_bound_reads, piece_hi_reads, primitive_unit,
                          two_tract_set)
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")


def rec(x):
    return tuple(int(v) for v in x)


def same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in T.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at record %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def unit_key(text):
    return len(text), P.canonical(P.pack_unit([P.CODE[c] for c in text]), len(text))


def keys(recs, i):
    return {(int(x["period"]), P.canonical(x["unit"], int(x["period"]))) for x in recs[recs["read"] == i]}


@pytest.fixture(scope="module")
def two_tract():
    """(planted, reads, {penalty: (reference records, counts)}), the reference computed once"""
    fs = two_tract_set()
    reads = [r for r, _ in fs]
    return [p for _, p in fs], reads, {p: T.tandems(reads, 1, 32, p, 24) for p in (1, 3, 64)}


def test_record_layout():
    assert tuple(capi.TANDEM_DTYPE.names) == T.FIELDS == tuple(n for n, _ in capi.Tandem._fields_) == ("read", "depth") + R.FIELDS
    assert capi.TANDEM_DTYPE.itemsize == T.DTYPE.itemsize == C.sizeof(capi.Tandem) == 72
    offsets = list(range(0, 56, 4)) + [56, 64]  # the u64 units stay 8-byte aligned
    assert [capi.TANDEM_DTYPE.fields[f][1] for f in T.FIELDS] == [T.DTYPE.fields[f][1] for f in T.FIELDS] == offsets
    assert [getattr(capi.Tandem, f).offset for f in T.FIELDS] == offsets


@pytest.mark.parametrize("read,want", HAND)
def test_hand_worked_vectors(read, want):
    assert sorted(T.tandems_read(read), key=lambda x: x[1 + T.START]) == want
    for shape in (T.tandems_read, None):
        got, counts = T.tandems([read], shape=shape)
        assert [rec(x)[1:] for x in got] == want and counts.tolist() == [len(want)]
    got, counts, found = capi.tandems_host([read])
    assert [rec(x)[1:] for x in got] == want and counts.tolist() == [len(want)] and found == len(want)


def test_the_weak_read_is_what_it_is_meant_to_be():
    """a periods score of 48 and a refined score of 23 at the defaults: step 1 promises a repeat that no single unit aligns to"""
    per, x = P.period_read(WEAK), R.refine_read(WEAK)
    assert per[P.FIELDS.index("score")] == 48 and (per[T.P_START], per[T.P_END]) == (0, 60)
    assert x[T.SCORE] == 23 and x != R.ZERO
    assert T.tandems_read(WEAK) == []
    # beside a strong tract: the weak piece is walked first and the strong tract is found below it, or the other way round
    (first,) = T.tandems_read(WEAK_FIRST)
    assert first[0] == 1 and first[1 + T.START] >= 60  # depth 1: the weak piece has a depth but no record
    (strong,) = T.tandems_read(STRONG_FIRST)
    assert strong[0] == 0
    assert R.refine_read(WEAK_FIRST)[T.SCORE] < 24 <= R.refine_read(STRONG_FIRST)[T.SCORE]


def test_children_lie_around_the_refined_tract_not_the_periods_tract():
    read = extent_read()
    per, x = P.period_read(read), R.refine_read(read)
    assert x[T.SCORE] >= 24 and x[T.START] <= per[T.P_START] and x[T.END] >= per[T.P_END] + 3 * len(EXTENT_UNIT)  # wider by whole copies
    # the copies between the two ends would be a tract of their own, were the children formed from the periods tract
    assert P.period_read(read[per[T.P_END]:x[T.END]]) != P.ZERO
    got = sorted(T.tandems_read(read), key=lambda r: r[1 + T.START])
    assert [r[0] for r in got] == [0, 1] and got[0][1:] == x and got[1][1] == 5 and got[1][1 + T.START] >= x[T.END]
    host, _, _ = capi.tandems_host([read])
    assert [rec(r)[1:] for r in host] == got


@pytest.mark.parametrize("k", [1, 6, 32])
def test_pieces_that_start_and_end_mid_word(k):
    """the reads of tests/test_gpu_tandems.py whose child pieces start at lo and end at hi at chosen bits: the host definition
    against the reference, and the child's tract at the piece's first or last base"""
    reads, wanted = piece_bound_reads(k)
    want, counts = T.tandems(reads)
    same(capi.tandems_host(reads)[0], want)
    for i, (lo, at_start) in enumerate(wanted):
        mine = want[want["read"] == i]
        assert len(mine) == 2 and int(mine[mine["depth"] == 0][0]["end"]) == lo
        child = mine[mine["depth"] == 1][0]
        assert int(child["start"]) == lo if at_start else int(child["end"]) == len(reads[i])
    reads, wanted = piece_hi_reads(k)
    want, counts = T.tandems(reads)
    same(capi.tandems_host(reads)[0], want)
    for i, (lo, hi, shape) in enumerate(wanted):
        mine = want[want["read"] == i]
        assert int(mine[mine["depth"] == 0][0]["start"]) == hi
        (child,) = [x for x in mine if int(x["end"]) == hi]
        assert int(child["depth"]) == (1 if shape == "end" else 2) and (shape == "end" or int(child["start"]) == lo)


def test_reference_forms_agree():
    """depth-first on read[lo:hi] with the plain-tuple refine against round by round with the vectorised refine (which prunes
    the pieces that cannot have a periods record): short reads with one to three tracts, all three penalties"""
    rnd = random.Random(11)
    reads = [WEAK, WEAK_FIRST, STRONG_FIRST, extent_read(), "", "A", "N" * 50]
    for k in (1, 2, 3, 5, 6, 7, 11, 16, 32):
        for _ in range(2):
            s = junk(rnd, rnd.randint(0, 12), "ACGTN")
            for _ in range(rnd.randint(1, 3)):
                s += noisy(rnd, junk(rnd, rnd.choice([k, k, 4, 6])), rnd.randint(30, 50 + 3 * k), 0.04, 0.08, 0.01) + junk(rnd, rnd.randint(0, 25))
            reads.append(s)
    total = 0
    for penalty, min_score in ((1, 10), (3, 24), (3, 12), (64, 5)):
        a, ca = T.tandems(reads, 1, 32, penalty, min_score, shape=T.tandems_read)
        b, cb = T.tandems(reads, 1, 32, penalty, min_score)
        same(b, a)
        assert ca.tolist() == cb.tolist()
        total += len(a)
    assert total >= 3 * len(reads) and (np.bincount(a["read"]) >= 2).sum() >= 5  # several tracts a read


def planted_found(planted, recs):
    """the reads in which every planted unit is the unit of a record, compared as canonical"""
    return sum(1 for i, pl in enumerate(planted) if all(unit_key(u) in keys(recs, i) for u, _, _ in pl))


def covered(planted, recs):
    """the reads in which every planted tract is covered to at least 90 % by ONE record"""
    n = 0
    for i, pl in enumerate(planted):
        mine = recs[recs["read"] == i]
        n += all(any(10 * (min(e, int(x["end"])) - max(s, int(x["start"]))) >= 9 * (e - s) for x in mine) for _, s, e in pl)
    return n


def test_purpose_condition_and_library_against_reference(two_tract):
    """What the measure is for, by the reference alone: on reads with two noisy tracts (substitutions 0.03, indels 0.06) it
    finds both planted units in at least 24 of 30 reads and in more reads than `repeats`, covers every planted tract to 90 %
    with one record in at least 27 reads, and needs at most half the records of `repeats`; and the library gives the
    reference's records.  With the committed seed: both units 29 (repeats 21), covered 30, records 60 against 144."""
    planted, reads, want = two_tract
    assert TWO_TRACT_SEED == 20251015 and len(reads) == 30
    assert all(len(pl) == 2 and all(2 <= len(u) <= 12 and 300 <= e - s <= 700 for u, s, e in pl) for pl in planted)
    recs, counts = want[3]
    theirs, _ = repeat_ref.repeats(reads)
    ours_n, theirs_n, cov = planted_found(planted, recs), planted_found(planted, theirs), covered(planted, recs)
    print("reads %d: both planted units by tandems %d, by repeats %d; covered %d; records %d against %d" % (
        len(reads), ours_n, theirs_n, cov, len(recs), len(theirs)))
    assert ours_n >= 24 and ours_n > theirs_n
    assert cov >= 27
    assert 2 * len(recs) <= len(theirs)
    got, got_counts, found = capi.tandems_host(reads)
    same(got, recs)
    assert got_counts.tolist() == counts.tolist() and found == len(recs)


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_host_against_reference(two_tract, penalty):
    _, reads, want = two_tract
    recs, counts = want[penalty]
    got, got_counts, found = capi.tandems_host(reads, 1, 32, penalty, 24)
    same(got, recs)
    assert got_counts.tolist() == counts.tolist() and found == len(recs) == int(counts.sum())


def check_consequences(reads, recs, counts, args):
    """the consequences of the definition that need no second implementation of the recursion"""
    ref = capi.refine_host(reads, *args)
    per = capi.periods_host(reads, *args)
    assert (recs["score"] >= args[3]).all()
    assert (np.bincount(recs["read"], minlength=len(reads)) == counts).all()
    for i in range(len(reads)):
        mine = recs[recs["read"] == i]
        if int(per[i]["period"]) == 0:
            assert len(mine) == 0  # a read without a periods record has no tract
            continue
        top = mine[mine["depth"] == 0]
        if int(ref[i]["score"]) >= args[3]:  # the depth-0 record is the read's refine record, field for field
            assert len(top) == 1 and rec(top[0])[2:] == rec(ref[i])
        else:  # a weak read: depth 0 has no record
            assert len(top) == 0
        assert (mine["start"][1:] >= mine["end"][:-1]).all() and (mine["start"] < mine["end"]).all()  # sorted by start: disjoint
        assert (mine["end"] <= len(reads[i])).all()


def test_consequences(two_tract):
    _, reads, want = two_tract
    for penalty, (recs, counts) in want.items():
        check_consequences(reads, recs, counts, (1, 32, penalty, 24))
    extra = [WEAK, WEAK_FIRST, STRONG_FIRST, extent_read(), "", "ACGTTGCATGCA"]
    recs, counts, _ = capi.tandems_host(extra)
    check_consequences(extra, recs, counts, (1, 32, 3, 24))


def test_records_do_not_depend_on_the_batch(two_tract):
    _, reads, want = two_tract
    recs, _ = want[3]
    order = list(range(len(reads)))
    random.Random(5).shuffle(order)
    got, counts, _ = capi.tandems_host([reads[i] for i in order] + ["", WEAK])
    for pos, i in enumerate(order):
        assert [rec(x)[1:] for x in got[got["read"] == pos]] == [rec(x)[1:] for x in recs[recs["read"] == i]]
    assert counts.tolist()[-2:] == [0, 0]
    for i in (0, 7, 29):  # and a read on its own
        alone, _, _ = capi.tandems_host([reads[i]])
        assert [rec(x)[1:] for x in alone] == [rec(x)[1:] for x in recs[recs["read"] == i]]


def test_pieces_that_cannot_score_are_not_worth_walking():
    """a piece with hi - lo - min_period < min_score has no periods record (score_k <= length - k): the round-by-round form drops
    such pieces, the depth-first form and the host walk them, and all three agree; at the edge itself a piece of min_score +
    min_period bases does have one"""
    edge = "A" * 25
    assert [rec(x)[1:] for x in capi.tandems_host([edge])[0]] == [(0, 1, 1, 1, 0, 25, 0, 25, 25, 25, 25, 25, 0, 3, 3)]
    assert len(capi.tandems_host([edge[:24]])[0]) == 0 and len(capi.tandems_host([edge], min_period=2)[0]) == 0
    rnd = random.Random(3)
    reads = [junk(rnd, rnd.randint(0, 30)) + "TTAGGG" * rnd.randint(5, 9) + junk(rnd, rnd.randint(20, 30)) + "AC" * rnd.randint(10, 16) + junk(rnd, rnd.randint(0, 30))
             for _ in range(20)]
    for args in ((1, 32, 3, 24), (1, 32, 3, 20), (3, 8, 2, 28)):
        a, ca = T.tandems(reads, *args, shape=T.tandems_read)
        b, cb = T.tandems(reads, *args)
        got, counts, _ = capi.tandems_host(reads, *args)
        same(b, a)
        same(got, a)
        assert ca.tolist() == cb.tolist() == counts.tolist()


def test_perfect_repeats_agree_with_repeats_and_align():
    rnd = random.Random(4)
    reads = []
    for k1, k2 in ((3, 5), (6, 7), (12, 5), (16, 3), (17, 6), (31, 5), (32, 6), (5, 5)):
        u1, u2 = primitive_unit(rnd, k1), primitive_unit(rnd, k2)
        reads.append(junk(rnd, 9) + u1 * max(8, 64 // k1) + junk(rnd, 21) + u2 * max(6, 48 // k2) + junk(rnd, 9))
    got, counts, _ = capi.tandems_host(reads)
    want, _ = T.tandems(reads)
    same(got, want)
    theirs, their_counts, _ = capi.repeats_host(reads)
    assert counts.tolist() == their_counts.tolist() and (counts >= 2).all()
    for x, p in zip(got, theirs):  # both sorted by (read, start)
        d = int(x["period"])
        assert (int(x["read"]), d, int(x["changed"])) == (int(p["read"]), int(p["period"]), 0)
        assert P.canonical(x["unit"], d) == P.canonical(p["unit"], d)
        if d >= 3:
            a = capi.align_host([reads[int(x["read"])]], [P.unit_text(p["unit"], d)], 3)[0, 0]
            assert (int(x["score"]), int(x["start"]), int(x["end"])) == (int(a["score_fwd"]), int(a["start_fwd"]), int(a["end_fwd"]))


def test_host_packed_planes_lower_case_ranges_and_cap():
    rnd = random.Random(12)
    reads = [junk(rnd, rnd.randint(0, 40), "ACGTacgtNn") + noisy(rnd, junk(rnd, rnd.choice([1, 2, 3, 6, 11, 32])), rnd.randint(0, 160), 0.03, 0.06, 0.01).lower()
             + junk(rnd, rnd.randint(0, 30)) + noisy(rnd, junk(rnd, rnd.choice([2, 4, 7])), rnd.randint(0, 120), 0.02, 0.04) for _ in range(30)] + ["", "A", "N" * 40]
    for args in ((1, 32, 3, 24), (2, 12, 5, 9), (7, 32, 1, 1)):
        want, counts = T.tandems([r.upper() for r in reads], *args)
        got, got_counts, found = capi.tandems_host(reads, *args)
        same(got, want)
        same(capi.tandems_host(capi.pack_reads(reads), *args)[0], want)
        assert got_counts.tolist() == counts.tolist() and found == len(want)
        check_consequences([r.upper() for r in reads], want, counts, args)
        few, few_counts, found = capi.tandems_host(reads, *args, cap=3)  # the first ones of the sorted order; the numbers stay exact
        same(few, want[:3])
        assert few_counts.tolist() == counts.tolist() and found == len(want) > 3


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path, two_tract):
    exe = str(tmp_path / "tandems_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "tandems_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    _, reads, _ = two_tract
    reads = [r.encode() for r in reads[::5]] + [b"", b"A", b"N" * 70, b"TTAGGG" * 300, WEAK.encode(), WEAK_FIRST.encode(), STRONG_FIRST.encode(),
                                               extent_read().encode()]
    for args in ((1, 32, 1, 24), (1, 32, 3, 10), (1, 32, 64, 24), (5, 9, 3, 1)):
        r = subprocess.run([exe, *[str(a) for a in args]], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        want, counts, found = capi.tandems_host(reads, *args)
        assert r.stdout.decode() == "n %d\n%s\n" % (found, " ".join(str(int(c)) for c in counts)) + "".join(
            " ".join(str(int(x[f])) for f in T.FIELDS) + "\n" for x in want)
    r = subprocess.run([exe, "1", "32", "3", "24"], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"n 0\n0 0\n" and r.stderr == b""


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Period) == 40 and C.sizeof(capi.Repeat) == 48 and C.sizeof(capi.Refined) == 64
    for sym in ("trew_hip_tandems", "trew_hip_tandems_results", "trew_tandems_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    import trew_amd
    assert trew_amd.tandems is capi.tandems
    x = np.zeros(2, dtype=capi.TANDEM_DTYPE)
    x["period"], x["score"], x["start"], x["end"], x["consumed"], x["matches"] = 6, 56, 0, 60, 60, 59
    assert {k: v.tolist() for k, v in capi.tandem_columns(x, 3).items()} == {k: v.tolist() for k, v in capi.refine_columns(x, 3).items()}
    assert capi.tandem_columns(x, 3)["copies"].tolist() == [10, 10]


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 5), (3, 2), (1, 33)):
        with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
            capi.tandems_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.tandems_host(reads, penalty=penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.tandems_host(reads, min_score=0)
    lib = capi.load()
    n = C.c_uint64(0)
    assert lib.trew_tandems_host(None, None, None, 1, 1, 32, 3, 24, None, 0, C.byref(n), None) != 0
    assert b"trew_tandems_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_tandems_host(None, None, None, 0, 1, 32, 3, 24, None, 0, None, None) != 0
    assert b"trew_tandems_host: n must not be null" in lib.trew_hip_last_error(None)
    assert lib.trew_tandems_host(None, None, None, 0, 1, 32, 3, 24, None, 4, C.byref(n), None) != 0
    assert b"trew_tandems_host: out must not be null" in lib.trew_hip_last_error(None)
    n.value = 7
    assert lib.trew_tandems_host(None, None, None, 0, 1, 32, 3, 24, None, 0, C.byref(n), None) == 0 and n.value == 0  # no reads


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched
    (the cap / *n rules with a context: tests/test_gpu_tandems.py)"""
    lib = capi.load()
    n = C.c_uint64(7)
    assert lib.trew_hip_tandems(None, None, 0, 1, 32, 3, 24, 1) == -1
    assert lib.trew_hip_tandems_results(None, 0, None, 0, C.byref(n), None, None) == -1 and n.value == 7


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_tandems.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.tandems([b"TTAGGGTTAGGG" * 5])
    r = subprocess.run([TREW, "tandems", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["tandems"], "FASTQ is required."),
        (["tandems", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["tandems", FQ, "--max_period", "33"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["tandems", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["tandems", FQ, "--min_period", "x"], "MIN_PERIOD must be a number."),
        (["tandems", FQ, "--max_period", "x"], "MAX_PERIOD must be a number."),
        (["tandems", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["tandems", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["tandems", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["tandems", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["tandems", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["tandems", FQ, "-t", "0"], "number of threads must be positive."),
        (["tandems", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["tandems", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["tandems", FQ, "--devices", "0,x"], "Usage: tandems"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: tandems" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_tandems():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "tandems" in r.stderr and "refine" in r.stderr and "short" in r.stderr and "long" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  tandems " in r.stderr
    r = subprocess.run([TREW, "tandems", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: tandems" in r.stderr and "--penalty" in r.stderr and "--min_period" in r.stderr and r.stdout == ""


def test_cli_lines_of_the_reference():
    """the text form that tests/test_gpu_tandems.py compares `trew tandems` with: header, one row per record, the summary"""
    reads = [HAND[0][0], WEAK, WEAK_FIRST]
    recs, _ = T.tandems(reads)
    rows, tail = T.cli_lines(FQ, reads, recs, 3)
    assert rows[0] == ">" + os.path.realpath(FQ)
    assert rows[1] == ("read,length,depth,period,unit,canonical,start,end,score,copies,consumed,matches,mismatches,insertions,deletions,seed_period,seed_unit,"
                       "seed_score,changed,scored_period")
    assert rows[2:] == ["0,140,1,6,TTAGGG,TTAGGG,8,68,60,10,60,60,0,0,0,6,TTAGGG,60,0,6", "0,140,0,5,AATGG,TTCCA,76,137,61,12,61,61,0,0,0,5,AATGG,61,0,5",
                        "2,104,1,6,TTAGGG,TTAGGG,64,100,36,6,36,36,0,0,0,6,TTAGGG,36,0,6"]
    assert tail == [">Summary", "period,canonical,reads,tracts,bases,copies", "6,TTAGGG,2,2,96,16", "5,TTCCA,1,1,61,12"]
