"""De novo repeats under indels (seed, wraparound alignment, re-voted unit), the parts that need no GPU: the two forms of
refine_ref.py against hand-worked vectors and against each other, the consequences of the definition, what the measure is
for (the planted unit of noisy long tracts, against `periods`), the host definition (trew_refine_host) against the reference,
the stand-alone sanitizer harness, the additive ABI, the argument errors of the C ABI and of `trew refine`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_ref
import period_ref as P
import refine_ref as R
from refine_cases import HAND, SEED_KEPT, T10, TEL, fuzz_set, replaced, with_deletion, with_insertion
from period_cases import junk, noisy
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")


def rec(x):
    return tuple(int(v) for v in x)


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at read %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def unit_word(text):
    return P.pack_unit([P.CODE[c] for c in text])


@pytest.fixture(scope="module")
def fuzz():
    """(units, reads, {penalty: reference records}), the reference computed once"""
    fs = fuzz_set()
    reads = [r for _, r in fs]
    return [u for u, _ in fs], reads, {p: R.refine(reads, 1, 32, p, 24) for p in (1, 3, 64)}


def test_record_layout():
    assert tuple(capi.REFINE_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.Refined._fields_)
    assert capi.REFINE_DTYPE.itemsize == R.DTYPE.itemsize == C.sizeof(capi.Refined) == 64
    assert [capi.REFINE_DTYPE.fields[f][1] for f in R.FIELDS] == [R.DTYPE.fields[f][1] for f in R.FIELDS] == list(range(0, 48, 4)) + [48, 56]


@pytest.mark.parametrize("read,args,want", HAND)
def test_hand_worked_vectors(read, args, want):
    assert R.refine_read(read, *args) == want
    assert rec(R.refine([read], *args)[0]) == want
    assert rec(capi.refine_host([read.encode()], *args)[0]) == want


def test_seed_is_kept_when_the_revoted_unit_scores_lower():
    c = P.codes(SEED_KEPT)
    x = [int(v) for v in c]
    S = R.seed(c, P.period_read(SEED_KEPT, 1, 32, 3, 10))
    a1 = align_ref.align_strand(x, S, 3)
    u0, _, changed = R.revote(S, R.vote_plain(x[a1[1]:a1[2]], S, 3))
    assert changed == 1 and align_ref.align_strand(x, u0, 3)[0] < a1[0]  # the case is what it is meant to be
    want = R.refine_read(SEED_KEPT, 1, 32, 3, 10)
    assert want[:4] == (5, 5, 5, 0) and want[4] == want[9] == a1[0] and want[12] == want[13] == P.pack_unit(S)
    assert rec(R.refine([SEED_KEPT], 1, 32, 3, 10)[0]) == want == rec(capi.refine_host([SEED_KEPT], 1, 32, 3, 10)[0])


def test_one_deleted_inserted_and_replaced_base_at_every_position():
    """(TTAGGG) x 10: away from the ends the unit is unchanged and the one error is found by kind"""
    reads, kinds = [], []
    for at in range(60):
        for kind, read in (("del", with_deletion(T10, at)), ("ins", with_insertion(T10, at, "C")), ("sub", replaced(T10, at))):
            reads.append(read)
            kinds.append((kind, at))
    want = [R.refine_read(r) for r in reads]
    assert [rec(x) for x in R.refine(reads)] == want == [rec(x) for x in capi.refine_host(reads)]
    for (kind, at), w in zip(kinds, want):
        assert w[0] == w[1] == w[2] == 6 and w[3] == 0
        assert P.canonical(w[12], 6) == P.canonical(unit_word(TEL), 6)  # the unit is unchanged
        c = R.columns(w, 3)
        errors = (c["mismatches"], c["insertions"], c["deletions"])
        if kind == "del" and 6 <= at <= 55:  # further out the flank is no dearer to drop than to bridge (test_align_cpu.py)
            assert errors == (0, 0, 1) and (w[5], w[6], w[7]) == (0, 59, 60) and w[4] == 59 - 3
        if kind == "ins" and 4 <= at <= 56:
            assert errors == (0, 1, 0) and (w[5], w[6], w[7]) == (0, 61, 60)
        if kind == "sub" and 4 <= at <= 55:
            assert errors == (1, 0, 0) and (w[5], w[6], w[7]) == (0, 60, 60)


def test_reference_forms_agree():
    """the definition in plain tuples against the vectorised form, for every unit length: short reads, all three penalties"""
    rnd = random.Random(9)
    reads = []
    for k in range(1, 33):
        unit = junk(rnd, k)
        reads += [junk(rnd, rnd.randint(0, 12), "ACGTN") + noisy(rnd, unit, rnd.randint(30, 40 + 4 * k), 0.04, 0.08, 0.01) + junk(rnd, rnd.randint(0, 12))
                  for _ in range(2)]
    nonzero = changed = 0
    for penalty, min_score in ((1, 10), (3, 10), (64, 5)):
        got = R.refine(reads, 1, 32, penalty, min_score)
        for r, read in enumerate(reads):
            assert rec(got[r]) == R.refine_read(read, 1, 32, penalty, min_score), (read, penalty)
        nonzero += int((got["period"] > 0).sum())
        changed += int((got["changed"] > 0).sum())
    assert nonzero >= len(reads) and changed >= 3


def planted(units, recs):
    """the reads whose unit is the planted one, compared as canonical"""
    return sum(1 for u, x in zip(units, recs) if int(x["period"]) == len(u) and P.canonical(x["unit"], len(u)) == P.canonical(unit_word(u), len(u)))


def test_fuzz_set_condition_and_library_against_reference(fuzz):
    """What the measure is for, by the reference alone: on noisy long tracts (substitutions 0.03, indels 0.06) it finds the
    planted unit in at least three quarters of the reads and in at least 1.25 times as many reads as `periods`; and the library
    gives the reference's records.  With the committed seed: 78 and 62 of 93."""
    units, reads, want = fuzz
    assert sorted(set(len(u) for u in units)) == list(range(2, 33)) and all(600 <= len(r) <= 1620 for r in reads)
    ours, theirs = planted(units, want[3]), planted(units, P.periods(reads))
    print("reads %d, planted unit found by refine %d, by periods %d" % (len(reads), ours, theirs))
    assert 4 * ours >= 3 * len(reads)
    assert 4 * ours >= 5 * theirs
    same(capi.refine_host(reads), want[3])


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_host_against_reference_on_the_fuzz_set(fuzz, penalty):
    _, reads, want = fuzz
    same(capi.refine_host(reads, 1, 32, penalty, 24), want[penalty])


def check_consequences(reads, recs, penalty, args=(1, 32, None, 24)):
    """the consequences of the definition that need no second implementation, and the cross-check of A1 and A2 against `align`"""
    per = capi.periods_host(reads, args[0], args[1], penalty, args[3])
    assert ((recs["period"] == 0) == (per["period"] == 0)).all()  # a zero periods record gives a zero record, and only that
    zero = recs[recs["period"] == 0]
    assert all(rec(x) == R.ZERO for x in zero)
    assert (recs["score"] >= recs["seed_score"]).all() and (recs["scored_period"] == per["scored_period"]).all()
    cols = capi.refine_columns(recs, penalty)
    for name, v in cols.items():
        assert (v >= 0).all(), name
    for read, x in zip(reads, recs):
        d, sd = int(x["period"]), int(x["seed_period"])
        if d == 0:
            continue
        u = [(int(x["unit"]) >> (2 * (d - 1 - j))) & 3 for j in range(d)]
        assert P.primitive(u) == d and int(x["scored_period"]) % sd == 0
        c = R.columns(x, penalty)
        assert int(x["score"]) == int(x["matches"]) - penalty * (c["mismatches"] + c["insertions"] + c["deletions"])
        if sd >= 3:  # A1 against a merged measure
            a = capi.align_host([read], [P.unit_text(x["seed_unit"], sd)], penalty)[0, 0]
            assert int(a["score_fwd"]) == int(x["seed_score"])
            if int(x["changed"]) == 0:
                assert rec(a)[:5] == rec(x)[4:9]
        if d >= 3 and int(x["changed"]):
            a = capi.align_host([read], [P.unit_text(x["unit"], d)], penalty)[0, 0]
            assert rec(a)[:5] == rec(x)[4:9]


def test_consequences_on_the_fuzz_set(fuzz):
    _, reads, want = fuzz
    for penalty, recs in want.items():
        check_consequences(reads, recs, penalty)
    assert (want[3]["changed"] > 0).sum() >= 5  # the re-vote does something here


def test_perfect_repeats_agree_with_periods_and_align():
    rnd = random.Random(4)
    reads, units = [], []
    for k in (3, 5, 6, 7, 12, 16, 17, 31, 32):
        unit = junk(rnd, k)
        while P.primitive(P.codes(unit).tolist()) != k:
            unit = junk(rnd, k)
        for flank in (0, 9):
            reads.append(junk(rnd, flank) + unit * max(8, 48 // k) + junk(rnd, flank))
            units.append(unit)
    got = capi.refine_host(reads)
    per = capi.periods_host(reads)
    same(got, R.refine(reads))
    for read, unit, x, p in zip(reads, units, got, per):
        assert int(x["period"]) == int(p["period"]) == len(unit) and int(x["changed"]) == 0
        assert P.canonical(x["unit"], len(unit)) == P.canonical(p["unit"], len(unit))
        a = capi.align_host([read], [P.unit_text(p["unit"], len(unit))], 3)[0, 0]
        assert (int(x["score"]), int(x["start"]), int(x["end"])) == (int(a["score_fwd"]), int(a["start_fwd"]), int(a["end_fwd"]))


def test_host_packed_planes_lower_case_and_ranges():
    rnd = random.Random(12)
    reads = [junk(rnd, rnd.randint(0, 60), "ACGTacgtNn") + noisy(rnd, junk(rnd, rnd.choice([1, 2, 3, 6, 11, 32])), rnd.randint(0, 200), 0.03, 0.06, 0.01).lower()
             + junk(rnd, rnd.randint(0, 30)) for _ in range(40)] + ["", "A", "N" * 40]
    for args in ((1, 32, 3, 24), (2, 12, 5, 9), (7, 32, 1, 1)):
        want = R.refine(reads, *args)
        same(capi.refine_host(reads, *args), want)
        same(capi.refine_host(capi.pack_reads(reads), *args), want)
        check_consequences(reads, want, args[2], args)


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path, fuzz):
    exe = str(tmp_path / "refine_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "refine_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    _, reads, _ = fuzz
    reads = [r.encode() for r in reads[::4]] + [b"", b"A", b"N" * 70, TEL.encode() * 400, SEED_KEPT.encode(), T10[:14].encode() + b"N" + T10[15:].encode()]
    for args in ((1, 32, 1, 24), (1, 32, 3, 10), (1, 32, 64, 24), (5, 9, 3, 1)):
        r = subprocess.run([exe, *[str(a) for a in args]], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        want = capi.refine_host(reads, *args)
        assert r.stdout.decode() == "".join(" ".join(str(int(x[f])) for f in R.FIELDS) + "\n" for x in want)
    r = subprocess.run([exe, "1", "32", "3", "24"], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0 0 0 0 0 0 0 0 0 0 0 0 0 0\n" * 2 and r.stderr == b""


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Period) == 40 and C.sizeof(capi.Alignment) == 40
    for sym in ("trew_hip_refine", "trew_hip_refine_results", "trew_refine_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    import trew_amd
    assert trew_amd.refine is capi.refine


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 5), (3, 2), (1, 33)):
        with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
            capi.refine_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.refine_host(reads, penalty=penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.refine_host(reads, min_score=0)
    lib = capi.load()
    assert lib.trew_refine_host(None, None, None, 1, 1, 32, 3, 24, None) != 0
    assert b"trew_refine_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_refine_host(None, None, None, 0, 1, 32, 3, 24, None) == 0  # no reads: nothing is read or written


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched
    (the cap / *n rule with a context: tests/test_gpu_refine.py)"""
    lib = capi.load()
    n = C.c_uint64(7)
    assert lib.trew_hip_refine(None, None, 0, 1, 32, 3, 24) == -1
    assert lib.trew_hip_refine_results(None, 0, None, 0, C.byref(n), None) == -1 and n.value == 7


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_refine.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.refine([b"TTAGGGTTAGGG" * 5])
    r = subprocess.run([TREW, "refine", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["refine"], "FASTQ is required."),
        (["refine", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["refine", FQ, "--max_period", "33"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["refine", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["refine", FQ, "--min_period", "x"], "MIN_PERIOD must be a number."),
        (["refine", FQ, "--max_period", "x"], "MAX_PERIOD must be a number."),
        (["refine", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["refine", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["refine", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["refine", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["refine", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["refine", FQ, "-t", "0"], "number of threads must be positive."),
        (["refine", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["refine", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["refine", FQ, "--devices", "0,x"], "Usage: refine"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: refine" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_refine():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "refine" in r.stderr and "periods" in r.stderr and "short" in r.stderr and "long" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  refine " in r.stderr
    r = subprocess.run([TREW, "refine", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: refine" in r.stderr and "--penalty" in r.stderr and "--min_period" in r.stderr and r.stdout == ""
