"""Refine's unit with the period chosen by alignment (`resolve`), the parts that need no GPU: the two forms of resolve_ref.py
against hand-worked vectors and against each other, the consequences of the definition, what the measure is for (the planted
unit of the committed fuzz set, against `refine`), the host definition (trew_resolve_host) against the reference, the
stand-alone sanitizer harness, the additive ABI, the argument errors of the C ABI and of `trew resolve`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import period_ref as P
import refine_ref as R
import resolve_ref as V
from period_cases import fuzz_reads, junk, noisy
from refine_cases import HAND as REFINE_HAND, fuzz_set
from resolve_cases import ARGS, FLANK, HAND, N_IN_SEED, ROTATED_SEED, SCORE_TIE, SEED_KEPT, SHORT_REPAIRED, T10, TEL, rotations, seeds_of, short_repaired
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
CS = (1, 2, 3, 4)


def rec(x):
    return tuple(int(v) for v in x)


def same(got, want, fields=V.FIELDS):
    assert got.shape == want.shape
    for f in fields:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at read %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def unit_word(text):
    return P.pack_unit([P.CODE[c] for c in text])


def planted(units, recs):
    """per read: the unit is the planted one, compared as canonical (as test_refine_cpu.py compares them)"""
    return [int(x["period"]) == len(u) and P.canonical(x["unit"], len(u)) == P.canonical(unit_word(u), len(u)) for u, x in zip(units, recs)]


@pytest.fixture(scope="module")
def fuzz():
    """(units, reads, refine's reference records, {C: resolve's reference records}), each computed once"""
    fs = fuzz_set()
    reads = [r for _, r in fs]
    return [u for u, _ in fs], reads, R.refine(reads), {c: V.resolve(reads, *ARGS, c) for c in CS}


def test_record_layout():
    assert tuple(capi.RESOLVE_DTYPE.names) == V.FIELDS == tuple(n for n, _ in capi.Resolved._fields_)
    assert capi.RESOLVE_DTYPE.itemsize == V.DTYPE.itemsize == C.sizeof(capi.Resolved) == 80
    assert [capi.RESOLVE_DTYPE.fields[f][1] for f in V.FIELDS] == [V.DTYPE.fields[f][1] for f in V.FIELDS] == list(range(0, 48, 4)) + [48, 56, 64, 68, 72, 76]
    assert V.FIELDS[:14] == R.FIELDS == tuple(capi.REFINE_DTYPE.names) and capi.RESOLVE_MAX_CANDIDATES == V.MAX_CANDIDATES == 4


@pytest.mark.parametrize("read,args,candidates,want", HAND)
def test_hand_worked_vectors(read, args, candidates, want):
    assert V.resolve_read(read, *args, candidates) == want
    assert rec(V.resolve([read], *args, candidates)[0]) == want
    assert rec(capi.resolve_host([read.encode()], *args, candidates)[0]) == want


def test_perfect_repeats_rank_zero_and_three_candidates():
    """the multiples 2k and 3k are the other candidates, their seeds reduce to the same unit and the tie goes to candidate 0"""
    for read, k in (("A" * 40, 1), (T10, 6), (FLANK + T10 + FLANK, 6)):
        c = P.codes(read)
        assert [t[1] for t in V.period_scores(c, 1, 32, 3)[:3]] == [k, 2 * k, 3 * k]
        assert len({tuple(s) for s in seeds_of(read, 3)}) == 1
        x = V.resolve_read(read)
        assert x[14:16] == (3, 0) and x[:14] == R.refine_read(read)


def test_seed_kept_and_n_in_the_seed_window():
    args = (1, 32, 3, 10)
    for c in CS:
        want = V.resolve_read(SEED_KEPT, *args, c)
        assert rec(V.resolve([SEED_KEPT], *args, c)[0]) == want == rec(capi.resolve_host([SEED_KEPT], *args, c)[0])
        assert want[16:] == R.refine_read(SEED_KEPT, *args)[0:1] + R.refine_read(SEED_KEPT, *args)[4:5]
    assert V.resolve_read(SEED_KEPT, *args, 1)[:14] == R.refine_read(SEED_KEPT, *args)  # the seed is kept there: changed = 0
    x = V.resolve_read(N_IN_SEED)
    assert x[:14] == R.refine_read(N_IN_SEED) and x[14:16] == (3, 0)


def test_score_tie_the_smaller_k_is_the_earlier_candidate():
    c = P.codes(SCORE_TIE)
    order = V.period_scores(c, 1, 32, 3)
    assert order[0][:2] == (30, 3) and order[1][:2] == (30, 5) and order[2][0] < 30
    cands = V.candidate_records(c, *ARGS, 2)
    assert [x[1] for x in cands] == [3, 5]
    want = V.resolve_read(SCORE_TIE, *ARGS, 2)
    assert want[:3] == (5, 5, 5) and want[14:] == (2, 1, 3, 33)  # and the alignment prefers the later one
    assert V.resolve_read(SCORE_TIE, *ARGS, 1)[:3] == (3, 3, 3)
    for n in CS:
        assert rec(capi.resolve_host([SCORE_TIE], *ARGS, n)[0]) == V.resolve_read(SCORE_TIE, *ARGS, n) == rec(V.resolve([SCORE_TIE], *ARGS, n)[0])


def test_rotated_seed_and_short_repaired_read_are_what_they_are_meant_to_be():
    s = seeds_of(ROTATED_SEED)
    assert len(s) == 2 and s[0] != s[1] and "".join(map(str, s[1])) in rotations("".join(map(str, s[0])))
    assert rec(capi.resolve_host([ROTATED_SEED])[0]) == V.resolve_read(ROTATED_SEED)
    assert short_repaired() == SHORT_REPAIRED and len(SHORT_REPAIRED) < 400
    want = V.resolve_read(SHORT_REPAIRED)
    assert want[15] == 1 and want[4] > want[17] and rec(capi.resolve_host([SHORT_REPAIRED])[0]) == want


def test_reference_forms_agree():
    """the definition in plain tuples against the vectorised form: short reads, every unit length, all penalties and C"""
    rnd = random.Random(11)
    reads = ["", "A", "AC", "ACA"]
    for k in range(1, 33):
        reads.append(junk(rnd, rnd.randint(0, 12), "ACGTN") + noisy(rnd, junk(rnd, k), rnd.randint(30, 40 + 4 * k), 0.04, 0.08, 0.01) + junk(rnd, rnd.randint(0, 12)))
    repaired = 0
    for (penalty, min_score), c in zip(((1, 10), (3, 10), (64, 5), (3, 1)), (3, 4, 2, 1)):
        got = V.resolve(reads, 1, 32, penalty, min_score, c)
        for r, read in enumerate(reads):
            assert rec(got[r]) == V.resolve_read(read, 1, 32, penalty, min_score, c), (read, penalty, c)
        same(capi.resolve_host(reads, 1, 32, penalty, min_score, c), got)
        repaired += int((got["rank"] > 0).sum())
    assert repaired >= 3


def test_fuzz_set_gains_and_library_against_reference(fuzz):
    """What the measure is for, by the reference alone, on the committed fuzz set with C = 3: no read that `refine` gets right
    is lost and at least 6 are gained; and the library gives the reference's records.  With the committed seed: `refine` 78
    of 93, `resolve` 86 (8 gained, none lost; 85 with C = 2, 86 with C = 4), the period alone right in 86 against 81, the sum
    of the final scores 62538 against 61082, 2.31 candidates a read, the winner's rank 0 / 1 / 2 in 82 / 10 / 1 reads."""
    units, reads, ref, want = fuzz
    old, new = planted(units, ref), planted(units, want[3])
    gained, lost = sum(b and not a for a, b in zip(old, new)), sum(a and not b for a, b in zip(old, new))
    print("reads %d, planted unit found by refine %d, by resolve %d (C = 2: %d, C = 4: %d), gained %d, lost %d, mean candidates %.2f, ranks %s" % (
        len(reads), sum(old), sum(new), sum(planted(units, want[2])), sum(planted(units, want[4])), gained, lost, want[3]["candidates"].mean(),
        [int((want[3]["rank"] == r).sum()) for r in range(3)]))
    assert lost == 0
    assert gained >= 6
    assert int(want[3]["score"].sum()) > int(ref["score"].sum())
    same(capi.resolve_host(reads), want[3])


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_host_against_reference_on_the_fuzz_set(fuzz, penalty):
    _, reads, _, want = fuzz
    part = reads[::3] if penalty != 3 else reads
    for c in CS:
        same(capi.resolve_host(part, 1, 32, penalty, 24, c), want[c] if penalty == 3 else V.resolve(part, 1, 32, penalty, 24, c))


def check_consequences(reads, recs, penalty, args, candidates):
    """the consequences of the definition, and the cross-check of the winner against `align`"""
    ref = capi.refine_host(reads, args[0], args[1], penalty, args[3])
    assert ((recs["period"] == 0) == (ref["period"] == 0)).all()  # a zero refine record gives a zero record, and the reverse
    assert all(rec(x) == V.ZERO for x in recs[recs["period"] == 0])
    assert (recs["score"] >= recs["first_score"]).all() and (recs["first_score"] == ref["score"]).all() and (recs["first_score"] >= ref["seed_score"]).all()
    assert (recs["first_period"] == ref["period"]).all() and (recs["reserved"] == 0).all()
    nz = recs["period"] > 0
    assert (recs["candidates"][nz] >= 1).all() and (recs["candidates"] <= candidates).all() and (recs["rank"][nz] < recs["candidates"][nz]).all()
    first = recs["rank"] == 0
    same(V.refined(recs[first]), ref[first].astype(R.DTYPE), R.FIELDS)  # rank 0: the sixteen words are refine's
    if candidates == 1:
        assert first.all()
    later = recs[~first]
    assert ((later["score"] > later["first_score"]) | ((later["score"] == later["first_score"]) & (later["period"] < later["first_period"]))).all()
    cols = capi.refine_columns(recs, penalty)  # takes the first sixteen words as they are
    for name, v in cols.items():
        assert (v >= 0).all(), name
    for read, x in zip(reads, recs):
        d, sd = int(x["period"]), int(x["seed_period"])
        if d == 0:
            continue
        assert int(x["scored_period"]) % sd == 0
        if sd >= 3 and (int(x["changed"]) == 0 or d >= 3):
            a = capi.align_host([read], [P.unit_text(x["unit"], d)], penalty)[0, 0]
            assert rec(a)[:5] == rec(x)[4:9]


def test_consequences_on_the_fuzz_set(fuzz):
    _, reads, _, want = fuzz
    for c in CS:
        check_consequences(reads, want[c], 3, ARGS, c)
    assert (want[3]["rank"] > 0).sum() >= 8 and (want[3]["rank"] == 2).sum() >= 1


def test_candidates_one_is_refine():
    rnd = random.Random(3)
    reads = [r for r, _, _ in REFINE_HAND] + [r for _, r in fuzz_set()][::5] + [r.decode() for r in fuzz_reads(5, n=80, max_len=300)]
    reads += [junk(rnd, rnd.randint(0, 200)) for _ in range(20)]
    for args in (ARGS, (2, 12, 5, 9), (7, 32, 1, 1)):
        got = capi.resolve_host(reads, *args, 1)
        want = capi.refine_host(reads, *args)
        same(V.refined(got), want.astype(R.DTYPE), R.FIELDS)
        assert (got["rank"] == 0).all() and (got["candidates"] == (want["period"] > 0)).all()
        assert (got["first_period"] == want["period"]).all() and (got["first_score"] == want["score"]).all()


def test_host_packed_planes_lower_case_and_ranges():
    rnd = random.Random(12)
    reads = [junk(rnd, rnd.randint(0, 60), "ACGTacgtNn") + noisy(rnd, junk(rnd, rnd.choice([1, 2, 3, 6, 11, 32])), rnd.randint(0, 200), 0.03, 0.06, 0.01).lower()
             + junk(rnd, rnd.randint(0, 30)) for _ in range(40)] + ["", "A", "N" * 40]
    for args, c in (((1, 32, 3, 24), 3), ((2, 12, 5, 9), 4), ((7, 32, 1, 1), 2)):
        want = V.resolve(reads, *args, c)
        same(capi.resolve_host(reads, *args, c), want)
        same(capi.resolve_host(capi.pack_reads(reads), *args, c), want)
        check_consequences(reads, want, args[2], args, c)


def test_decompose_anchor_takes_the_record():
    x = capi.resolve_host([SHORT_REPAIRED])[0]
    assert capi.decompose_anchor(x) == int(x["unit"])  # reserved = 0: the unit itself


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path):
    exe = str(tmp_path / "resolve_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "resolve_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.encode() for _, r in fuzz_set()[::6]]
    reads += [b"", b"A", b"AA", b"AAA", b"N" * 70, TEL.encode() * 400, SEED_KEPT.encode(), N_IN_SEED.encode(), SCORE_TIE.encode(), SHORT_REPAIRED.encode()]
    for args in ((1, 32, 1, 24, 3), (1, 32, 3, 10, 4), (1, 32, 64, 24, 2), (5, 9, 3, 1, 1), (31, 32, 3, 1, 4)):
        r = subprocess.run([exe, *[str(a) for a in args]], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        want = capi.resolve_host(reads, *args)
        assert r.stdout.decode() == "".join(" ".join(str(int(x[f])) for f in V.FIELDS) + "\n" for x in want)
    r = subprocess.run([exe, "1", "32", "3", "24", "3"], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b" ".join([b"0"] * 18) + b"\n" + b" ".join([b"0"] * 18) + b"\n" and r.stderr == b""
    r = subprocess.run([exe, "1", "32", "3", "24", "5"], input=b"A\n", capture_output=True, timeout=60)
    assert r.returncode == 3 and b"1 <= candidates <= 4" in r.stderr


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Refined) == 64 and C.sizeof(capi.Tandem) == 72
    for sym in ("trew_hip_resolve", "trew_hip_resolve_results", "trew_resolve_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    import trew_amd
    assert trew_amd.resolve is capi.resolve


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 5), (3, 2), (1, 33)):
        with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
            capi.resolve_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.resolve_host(reads, penalty=penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.resolve_host(reads, min_score=0)
    for c in (0, 5, -1):
        with pytest.raises(capi.TrewHipError, match="resolve: 1 <= candidates <= 4 is required"):
            capi.resolve_host(reads, candidates=c)
    lib = capi.load()
    assert lib.trew_resolve_host(None, None, None, 1, 1, 32, 3, 24, 3, None) != 0
    assert b"trew_resolve_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_resolve_host(None, None, None, 0, 1, 32, 3, 24, 3, None) == 0  # no reads: nothing is read or written


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched
    (the candidates check and the cap / *n rule with a context: tests/test_gpu_resolve.py)"""
    lib = capi.load()
    n = C.c_uint64(7)
    assert lib.trew_hip_resolve(None, None, 0, 1, 32, 3, 24, 3) == -1
    assert lib.trew_hip_resolve_results(None, 0, None, 0, C.byref(n), None) == -1 and n.value == 7


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_resolve.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.resolve([b"TTAGGGTTAGGG" * 5])
    r = subprocess.run([TREW, "resolve", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["resolve"], "FASTQ is required."),
        (["resolve", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["resolve", FQ, "--max_period", "33"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["resolve", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["resolve", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["resolve", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["resolve", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["resolve", FQ, "--candidates", "0"], "CANDIDATES must be in range 1 to 4."),
        (["resolve", FQ, "--candidates", "5"], "CANDIDATES must be in range 1 to 4."),
        (["resolve", FQ, "--candidates", "x"], "CANDIDATES must be a number."),
        (["resolve", FQ, "--candidates"], "--candidates: expected 1 argument(s). 0 provided."),
        (["resolve", FQ, "-t", "0"], "number of threads must be positive."),
        (["resolve", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["resolve", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: resolve" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_resolve():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "resolve" in r.stderr and "refine" in r.stderr and "short" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  resolve " in r.stderr
    r = subprocess.run([TREW, "resolve", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: resolve" in r.stderr and "--candidates" in r.stderr and r.stdout == ""
