"""De novo repeats, every tract of a read, the parts that need no GPU: the two shapes of repeat_ref.py against each other, the
host definition (trew_repeats_host) against the reference, every consequence of the definition, hand vectors, random sequence
gives nothing, the stand-alone sanitizer harness, the cap / n / counts contract, the additive ABI, the argument errors of the
C ABI and of `trew repeats`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import period_ref as R
import repeat_ref as RR
from period_cases import TEL, fuzz_reads, junk, noisy, rep
from repeat_cases import SAT, edge_reads, stack_reads, two_satellites
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
# the (min_period, max_period) of the six cases of test_periods_cpu.py (two of them share 1 .. 32)
RANGES = [(1, 32), (1, 32), (1, 1), (32, 32), (5, 7), (2, 31)]


def same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    for f in RR.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at record %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def both(reads, *args):
    """host == reference, records and counts; returns them"""
    got, counts, found = capi.repeats_host(reads, *args)
    want, want_counts = RR.repeats(reads, *args)
    same(got, want)
    assert found == len(want) == counts.sum() and (counts == want_counts).all()
    return got, counts


def abutting(recs):
    return sum(1 for a, b in zip(recs[:-1], recs[1:]) if a["read"] == b["read"] and b["start"] == a["end"])


# ---- the reference
def test_reference_shapes_agree():
    rnd = random.Random(7)
    reads = [r.decode() for r in fuzz_reads(3, 150, 500)] + stack_reads() + [two_satellites(rnd, s) for s in (0, 0.02, 0.1)]
    deep = 0
    for i, r in enumerate(reads):
        args = ((1, 32, 3, 24), (1, 32, 3, 8), (2, 12, 1, 10), (1, 32, 64, 8))[i % 4]
        a, b = RR.repeats_read(r, *args), RR.repeats_read_rounds(r, *args)
        assert sorted(a) == sorted(b) and len(set(a)) == len(a), (i, args)
        assert [x[0] for x in b] == sorted(x[0] for x in b)  # the rounds ascend in depth
        deep = max([deep] + [x[0] for x in a])
    assert deep >= 4


# ---- the host definition against the reference
@pytest.mark.parametrize("seed", [1, 2])
def test_host_fuzz_against_reference(seed):
    reads = fuzz_reads(seed, 400, 700)
    stats = {}
    for min_score in (24, 8):
        for penalty in (1, 3, 64):
            for lo, hi in sorted(set(RANGES)):
                got, counts = both(reads, lo, hi, penalty, min_score)
                if (lo, hi, penalty) == (1, 32, 3):
                    stats[min_score] = ((counts >= 3).sum(), abutting(got), int(got["depth"].max()))
    print("seed %d: (reads with three or more tracts, abutting pairs, largest depth) by min_score: %s" % (seed, stats))
    assert stats[8][0] >= 30 and stats[8][1] >= 25  # the set is not trivial
    assert stats[8][2] >= (3 if seed == 1 else 5)   # depth >= 3 over the two seeds together, and where it is reached


def test_depth_over_both_fuzz_seeds():
    deepest = max(int(capi.repeats_host(fuzz_reads(seed, 400, 700), 1, 32, 3, 8)[0]["depth"].max()) for seed in (1, 2))
    assert deepest >= 3


# ---- consequences of the definition
@pytest.mark.parametrize("args", [(1, 32, 3, 24), (1, 32, 3, 8), (5, 7, 1, 8), (1, 32, 64, 8)])
def test_consequences(args):
    lo, hi, penalty, min_score = args
    reads = fuzz_reads(21, 300, 700) + [r.encode() for r in stack_reads()]
    got, counts, found = capi.repeats_host(reads, *args)
    per = capi.periods_host(reads, *args)
    assert found == len(got) == counts.sum() and (counts >= 3).sum() >= 3
    # the depth-0 record of a read is its periods record, field for field; a read without one has no tract
    zero = got[got["depth"] == 0]
    assert (zero["read"] == np.flatnonzero(per["period"] > 0)).all()
    for f in R.FIELDS:
        assert (zero[f] == per[f][zero["read"]]).all(), f
    assert ((counts > 0) == (per["period"] > 0)).all()
    at = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    for r in range(len(reads)):
        mine = got[at[r]:at[r + 1]]
        assert (mine["read"] == r).all()
        if len(mine) == 0:
            continue
        n = len(reads[r])
        # disjoint and inside the read, sorted by start
        assert (mine["start"][1:] >= mine["end"][:-1]).all() and mine["end"][-1] <= n and (mine["start"] < mine["end"]).all()
        # none scores above the depth-0 tract, and a child not above its parent's piece allows
        assert (mine["score"] <= per["score"][r]).all() and (mine["score"] >= min_score).all()
        assert (mine["depth"] == 0).sum() == 1
        # at most n / (min_score + 1) tracts: every tract has end - start >= score + scored_period >= min_score + 1 bases
        assert len(mine) <= n // (min_score + 1)
        assert (mine["end"].astype(np.int64) - mine["start"] >= mine["score"].astype(np.int64) + mine["scored_period"]).all()
    # a read's records do not depend on the rest of the batch
    rnd = random.Random(5)
    order = list(range(len(reads)))
    rnd.shuffle(order)
    shuffled = capi.repeats_host([reads[i] for i in order], *args)[0]
    for new, old in list(enumerate(order))[:60]:
        a, b = shuffled[shuffled["read"] == new].copy(), got[at[old]:at[old + 1]].copy()
        a["read"] = b["read"] = 0
        same(a, b)
        alone = capi.repeats_host([reads[old]], *args)[0]
        same(alone, b)


def test_pruned_pieces_have_no_record():
    """hi - lo - min_period < min_score: no record, since score_k <= len - k"""
    rnd = random.Random(11)
    for min_period, min_score in ((1, 24), (6, 8), (32, 1), (1, 1)):
        for n in (min_score + min_period - 1, min_score + min_period - 2, 1, 0):
            if n < 0:
                continue
            reads = [rep(u, n) for u in ("A", TEL, "TG")] + [junk(rnd, n)]
            got, counts, found = capi.repeats_host(reads, min_period, 32, 3, min_score)
            assert found == 0 and not counts.any()
        reads = [rep("A", min_score + min_period)]  # one base more: the homopolymer scores len - min_period = min_score
        assert capi.repeats_host(reads, min_period, 32, 3, min_score)[2] == 1


# ---- hand vectors
@pytest.mark.parametrize("sub", [0, 0.02, 0.05])
def test_two_satellites(sub):
    rnd = random.Random(int(sub * 100))
    read = two_satellites(rnd, sub)
    got, counts = both([read])
    assert counts.tolist() == [2] and got["depth"].tolist() == [0, 1]
    assert [int(x["scored_period"]) % 5 for x in got[:1]] == [0] and int(got["scored_period"][1]) % 6 == 0
    assert abs(int(got["start"][0]) - 300) <= 6 and abs(int(got["end"][0]) - 1200) <= 6
    assert abs(int(got["start"][1]) - 1700) <= 6 and abs(int(got["end"][1]) - 2300) <= 6
    if sub <= 0.02:
        assert got["period"].tolist() == [5, 6]
        assert R.canonical(got["unit"][0], 5) == R.canonical(R.pack_unit(R.codes(SAT).tolist()), 5)
        assert R.canonical(got["unit"][1], 6) == R.canonical(R.pack_unit(R.codes(TEL).tolist()), 6)


def test_tract_split_by_an_error_cluster():
    """sixty bases of background in the middle of a (TTAGGG)n tract cost more than the shorter half gains: two tracts, the
    longer at depth 0, the other its child, and the cluster belongs to neither; eight substituted bases do not split it"""
    rnd = random.Random(3)
    whole = rep(TEL, 480)
    read = junk(rnd, 40) + whole[:300] + junk(rnd, 60) + whole[360:] + junk(rnd, 40)
    got, counts = both([read], 1, 32, 3, 24)
    assert counts.tolist() == [2] and got["period"].tolist() == [6, 6] and got["depth"].tolist() == [0, 1]
    assert int(got["end"][0]) <= 40 + 300 + 6 and int(got["start"][1]) >= 40 + 360 - 6
    few = "".join(rnd.choice([y for y in "ACGT" if y != c]) for c in whole[300:308])
    one = capi.repeats_host([junk(rnd, 40) + whole[:300] + few + whole[308:] + junk(rnd, 40)])[1]
    assert one.tolist() == [1]


def test_no_tract_small_reads_and_all_n():
    rnd = random.Random(4)
    reads = [junk(rnd, 600), "", "A", "N" * 100, "N" * 3000, "ACGT" * 3]
    got, counts = both(reads, 1, 32, 3, 24)
    assert len(got) == 0 and not counts.any()
    for k in (1, 2, 6, 32):  # n <= min_period: no admissible k
        for n in (0, 1, k - 1, k):
            assert capi.repeats_host([rep("ACGGT" * 8, max(n, 0))], k, 32, 3, 1)[2] == 0
        got, counts = both([rep(("ACGGT" * 8)[:k], k + 1)], k, k, 3, 1)
        assert counts.tolist() == [1] and (int(got["start"][0]), int(got["end"][0]), int(got["score"][0])) == (0, k + 1, 1)
    assert capi.repeats_host(["N" * 100], 1, 32, 3, 1)[2] == 0
    # N between two tracts: each piece is scored on its own
    got, counts = both([rep(TEL, 120) + "N" * 50 + rep(SAT, 90)], 1, 32, 3, 24)
    assert counts.tolist() == [2] and got["period"].tolist() == [6, 5]


def test_edge_reads_of_equal_units_give_two_records():
    """the reads the GPU test sweeps: with equal units, 0 < g < k substituted bases and penalty 64 the reference says two
    tracts, although the bases on either side of the piece boundary match at period k"""
    for k in (2, 3, 6, 31, 32):
        reads, equal = edge_reads(k)
        pick = [i for i, e in enumerate(equal) if e and 0 < e[0] < k][::7]
        assert len(pick) >= 8
        got, counts = both([reads[i] for i in pick], 1, 32, 64, 20)
        assert (counts == 2).all(), (k, counts)
        for a, b in zip(got[0::2], got[1::2]):
            assert 0 < int(b["start"]) - int(a["end"]) < k  # the gap
    reads = stack_reads()
    got, counts = both(reads, 1, 32, 3, 24)
    assert counts.tolist() == [6, 6, 6, 64]
    assert [int(got[got["read"] == r]["depth"].max()) for r in range(3)] == [5, 5, 2]


def test_random_background_gives_no_record():
    """2000 random 10 kb reads at the default min_score: no tract"""
    rnd = random.Random(2024)
    reads = ["".join(rnd.choices("ACGT", k=10000)) for _ in range(2000)]
    got, counts, found = capi.repeats_host(capi.pack_reads(reads))
    assert found == 0 and len(got) == 0 and not counts.any()


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path):
    exe = str(tmp_path / "repeats_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "repeats_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.decode().upper().encode() for r in fuzz_reads(31, n=250)] + [b"", b"A", TEL.encode() * 400] + [r.encode() for r in stack_reads()]

    def text(recs, counts, found):
        return "%d\n%s\n" % (found, " ".join(str(int(c)) for c in counts)) + "".join(" ".join(str(int(x[f])) for f in RR.FIELDS) + "\n" for x in recs)

    for args in ((1, 32, 3, 24), (1, 32, 3, 8), (1, 1, 1, 1), (32, 32, 64, 1), (3, 12, 7, 10)):
        r = subprocess.run([exe] + [str(a) for a in args], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        assert r.stdout.decode() == text(*capi.repeats_host(reads, *args))
    for cap in (0, 1, 7):  # a buffer smaller than the tracts found: exactly cap records are written
        r = subprocess.run([exe, "1", "32", "3", "8", str(cap)], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
        assert r.stdout.decode() == text(*capi.repeats_host(reads, 1, 32, 3, 8, cap=cap))
    r = subprocess.run([exe, "1", "32", "3", "24"], input=b"", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0\n\n" and r.stderr == b""


# ---- cap, n and counts
def test_cap_n_and_counts():
    reads = fuzz_reads(2, 400, 700)
    full, counts, found = capi.repeats_host(reads, 1, 32, 3, 8)
    assert found == len(full) > 400
    for cap in (0, 1, found - 1, found, found + 5):
        part, c, n = capi.repeats_host(reads, 1, 32, 3, 8, cap=cap)
        assert n == found and (c == counts).all() and len(part) == min(cap, found)
        same(part, full[:cap])  # the first ones of the sorted order
    lib = capi.load()
    words, offsets, lengths = capi.pack_reads(reads)
    n = C.c_uint64(0)
    args = (words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), 1, 32, 3, 8)
    assert lib.trew_repeats_host(*args, None, 0, C.byref(n), None) == 0 and n.value == found  # counts may be NULL
    assert lib.trew_repeats_host(*args, None, 0, None, None) != 0 and b"n must not be null" in lib.trew_hip_last_error(None)
    assert lib.trew_repeats_host(*args, None, 4, C.byref(n), None) != 0 and b"out must not be null" in lib.trew_hip_last_error(None)
    assert lib.trew_repeats_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, 0, 1, 32, 3, 8, None, 0, C.byref(n), None) == 0 and n.value == 0


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Repeat) == 48 and capi.REPEAT_DTYPE.itemsize == 48
    assert tuple(capi.REPEAT_DTYPE.names) == RR.FIELDS == tuple(n for n, _ in capi.Repeat._fields_)
    assert RR.FIELDS == ("read", "depth", "period", "scored_period", "score", "start", "end", "matches", "support", "reserved", "unit")
    assert capi.REPEAT_DTYPE.fields["unit"][1] == 40
    assert C.sizeof(capi.Period) == 40  # periods keeps its record
    for sym in ("trew_hip_repeats", "trew_hip_repeats_results", "trew_repeats_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 5), (3, 2), (1, 33), (33, 33), (-1, 4)):
        with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
            capi.repeats_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.repeats_host(reads, penalty=penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.repeats_host(reads, min_score=0)


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_repeats.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.repeats([b"TTAGGGTTAGGG"])
    r = subprocess.run([TREW, "repeats", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["repeats"], "FASTQ is required."),
        (["repeats", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["repeats", FQ, "--max_period", "33"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["repeats", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["repeats", FQ, "--min_period", "x"], "MIN_PERIOD must be a number."),
        (["repeats", FQ, "--max_period", "x"], "MAX_PERIOD must be a number."),
        (["repeats", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["repeats", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["repeats", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["repeats", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["repeats", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["repeats", FQ, "-t", "0"], "number of threads must be positive."),
        (["repeats", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["repeats", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["repeats", FQ, "--devices", "0,x"], "Usage: repeats"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: repeats" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_repeats():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "repeats" in r.stderr and "periods" in r.stderr and "short" in r.stderr
    r = subprocess.run([TREW, "repeats", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: repeats" in r.stderr and "--min_score" in r.stderr and "--max_period" in r.stderr and r.stdout == ""
