"""De novo repeat period and unit per read, the parts that need no GPU: the two brute-force forms of period_ref.py against
hand-worked vectors and against each other, the host definition (trew_periods_host) against the reference, the consequences
of the definition, the properties that make the measure useful (planted tails come back as TTAGGG, random sequence gives
nothing), the stand-alone sanitizer harness, the additive ABI, the argument errors of the C ABI and of `trew periods`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import period_ref as R
from period_cases import KAT32, TEL, fuzz_reads, junk, tie_reads
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
LONG_N = 300  # generator reads; see test_tracts_cpu.py: 9 tails and 9 reverse-complemented tails of >= 1500 bases


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at read %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def rec(read, **kw):
    """the record of one read from the reference, checked against the host definition on the way"""
    want = R.period_read(read, **kw)
    got = capi.periods_host([read], **kw)[0]
    assert tuple(int(got[f]) for f in R.FIELDS) == want
    return dict(zip(R.FIELDS, want))


def long_reads(n=LONG_N):
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


# ---- the reference
def test_reference_forms_agree():
    rnd = random.Random(3)
    reads = []
    for i in range(2500):
        n = rnd.randint(0, 40)
        s = junk(rnd, n, "ACGTACGTNa" if i % 2 else "AC")
        if i % 3 == 0 and n > 8:
            unit = junk(rnd, rnd.randint(1, 6))
            at, ln = rnd.randint(0, n - 8), rnd.randint(4, 30)
            s = (s[:at] + (unit * 30)[:ln] + s[at + ln:])[:n]
        reads.append(s)
    n_rec = 0
    for i, s in enumerate(reads):
        kw = dict(min_period=1 + i % 3, max_period=(8, 32, 5)[i % 3], penalty=(1, 3, 64)[i % 3], min_score=1 + (i % 2) * 5)
        a = R.period_read(s, **kw)
        assert a == R.period_read(s, segment=R.segment_direct, **kw), (s, kw)
        if i % 5 == 0:  # and the host definition says what the two forms say
            assert tuple(int(x) for x in capi.periods_host([s], **kw)[0]) == a, (s, kw)
        n_rec += a != R.ZERO
    assert n_rec > 800


def test_hand_vectors():
    x = rec(TEL * 20)
    assert x == dict(period=6, scored_period=6, score=114, start=0, end=120, matches=114, support=120, reserved=0, unit=R.pack_unit([0, 0, 3, 1, 1, 1]))
    assert R.unit_text(x["unit"], 6) == TEL
    for motif in KAT32:
        x = rec(motif * 20)
        n, k = 20 * len(motif), len(motif)
        assert (x["period"], x["scored_period"], x["score"], x["start"], x["end"]) == (k, k, n - k, 0, n)
        assert R.unit_text(x["unit"], k) == motif and x["support"] == n
    x = rec("A" * 40)
    assert (x["period"], x["scored_period"], x["score"], R.unit_text(x["unit"], 1)) == (1, 1, 39, "A")
    x = rec("A" * 40, min_period=3)
    assert (x["period"], x["scored_period"], x["score"], x["unit"]) == (1, 3, 37, 3)
    x = rec(TEL * 20, min_period=7)
    assert (x["period"], x["scored_period"], x["score"], R.unit_text(x["unit"], 6)) == (6, 12, 108, TEL)
    assert rec("ttagggTTAGGGttagggTTAGGGttaggg")["period"] == 6  # lower-case bases are bases


@pytest.mark.parametrize("gap", [40, 70])
def test_tie_rules(gap):
    ab, ba, twice = tie_reads(gap)
    for read in (ab, ba):
        assert R.segment_prefix(R.eq_k(R.codes(read), 2), 3)[0] == R.segment_prefix(R.eq_k(R.codes(read), 6), 3)[0] == 18  # the tie is there
        x = rec(read, min_score=10)
        assert (x["scored_period"], x["period"], x["score"], R.unit_text(x["unit"], 2)) == (2, 2, 18, "TG")
        assert read[x["start"]:x["end"]] == "TG" * 10
    x = rec(twice, min_score=10)
    assert (x["period"], x["score"], x["start"], x["end"]) == (6, 42, 33, 33 + 48) and twice[33:33 + 48] == TEL * 8


def test_n_inside_a_tract_and_a_phase_of_only_n():
    read = TEL * 6 + "TTANGG" + TEL * 6
    x = rec(read)
    # the N breaks eq at its own position and at the one a period in front: 2 mismatches at penalty 3
    assert (x["period"], x["start"], x["end"], x["matches"], x["score"], x["support"]) == (6, 0, 78, 70, 70 - 2 * 3, 77)
    # k = 3 over "NAC" x 12 at penalty 1 (-1 +1 +1 a unit): the span starts on the first A, the phase of the N holds no
    # valid base and its consensus is code 0 = T
    x = rec("CGCGTGT" + "NAC" * 12 + "GGG", min_period=3, max_period=3, penalty=1, min_score=5)
    assert (x["scored_period"], x["period"], x["start"], x["end"], x["score"], x["matches"]) == (3, 3, 8, 43, 12, 22)
    assert R.unit_text(x["unit"], 3) == "ACT" and x["support"] == 24


def test_small_and_degenerate_reads():
    for k in (1, 2, 6, 32):
        for n in (0, 1, 2, k, k + 1):
            read = ("ACGGT" * 8)[:k] * 2
            assert rec(read[:n], min_period=k, max_period=k, min_score=1) == (
                dict(zip(R.FIELDS, R.ZERO)) if n <= k else dict(period=k, scored_period=k, score=1, start=0, end=k + 1, matches=1, support=k + 1, reserved=0,
                                                              unit=R.pack_unit(R.codes(read[:k]).tolist())))
    assert rec("N" * 100, min_score=1) == dict(zip(R.FIELDS, R.ZERO))
    score = rec(TEL * 5)["score"]
    assert score == 24
    assert rec(TEL * 5, min_score=score + 1)["period"] == 0 and rec(TEL * 5, min_score=score - 1)["period"] == 6 and rec(TEL * 5, min_score=score)["period"] == 6


# ---- the host definition against the reference
@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_host_ragged_noisy_reads(penalty):
    reads = fuzz_reads(11 + penalty)
    for lo, hi, ms in ((1, 32, 24), (1, 32, 1), (1, 1, 1), (32, 32, 1), (5, 7, 8), (2, 31, 24)):
        want = R.periods(reads, lo, hi, penalty, ms)
        if (lo, ms) == (1, 24):
            assert (want["period"] > 0).sum() >= 100 and len(set(want["period"].tolist())) >= 8
        same(capi.periods_host(reads, lo, hi, penalty, ms), want)


@pytest.fixture(scope="module")
def generator_long():
    reads = long_reads()
    return reads, capi.periods_host(reads)


def test_host_on_generator_long_reads(generator_long):
    reads, got = generator_long
    pick = [i for i in range(len(reads)) if got["period"][i]][:6] + [0, 1]
    same(got[pick], R.periods([reads[i] for i in pick]))


def test_host_accepts_packed_planes_and_a_read_is_independent_of_its_batch():
    reads = fuzz_reads(5, n=200)
    whole = capi.periods_host(capi.pack_reads(reads))
    same(whole, capi.periods_host(reads))
    rnd = random.Random(9)
    order = list(range(len(reads)))
    rnd.shuffle(order)
    same(capi.periods_host([reads[i] for i in order]), whole[order])
    for i in order[:20]:
        same(capi.periods_host([reads[i]]), whole[i:i + 1])


# ---- consequences of the definition
def test_consequences():
    reads = [r.decode().upper().encode() for r in fuzz_reads(21, n=300)]
    for penalty in (1, 3, 64):
        got = capi.periods_host(reads, penalty=penalty)
        rc = capi.periods_host([R.revcomp(r) for r in reads], penalty=penalty)
        assert (got["score"] == rc["score"]).all() and (got["scored_period"] == rc["scored_period"]).all()
        hit = got["period"] > 0
        assert hit.sum() >= 100
        g = got[hit]
        span = g["end"].astype(np.int64) - g["start"] - g["scored_period"]
        assert (g["matches"].astype(np.int64) * (1 + penalty) == g["score"] + penalty * span).all()
        assert (g["scored_period"] % g["period"] == 0).all()
        assert all(int(x["unit"]) >> (2 * int(x["period"])) == 0 for x in g)
        for r, x in zip([r for r, h in zip(reads, hit) if h], g):
            valid = sum(c in b"ACGT" for c in r[int(x["start"]):int(x["end"])])
            assert x["support"] <= valid and x["end"] <= len(r)


# ---- what makes the measure useful
def test_planted_tails_come_back_as_ttaggg(generator_long):
    """The generator's long reads that carry a (TTAGGG)n tail (found as test_tracts_cpu.py finds them: a tail tract of at least
    1500 bases at penalty 3), on either strand: period 6 and the canonical unit of TTAGGG.  At most 2 % may be left out."""
    reads, got = generator_long
    t = capi.tracts_host(reads, [TEL], 3)
    tailed = np.flatnonzero((t["tail_len_fwd"][:, 0] >= 1500) | (t["head_len_rev"][:, 0] >= 1500))
    assert len(tailed) >= 15
    canon = R.canonical(R.pack_unit(R.codes(TEL).tolist()), 6)
    ref = R.periods([reads[i] for i in tailed])  # first the definition alone: it stays inside the cap on these reads
    ref_ok = [x for x in ref if x["period"] == 6 and R.canonical(x["unit"], 6) == canon]
    assert len(tailed) - len(ref_ok) <= 0.02 * len(tailed)
    ok = [i for i in tailed if got["period"][i] == 6 and R.canonical(got["unit"][i], 6) == canon]
    assert len(tailed) - len(ok) <= 0.02 * len(tailed)
    same(got[tailed], ref)
    # the multiples of 6 do win on some of these reads: the reduction to the primitive root is what returns 6
    assert (got["scored_period"][tailed] % 6 == 0).all()


def test_random_background_gives_no_record():
    """2000 random 10 kb reads: nothing at the default min_score.  The largest score seen (min_score = 1) is the figure next
    to the default in DESIGN 4.7a."""
    rnd = random.Random(2024)
    reads = ["".join(rnd.choices("ACGT", k=10000)) for _ in range(2000)]
    packed = capi.pack_reads(reads)
    assert (capi.periods_host(packed)["period"] == 0).all()
    top = int(capi.periods_host(packed, min_score=1)["score"].max())
    print("largest score over k = 1 .. 32 in 2000 random 10 kb reads:", top)
    assert 8 <= top < 24


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path):
    exe = str(tmp_path / "periods_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "periods_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.decode().upper().encode() for r in fuzz_reads(31, n=250)] + [b"", b"A", TEL.encode() * 400]
    for args in ((1, 32, 3, 24), (1, 1, 1, 1), (32, 32, 64, 1), (3, 12, 7, 10)):
        r = subprocess.run([exe] + [str(a) for a in args], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        want = capi.periods_host(reads, *args)
        assert r.stdout.decode() == "".join(" ".join(str(int(x[f])) for f in R.FIELDS) + "\n" for x in want)
    r = subprocess.run([exe, "1", "32", "3", "24"], input=b"", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"" and r.stderr == b""


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Period) == 40 and capi.PERIOD_DTYPE.itemsize == 40
    assert tuple(capi.PERIOD_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.Period._fields_)
    assert capi.PERIOD_DTYPE.fields["unit"][1] == 32
    for sym in ("trew_hip_periods", "trew_hip_periods_results", "trew_periods_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 5), (3, 2), (1, 33), (33, 33), (-1, 4)):
        with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
            capi.periods_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.periods_host(reads, penalty=penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.periods_host(reads, min_score=0)


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_periods.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.periods([b"TTAGGGTTAGGG"])
    r = subprocess.run([TREW, "periods", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["periods"], "FASTQ is required."),
        (["periods", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["periods", FQ, "--max_period", "33"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["periods", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["periods", FQ, "--min_period", "x"], "MIN_PERIOD must be a number."),
        (["periods", FQ, "--max_period", "x"], "MAX_PERIOD must be a number."),
        (["periods", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["periods", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["periods", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["periods", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["periods", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["periods", FQ, "-t", "0"], "number of threads must be positive."),
        (["periods", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["periods", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["periods", FQ, "--devices", "0,x"], "Usage: periods"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: periods" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_periods():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "periods" in r.stderr and "variants" in r.stderr and "short" in r.stderr
    r = subprocess.run([TREW, "periods", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: periods" in r.stderr and "--min_score" in r.stderr and "--max_period" in r.stderr and r.stdout == ""
