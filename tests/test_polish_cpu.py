"""De novo repeats under indels for periods up to 256 (seed, monomers' alignment, re-voted unit), the parts that need no GPU:
the two forms of polish_ref.py against each other, the library (trew_polish_host) against the reference record for record,
the equality with `refine` at max_period 32, what the measure is for (the fuzz-set conditions, by the reference alone), the
consequences of the definition, the stand-alone sanitizer harness, the additive ABI, the argument errors of the C ABI and of
`trew polish`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import monomer_ref
import period_ref as P
import polish_cases as PC
import polish_ref as R
import refine_cases
import refine_ref
import satellite_ref as SR
from period_cases import junk, noisy
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")


def tuples(recs):
    return [R.as_tuple(x) for x in recs]


def same(got, want):
    """library records against reference tuples, record for record"""
    got = tuples(got)
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g == w, "read %d: got %s, want %s" % (r, g, w)


def text(codes):
    return R.text(codes)


@pytest.fixture(scope="module")
def fuzz():
    """(the fuzz set, its reads, the reference's records at P = 3), the reference computed once"""
    fs = PC.fuzz_set()
    reads = [r for _, r, _, _ in fs]
    return fs, reads, R.polish_tuples(reads)


def test_record_layout():
    assert tuple(capi.POLISH_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.Polished._fields_)
    assert capi.POLISH_DTYPE.itemsize == R.DTYPE.itemsize == C.sizeof(capi.Polished) == 176
    assert [capi.POLISH_DTYPE.fields[f][1] for f in R.FIELDS] == list(range(0, 48, 4)) + [48, 112]
    assert capi.POLISH_MAX_PERIOD == R.MAX_PERIOD == 256


# ---- the two forms of the reference
@pytest.mark.parametrize("penalty,min_score", [(2, 10), (3, 10), (64, 5)])
def test_reference_forms_agree(penalty, min_score):
    """the definition in plain tuples against the vectorised form at the unit lengths around the layouts' edges: short reads"""
    rnd = random.Random(9)
    reads = []
    for k in (1, 2, 3, 32, 33, 64, 65):
        unit = junk(rnd, k)
        reads += [junk(rnd, rnd.randint(0, 12), "ACGTN") + noisy(rnd, unit, rnd.randint(k + 30, 2 * k + 50), 0.05, 0.06, 0.01) + junk(rnd, rnd.randint(0, 12))
                  for _ in range(2)]
    got = R.polish_tuples(reads, 1, 256, penalty, min_score)
    for r, read in enumerate(reads):
        assert got[r] == R.polish_read(read, 1, 256, penalty, min_score), (read, penalty)
    assert sum(1 for g in got if g[0]) >= len(reads) - 2
    same(capi.polish_host(reads, 1, 256, penalty, min_score), got)


@pytest.mark.parametrize("k", [171, 256])
@pytest.mark.parametrize("penalty", [2, 3, 64])
def test_reference_forms_agree_at_the_large_k(k, penalty):
    """one read of k + 34 bases with one replaced base (O(n k^2) in Python: seconds a pass)"""
    unit = PC.unit_of(k, 2)
    read = "ACG" + PC.replaced(PC.rep(unit, k + 34, 5), k + 20) + "TT"
    want = R.polish_read(read, 1, 256, penalty, 10)
    assert want[0] == want[2] == k and want[4] >= 13
    assert R.polish_tuples([read], 1, 256, penalty, 10) == [want]
    same(capi.polish_host([read], 1, 256, penalty, 10), [want])


# ---- the library against the reference and against refine
@pytest.mark.parametrize("read,args,want", refine_cases.HAND)
def test_refine_hand_vectors_at_max_period_32(read, args, want):
    got = capi.polish_host([read.encode()], *args)[0]
    assert tuple(int(got[f]) for f in R.U32_FIELDS) == want[:12]
    assert text(R.as_tuple(got)[12]) == P.unit_text(want[12], want[0]) and text(R.as_tuple(got)[13]) == P.unit_text(want[13], want[1])
    assert R.polish_tuples([read], *args) == [R.as_tuple(got)]


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_equals_refine_at_max_period_32_on_refines_fuzz_set(penalty):
    reads = [r for _, r in refine_cases.fuzz_set()]
    got, ref = capi.polish_host(reads, 1, 32, penalty, 24), capi.refine_host(reads, 1, 32, penalty, 24)
    for f in R.U32_FIELDS:
        assert (got[f] == ref[f]).all(), f
    for g, x in zip(got, ref):
        assert SR.unit_text(g["unit"], g["period"]) == P.unit_text(x["unit"], int(x["period"]))
        assert SR.unit_text(g["seed_unit"], g["seed_period"]) == P.unit_text(x["seed_unit"], int(x["seed_period"]))
    if penalty == 3:
        want = refine_ref.refine(reads, 1, 32, 3, 24)
        assert [tuple(int(g[f]) for f in R.U32_FIELDS) for g in got] == [tuple(int(w[f]) for f in R.U32_FIELDS) for w in want]


def cover(start, end, b, d):
    return max(0, min(end, d) - max(start, b)) / (d - b)


def test_fuzz_set_conditions_and_library_against_reference(fuzz):
    """What the measure is for, by the reference alone, on 39 reads with 20 copies of a random unit of 33 .. 256 bases
    (substitutions 0.02 .. 0.03, indels 0.003 .. 0.01): the final alignment covers at least 0.9 of the planted array in at least
    nine tenths of the reads, `satellites`' depth-0 tract does so in at most a quarter of them, and the final score is at least
    0.9 of the forward score of `monomers` with the planted unit in at least nine tenths of the reads.  With the committed seed:
    39, 3 and 39 of 39; `period` is the planted one in 31 reads and `unit` in 21, for `satellites` 31 and 17 (reported only)."""
    fs, reads, want = fuzz
    assert tuple(sorted(set(len(u) for u, _, _, _ in fs))) == PC.FUZZ_KS and len(fs) == 3 * len(PC.FUZZ_KS)
    sat = [P.period_read(r, 1, 256, 3, 24) for r in reads]
    units = [[P.CODE[c] for c in u] for u, _, _, _ in fs]
    planted_score = []  # the forward strand of monomer_ref.monomers, read by read
    for u, r, _, _ in fs:
        c = monomer_ref.codes(r)
        planted_score.append(int(monomer_ref._strand_many(np.array([c], dtype=np.int64), np.array([len(c)]), monomer_ref.strand_codes(u, 0), 3)[0, 0]))
    covered = sum(1 for (_, _, b, d), w in zip(fs, want) if cover(w[5], w[6], b, d) >= 0.9)
    sat_covered = sum(1 for (_, _, b, d), s in zip(fs, sat) if cover(s[3], s[4], b, d) >= 0.9)
    scored = sum(1 for w, ps in zip(want, planted_score) if 10 * w[4] >= 9 * int(ps))
    canon = SR.canonical_codes
    period_ok = sum(1 for u, w in zip(units, want) if w[0] == len(u))
    unit_ok = sum(1 for u, w in zip(units, want) if w[0] == len(u) and canon(w[12]) == canon(u))
    sat_period_ok = sum(1 for u, s in zip(units, sat) if s[0] == len(u))
    sat_unit_ok = sum(1 for u, s in zip(units, sat) if s[0] == len(u) and canon(SR.unit_codes_of_int(s[8], s[0])) == canon(u))
    print("reads %d: covered %d, by satellites %d, score >= 0.9 planted %d; period %d, unit %d; satellites period %d, unit %d" % (
        len(fs), covered, sat_covered, scored, period_ok, unit_ok, sat_period_ok, sat_unit_ok))
    assert 10 * covered >= 9 * len(fs)
    assert 4 * sat_covered <= len(fs)
    assert 10 * scored >= 9 * len(fs)
    assert sum(1 for w in want if w[3]) >= 5  # the re-vote does something here
    same(capi.polish_host(reads), want)


@pytest.mark.parametrize("max_period", [64, 128, 256])
def test_same_period_subset_equals_refine(max_period):
    """short units (k = 2 .. 32, indels 0.01): every read whose step-1 scored_period is that of the range 1 .. 32 equals
    `refine`'s record in every field; by the reference at least three quarters of the reads are such (92, 90 and 86 of 93)"""
    reads = [r for _, r, _, _ in PC.short_set()]
    narrow = [P.period_read(r, 1, 32, 3, 24)[1] for r in reads]
    wide = [P.period_read(r, 1, max_period, 3, 24)[1] for r in reads]
    subset = [i for i in range(len(reads)) if narrow[i] == wide[i]]
    print("max_period %d: %d of %d reads keep their scored period" % (max_period, len(subset), len(reads)))
    assert 4 * len(subset) >= 3 * len(reads)
    got, ref = capi.polish_host(reads, 1, max_period, 3, 24), capi.refine_host(reads, 1, 32, 3, 24)
    assert [int(x) for x in got["scored_period"]] == wide
    for i in subset:
        assert tuple(int(got[i][f]) for f in R.U32_FIELDS) == tuple(int(ref[i][f]) for f in R.U32_FIELDS), i
        assert SR.unit_text(got[i]["unit"], got[i]["period"]) == P.unit_text(ref[i]["unit"], int(ref[i]["period"]))
        assert SR.unit_text(got[i]["seed_unit"], got[i]["seed_period"]) == P.unit_text(ref[i]["seed_unit"], int(ref[i]["seed_period"]))


def test_one_deleted_inserted_and_replaced_base_at_every_7th_position():
    """(a 68-base unit) x 8: away from the ends the unit is unchanged and the one error is found by kind"""
    cases = PC.one_error_reads()
    reads = [r for _, _, r in cases]
    want = R.polish_tuples(reads)
    same(capi.polish_host(reads), want)
    k, n = 68, 68 * 8
    unit = SR.canonical_codes([P.CODE[c] for c in PC.U68])
    for (kind, at, _), w in zip(cases, want):
        assert w[0] == w[1] == w[2] == k and w[3] == 0 and SR.canonical_codes(w[12]) == unit
        c = R.columns(w, 3)
        errors = (c["mismatches"], c["insertions"], c["deletions"])
        if not 7 <= at <= n - 8:
            continue  # further out the flank is no dearer to drop than to bridge
        if kind == "del":
            assert errors == (0, 0, 1) and (w[5], w[6], w[7]) == (0, n - 1, n)
        if kind == "ins":
            assert errors == (0, 1, 0) and (w[5], w[6], w[7]) == (0, n + 1, n)
        if kind == "sub":
            assert errors == (1, 0, 0) and (w[5], w[6], w[7]) == (0, n, n)


def test_hand_made_reads_above_32():
    """an N inside the seed window at phase 80 (the builder asserts that it lies there and that the seed takes the consensus' base
    for it), also between N flanks; the empty read and reads of 1, k and k + 1 bases"""
    unit = PC.unit_of(100, 12)
    reads = [PC.n_in_seed_window(), "", "A", unit, unit + unit[0], unit * 2, PC.n_in_seed_window(lead=90, tail=70)]
    want = R.polish_tuples(reads)
    same(capi.polish_host(reads), want)
    for w in (want[0], want[6]):
        assert w[:4] == (100, 100, 100, 0) and text(w[13]) == unit == text(w[12])  # the N took the consensus' base, the unit's
    assert want[1] == want[2] == want[3] == want[4] == R.ZERO and want[5][:4] == (100, 100, 100, 0)


@pytest.mark.parametrize("max_period,q,read,one_lane,two_lanes", PC.TIE_READS, ids=["%d-q%d-%d" % (t[0], t[1], len(t[2])) for t in PC.TIE_READS])
def test_tied_votes_where_the_smallest_phase_decides_the_record(max_period, q, read, one_lane, two_lanes):
    """Constructed by search: a voting row whose largest V is shared by several phases, and the record differs when another of
    them gets the vote -- in two slots of one lane of the kernel's layout (Q phases a lane, blocked), in two lanes, or both.
    The voted phases also include Q l - 1 and Q l of a lane seam, and phases 0 and k - 1."""
    _, _, S, a1, trace = R.seed_and_trace(read, 1, max_period, 3, 24)
    k = len(S)
    assert PC.q_of(k) == q and 64 * q >= max_period > 32 * q  # the layout the call runs on
    matters = R.tie_matters(S, trace)
    assert one_lane == any(a // q == b // q for _, a, b in matters) and two_lanes == any(a // q != b // q for _, a, b in matters)
    assert all(len(trace[row][0]) >= 2 and trace[row][0][0] == a < b for row, a, b in matters)  # j* is the smallest of the tied
    voted = {tied[0] for tied, votes, _ in trace if votes}
    assert {0, k - 1, 5 * q - 1, 5 * q, 9 * q - 1, 9 * q} <= voted
    if k <= 40:  # the trace against the cell-by-cell vote, where that is cheap
        assert R.trace_counts(trace, k) == refine_ref.vote_plain([int(v) for v in P.codes(read)][a1[1]:a1[2]], S, 3)
    want = R.polish_tuples([read], 1, max_period, 3, 24)
    assert want[0][0] == k
    same(capi.polish_host([read], 1, max_period, 3, 24), want)


def test_seed_is_kept_when_the_revoted_unit_scores_lower():
    read = PC.SEED_KEPT
    c = P.codes(read)
    x = [int(v) for v in c]
    S = refine_ref.seed(c, P.period_read(read, *PC.SEED_KEPT_ARGS))
    a1 = R.align_units([read], [S], 3)[0]
    u0, _, changed = refine_ref.revote(S, refine_ref.vote_plain(x[int(a1[1]):int(a1[2])], S, 3))
    assert len(S) > 32 and changed >= 1 and int(R.align_units([read], [u0], 3)[0][0]) < int(a1[0])  # the case is what it is meant to be
    want = R.polish_read(read, *PC.SEED_KEPT_ARGS)
    assert want[:4] == (len(S), len(S), len(S), 0) and want[4] == want[9] == int(a1[0]) and want[12] == want[13] == tuple(S)
    assert R.polish_tuples([read], *PC.SEED_KEPT_ARGS) == [want]
    same(capi.polish_host([read], *PC.SEED_KEPT_ARGS), [want])


def test_seed_period_is_a_proper_divisor_of_the_scored_period():
    read = PC.divisor_read()
    want = R.polish_tuples([read], 34, 256, 3, 24)
    assert want[0][:4] == (17, 17, 34, 0)
    same(capi.polish_host([read], 34, 256, 3, 24), want)


# ---- the consequences
def check_consequences(reads, recs, penalty, args):
    """the consequences of the definition that need no second implementation, and the cross-check of A1 and A2 against `monomers`"""
    sat, counts, _ = capi.satellites_host(reads, args[0], args[1], penalty, args[3])
    first = {}
    for s in sat:
        if int(s["depth"]) == 0:
            first[int(s["read"])] = s
    cols = capi.refine_columns(recs, penalty)
    for name, v in cols.items():
        assert (v >= 0).all(), name
    assert (recs["score"] >= recs["seed_score"]).all()
    for i, (read, x) in enumerate(zip(reads, recs)):
        d, sd = int(x["period"]), int(x["seed_period"])
        assert (d == 0) == (i not in first)  # a zero step-1 record gives a zero record, and only that
        if d == 0:
            assert R.as_tuple(x) == R.ZERO
            continue
        assert int(x["scored_period"]) == int(first[i]["scored_period"]) and int(x["scored_period"]) % sd == 0
        t = R.as_tuple(x)
        assert P.primitive(list(t[12])) == d and P.primitive(list(t[13])) == sd
        assert all(int(w) >> (2 * max(0, min(16, d - 16 * j))) == 0 for j, w in enumerate(x["unit"]) if d < 16 * (j + 1))
        c = R.columns(x, penalty)
        assert int(x["score"]) == int(x["matches"]) - penalty * (c["mismatches"] + c["insertions"] + c["deletions"])
        if sd >= 3:  # A1 against a merged measure
            a = capi.monomers_host([read], [text(t[13])], penalty)[0, 0]
            assert int(a["score_fwd"]) == int(x["seed_score"])
            if int(x["changed"]) == 0:
                assert tuple(int(v) for v in a)[:5] == t[4:9]
        if d >= 3 and int(x["changed"]):
            a = capi.monomers_host([read], [text(t[12])], penalty)[0, 0]
            assert tuple(int(v) for v in a)[:5] == t[4:9]


def test_consequences_on_the_fuzz_set_and_on_ragged_reads(fuzz):
    _, reads, _ = fuzz
    check_consequences(reads, capi.polish_host(reads), 3, (1, 256, 3, 24))
    rnd = random.Random(12)
    ragged = [junk(rnd, rnd.randint(0, 60), "ACGTacgtNn") + noisy(rnd, junk(rnd, rnd.choice([1, 2, 3, 6, 33, 64, 65, 100, 171])), rnd.randint(0, 700), 0.03, 0.03, 0.01).lower()
              + junk(rnd, rnd.randint(0, 30)) for _ in range(40)] + ["", "A", "N" * 300]
    for args in ((1, 256, 3, 24), (2, 100, 5, 9), (40, 256, 2, 1)):
        got = capi.polish_host(ragged, *args)
        same(got, R.polish_tuples(ragged, *args))
        same(capi.polish_host(capi.pack_reads(ragged), *args), R.polish_tuples(ragged, *args))
        check_consequences(ragged, got, args[2], args)


def test_perfect_repeats_agree_with_satellites_and_monomers():
    rnd = random.Random(4)
    reads, units = [], []
    for k in (3, 33, 64, 65, 100, 171, 256):
        unit = PC.unit_of(k, 4)
        for flank in (0, 9):
            reads.append(junk(rnd, flank) + unit * max(4, 36 // k) + junk(rnd, flank))
            units.append(unit)
    got = capi.polish_host(reads)
    same(got, R.polish_tuples(reads))
    sat, _, _ = capi.satellites_host(reads)
    first = {int(s["read"]): s for s in sat if int(s["depth"]) == 0}
    for i, (read, unit, x) in enumerate(zip(reads, units, got)):
        s = first[i]
        assert int(x["period"]) == int(s["period"]) == len(unit) and int(x["changed"]) == 0
        assert R.as_tuple(x)[12] == tuple(SR.unit_codes(s["unit"], s["period"]))  # the unit itself, not a rotation of it
        a = capi.monomers_host([read], [SR.unit_text(s["unit"], s["period"])], 3)[0, 0]
        assert (int(x["score"]), int(x["start"]), int(x["end"])) == (int(a["score_fwd"]), int(a["start_fwd"]), int(a["end_fwd"]))


@pytest.mark.parametrize("k,m", [(40, 6), (171, 4)])
def test_one_base_removed_or_added_is_one_deletion_or_insertion(k, m):
    unit = PC.unit_of(k, 6)
    body = unit * m
    at = k + k // 3  # not in the middle: two equal halves around one missing base are a perfect repeat of a period of their own
    shorter, longer = body[:at] + body[at + 1:], body[:at] + "ACGT"[("ACGT".index(body[at]) + 2) % 4] + body[at:]
    got = capi.polish_host([shorter, longer])
    canon = SR.canonical_codes([P.CODE[c] for c in unit])
    for x, (ins, dele), length in zip(got, ((0, 1), (1, 0)), (m * k - 1, m * k + 1)):
        c = capi.refine_columns(x, 3)
        assert (int(c["mismatches"]), int(c["insertions"]), int(c["deletions"])) == (0, ins, dele)
        assert (int(x["start"]), int(x["end"]), int(x["consumed"]), int(x["period"])) == (0, length, m * k, k)
        assert SR.canonical_codes(R.as_tuple(x)[12]) == canon


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path, fuzz):
    exe = str(tmp_path / "polish_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "polish_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    _, reads, _ = fuzz
    reads = [r.encode() for r in reads[::6]] + [b"", b"A", b"N" * 300, b"TTAGGG" * 100, PC.SEED_KEPT.encode(), PC.n_in_seed_window().encode(),
                                                PC.divisor_read().encode(), PC.unit_of(256, 1).encode() * 3]
    for args in ((1, 256, 2, 24), (1, 256, 3, 10), (1, 64, 64, 24), (34, 200, 3, 1), (1, 32, 3, 24)):
        r = subprocess.run([exe, *[str(a) for a in args]], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        want = capi.polish_host(reads, *args)
        assert r.stdout.decode() == "".join(" ".join([str(int(x[f])) for f in R.U32_FIELDS] + [str(int(w)) for w in x["unit"]] + [str(int(w)) for w in x["seed_unit"]])
                                            + "\n" for x in want)
    r = subprocess.run([exe, "1", "256", "3", "24"], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == (b" ".join([b"0"] * 44) + b"\n") * 2 and r.stderr == b""


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Refined) == 64 and C.sizeof(capi.Alignment) == 40 and C.sizeof(capi.Monomer) == 72
    header = open(os.path.join(ROOT, "include", "trew_hip.h")).read()
    assert "#define TREW_HIP_ABI_VERSION 4" in header and "#define TREW_POLISH_MAX_PERIOD 256" in header and "} trew_hip_polished;" in header
    for sym in ("trew_hip_polish", "trew_hip_polish_results", "trew_polish_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None and ("int %s(" % sym) in header
    import trew_amd
    assert trew_amd.polish is capi.polish


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 5), (3, 2), (1, 257)):
        with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 256"):
            capi.polish_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.polish_host(reads, penalty=penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.polish_host(reads, min_score=0)
    lib = capi.load()
    assert lib.trew_polish_host(None, None, None, 1, 1, 256, 3, 24, None) != 0
    assert b"trew_polish_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_polish_host(None, None, None, 0, 1, 256, 3, 24, None) == 0  # no reads: nothing is read or written


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched
    (the checks and the cap / *n rule with a context: tests/test_gpu_polish.py)"""
    lib = capi.load()
    n = C.c_uint64(7)
    assert lib.trew_hip_polish(None, None, 0, 1, 256, 3, 24) == -1
    assert lib.trew_hip_polish_results(None, 0, None, 0, C.byref(n), None) == -1 and n.value == 7


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_polish.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.polish([b"TTAGGGTTAGGG" * 5])
    r = subprocess.run([TREW, "polish", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["polish"], "FASTQ is required."),
        (["polish", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 256."),
        (["polish", FQ, "--max_period", "257"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 256."),
        (["polish", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["polish", FQ, "--min_period", "x"], "MIN_PERIOD must be a number."),
        (["polish", FQ, "--max_period", "x"], "MAX_PERIOD must be a number."),
        (["polish", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["polish", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["polish", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["polish", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["polish", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["polish", FQ, "-t", "0"], "number of threads must be positive."),
        (["polish", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["polish", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["polish", FQ, "--devices", "0,x"], "Usage: polish"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: polish" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_polish():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "polish" in r.stderr and "refine" in r.stderr and "short" in r.stderr and "long" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  polish " in r.stderr
    r = subprocess.run([TREW, "polish", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: polish" in r.stderr and "--penalty" in r.stderr and "--max_period" in r.stderr and r.stdout == ""
