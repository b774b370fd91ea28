"""Units in place with no motif given (refine's unit, anchored, and the traceback against it), the parts that need no GPU: the
two forms of decompose_ref.py against each other and against hand-worked vectors, the host definition (trew_decompose_host)
against the reference record for record and item for item, every consequence of the definition on refine's fuzz set, fact (a)
of kernels/trace.inc for the unit lengths 1 and 2, the stand-alone sanitizer harness, the additive ABI, the argument errors of
the C ABI and of `trew decompose`, and what the measure is for: planted variant units among indels, found without the motif."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import align_ref
import chain_ref
import decompose_ref as D
import period_ref as P
import refine_ref
import trace_ref as T
from align_cases import with_deletion, with_insertion
from decompose_cases import END_TIE, PLANTED_SEED, planted, rotation_reads, small_set
from period_cases import junk, noisy
from refine_cases import FLANK, SEED_KEPT, T10, TEL, fuzz_set, replaced
from trew_amd import capi

assert tuple(capi.TRACE_DTYPE.names) == T.ITEM_FIELDS and tuple(capi.REFINE_DTYPE.names) == refine_ref.FIELDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "trew_amd", "csrc")
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
WEAK = "AAAC" * 5 + "AAAG" * 5 + "AACG" * 5  # include/trew_hip.h: a periods score of 48 and a refined score of 23 at the defaults


def same(got, want):
    """(items, counts, records) against those of a reference"""
    gi, gc, gr = got[:3]
    wi, wc, wr = want[:3]
    assert gr.shape == wr.shape and gc.shape == wc.shape
    for f in wr.dtype.names:
        bad = np.flatnonzero(gr[f] != wr[f])
        assert len(bad) == 0, "record %s differs at read %d: got %s, want %s" % (f, bad[0], gr[bad[0]], wr[bad[0]])
    assert (gc == wc).all()
    assert len(gi) == len(wi)
    bad = np.flatnonzero(gi != wi)
    assert len(bad) == 0, "item %d differs: got %s, want %s" % (bad[0], gi[bad[0]], wi[bad[0]])


def tup(it):
    return tuple(int(v) for v in it)[3:11]


def rec(x):
    return tuple(int(v) for v in x)


def items_of(result, read):
    return [tup(it) for it in result[0] if it["read"] == read]


def text_of(word, k):
    return P.unit_text(word, k)


@pytest.fixture(scope="module")
def fuzz():
    """(reads of refine's fuzz set, the reference at P = 3, its columns), computed once"""
    reads = [r for _, r in fuzz_set()]
    cols = {}
    return reads, D.decompose(reads, columns=cols), cols


def test_reference_forms_agree():
    """the plain form (refine_read, the full table with the max over d, every rotation written out) against the vectorised one,
    on every third read of the small set at all three penalties; the doubling and the restarted table on some"""
    reads = [r for _, r in small_set()][::3]
    n = 0
    for penalty in (1, 3, 64):
        want = D.decompose(reads, penalty=penalty)
        for i, read in enumerate(reads):
            r, its = D.decompose_read(read, penalty=penalty)
            assert r == rec(want[2][i]) and its == items_of(want, i), (read, penalty)
            if i % 4 == 0:
                assert D.decompose_read(read, penalty=penalty, doubling=True, restarted=True) == (r, its)
            n += len(its)
    assert n > 300


def test_doubling_steps_give_the_defined_directions_for_unit_lengths_1_and_2():
    """fact (a) of kernels/trace.inc, which tests/test_trace_cpu.py checks for k = 3 .. 32: (op, d) of every cell of the doubling
    form equals the full table's, here for k = 1 and 2 at all three penalties, by the reference alone"""
    rnd = random.Random(31)
    cells = 0
    for unit in ("A", "T", "TG", "CA", "AC"):
        t = align_ref.codes(unit)
        reads = [junk(rnd, rnd.randint(0, 5), "ACGTN") + noisy(rnd, unit, rnd.randint(0, 70), 0.05, 0.1, 0.01) + junk(rnd, rnd.randint(0, 5)) for _ in range(6)]
        reads += ["", unit, unit * 20]
        for penalty in (1, 3, 64):
            for read in reads:
                x = align_ref.codes(read)
                full, dbl = T.table(x, t, penalty), T.table(x, t, penalty, doubling=True)
                assert full == dbl, (read, unit, penalty)
                assert full[0] == align_ref.align_strand(x, t, penalty)
                cells += len(x) * len(t)
    assert cells > 3000
    # and the vectorised form with a unit per read, cell by cell
    xs = [align_ref.codes(noisy(rnd, u, 60, 0.05, 0.1)) for u in ("A", "TG", "AAT")]
    X, lens = refine_ref._plane(xs)
    Tm, ks = refine_ref._units([align_ref.codes(u) for u in ("A", "TG", "AAT")])
    for penalty in (1, 3, 64):
        recs, jstar, dirs = D.dirs_units(X, lens, Tm, ks, penalty)
        for r, x in enumerate(xs):
            full = T.table(x, [int(v) for v in Tm[r, :ks[r]]], penalty)
            assert full[0] == tuple(int(v) for v in recs[r]) and (not full[0][0] or full[1] == int(jstar[r]))
            for i in range(1, len(x) + 1):
                assert [o | (d << 2) for o, d in zip(full[2][i], full[3][i])] == dirs[r, i, :ks[r]].tolist()


@pytest.mark.parametrize("penalty", [1, 3, 64])
def test_host_against_reference_on_the_small_set(penalty):
    reads = [r for _, r in small_set()]
    want = D.decompose(reads, penalty=penalty)
    assert (want[1] > 0).sum() >= 20
    got = capi.decompose_host(reads, penalty=penalty)
    same(got, want)
    assert got[3] == len(want[0])
    same(capi.decompose_host(capi.pack_reads(reads), penalty=penalty), want)
    same(capi.decompose_host([r.lower() for r in reads], penalty=penalty), want)


def test_host_against_reference_on_the_fuzz_set(fuzz):
    reads, want, _ = fuzz
    assert (want[1] > 0).sum() >= 85 and len(want[0]) > 5000
    same(capi.decompose_host(reads), want)
    # other period ranges and thresholds: a wrong scored_period is traced as it is
    for args in ((1, 32, 3, 400), (7, 19, 3, 24), (1, 32, 5, 60)):
        same(capi.decompose_host(reads[::4], *args), D.decompose(reads[::4], *args))


def test_consequences_on_the_fuzz_set(fuzz):
    """every consequence of the definition (include/trew_hip.h), on the reference's results"""
    reads, (items, counts, recs), cols = fuzz
    refined = refine_ref.refine(reads)
    host_refined = capi.refine_host(reads)
    traced = 0
    for i, read in enumerate(reads):
        r = recs[i]
        # the record equals refine's in every field but reserved
        for f in refined.dtype.names:
            if f != "reserved":
                assert r[f] == refined[f][i] == host_refined[f][i]
        assert refined["reserved"][i] == 0
        its = items_of((items,), i)
        # a read has items if and only if period > 0 and score >= min_score
        has = int(r["period"]) > 0 and int(r["score"]) >= 24
        assert (len(its) > 0) == has == (counts[i] > 0)
        if not has:
            assert r["reserved"] == 0
            continue
        traced += 1
        k, start, end = int(r["period"]), int(r["start"]), int(r["end"])
        m_word = D.anchor_word(r)
        u = D.unit_codes(r["unit"], k)
        rho = int(r["reserved"])
        assert m_word == P.pack_unit(u[rho:] + u[:rho]) == min(P.pack_unit(u[q:] + u[:q]) for q in range(k))
        # the alignment record of the traced table equals R, for every rotation of the unit
        x = align_ref.codes(read)
        if i % 9 == 0:
            for q in (0, rho, k - 1):
                assert align_ref.align_strand(x, u[q:] + u[:q], 3) == tuple(int(r[f]) for f in ("score", "start", "end", "consumed", "matches"))
        # the items tile [start, end); bases, consumed and the errors sum to the record's
        at = start
        for it in its:
            assert it[0] == at and it[1] >= 1
            at += it[1]
        assert at == end and sum(it[1] for it in its) == end - start and sum(it[4] for it in its) == int(r["consumed"])
        c = capi.refine_columns(r, 3)
        assert [sum(it[q] for it in its) for q in (5, 6, 7)] == [int(c["mismatches"]), int(c["insertions"]), int(c["deletions"])]
        assert all(it[3] == 0 for it in its[1:])  # only the first item has a phase
        # for k >= 3 the items are the forward-strand items of trew_trace_host with the motif M
        if k >= 3:
            tr = capi.trace_host([read], [text_of(m_word, k)], 3, 24)
            assert [tup(it) for it in tr[0] if it["strand"] == 0] == its
            assert rec(tr[2][0, 0])[:5] == tuple(int(r[f]) for f in ("score", "start", "end", "consumed", "matches"))
        # a read's items do not depend on the rest of the batch
        if i % 5 == 0:
            alone = capi.decompose_host([read])
            assert items_of(alone, 0) == its and rec(alone[2][0]) == rec(r)
    assert traced >= 85


def test_a_perfect_repeat_begun_at_each_rotation():
    """(TTAGGG) x 10 begun at each of its six rotations: the same M = TTAGGG (T < G < C < A in the scan's order), the first item's
    phase follows the rotation; with flanks the reference says where the tract begins"""
    reads = rotation_reads(TEL, 10)
    got = capi.decompose_host(reads)
    same(got, D.decompose(reads))
    for q, read in enumerate(reads):
        r = got[2][q]
        assert text_of(D.anchor_word(r), 6) == TEL and text_of(capi.decompose_anchor(r), 6) == TEL
        its = items_of(got, q)
        if q == 0:
            assert its == [(0, 60, 10, 0, 60, 0, 0, 0)]
        else:
            assert its == [(0, 6 - q, 1, q, 6 - q, 0, 0, 0), (6 - q, 54, 9, 0, 54, 0, 0, 0), (60 - q, q, 1, 0, q, 0, 0, 0)]
    flanked = [FLANK + r + FLANK for r in reads]
    got = capi.decompose_host(flanked)
    want = D.decompose(flanked)
    same(got, want)
    assert {text_of(D.anchor_word(r), 6) for r in got[2]} == {TEL}
    assert [rec(x)[:ANCHOR_AT] for x in got[2]] == [D.decompose_read(r)[0][:ANCHOR_AT] for r in flanked]
    # every rotation of other units as well: one M a unit
    for unit in ("TG", "AAT", "GATTACAGGCTTAACGT"):
        got = capi.decompose_host(rotation_reads(unit, 20))
        k = len(unit)
        m = sorted({capi.decompose_anchor(r) for r in got[2]})
        assert len(m) == 1 and text_of(m[0], k) in [unit[q:] + unit[:q] for q in range(k)]
        first = [items_of(got, q)[0][3] for q in range(k)]
        assert first == [(first[0] + q) % k for q in range(k)] and sorted(first) == list(range(k))


ANCHOR_AT = refine_ref.FIELDS.index("reserved")


def test_hand_worked_vectors():
    # unit lengths 1 and 2: a run of copies of one and of two bases
    for read, k, unit, its in (("A" * 40, 1, "A", [(0, 40, 40, 0, 40, 0, 0, 0)]), ("TG" * 30, 2, "TG", [(0, 60, 30, 0, 60, 0, 0, 0)]),
                               ("GT" * 30, 2, "TG", [(0, 1, 1, 1, 1, 0, 0, 0), (1, 58, 29, 0, 58, 0, 0, 0), (59, 1, 1, 0, 1, 0, 0, 0)]),
                               ("ACGT" + "A" * 20 + "C" + "A" * 20 + "GT", 1, "A", [(4, 20, 20, 0, 20, 0, 0, 0), (24, 1, 1, 0, 1, 1, 0, 0), (25, 20, 20, 0, 20, 0, 0, 0)])):
        r, mine = D.decompose_read(read)
        assert r[0] == k and text_of(P.pack_unit(D.anchor(D.unit_codes(r[12], k))[1]), k) == unit and mine == its
        got = capi.decompose_host([read])
        assert items_of(got, 0) == its and rec(got[2][0]) == r
    # a palindromic unit: its reverse complement is itself, the strand is +
    read = "AATT" * 12
    got = capi.decompose_host([read])
    r = got[2][0]
    assert int(r["period"]) == 4 and P.canonical(r["unit"], 4) == D.anchor_word(r) == P.revcomp_word(D.anchor_word(r), 4)
    assert D.cli_lines(FQ, [read], got, 3)[0][2].split(",")[-4] == "+"
    same(got, D.decompose([read]))
    # a unit whose reverse complement has the smaller rotation: the strand is -
    got = capi.decompose_host(["CCCTAA" * 10])
    assert text_of(D.anchor_word(got[2][0]), 6) == "TAACCC" and text_of(P.canonical(got[2][0]["unit"], 6), 6) == TEL
    assert D.cli_lines(FQ, ["CCCTAA" * 10], got, 3)[0][2].split(",")[-5:] == ["TAACCC", "-", "9", "0", "ccc =9 taa"]
    # an N inside the tract: one copy with one mismatch
    read = T10[:14] + "N" + T10[15:]
    got = capi.decompose_host([read])
    assert items_of(got, 0) == [(0, 12, 2, 0, 12, 0, 0, 0), (12, 6, 1, 0, 6, 1, 0, 0), (18, 42, 7, 0, 42, 0, 0, 0)]
    assert D.decompose_read(read)[1] == items_of(got, 0) and int(got[2][0]["reserved"]) == 3  # the unit was cut as GGGTTA
    # the read whose re-voted unit scores lower: the seed is kept, and traced
    want = D.decompose_read(SEED_KEPT, 1, 32, 3, 10)
    got = capi.decompose_host([SEED_KEPT], 1, 32, 3, 10)
    assert want[0][:4] == (5, 5, 5, 0) and rec(got[2][0]) == want[0] and items_of(got, 0) == want[1] and len(want[1]) > 5
    # a refine record below min_score: no items, anchor 0; the empty read; a read without a periods record
    for read in (WEAK, "", "ACGTTGCATGCA"):
        got = capi.decompose_host([read])
        assert got[3] == 0 and got[1][0] == 0 and got[2][0]["reserved"] == 0 and rec(got[2][0]) == D.decompose_read(read)[0]
        assert D.decompose_read(read)[1] == []
    weak = capi.decompose_host([WEAK])[2][0]
    assert int(weak["period"]) > 0 and 0 < int(weak["score"]) < 24
    assert capi.decompose_host([WEAK], min_score=int(weak["score"]))[3] > 0


def test_end_phase_tie():
    """rule 3 against a read's own unit: two phases of row `end` hold the record's tuple, the smaller one is the end cell"""
    read, penalty, min_score, phases = END_TIE
    r, its = D.decompose_read(read, 1, 32, penalty, min_score)
    k = r[0]
    M = D.anchor(D.unit_codes(r[12], k))[1]
    for row0, row_end in ((0, None), (r[5], r[6])):  # the full table and the restarted one
        ties = {}
        arec, jstar, _, _ = T.table(align_ref.codes(read), M, penalty, row0=row0, row_end=row_end, ties=ties)
        assert arec == r[4:9] and ties["end"] == phases and jstar == phases[0]
    got = capi.decompose_host([read], 1, 32, penalty, min_score)
    assert rec(got[2][0]) == r and items_of(got, 0) == its and len(its) >= 3
    same(got, D.decompose([read], 1, 32, penalty, min_score))


def test_one_deleted_inserted_and_replaced_base_land_in_their_copy():
    """(TTAGGG) x 10 with one error at every position: away from the ends M is TTAGGG and the error lies in the copy it was made in"""
    run = lambda a, b: (a, b - a, (b - a) // 6, 0, b - a, 0, 0, 0)  # noqa: E731
    reads = [f(T10, at) for at in range(60) for f in (with_deletion, lambda r, a: with_insertion(r, a, "C"), replaced)]
    got = capi.decompose_host(reads)
    same(got, D.decompose(reads))
    for at in range(60):
        for q, kind in enumerate(("del", "ins", "sub")):
            i = 3 * at + q
            its = items_of(got, i)
            assert D.decompose_read(reads[i])[1] == its
            if kind == "del" and 6 <= at <= 55:
                c = 6 * (at // 6)
                assert its == [run(0, c)] * (c > 0) + [(c, 5, 1, 0, 6, 0, 0, 1)] + [run(c + 5, 59)] * (c + 5 < 59), at
            if kind == "ins" and 4 <= at <= 56:
                c = 6 * ((at - 1) // 6)  # an inserted base in front of a copy stays in the copy before it
                assert its == [run(0, c)] * (c > 0) + [(c, 7, 1, 0, 6, 0, 1, 0)] + [run(c + 7, 61)] * (c + 7 < 61), at
            if kind == "sub" and 4 <= at <= 55:
                c = 6 * (at // 6)
                assert its == [run(0, c)] * (c > 0) + [(c, 6, 1, 0, 6, 1, 0, 0)] + [run(c + 6, 60)] * (c + 6 < 60), at
            if its and 6 <= at <= 53:
                assert text_of(capi.decompose_anchor(got[2][i]), 6) == TEL


def test_host_cap_and_count(fuzz):
    reads = fuzz[0][:12]
    items, counts, records, n = capi.decompose_host(reads)
    assert n == len(items) == counts.sum() and n > 100
    part, counts2, records2, n2 = capi.decompose_host(reads, cap=5)
    assert n2 == n and len(part) == 5 and (part == items[:5]).all() and (counts2 == counts).all() and (records2 == records).all()
    none, _, _, n3 = capi.decompose_host(reads, cap=0)
    assert n3 == n and len(none) == 0
    # counts and records may be NULL; a min_score above every score gives no items
    lib = capi.load()
    words, offsets, lengths = capi.pack_reads(reads)
    got = C.c_uint64(0)
    assert lib.trew_decompose_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), 1, 32, 3, 24, None, 0, C.byref(got), None, None) == 0
    assert got.value == n
    top = int(records["score"].max())
    assert capi.decompose_host(reads, min_score=top + 1)[3] == 0 and capi.decompose_host(reads, min_score=100)[3] > 0


def test_signature_of_a_read():
    read = "ACGTACGT" + T10[:27] + "C" + T10[28:40] + T10[41:] + "ACGT"
    items, _, recs, _ = capi.decompose_host([read])
    assert text_of(capi.decompose_anchor(recs[0]), 6) == TEL
    sig = capi.trace_signature(items, read, 6)
    assert sig == T.signature(read, 6, 0, [tup(it) for it in items]) == (10, 2, "=4 TTACGG =1 TTAGG =3")


# ---- what the measure is for
def planted_figures(seed):
    """(reads, reads kept, reads with all three planted variants found by decompose, the same with the item a copy with that one
    error alone, the same by chain_ref given the true unit), by the reference alone.  Kept: refine reports the planted unit
    (its period and, as M, its smallest rotation).  Found: the item that holds the planted read position has exactly one
    mismatch, and the column of that position is the mismatch.  chain: a variant item at the planted copy's start with its bin."""
    cases = planted(seed)
    reads = [r for _, r, _ in cases]
    cols = {}
    items, counts, recs = D.decompose(reads, columns=cols)
    kept = found = alone = chained = 0
    for i, (unit, read, plants) in enumerate(cases):
        k = len(unit)
        r = recs[i]
        true_m = min(align_ref.codes(unit[q:] + unit[:q]) for q in range(k))
        if int(r["period"]) != k or int(r["score"]) < 24 or D.anchor(D.unit_codes(r["unit"], k))[1] != true_m:
            continue
        kept += 1
        subs = {b for kind, b, _ in cols[i] if kind == "sub"}
        a = b = 0
        for _, pos, _, _ in plants:
            it = next(it for it in items_of((items,), i) if it[0] <= pos < it[0] + it[1])
            hit = it[5] == 1 and pos in subs
            a += hit
            b += hit and it[6] == 0 and it[7] == 0 and it[4] == k
        found += a == 3
        alone += b == 3
        fwd = chain_ref.chain_read_marks(read, unit)[0]
        chained += sum(any(bn != chain_ref.NONE and st == pos - j and bn == 4 * j + chain_ref.CODE[base] for st, _, bn in fwd)
                       for _, pos, j, base in plants) == 3
    return len(cases), kept, found, alone, chained


def test_planted_variant_units_are_found_without_the_motif():
    """60 reads of (unit) x m, k = 3 .. 12, m = 40 .. 60, three planted one-substitution copies each, indels at 0.04 elsewhere
    (decompose_cases.planted).  By the reference alone, over the committed seed and its eight neighbours (reads kept / all three
    found / found in an item with that error alone / chain_ref given the true unit, over the kept reads):
        20251019: 58 / 57 / 45 / 50        neighbours: kept 59 .. 60, found 57 .. 60, alone 42 .. 51, chain 44 .. 57
    The spread over the neighbours is 3 reads for found and 13 for chain; the committed seed's figures are asserted with these
    margins.  At most a quarter of the reads may be left out (refine does not report the planted unit): two are, reads whose
    scored_period is a multiple of the unit length.  `alone` is smaller because the copies are cut at M, not where the generator
    cut them: a copy of M that holds a planted base usually also holds a piece of the noisy neighbour copy, with its indels."""
    n, kept, found, alone, chained = planted_figures(PLANTED_SEED)
    print("reads %d, kept %d, all three found %d, in an item with that error alone %d, chain given the unit %d" % (n, kept, found, alone, chained))
    assert n == 60 and 4 * kept >= 3 * n
    assert found >= 57 - 3
    assert abs(chained - 50) <= 13
    assert found <= kept and alone <= found


# ---- the stand-alone harness under sanitizers
def test_definition_runs_clean_under_sanitizers_and_agrees_with_the_library(tmp_path, fuzz):
    exe = str(tmp_path / "decompose_host_harness")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "decompose_host_harness.cpp"), os.path.join(CSRC, "trew_measures_host.cpp")], check=True)
    reads = [r.upper().encode() for r in fuzz[0][::4]] + [r.upper().encode() for _, r in small_set()[:8]] + [b"", b"A", b"A" * 50, b"TG" * 40, TEL.encode() * 400]

    def text(items, counts, records):
        return ("".join(" ".join(str(int(v)) for v in it) + "\n" for it in items) + "".join("%d " % c for c in counts) + "\n"
                + "".join(" ".join(str(int(x[f])) for f in refine_ref.FIELDS) + "\n" for x in records))

    for args, cap in (((1, 32, 1, 24), 1 << 20), ((1, 32, 3, 24), 1 << 20), ((1, 32, 64, 10), 1 << 20), ((5, 32, 3, 24), 7), ((1, 32, 3, 24), 0)):
        r = subprocess.run([exe, *[str(a) for a in args], str(cap)], input=b"".join(x + b"\n" for x in reads), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stderr == b""
        items, counts, records, n = capi.decompose_host(reads, *args)
        assert n > (100 if args[2] < 64 else 5)
        assert r.stdout.decode() == "%d\n" % n + text(items[:cap], counts, records)
    r = subprocess.run([exe, "1", "32", "3", "24", "4"], input=b"\n\n", capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stdout == b"0\n0 0 \n" + b"0 0 0 0 0 0 0 0 0 0 0 0 0 0\n" * 2 and r.stderr == b""
    r = subprocess.run([exe, "0", "32", "3", "24", "4"], input=b"ACGT\n", capture_output=True, timeout=60)
    assert r.returncode == 3 and b"min_period" in r.stderr


# ---- ABI and errors
def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.TraceItem) == 48 and C.sizeof(capi.Refined) == 64
    for sym in ("trew_hip_decompose", "trew_hip_decompose_results", "trew_decompose_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None
    hdr = open(os.path.join(ROOT, "include", "trew_hip.h")).read()
    assert "#define TREW_HIP_ABI_VERSION 4" in hdr and "int trew_hip_decompose(" in hdr


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    for lo, hi in ((0, 32), (1, 33), (7, 6)):
        with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
            capi.decompose_host(reads, lo, hi)
    for penalty in (0, 65, -1):
        with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
            capi.decompose_host(reads, 1, 32, penalty)
    with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
        capi.decompose_host(reads, 1, 32, 3, 0)
    lib = capi.load()
    n = C.c_uint64(0)
    assert lib.trew_decompose_host(None, None, None, 1, 1, 32, 3, 24, None, 0, C.byref(n), None, None) != 0
    assert b"trew_decompose_host: null argument" in lib.trew_hip_last_error(None)
    assert lib.trew_decompose_host(None, None, None, 0, 1, 32, 3, 24, None, 0, None, None, None) != 0
    assert lib.trew_decompose_host(None, None, None, 0, 1, 32, 3, 24, None, 4, C.byref(n), None, None) != 0  # a capacity without a buffer
    assert lib.trew_decompose_host(None, None, None, 0, 1, 32, 3, 24, None, 0, C.byref(n), None, None) == 0 and n.value == 0  # no reads


def test_device_entry_points_refuse_a_missing_context():
    """the argument errors of the device calls that need no GPU: without a context the status is -1 and nothing is touched"""
    lib = capi.load()
    n, rows = C.c_uint64(7), C.c_uint64(9)
    assert lib.trew_hip_decompose(None, None, 0, 1, 32, 3, 24, 16, 16) == -1
    assert lib.trew_hip_decompose_results(None, 0, None, 0, C.byref(n), C.byref(rows), None, None, None) == -1 and (n.value, rows.value) == (7, 9)


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_decompose.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.decompose([b"TTAGGGTTAGGG"])
    r = subprocess.run([TREW, "decompose", FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["decompose"], "FASTQ is required."),
        (["decompose", FQ, "--min_period", "0"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["decompose", FQ, "--max_period", "33"], "MIN_PERIOD and MAX_PERIOD must be in range 1 to 32."),
        (["decompose", FQ, "--min_period", "7", "--max_period", "6"], "MIN_PERIOD must not be greater than MAX_PERIOD."),
        (["decompose", FQ, "--min_period", "x"], "MIN_PERIOD must be a number."),
        (["decompose", FQ, "--max_period", "x"], "MAX_PERIOD must be a number."),
        (["decompose", FQ, "--penalty", "x"], "PENALTY must be a number."),
        (["decompose", FQ, "--penalty", "0"], "PENALTY must be in range 1 to 64."),
        (["decompose", FQ, "--penalty", "65"], "PENALTY must be in range 1 to 64."),
        (["decompose", FQ, "--min_score", "0"], "MIN_SCORE must be greater than or equal to 1."),
        (["decompose", FQ, "--min_score", "x"], "MIN_SCORE must be a number."),
        (["decompose", FQ, "--items", "3"], "3 : file not found"),
        (["decompose", FQ, "-t", "0"], "number of threads must be positive."),
        (["decompose", FQ, "--bogus"], "Unknown argument: --bogus"),
        (["decompose", "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["decompose", FQ, "--devices", "0,x"], "Usage: decompose"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: decompose" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_decompose():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "decompose" in r.stderr and "refine" in r.stderr and "trace" in r.stderr and "short" in r.stderr
    r = subprocess.run([TREW, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "  decompose " in r.stderr
    r = subprocess.run([TREW, "decompose", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: decompose" in r.stderr and "--penalty" in r.stderr and "--min_period" in r.stderr and "--items" in r.stderr and r.stdout == ""
