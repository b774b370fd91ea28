"""Gap-tolerant motif intervals, the parts that need no GPU: the brute-force reference against hand-worked vectors and
against itself, the host implementation (trew_intervals_host) against the reference, invariants that tie the intervals to
the annotation and the tracts, the sort order and the cap / found contract, the additive ABI, the argument errors of the
entry points and of `trew intervals`."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as A
import interval_cases as K
import interval_ref as R
import tract_ref as T
from trew_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
FQ = os.path.join(ROOT, "tests", "golden", "test.fastq")
TEL = K.TEL

# 10 bases of spacer, four units, one unit with a substitution (base 35 is the only one it leaves uncovered), three units,
# 13 bases of spacer of which the first two complete a window and the last continues the rotated repeat behind it (11
# uncovered bases), two rotated units, two bases
WORKED = "ACGTACGTAC" + "TTAGGG" * 4 + "TCAGGG" + "TTAGGG" * 3 + "ACGTACGTACGTA" + "GGGTTA" * 2 + "AC"

HAND = [
    # read, motif, max_gap, min_len, forward, reverse
    (WORKED, TEL, 0, 1, [(10, 35, 25), (36, 58, 22), (69, 83, 14)], []),
    (WORKED, TEL, 1, 1, [(10, 58, 47), (69, 83, 14)], []),
    (WORKED, TEL, 10, 1, [(10, 58, 47), (69, 83, 14)], []),
    (WORKED, TEL, 11, 1, [(10, 83, 61)], []),
    (WORKED, TEL, 2 ** 32 - 1, 1, [(10, 83, 61)], []),
    (WORKED, TEL, 0, 23, [(10, 35, 25)], []),  # min_len: 22 and 14 bases are dropped
    (WORKED, TEL, 0, 22, [(10, 35, 25), (36, 58, 22)], []),
    (WORKED, TEL, 1, 49, [], []),
    ("TTAGGG" * 5, TEL, 0, 30, [(0, 30, 30)], []),  # begins at base 0, ends at n, exactly min_len
    ("TTAGGG" * 5, TEL, 0, 31, [], []),
    ("CCCTAA" * 3 + "GATTACA", TEL, 0, 1, [], [(0, 18, 18)]),
    ("ACGT" * 4, "ACGT", 0, 1, [(0, 16, 16)], [(0, 16, 16)]),  # a self-reverse-complementary class: both strands
    ("TTAGG", TEL, 0, 1, [], []),  # n < k
    ("", TEL, 0, 1, [], []),
    ("ttagggTTAGGGttaggg", TEL, 0, 1, [(0, 18, 18)], []),  # lower-case bases are bases
    ("TTAGGGTTAGGGNTTAGGGTTAGGG", TEL, 0, 1, [(0, 12, 12), (13, 25, 12)], []),  # an N is an uncovered base
    ("TTAGGGTTAGGGNTTAGGGTTAGGG", TEL, 1, 1, [(0, 25, 24)], []),
    ("NNNNNNNN", TEL, 5, 1, [], []),
]


@pytest.mark.parametrize("read,motif,max_gap,min_len,fwd,rev", HAND)
def test_hand_worked_vectors(read, motif, max_gap, min_len, fwd, rev):
    assert R.intervals_read(read, motif, max_gap, min_len) == (fwd, rev)
    for recs, counts in (R.intervals([read], [motif], max_gap, min_len), capi.intervals_host([read], [motif], max_gap, min_len)[:2]):
        assert K.triples(recs, strand=0) == fwd and K.triples(recs, strand=1) == rev
        assert counts.tolist() == [[[len(fwd), len(rev)]]]


def test_worked_example_gaps():
    """what the issue's table rests on: n = 85, one uncovered base at 35, eleven in the spacer"""
    cov = R.coverage_read(WORKED, TEL)[0]
    assert len(WORKED) == 85
    assert [p for p in range(10, 83) if not cov[p]] == [35] + list(range(58, 69))
    assert sum(cov) == 61 and not any(cov[:10]) and not any(cov[83:])


def test_reference_forms_agree():
    rnd = random.Random(1)
    reads = [bytes(rnd.choice(b"ACGTACGTNa") for _ in range(rnd.randint(0, 80))) for _ in range(150)]
    reads += [b"TTAGGG" * 9, b"AATAATAATAATCCCTAACCCTAACCCTAA", b"TTAGGGTTAGGcTTAGGGTTnGGGTTAGGGACGTTTAGGGTTAGGG", WORKED.encode()]
    motifs = ["AAT", TEL, "TGTG", "AAAA"]
    for max_gap, min_len in ((0, 1), (2, 1), (7, 5), (100, 12)):
        recs, counts = R.intervals(reads, motifs, max_gap, min_len)
        for r, read in enumerate(reads):
            for m, motif in enumerate(motifs):
                fwd, rev = R.intervals_read(read, motif, max_gap, min_len)
                assert K.triples(recs, r, m, 0) == fwd and K.triples(recs, r, m, 1) == rev
                assert counts[r, m].tolist() == [len(fwd), len(rev)]


@pytest.fixture(scope="module")
def ragged():
    reads = K.ragged_reads()
    want = {rule: R.intervals(reads, K.RAGGED_MOTIFS, *K.rule_values(rule, K.RAGGED_MOTIFS)) for rule in K.RULES}
    return reads, want


@pytest.fixture(scope="module")
def generator_long():
    reads = K.long_reads()
    return reads, R.intervals(reads, [TEL], 18, 24)  # the defaults 3 k and 4 k


@pytest.mark.parametrize("rule", K.RULES, ids=lambda r: "%s-%s" % r)
def test_host_ragged_with_n_and_lower_case(ragged, rule):
    reads, want = ragged
    recs, counts = want[rule]
    for mi in range(len(K.RAGGED_MOTIFS)):  # not vacuous: every motif has intervals on many reads
        assert (counts[:, mi].sum(axis=1) > 0).sum() >= 50
    got = capi.intervals_host(reads, K.RAGGED_MOTIFS, *K.rule_values(rule, K.RAGGED_MOTIFS))
    K.same(got, want[rule])
    assert got[2] == len(recs)
    # the counts array equals the per-key number of records
    per_key = np.zeros_like(counts)
    np.add.at(per_key, (got[0]["read"], got[0]["motif"], got[0]["strand"]), 1)
    assert (per_key == got[1]).all()


def test_host_generator_long_reads_at_the_defaults(generator_long):
    reads, want = generator_long
    recs = want[0]
    # not vacuous, by the reference alone: planted 2-6 kb tails come back as long intervals on both strands
    ln = recs["end"].astype(np.int64) - recs["start"]
    assert ((ln >= 1500) & (recs["strand"] == 0)).sum() >= 5 and ((ln >= 1500) & (recs["strand"] == 1)).sum() >= 5
    got = capi.intervals_host(reads, [TEL])  # None: the defaults
    K.same(got, want)
    K.same(capi.intervals_host(reads, [TEL], 18, 24), want)


def test_covered_sums_to_the_tracts_covered(ragged, generator_long):
    """min_len = 1 drops nothing: the covered bases of a key's intervals are all of its covered bases, whatever max_gap"""
    reads, want = ragged
    tr = T.tracts(reads, K.RAGGED_MOTIFS, 3)
    for rule in K.RULES:
        if rule[1] != 1:
            continue
        recs = want[rule][0]
        for strand, name in enumerate(("covered_fwd", "covered_rev")):
            total = np.zeros(tr.shape, dtype=np.int64)
            sel = recs[recs["strand"] == strand]
            np.add.at(total, (sel["read"], sel["motif"]), sel["covered"])
            assert (total == tr[name]).all()
    lreads, _ = generator_long
    recs = R.intervals(lreads, [TEL], 7, 1)[0]
    tr = T.tracts(lreads, [TEL], 3)
    for strand, name in enumerate(("covered_fwd", "covered_rev")):
        total = np.zeros(len(lreads), dtype=np.int64)
        sel = recs[recs["strand"] == strand]
        np.add.at(total, sel["read"], sel["covered"])
        assert (total == tr[name][:, 0]).all()


def test_gap_zero_contains_the_longest_uninterrupted_tract(ragged):
    reads, want = ragged
    recs = want[(0, 1)][0]
    an = A.annotate(reads, K.RAGGED_MOTIFS)
    checked = 0
    for strand, sfx in enumerate(("fwd", "rev")):
        for r, m in np.argwhere(an["tract_len_" + sfx] > 0):
            s, ln = int(an["tract_start_" + sfx][r, m]), int(an["tract_len_" + sfx][r, m])
            assert any(a <= s and s + ln <= b for a, b, _ in K.triples(recs, r, m, strand)), (r, m, strand)
            checked += 1
    assert checked >= 1000


def test_growing_the_gap_only_merges(ragged):
    reads, want = ragged
    order = [(0, 1), (1, 1), (40, 1), (5000, 1)]
    for small, large in zip(order, order[1:]):
        a, b = want[small][0], want[large][0]
        assert len(b) < len(a)
        # every interval at the smaller gap lies inside one at the larger: find the last one of its key that starts at or before it
        key_b = (b["read"].astype(np.int64) << 8 | b["motif"] << 1 | b["strand"]) << 32 | b["start"]
        key_a = (a["read"].astype(np.int64) << 8 | a["motif"] << 1 | a["strand"]) << 32 | a["start"]
        at = np.searchsorted(key_b, key_a, side="right") - 1
        assert (at >= 0).all()
        host = b[at]
        assert ((host["read"] == a["read"]) & (host["motif"] == a["motif"]) & (host["strand"] == a["strand"])).all()
        assert ((host["start"] <= a["start"]) & (a["end"] <= host["end"])).all()


def test_sort_order_cap_and_found():
    reads = K.ragged_reads(300)
    recs, counts, found = capi.intervals_host(reads, K.RAGGED_MOTIFS, 0, 1)
    assert found == len(recs) == int(counts.sum()) and found > 1000
    key = [tuple(int(x[f]) for f in ("read", "motif", "strand", "start")) for x in recs]
    assert key == sorted(key) and len(set(key)) == len(key)
    # a smaller buffer: found is still exact and so are the counts; the records are the first ones of the order
    for cap in (0, 1, 7, found - 1, found, found + 5):
        part, pcounts, pfound = capi.intervals_host(reads, K.RAGGED_MOTIFS, 0, 1, cap=cap)
        assert pfound == found and (pcounts == counts).all()
        assert len(part) == min(cap, found) and (part == recs[:len(part)]).all()
    # packed planes are accepted as they are
    K.same(capi.intervals_host(capi.pack_reads(reads), K.RAGGED_MOTIFS, 0, 1), (recs, counts))


def test_per_motif_rules():
    reads = K.ragged_reads(300)
    gaps, mins = [0, 3, 40, 2 ** 32 - 1], [1, 9, 2, 30]
    K.same(capi.intervals_host(reads, K.RAGGED_MOTIFS, gaps, mins), R.intervals(reads, K.RAGGED_MOTIFS, gaps, mins))


def test_host_rejects_bad_arguments():
    reads = [b"ACGTACGT"]
    with pytest.raises(capi.TrewHipError, match="min_len must be at least 1"):
        capi.intervals_host(reads, ["AAT"], 0, 0)
    with pytest.raises(capi.TrewHipError, match="min_len must be at least 1"):
        capi.intervals_host(reads, ["AAT", "TGTG"], 0, [5, 0])
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.intervals_host(reads, ["AAT"] * 9, 0, 1)
    with pytest.raises(capi.TrewHipError, match="n_motifs"):
        capi.intervals_host(reads, [], 0, 1)
    with pytest.raises(capi.TrewHipError, match="k must be"):
        capi.intervals_host(reads, [capi.Motif(33, 0, 0)], 0, 1)
    with pytest.raises(capi.TrewHipError, match="2 values for 1 motifs"):
        capi.intervals_host(reads, ["AAT"], [0, 1], 1)
    # null pointers, straight at the C entry point
    lib = capi.load()
    words, offsets, lengths = capi.pack_reads(reads)
    m = (capi.Motif * 1)(capi.motif("AAT"))
    rule = (capi.IntervalRule * 1)(capi.IntervalRule(0, 1))
    n = C.c_uint64(0)
    out = np.zeros(4, dtype=capi.INTERVAL_DTYPE)
    args = [words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, 1, m, rule, 1, out.ctypes.data, 4, C.byref(n), None]
    assert lib.trew_intervals_host(*args) == 0 and n.value == 0
    for i, text in ((0, "null argument"), (1, "null argument"), (2, "null argument"), (4, "motifs is NULL"), (5, "rules must not be null"),
                    (7, "null argument"), (9, "null argument")):
        bad = list(args)
        bad[i] = None
        assert lib.trew_intervals_host(*bad) != 0
        assert text in lib.trew_hip_last_error(None).decode()


def test_abi_is_additive():
    lib = capi.load()
    assert lib.trew_hip_abi_version() == 4
    assert C.sizeof(capi.Interval) == 24 and capi.INTERVAL_DTYPE.itemsize == 24 and C.sizeof(capi.IntervalRule) == 8
    assert tuple(capi.INTERVAL_DTYPE.names) == R.FIELDS == tuple(n for n, _ in capi.Interval._fields_)
    assert [n for n, _ in capi.IntervalRule._fields_] == ["max_gap", "min_len"]
    assert C.sizeof(capi.Motif) == 16 and C.sizeof(capi.Annot) == 24 and C.sizeof(capi.Tract) == 40
    for sym in ("trew_hip_intervals", "trew_hip_intervals_results", "trew_intervals_host"):
        assert sym in capi.EXPORTED_SYMBOLS and getattr(lib, sym) is not None


def test_compute_fails_loudly_without_gpu():
    import torch
    import trew_amd

    if torch.cuda.is_available():
        return  # with a GPU the same calls are checked for their results (test_gpu_intervals.py)
    with pytest.raises(capi.TrewHipError):
        trew_amd.intervals([b"TTAGGGTTAGGG"], [TEL])
    r = subprocess.run([TREW, "intervals", TEL, FQ], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and "no HIP device" in r.stderr


@pytest.mark.parametrize(
    "args,msg",
    [
        (["intervals"], "MOTIF is required."),
        (["intervals", TEL], "FASTQ is required."),
        (["intervals", "TTAGGN", FQ], "must consist of A, C, G and T."),
        (["intervals", "TTAGGG,", FQ], "the length must be in range 3 to 32."),
        (["intervals", "AC", FQ], "the length must be in range 3 to 32."),
        (["intervals", "A" * 33, FQ], "the length must be in range 3 to 32."),
        (["intervals", ",".join(["AAT"] * 9), FQ], "At most 8 motifs can be given."),
        (["intervals", TEL, FQ, "--max_gap", "x"], "MAX_GAP must be a number in range 0 to 4294967295."),
        (["intervals", TEL, FQ, "--max_gap", "-1"], "MAX_GAP must be a number in range 0 to 4294967295."),
        (["intervals", TEL, FQ, "--max_gap", "4294967296"], "MAX_GAP must be a number in range 0 to 4294967295."),
        (["intervals", TEL, FQ, "--min_len", "0"], "MIN_LEN must be a number in range 1 to 4294967295."),
        (["intervals", TEL, FQ, "--min_len", "x"], "MIN_LEN must be a number in range 1 to 4294967295."),
        (["intervals", TEL, FQ, "--min_len"], "--min_len: expected 1 argument(s). 0 provided."),
        (["intervals", TEL, FQ, "-t", "0"], "number of threads must be positive."),
        (["intervals", TEL, FQ, "--bogus"], "Unknown argument: --bogus"),
        (["intervals", TEL, FQ, "--penalty", "3"], "Unknown argument: --penalty"),
        (["intervals", TEL, "/nonexistent.fastq"], "/nonexistent.fastq : file not found"),
        (["intervals", TEL, FQ, "--devices", "0,x"], "Usage: intervals"),
    ],
)
def test_cli_argument_errors(args, msg):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert msg in r.stderr and "Usage: intervals" in r.stderr
    assert r.stdout == ""


def test_cli_usage_lists_intervals():
    r = subprocess.run([TREW], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "intervals" in r.stderr and "tracts" in r.stderr and "annotate" in r.stderr
    r = subprocess.run([TREW, "intervals", "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "Usage: intervals" in r.stderr and "--max_gap" in r.stderr and "--min_len" in r.stderr and r.stdout == ""
