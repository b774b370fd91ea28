"""Gap-tolerant motif intervals on the GPU (trew_hip_intervals through ctypes) against the brute-force reference of
interval_ref.py.  Every record and every count of every batch is compared, integer for integer, after sorting."""
import ctypes as C
import gzip
import os
import random
import subprocess

import numpy as np
import pytest

import annot_ref as A
import interval_cases as K
import interval_ref as R
import oracle as O
import tract_ref as T
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
TEL = K.TEL
BIG = 1 << 18  # a log no test batch fills


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_intervals(reads, motifs, max_gap, min_len, max_intervals=BIG, mode=capi.MODE_SHORT, contiguous=False):
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        t.intervals(t.host_batch(words, offsets, lengths, contiguous=contiguous), motifs, max_gap, min_len, max_intervals)
        return t.intervals_results()


def rep(n, unit=TEL):
    return (unit * (n // len(unit) + 2))[:n]


def short_reads(n):
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, 150)
    return [buf[s:e + 1] for s, e in zip(st, nd)]


# ---- gap edges at every seam
def seam_reads(g):
    """Reads of two perfect repeat blocks with exactly g uncovered bases between them (a spacer of C: no window that holds a
    C is a rotation of TTAGGG), the gap [e - g, e) placed so that it ends at bit 31 / 32 / 33 of a word, straddles a word
    boundary, ends at or straddles the iteration boundary 2047 / 2048.  Returns [(read, e)]."""
    wb = 32 * ((g + 12 + 31) // 32) + 32  # a word boundary with room for the gap and a block in front of it
    ends = {wb - 1, wb, wb + 1, wb + g // 2, wb + 1 + g // 2, 2047, 2048, 2049, 2048 + g // 2, 2048 + (g + 1) // 2}
    out = []
    for e in sorted(ends):
        if e - g >= 6:
            out.append((rep(e - g) + "C" * g + TEL * 4 + "CC", e))
    return out


def check_seams(t, G, gs, placed):
    for g in gs:
        reads = [r for r, _ in placed(g)]
        want = R.intervals(reads, [TEL], G, 1)
        # under the reference: the uncovered gap is exactly g, merged at g <= G and split at g = G + 1
        for i, (read, e) in enumerate(placed(g)):
            if i < 3 or g > 1000:
                cov = R.coverage_read(read, TEL)[0]
                assert [p for p in range(len(read) - 2) if not cov[p]] == list(range(e - g, e))
            assert K.triples(want[0], i) == ([(0, e + 24, e + 24 - g)] if g <= G else [(0, e - g, e - g), (e, e + 24, 24)])
        t.intervals(t.host_batch(*capi.pack_reads(reads)), [TEL], G, 1, BIG)
        K.same(t.intervals_results(), want)


def test_gap_edges_at_word_and_iteration_seams():
    with ctx() as t:
        for G in (0, 1, 5, 31, 32, 33, 100):
            check_seams(t, G, (G, G + 1), seam_reads)


def test_gap_over_a_whole_uncovered_iteration():
    def placed(g):  # the gap [2040, 2040 + g) holds all of iteration 1 (bases 2048 .. 4095)
        assert g >= 2100
        return [(rep(2040) + "C" * g + TEL * 4 + "CC", 2040 + g), (rep(100) + "C" * g + TEL * 4 + "CC", 100 + g)]

    with ctx() as t:
        check_seams(t, 2100, (2100, 2101), placed)


# ---- interval shapes
def test_interval_shapes():
    reads = [TEL]  # n = k
    for n in (31, 32, 33, 2047, 2048, 2049, 4096):
        reads.append("C" * 9 + rep(n - 9))  # ends at n
        reads.append(rep(n - 9) + "C" * 9)  # begins at base 0
        reads.append(rep(n))  # both
    reads.append(rep(6200))  # three iterations and a piece
    reads.append("C" * 5 + rep(6190) + "C" * 5)
    reads.append("C" * 2000 + rep(4200))
    want = R.intervals(reads, [TEL], 0, 1)
    assert K.triples(want[0], 0) == [(0, 6, 6)] and K.triples(want[0], 1) == [(9, 31, 22)] and K.triples(want[0], 22) == [(0, 6200, 6200)]
    assert K.triples(want[0], 23) == [(5, 6195, 6190)] and int(want[1].sum()) == len(reads)
    K.same(gpu_intervals(reads, [TEL], 0, 1), want)
    K.same(gpu_intervals(reads, [TEL], 18, 24), R.intervals(reads, [TEL], 18, 24))


def test_min_len_edge():
    """one interval of exactly L bases is kept, one of L - 1 is dropped, in the same read; both orders, L across a word"""
    reads, keep = [], []
    for L in (7, 30, 33, 2049):
        reads.append(rep(L) + "C" * 20 + rep(L - 1) + "CCC")
        keep.append((0, L, L))
        reads.append("C" + rep(L - 1) + "C" * 20 + rep(L))
        keep.append((L + 20, 2 * L + 20, L))
    for i, L in enumerate((7, 7, 30, 30, 33, 33, 2049, 2049)):
        one = [reads[i]]
        want = R.intervals(one, [TEL], 0, L)
        assert K.triples(want[0]) == [keep[i]] and int(R.intervals(one, [TEL], 0, L - 1)[1].sum()) == 2
        K.same(gpu_intervals(one, [TEL], 0, L), want)


# ---- many starts in one word
def busy_reads():
    """k = 3, max_gap 0: `AATC` units give eight intervals of three bases per word, in every word of every lane; the units of
    some reads are shifted or belong to the other strand"""
    reads = []
    for i in range(64):
        unit = ("AATC", "ATCA", "GATT", "CAAT")[i % 4]
        reads.append(rep(2048, unit))
    return reads


def test_many_starts_in_every_word():
    reads = busy_reads()
    want = R.intervals(reads, ["AAT"], 0, 1)
    assert want[1][0].tolist() == [[512, 0]] and want[1][2].tolist() == [[0, 512]] and len(want[0]) >= 64 * 511
    assert K.triples(want[0], 0)[:3] == [(0, 3, 3), (4, 7, 3), (8, 11, 3)]
    K.same(gpu_intervals(reads, ["AAT"], 0, 1), want)
    K.same(gpu_intervals(reads, ["AAT"], 0, 3), want)  # every interval sits exactly on min_len
    got = gpu_intervals(reads, ["AAT"], 0, 4)
    assert got[2] == 0 and len(got[0]) == 0 and not got[1].any()


# ---- degenerate reads
def test_degenerate_reads():
    reads = ["", "T", "TTAGG", "N" * 31, "N" * 5000, "", rep(40)[:20] + "N" + rep(40)[21:], rep(4200)[:2048] + "N" + rep(4200)[2049:],
             "ttagggTTAGGGttaggg", "n" * 7 + rep(30).lower() + "N", TEL, ""]
    for G, L in ((0, 1), (1, 1), (18, 24)):
        want = R.intervals(reads, [TEL], G, L)
        K.same(gpu_intervals(reads, [TEL], G, L), want)
    want = R.intervals(reads, [TEL], 0, 1)
    assert want[1][:6].sum() == 0 and K.triples(want[0], 6) == [(0, 20, 20), (21, 40, 19)] and K.triples(want[0], 8) == [(0, 18, 18)]
    # a batch of nothing but empty reads
    got = gpu_intervals(["", "", ""], [TEL], 0, 1)
    assert got[2] == 0 and got[1].shape == (3, 1, 2) and not got[1].any()


# ---- overflow
def test_overflow_protocol():
    reads = busy_reads()[:4] + [rep(100), "C" * 50]
    want = R.intervals(reads, ["AAT", TEL], 0, 1)
    F = len(want[0])
    assert F >= 1000
    ref_keys = {tuple(int(v) for v in x) for x in want[0]}
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(words=1 << 14, reads=16) as t:
        b = t.host_batch(words, offsets, lengths)
        for cap in (1, F - 1):
            t.intervals(b, ["AAT", TEL], 0, 1, cap)  # no error: the call returns 0
            recs, counts, found = t.intervals_results()
            assert found == F and (counts == want[1]).all()
            assert len(recs) == cap
            keys = [tuple(int(v) for v in x) for x in recs]
            assert len(set(keys)) == cap and set(keys) <= ref_keys and keys == sorted(keys)
        t.intervals(b, ["AAT", TEL], 0, 1, F)  # the retry: exactly enough
        K.same(t.intervals_results(), want)
        # a smaller call on the same slot afterwards: nothing stale left over
        small = ["C" * 9 + rep(31), "ACGT" * 5]
        t.intervals(t.host_batch(*capi.pack_reads(small)), [TEL], 0, 1, 8)
        got = t.intervals_results()
        K.same(got, R.intervals(small, [TEL], 0, 1))
        assert got[2] == 1
        # a caller's buffer smaller than the log: found is reported, the first `cap` of the sorted records are copied
        t.intervals(b, ["AAT", TEL], 0, 1, F)
        n = C.c_uint64(0)
        few = np.zeros(5, dtype=capi.INTERVAL_DTYPE)
        assert t.lib.trew_hip_intervals_results(t.ctx, 0, few.ctypes.data, 5, C.byref(n), None, None) == 0
        assert n.value == F and (few == want[0][:5]).all()


def test_convenience_entry_point_retries_once():
    """`trew intervals` starts every batch with a log of one record per read and resubmits on overflow; the same protocol
    through trew_amd.intervals, whose first log is made too small on purpose"""
    import trew_amd

    reads = busy_reads()[:3] + [rep(300)]
    want = R.intervals(reads, ["AAT"], 0, 1)
    assert len(want[0]) > 1000 > len(reads)
    K.same(trew_amd.intervals(reads, ["AAT"], 0, 1), want)  # default log: one record per read, so this call retries
    K.same(trew_amd.intervals(reads, ["AAT"], 0, 1, max_intervals=2), want)
    K.same(trew_amd.intervals(reads, [TEL]), R.intervals(reads, [TEL], 18, 24))  # the defaults 3 k and 4 k; no retry


# ---- mixed batches
@pytest.fixture(scope="module")
def ragged():
    return K.ragged_reads()


@pytest.fixture(scope="module")
def generator_long():
    reads = K.long_reads()
    return reads, R.intervals(reads, [TEL], 18, 24)


@pytest.mark.parametrize("rule", K.RULES, ids=lambda r: "%s-%s" % r)
def test_ragged(ragged, rule):
    gaps, mins = K.rule_values(rule, K.RAGGED_MOTIFS)
    K.same(gpu_intervals(ragged, K.RAGGED_MOTIFS, gaps, mins), R.intervals(ragged, K.RAGGED_MOTIFS, gaps, mins))


def test_generator_long_reads_at_the_defaults(generator_long):
    reads, want = generator_long
    ln = want[0]["end"].astype(np.int64) - want[0]["start"]
    assert (ln >= 1500).sum() >= 10
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(mode=capi.MODE_LONG, words=len(words) + 64, reads=K.LONG_N) as t:
        t.intervals(t.host_batch(words, offsets, lengths), [TEL])  # every default: rules and one log record per read
        got = t.intervals_results(want_ms=True)
        assert got[3] > 0
        K.same(got, want)


def test_eight_motifs_with_rules_of_their_own():
    rnd = random.Random(2025)
    u12, u31, u32 = ("".join(rnd.choice("ACGT") for _ in range(k)) for k in (12, 31, 32))
    motifs = ["AAT", "TGTG", "CCCTA", TEL, "GGGTTAG", u12, u31, u32]
    gaps = [0, 4, 5, 18, 2 ** 32 - 1, 31, 100, 2100]
    mins = [1, 16, 1, 24, 50, 12, 31, 1]
    reads = []
    for i in range(64):
        n = rnd.randint(1000, 10000)
        unit = motifs[i % 8] if i % 3 else A.revcomp(motifs[i % 8])
        rate = min(0.05, 0.2 / len(unit))
        parts = []
        while sum(len(p) for p in parts) < n:
            ln = rnd.randint(20, 3000)
            if rnd.random() < 0.5:
                s = rep(ln, unit)
                parts.append("".join(rnd.choice([x for x in "ACGT" if x != c]) if rnd.random() < rate else c for c in s))
            else:
                parts.append("".join(rnd.choice("ACGTACGTACGTN") for _ in range(ln)))
        reads.append("".join(parts)[:n])
    want = R.intervals(reads, motifs, gaps, mins)
    for mi in range(8):
        assert want[1][:, mi].sum() >= 8
    K.same(gpu_intervals(reads, motifs, gaps, mins), want)


def test_self_reverse_complementary_motif():
    reads = ["ACGT" * 20, "CC" + "ACGT" * 300 + "TT" + "CGTA" * 400, "AATT" * 9 + "C" * 40 + "TTAA" * 9, "GATTACA" * 9]
    motifs = ["ACGT", "AATT"]
    want = R.intervals(reads, motifs, 1, 1)
    fwd, rev = want[0][want[0]["strand"] == 0], want[0][want[0]["strand"] == 1]
    assert len(fwd) >= 4 and all((fwd[f] == rev[f]).all() for f in ("read", "motif", "start", "end", "covered"))
    K.same(gpu_intervals(reads, motifs, 1, 1), want)


# ---- batch plumbing
@pytest.mark.parametrize("shape", ["host_ragged", "contiguous", "host_uniform", "device_uniform"])
def test_batch_shapes(shape):
    n, L = 4000, 150
    reads = short_reads(n)
    want = R.intervals(reads, [TEL, "AAT"], [18, 0], [24, 3])
    assert want[1][:, 0, 0].astype(bool).sum() >= 20 and want[1][:, 0, 1].astype(bool).sum() >= 20
    words, offsets, lengths = capi.pack_reads(reads)
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 20) as t:
        d = None
        if shape == "host_ragged":
            b = t.host_batch(words, offsets, lengths)
        elif shape == "contiguous":
            b = t.host_batch(words, offsets, lengths, contiguous=True)
        elif shape == "host_uniform":
            w = np.ascontiguousarray(words, dtype=np.uint32)
            b = capi.Batch(w.ctypes.data, len(w), None, None, L, stride, n, 0, 0)
            b._keep = (w,)
        else:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(20250218, 0, n, L, d)
            b = t.device_uniform_batch(d, n, L)
        t.intervals(b, [TEL, "AAT"], [18, 0], [24, 3], BIG)
        got = t.intervals_results()
        if d is not None:
            t.free(d)
    K.same(got, want)


def test_pair_mode_context_and_two_slots():
    reads = short_reads(2000)
    a, b = reads[:1200], reads[1200:]
    want_a, want_b = R.intervals(a, [TEL], 6, 12), R.intervals(b, [TEL], 0, 1)
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.intervals(ba, [TEL], 6, 12, BIG, slot=0)
        t.intervals(bb, [TEL], 0, 1, BIG, slot=1)
        K.same(t.intervals_results(1), want_b)
        K.same(t.intervals_results(0), want_a)


# ---- independence
def test_independent_of_scan_annotate_and_tracts():
    reads = short_reads(12000)
    a, b = reads[:7000], reads[7000:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = R.intervals(a, motifs, 6, 12), R.intervals(b, motifs, 6, 12)
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        # without any intervals call
        t.annotate(ba, motifs)
        alone_a = t.annotate_results()
        t.tracts(ba, motifs, 3)
        alone_t = t.tracts_results()
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18) as t:
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        # scan, annotate, tracts and intervals interleaved on slot 0, intervals and a scan on slot 1; nothing collected until the end
        t.submit(ba, slot=0)
        t.intervals(ba, motifs, 6, 12, BIG, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.intervals(bb, motifs, 6, 12, BIG, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.submit(bb, slot=1)
        got_i1 = t.intervals_results(1)
        got_i0 = t.intervals_results(0)
        got_a = t.annotate_results(0)
        got_t = t.tracts_results(0)
        tables = t.collect()
    K.same(got_i0, want_a)
    K.same(got_i1, want_b)
    assert (got_a == alone_a).all() and (alone_a == A.annotate(a, motifs)).all()
    assert (got_t == alone_t).all() and (alone_t == T.tracts(a, motifs, 3)).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


def test_errors():
    with ctx() as t:
        b = t.host_batch(*capi.pack_reads([b"ACGTACGTAC"]))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_intervals"):
            t.intervals_results()
        t.tracts(b, ["ACG"], 3)  # a tracts call is no intervals call: the buffers are separate
        t.tracts_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_intervals"):
            t.intervals_results()
        with pytest.raises(capi.TrewHipError, match="min_len must be at least 1"):
            t.intervals(b, [TEL], 0, 0)
        with pytest.raises(capi.TrewHipError, match="max_intervals must be at least 1"):
            t.intervals(b, [TEL], 0, 1, 0)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.intervals(b, ["AAT"] * 9, 0, 1)
        with pytest.raises(capi.TrewHipError, match="n_motifs"):
            t.intervals(b, [], 0, 1)
        with pytest.raises(capi.TrewHipError, match=r"k must be in \[3, 32\]"):
            t.intervals(b, [capi.Motif(2, 0, 5)], 0, 1)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.intervals(b, [TEL], 0, 1, slot=3)
        m = (capi.Motif * 1)(capi.motif("ACG"))
        assert t.lib.trew_hip_intervals(t.ctx, C.byref(b), 0, m, None, 1, 4) != 0
        assert "rules must not be null" in t.lib.trew_hip_last_error(t.ctx).decode()
        assert t.lib.trew_hip_intervals(t.ctx, C.byref(b), 0, None, (capi.IntervalRule * 1)(capi.IntervalRule(0, 1)), 1, 4) != 0
        assert "motifs is NULL" in t.lib.trew_hip_last_error(t.ctx).decode()
        assert t.lib.trew_hip_intervals(None, C.byref(b), 0, m, None, 1, 4) != 0
        t.intervals(b, ["ACG"], 0, 1, 4)
        assert t.lib.trew_hip_intervals_results(t.ctx, 0, None, 0, None, None, None) != 0
        assert "n must not be null" in t.lib.trew_hip_last_error(t.ctx).decode()
        K.same(t.intervals_results(), R.intervals([b"ACGTACGTAC"], ["ACG"], 0, 1))


# ---- the `trew intervals` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with (gzip.open(path, "wb") if path.endswith(".gz") else open(path, "wb")) as f:
        f.write(data)


expected_cli = R.cli_lines


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines(), r.stderr


@pytest.mark.parametrize("suffix", [".fastq", ".fastq.gz"])
def test_cli_synthetic_long(tmp_path, generator_long, suffix):
    reads, want = generator_long
    path = str(tmp_path / ("long" + suffix))
    write_fastq(path, reads)
    lines = expected_cli(path, reads, [TEL], want)
    assert len(lines) - 5 >= 18  # rows: the planted tails, in pieces, and a few chance intervals
    assert run_cli("intervals", TEL, path, "-t", "1")[0] == lines
    assert run_cli("intervals", TEL, path, "-t", "8")[0] == lines
    if suffix == ".fastq":
        # two motifs under rules of the command line; max_gap 0 and min_len 1 find far more intervals than the file has reads,
        # so the first log of every batch (one record per read) overflows and the batch is resubmitted: --stats says so
        motifs = [TEL, "AAT"]
        lines = expected_cli(path, reads, motifs, R.intervals(reads, motifs, 0, 1))
        assert len(lines) - 6 > 10 * len(reads)
        out, err = run_cli("intervals", ",".join(motifs), path, "--max_gap", "0", "--min_len", "1", "-t", "3", "--stats")
        assert out == lines
        assert " batch(es) resubmitted with a larger log" in err and " 0 batch(es) resubmitted" not in err
