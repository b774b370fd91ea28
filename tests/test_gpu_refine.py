"""De novo repeats under indels on the GPU (trew_hip_refine through ctypes).  Every read of every batch is compared, integer
for integer, with tests/refine_ref.py where the reads are few or short, and with trew_refine_host (itself checked against
refine_ref in test_refine_cpu.py) everywhere."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import oracle as O
import period_ref as P
import refine_ref as R
from period_cases import fuzz_reads, junk, noisy, rep
from refine_cases import GPU_KS, HAND, SEED_KEPT, T10, TEL, UNITS, fuzz_set, replaced, run_at, with_deletion, with_insertion
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")


def rec(x):
    return tuple(int(v) for v in x)


def same(got, want):
    assert got.shape == want.shape
    for f in R.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s differs at read %d: got %s, want %s" % (f, bad[0], got[bad[0]], want[bad[0]])


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16)


def gpu_refine(reads_or_packed, *args, mode=capi.MODE_LONG):
    words, offsets, lengths = reads_or_packed if isinstance(reads_or_packed, tuple) else capi.pack_reads(reads_or_packed)
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(offsets), 16)) as t:
        t.refine(t.host_batch(words, offsets, lengths), *args)
        return t.refine_results()


def check(reads, *args, ref=True):
    """GPU == reference on every read (ref: also the host definition == reference); without ref, GPU == host definition"""
    got = gpu_refine(reads, *args)
    want = capi.refine_host(reads, *args)
    if ref:
        same(want, R.refine(reads, *args))
    same(got, want)
    return want


# ---- shapes and sizes
def test_hand_worked_vectors():
    for args in sorted({a for _, a, _ in HAND}):
        rows = [(r, w) for r, a, w in HAND if a == args]
        got = gpu_refine([r.encode() for r, _ in rows], *args)
        assert [rec(g) for g in got] == [w for _, w in rows]


@pytest.mark.parametrize("k", GPU_KS)
def test_unit_lengths_and_read_lengths(k):
    """perfect, shifted, noisy and random reads of every listed length, for the unit length k"""
    rnd = random.Random(k)
    unit = UNITS[k]
    short, long_ = [], []
    for n in (0, 1, k, 2 * k - 1, 2 * k, 31, 32, 33, 2047, 2048, 2049):
        into = short if n <= 64 else long_
        into.append(rep(unit, n))
        into.append(rep(unit, n, rnd.randrange(k)))
        into.append(noisy(rnd, unit, n, 0.03, 0.06, 0.004))
        into.append(junk(rnd, n, "ACGTN" if n % 2 else "ACGT"))
    for args in ((1, 32, 3, 1), (1, 32, 1, 24), (1, 32, 64, 1)):
        check(short, *args)
    want = check(long_, 1, 32, 3, 24)
    assert (want["period"][:2] == k).all() and (want["changed"][:2] == 0).all()
    check(long_, 1, 32, 1, 1, ref=False)
    check(long_, k, k, 64, 1, ref=False)


# ---- seams of the longest run
def with_subs(read, subs):
    for at in subs:
        read = replaced(read, at)
    return read


def runs_of(read, k):
    """[(start, length)] of the runs of eq_k of a read"""
    eq = P.eq_k(P.codes(read), k).tolist() + [False]
    out, i = [], 0
    while i < len(eq):
        if eq[i]:
            j = i
            while eq[j]:
                j += 1
            out.append((i, j - i))
            i = j
        else:
            i += 1
    return out


def runs_read(unit, start, length, count=1):
    """A perfect repeat with replaced bases: a replaced base at p clears eq_k at p - k and at p, so the runs lie between them.
    `count` runs of `length` positions, the first at `start`, one replaced base between two of them; every other run has 39."""
    k = len(unit)
    ends = [start + (i + 1) * (length + k + 1) - 1 for i in range(count)]
    n = ends[-1] + 100
    read = with_subs(rep(unit, n), list(range(start - 1, -1, -(40 + k))) + ends + list(range(ends[-1] + 40 + k, n, 40 + k)))
    longest = sorted(runs_of(read, k), key=lambda r: (-r[1], r[0]))
    assert longest[:count] == [(start + i * (length + k + 1), length) for i in range(count)] and longest[count][1] < length
    return read


@pytest.mark.parametrize("k", [2, 6, 17, 32])
def test_longest_run_at_word_and_iteration_seams(k):
    """The longest run starts (first set) or ends (second set) at bit 31, bit 0 and bit 1 of a word and at the 64-word seam;
    then one base is removed and one is added right there."""
    unit = UNITS[k]
    length = 70 + 3 * k
    reads = []
    for seam in (31, 32, 33, 64, 2047, 2048, 2049):
        pair = [runs_read(unit, seam, length)] + ([runs_read(unit, seam - length, length)] if seam > length else [])
        reads += pair
        for base in pair:
            reads.append(with_deletion(base, seam))
            reads.append(with_insertion(base, seam, "C"))
    # the run in a random background: it is the whole tract, from bit 31, 0 and 1
    rnd = random.Random(k)
    reads += [run_at(unit, lead, 90, 40, rnd) for lead in (31, 32, 33, 2047, 2048, 2049)]
    want = check(reads, 1, 32, 3, 24)
    assert (want["period"] == k).all()
    check(reads, k, k, 1, 1, ref=False)


def test_two_runs_of_equal_length_the_first_wins():
    reads = []
    for k in (6, 32):
        length = 100 + k
        # in one word row; the first ends at the 64-word seam and the second starts behind it; both behind it
        reads += [runs_read(UNITS[k], start, length, 2) for start in (40, 2048 - length, 2048 - length - k - 1, 2049, 4096 - length)]
        reads.append(runs_read(UNITS[k], 33, length, 3))
    check(reads, 1, 32, 3, 24)


# ---- vote and seed edges
def votes_of(read, *args):
    """(S, cnt) of the reference"""
    c = P.codes(read)
    x = [int(v) for v in c]
    S = R.seed(c, P.period_read(read, *args))
    a1 = R.align_ref.align_strand(x, S, args[2])
    return S, R.vote_plain(x[a1[1]:a1[2]], S, args[2])


def test_vote_and_seed_edges():
    args = (1, 32, 3, 10)
    n_seed = T10[:14] + "N" + T10[15:]
    # TTAGGG and TTACGG mixed: four votes each for G and C at one phase of the unit of 6, two each at one of the unit of 12
    tie = "TTACGGTTACGGTTAGGGTTACGGTTACGGTTAGGGTTAGGGTTAGGGTTACGGTTACGG"
    tie12 = "TTACGGTTAGGGTTACGGTTACGGTTACGGTTACGGTTAGGGTTACGGTTAGGGTTACGG"
    unit = UNITS[17]
    no_vote = "".join(unit[:5] + "N" + unit[6:] for _ in range(4))  # phase 5 has no valid base: no votes, the seed's N is the consensus' T
    reads = [n_seed, tie, no_vote, SEED_KEPT, tie12, "N" * 90 + n_seed + "N" * 70, TEL * 3 + "N" * 6 + TEL * 3]
    for read, k in ((tie, 6), (tie12, 12)):
        S, cnt = votes_of(read, *args)
        assert len(S) == k and any(sorted(c)[-1] == sorted(c)[-2] > 0 for c in cnt)  # the tie is there
    S, cnt = votes_of(no_vote, *args)
    assert len(S) == 17 and any(sum(c) == 0 for c in cnt)  # and so is the phase without votes
    want = check(reads, *args)
    assert rec(want[3])[:4] == (5, 5, 5, 0) and (want["period"][:3] == (6, 6, 17)).all()


# ---- long reads
def test_long_perfect_repeat_and_long_noisy_read():
    rnd = random.Random(70000)
    perfect = rep(TEL, 70_000, 2)
    noisy_read = junk(rnd, 1500) + noisy(rnd, TEL, 200_000 - 2500, 0.03, 0.06, 0.001) + junk(rnd, 1000)
    want = check([perfect, noisy_read], ref=False)
    assert rec(want[0])[:9] == (6, 6, 6, 0, 70_000, 0, 70_000, 70_000, 70_000)
    assert want["period"][1] == 6 and want["end"][1] - want["start"][1] >= 190_000 and P.canonical(want["unit"][1], 6) == P.canonical(213, 6)
    cols = capi.refine_columns(want, 3)
    assert cols["insertions"][1] >= 3000 and cols["deletions"][1] >= 3000


# ---- the fuzz set, and A1 against the merged measure on the GPU
@pytest.fixture(scope="module")
def fuzz():
    reads = [r for _, r in fuzz_set()]
    return reads, R.refine(reads)


def test_fuzz_set(fuzz):
    reads, want = fuzz
    same(gpu_refine(reads), want)
    same(capi.refine_host(reads), want)
    assert (want["changed"] > 0).sum() >= 5 and (want["period"] > 0).sum() >= 90


def test_seed_alignment_equals_trew_hip_align_on_the_gpu(fuzz):
    """seed_score, and with changed = 0 the whole of A2 = A1, equal the forward fields of trew_hip_align with the motif S;
    with changed > 0 the fields of A2 equal those with the motif U"""
    reads, _ = fuzz
    packed = capi.pack_reads(reads)
    checked = 0
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        t.refine(b)
        got = t.refine_results()
        idx = [i for i in range(len(reads)) if got["seed_period"][i] >= 3]
        for at in range(0, len(idx), 8):
            part = idx[at:at + 8]
            t.align(b, [P.unit_text(got["seed_unit"][i], int(got["seed_period"][i])) for i in part], 3)
            a = t.align_results()
            for m, i in enumerate(part):
                assert int(a["score_fwd"][i, m]) == int(got["seed_score"][i])
                if got["changed"][i] == 0:
                    assert rec(a[i, m])[:5] == rec(got[i])[4:9]
                    checked += 1
        idx = [i for i in range(len(reads)) if got["changed"][i] > 0 and got["period"][i] >= 3]
        for at in range(0, len(idx), 8):
            part = idx[at:at + 8]
            t.align(b, [P.unit_text(got["unit"][i], int(got["period"][i])) for i in part], 3)
            a = t.align_results()
            for m, i in enumerate(part):
                assert rec(a[i, m])[:5] == rec(got[i])[4:9]
                checked += 1
    assert checked >= 80


# ---- repeatability
def test_many_copies_and_repeated_calls():
    rnd = random.Random(4096)
    one = junk(rnd, 300) + noisy(rnd, TEL, 500, 0.05, 0.06) + junk(rnd, 77)
    want1 = capi.refine_host([one])
    assert want1["period"][0] == 6
    same(gpu_refine([one] * 1024), np.repeat(want1, 1024))
    reads = fuzz_reads(99, n=600, max_len=400)
    packed = capi.pack_reads(reads)
    want = capi.refine_host(packed)
    assert 60 <= (want["period"] > 0).sum() <= 540
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads)) as t:
        b = t.host_batch(*packed)
        for _ in range(3):
            t.refine(b)
            same(t.refine_results(), want)


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_ragged_reads_and_parameters(seed):
    rnd = random.Random(seed)
    reads = fuzz_reads(2000 + seed, n=300)
    for penalty in (1, 3, 64):
        lo = rnd.randint(1, 32)
        check(reads, lo, rnd.randint(lo, 32), penalty, rnd.choice((1, 24)), ref=False)
    want = check(reads[:60], 1, 32, 3, 24)
    assert (want["period"] > 0).sum() >= 15


# ---- batch shapes and contexts
@pytest.fixture(scope="module")
def uniform150():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 4000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = capi.refine_host(reads)
    assert (want["period"] == 6).sum() >= 30
    return reads, want


@pytest.mark.parametrize("shape", ["host_ragged", "offsets_lengths_words", "words_offsets_lengths", "host_uniform", "device_uniform"])
def test_batch_shapes(uniform150, shape):
    n, L = 4000, 150
    reads, want = uniform150
    words, offsets, lengths = (np.ascontiguousarray(a, dtype=np.uint32) for a in capi.pack_reads(reads))
    stride = 3 * ((L + 31) // 32)
    with ctx(reads=n, words=1 << 20) as t:
        d = None
        if shape == "host_ragged":
            b = t.host_batch(words, offsets, lengths)
        elif shape == "offsets_lengths_words":
            b = t.host_batch(words, offsets, lengths, contiguous=True)
        elif shape == "words_offsets_lengths":
            buf = np.concatenate([words, offsets, lengths])
            base = buf.ctypes.data
            b = capi.Batch(base, len(words), base + 4 * len(words), base + 4 * (len(words) + n), 0, 0, n, 0, 0)
            b._keep = (buf,)
        elif shape == "host_uniform":
            b = capi.Batch(words.ctypes.data, len(words), None, None, L, stride, n, 0, 0)
            b._keep = (words,)
        else:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(20250218, 0, n, L, d)
            b = t.device_uniform_batch(d, n, L)
        t.refine(b)
        got = t.refine_results()
        if d is not None:
            t.free(d)
    same(got, want)


@pytest.mark.parametrize("max_length", ["known", "unknown"])
def test_device_resident_ragged(max_length):
    n = 60
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    want = capi.refine_host([buf[s:e + 1] for s, e in zip(st, nd)])
    assert (want["period"] == 6).sum() >= 2
    with ctx(mode=capi.MODE_LONG, reads=n, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, n)
        if max_length == "unknown":
            b.max_length = 0
        t.refine(b)
        got, ms = t.refine_results(want_ms=True)
        for p in ptrs:
            t.free(p)
    assert ms > 0
    same(got, want)


def test_pair_mode_context_two_slots_and_errors():
    a, b = fuzz_reads(41, n=250), fuzz_reads(42, n=151)  # an odd number of reads is refused in pair mode
    with ctx(mode=capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba = t.host_batch(*capi.pack_reads(a))
        with pytest.raises(capi.TrewHipError, match="no trew_hip_refine"):
            t.refine_results()
        t.periods(ba)  # a periods call is no refine call: the buffers are separate
        t.periods_results()
        with pytest.raises(capi.TrewHipError, match="no trew_hip_refine"):
            t.refine_results()
        with pytest.raises(capi.TrewHipError, match="even number of reads"):
            t.refine(t.host_batch(*capi.pack_reads(b)))
        bb = t.host_batch(*capi.pack_reads(b[:150]))
        t.refine(ba, 1, 32, 3, 24, slot=0)  # the mates are two reads; the two slots overlap
        t.refine(bb, 2, 12, 7, 5, slot=1)
        same(t.refine_results(1), capi.refine_host(b[:150], 2, 12, 7, 5))
        same(t.refine_results(0), capi.refine_host(a))
        for lo, hi in ((0, 5), (3, 2), (1, 33)):
            with pytest.raises(capi.TrewHipError, match="1 <= min_period <= max_period <= 32"):
                t.refine(ba, lo, hi)
        for penalty in (0, 65):
            with pytest.raises(capi.TrewHipError, match=r"penalty must be in \[1, 64\]"):
                t.refine(ba, penalty=penalty)
        with pytest.raises(capi.TrewHipError, match="min_score must be at least 1"):
            t.refine(ba, min_score=0)
        with pytest.raises(capi.TrewHipError, match="slot out of range"):
            t.refine(ba, slot=3)
        # results larger than the caller's buffer: the count is reported, cap records are copied
        t.refine(ba)
        n = C.c_uint64(0)
        three = np.zeros(3, dtype=capi.REFINE_DTYPE)
        assert t.lib.trew_hip_refine_results(t.ctx, 0, three.ctypes.data, 3, C.byref(n), None) == 0
        assert n.value == 250
        same(three, capi.refine_host(a[:3]))
        assert t.lib.trew_hip_refine_results(t.ctx, 0, None, 0, C.byref(n), None) == 0 and n.value == 250


def test_convenience_entry_point():
    import trew_amd

    reads = fuzz_reads(77, n=120)
    same(trew_amd.refine(reads), capi.refine_host(reads))
    same(trew_amd.refine(reads, 3, 8, penalty=5, min_score=9), capi.refine_host(reads, 3, 8, 5, 9))


# ---- independence
def test_independent_of_scan_and_the_other_measures():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]
    motifs = [TEL, "CCCTA"]
    want_a, want_b = capi.refine_host(a), capi.refine_host(b, 2, 12, 5, 12)
    LOG = 1 << 16

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    def fetch(t, slot=0):
        return ((t.annotate_results(slot), t.tracts_results(slot)) + t.intervals_results(slot) + t.variants_results(slot) + (t.periods_results(slot),) +
                t.chain_results(slot) + t.repeats_results(slot) + t.satellites_results(slot) + (t.align_results(slot),))

    with fresh() as t:  # without any refine call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.annotate(ba, motifs)
        t.tracts(ba, motifs, 3)
        t.intervals(ba, motifs, 6, 12, LOG)
        t.variants(ba, motifs)
        t.periods(ba)
        t.chain(ba, motifs, 8 * LOG)
        t.repeats(ba, max_records=LOG)
        t.satellites(ba, 1, 64, max_records=LOG)
        t.align(ba, motifs, 3)
        alone = fetch(t)
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # refine calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        t.refine(ba, slot=0)
        t.annotate(ba, motifs, slot=0)
        t.refine(bb, 2, 12, 5, 12, slot=1)
        t.tracts(ba, motifs, 3, slot=0)
        t.intervals(ba, motifs, 6, 12, LOG, slot=0)
        t.variants(ba, motifs, slot=0)
        t.periods(ba, slot=0)
        t.chain(ba, motifs, 8 * LOG, slot=0)
        t.repeats(ba, max_records=LOG, slot=0)
        t.satellites(ba, 1, 64, max_records=LOG, slot=0)
        t.align(ba, motifs, 3, slot=0)
        t.submit(bb, slot=1)
        got_1 = t.refine_results(1)
        got_0 = t.refine_results(0)
        got = fetch(t)
        tables = t.collect()
    same(got_0, want_a)
    same(got_1, want_b)
    assert len(got) == len(alone)
    for x, y in zip(got, alone):
        assert (np.asarray(x) == np.asarray(y)).all()
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- the `trew refine` subcommand, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def noisy_tail_reads(n=40, seed=8):
    """generator long reads, cut to at most 6 kb, with a planted tail of 0.3 - 2 kb of one of four units that carries
    substitutions and indels"""
    rnd = random.Random(seed)
    buf, st, nd = capi.synth_long_ascii(20250218, 0, n)
    out = []
    for i, (s, e) in enumerate(zip(st, nd)):
        body = buf[s:e + 1].decode()[:rnd.randint(500, 6000)]
        out.append((body + noisy(rnd, [TEL, "CCCTAA", "AATGG", UNITS[17]][i % 4], rnd.randint(300, 2000), 0.03, 0.06, 0.002)).encode())
    return out


def test_cli_generator_long_reads_with_noisy_tails(tmp_path):
    reads = noisy_tail_reads()
    path = str(tmp_path / "tails.fastq")
    write_fastq(path, reads)
    # rows formatted from the reference itself for the first reads, from the host definition (equal to it) for all
    host3 = capi.refine_host(reads)
    same(host3[:4], R.refine(reads[:4]))
    rows, summary = R.cli_lines(path, reads, host3, 3)
    assert len(rows) - 2 >= len(reads) - 2 and len(summary) - 2 >= 4  # the planted tails are found
    assert run_cli("refine", path, "-t", "2") == rows + summary
    assert run_cli("refine", path, "-t", "5") == rows + summary
    # MIN_SCORE is the minimum of step 1 (the score of `periods`) as well as of the rows
    rows, summary = R.cli_lines(path, reads, capi.refine_host(reads, 5, 12, 7, 60), 7, min_score=60)
    assert 5 <= len(rows) - 2 <= 35  # the units of 17 are out of the range, and P = 7 leaves the noisier tails below 60
    assert run_cli("refine", path, "--min_period", "5", "--max_period", "12", "--penalty", "7", "--min_score", "60", "-t", "3") == rows + summary
    # two files: the summary is over both
    got = run_cli("refine", path, path)
    assert got.count(">" + os.path.realpath(path)) == 2
    both = R.cli_lines(path, reads + reads, np.concatenate([host3] * 2), 3)[1]
    assert got[got.index(">Summary"):] == both
