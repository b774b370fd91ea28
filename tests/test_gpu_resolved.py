"""tandems, decompose and dissect with resolve's period choice per piece on the GPU (trew_hip_tandems_resolved,
trew_hip_decompose_resolved and trew_hip_dissect_resolved through ctypes) against the reference of resolved_ref.py: every record,
count and item of every read, field for field.  Two sets are too large for the reference in a few seconds (3000 reads on one CU,
the generator's long reads); there the yardstick is the host definition, which tests/test_resolved_cpu.py holds against the
reference.  The resolved entry points are called as such for every C, one included: capi's `candidates=1` takes the plain path."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import decompose_ref
import dissect_cases as DC
import dissect_ref
import oracle as O
import resolve_cases as VC
import resolved_cases as RC
import resolved_ref as X
import tandem_cases as TC
import tandem_ref
from trew_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREW = os.path.join(ROOT, "trew_amd", "bin", "trew")
BIG = 1 << 22  # rows (128 MB of workspace): no test batch claims more
ARGS = RC.ARGS
ROOM = {"tandems": (1 << 16,), "decompose": (1 << 20, BIG), "dissect": (1 << 16, 1 << 20, BIG)}
NAMES = ("tandems", "decompose", "dissect")


def ctx(mode=capi.MODE_SHORT, n_slots=1, words=1 << 22, reads=1 << 18, flags=0):
    return capi.TrewHip(mode=mode, n_slots=n_slots, max_batch_words=words, max_batch_reads=reads, table_log2_slots=16, flags=flags)


def queue(t, name, b, args, c, room=None, slot=0):
    """the resolved entry point of `name`, whatever c is"""
    room = ROOM[name] if room is None else tuple(int(v) for v in room)
    t._queue(name, slot, b, None, 1, shape=room)
    f = getattr(t.lib, "trew_hip_%s_resolved" % name)
    t._chk(f(t.ctx, C.byref(b), slot, *[int(a) for a in args], int(c), *room), f.__name__)


def fetch(t, name, slot=0):
    return getattr(t, name + "_results")(slot)


def gpu(reads, c, args=ARGS, mode=capi.MODE_SHORT, names=NAMES, plain=False):
    """{name: results} of the resolved entry points (plain: of the plain ones) on one context"""
    words, offsets, lengths = capi.pack_reads(reads)
    out = {}
    with ctx(mode, words=max(len(words) + 64, 1 << 12), reads=max(len(reads), 16)) as t:
        b = t.host_batch(words, offsets, lengths)
        for name in names:
            if plain:
                getattr(t, name)(b, *args, *ROOM[name])
            else:
                queue(t, name, b, args, c)
            out[name] = fetch(t, name)
    return out


def same_arrays(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in want.dtype.names:
        bad = np.flatnonzero(got[f] != want[f])
        assert len(bad) == 0, "%s: %s differs at %d: got %s, want %s" % (what, f, bad[0], got[bad[0]], want[bad[0]])


def same(got, want_dissect, want_decompose):
    """{name: results} of the device against resolved_ref.dissect's (records, items, counts, rows) and resolved_ref.decompose's
    (items, counts, records), or the host definitions' results, which begin alike; tandems' records are dissect's but for the anchor"""
    if "dissect" in got:
        g, w = got["dissect"], want_dissect
        same_arrays(g[0], w[0], "dissect records")
        assert (g[2] == w[2]).all()
        same_arrays(g[1], w[1], "dissect items")
        assert g[3:6] == (len(w[0]), len(w[1]), int((w[0]["end"].astype(np.int64) - w[0]["start"]).sum()))
    if "tandems" in got:
        g, w = got["tandems"], want_dissect
        plain = w[0].copy()
        plain["reserved"] = 0
        same_arrays(g[0], plain, "tandems records")
        assert (g[1] == w[2][:, 0]).all() and g[2] == len(w[0])
    if "decompose" in got:
        g, w = got["decompose"], want_decompose
        same_arrays(g[2], w[2], "decompose records")
        assert (g[1] == w[1]).all()
        same_arrays(g[0], w[0], "decompose items")


def ref(reads, c, args=ARGS):
    return X.dissect(reads, *args, c), X.decompose(reads, *args, c)


def host(reads, c, args=ARGS):
    return capi.dissect_host(reads, *args, candidates=c), capi.decompose_host(reads, *args, candidates=c)


def identical(a, b):
    """two {name: results} word for word"""
    assert a.keys() == b.keys()
    for name in a:
        for x, y in zip(a[name], b[name]):
            assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y, name


def rows(recs, read=0):
    return [(int(x["depth"]), int(x["period"]), int(x["start"]), int(x["end"]), int(x["score"])) for x in recs[recs["read"] == read]]


# ---- shapes: every unit length and read length at which the kernels take another path
@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("k", VC.GPU_KS)
def test_unit_and_read_lengths(k, c):
    short, long_ = VC.shape_reads(k, random.Random(100 + k))
    reads = short + long_
    got = gpu(reads, c, mode=capi.MODE_LONG)
    same(got, *ref(reads, c))
    if c == 1:
        identical(got, gpu(reads, 1, mode=capi.MODE_LONG, plain=True))


# ---- the cases that fail without the candidate loop
def test_rows_that_only_the_candidate_loop_finds():
    reads = [VC.SHORT_REPAIRED] + RC.child_reads(VC.SHORT_REPAIRED) + [TC.WEAK_FIRST]
    want = {c: ref(reads, c) for c in (1, 3)}
    one, three = want[1][0][0], want[3][0][0]
    assert rows(one, 0) == [(0, 25, 4, 114, 75)] and rows(three, 0) == [(0, 26, 4, 151, 88)]
    for i, lo in enumerate(RC.CHILD_LOS, 1):  # the child piece begins where the depth-0 tract ends: at lo
        assert rows(one, i)[0][3] == lo == rows(three, i)[0][3] and rows(one, i)[0][:2] == (0, 5)
        assert rows(one, i)[1] == (1, 25, lo + 4, lo + 114, 75) and rows(three, i)[1] == (1, 26, lo + 4, lo + 151, 88)
    last = len(reads) - 1
    assert rows(one, last) == [(1, 6, 64, 100, 36)] and rows(three, last) == [(0, 6, 64, 100, 36)]
    for c in (1, 3):
        same(gpu(reads, c, mode=capi.MODE_LONG), *want[c])


def test_tied_and_rotated_candidates_inside_a_child_piece():
    reads = RC.child_reads(VC.SCORE_TIE) + RC.child_reads(VC.ROTATED_SEED) + [VC.SCORE_TIE, VC.ROTATED_SEED]
    for c in (2, 3, 4):
        want = ref(reads, c)
        for i, lo in enumerate(RC.CHILD_LOS + RC.CHILD_LOS):
            assert rows(want[0][0], i)[0][3] == lo  # the depth-0 tract ends at lo
        same(gpu(reads, c, mode=capi.MODE_LONG), *want)


@pytest.mark.parametrize("k", [6, 17, 32])
def test_child_pieces_at_word_and_seam_bounds(k):
    reads = TC.piece_bound_reads(k)[0] + TC.piece_hi_reads(k)[0]
    got = gpu(reads, 3, mode=capi.MODE_LONG)
    same(got, *ref(reads, 3))
    identical(gpu(reads, 1, mode=capi.MODE_LONG), gpu(reads, 1, mode=capi.MODE_LONG, plain=True))


def test_long_units_two_tracts_a_read():
    reads = [r for r, _ in RC.long_unit_set()][:6]
    for c in (1, 3):
        same(gpu(reads, c, mode=capi.MODE_LONG), *ref(reads, c))


def test_child_tracts_around_the_row_block_and_the_end_phase_tie():
    reads = DC.child_block_reads()
    args = (1, 32, 3, 20)
    same(gpu(reads, 3, args), *ref(reads, 3, args))
    read, penalty, min_score, _, _ = DC.end_tie_child()
    pair, args = [read, read[3:] + "ACGT"], (1, 32, penalty, min_score)
    same(gpu(pair, 3, args), *ref(pair, 3, args))


# ---- capacities
def test_overflow_of_each_capacity_is_repeated_once_with_the_exact_numbers():
    reads = [r for r, _ in RC.long_unit_set()][:6] + RC.child_reads(VC.SHORT_REPAIRED)[:2]
    want_x, want_d = ref(reads, 3)
    nr, ni, nw = len(want_x[0]), len(want_x[1]), want_x[3]
    with ctx(capi.MODE_LONG, words=1 << 16, reads=16) as t:
        b = t.host_batch(*capi.pack_reads(reads))
        # rows that do not fit: every tract is traced by recomputing its blocks; the counts are exact
        for room in ((1 << 12, 1 << 16, 1), (1, 1 << 16, BIG), (1 << 12, 1, BIG), (nr - 1, ni - 1, nw - 1)):
            queue(t, "dissect", b, ARGS, 3, room)
            got = t.dissect_results()
            assert len(got[0]) == 0 and len(got[1]) == 0 and got[3:] == (nr, ni, nw) and (got[2] == want_x[2]).all()
            queue(t, "dissect", b, ARGS, 3, got[3:])
            same({"dissect": t.dissect_results()}, want_x, want_d)
        # the first tract's rows fit, the others are recomputed
        first_rows = int(want_x[0]["end"][0] - want_x[0]["start"][0])
        queue(t, "dissect", b, ARGS, 3, (nr, ni, first_rows))
        assert t.dissect_results()[3:] == (nr, ni, nw)
        d_items, d_rows = len(want_d[0]), int((want_d[2]["end"].astype(np.int64) - want_d[2]["start"])[want_d[1] > 0].sum())
        for room in ((1 << 16, 1), (1, BIG), (d_items - 1, d_rows - 1)):
            queue(t, "decompose", b, ARGS, 3, room)
            got = t.decompose_results()
            assert len(got[0]) == 0 and got[3:] == (d_items, d_rows) and (got[1] == want_d[1]).all()
            queue(t, "decompose", b, ARGS, 3, got[3:])
            same({"decompose": t.decompose_results()}, want_x, want_d)
        queue(t, "tandems", b, ARGS, 3, (1,))
        got = t.tandems_results()
        assert len(got[0]) == 0 and got[2] == nr and (got[1] == want_x[2][:, 0]).all()
        queue(t, "tandems", b, ARGS, 3, (got[2],))
        same({"tandems": t.tandems_results()}, want_x, want_d)
    import trew_amd

    got = trew_amd.dissect(reads, candidates=3, max_records=1, max_items=1, max_rows=1)  # the convenience call retries inside
    same_arrays(got[0], want_x[0], "records")
    same_arrays(got[1], want_x[1], "items")
    same({"tandems": trew_amd.tandems(reads, candidates=3, max_records=1) + (nr,)}, want_x, want_d)
    same_arrays(trew_amd.decompose(reads, candidates=3, max_items=1, max_rows=1)[2], want_d[2], "decompose")


# ---- batch shapes, slots, repeated and alternating calls
def test_batch_shapes_pair_mode_two_slots_and_alternating_calls():
    reads = VC.mixed_reads(11, 200) + [VC.SHORT_REPAIRED, TC.WEAK_FIRST] * 3
    other = VC.mixed_reads(12, 120)
    want, want_other, plain = ref(reads, 3), ref(other, 2, (2, 20, 2, 12)), ref(reads, 1)
    assert want[0][0].tobytes() != plain[0][0].tobytes()
    words, offsets, lengths = capi.pack_reads(reads)
    with ctx(capi.MODE_LONG, words=len(words) + 64, reads=len(reads)) as t:  # ragged and contiguous host batches
        for b in (t.host_batch(words, offsets, lengths), t.host_batch(words, offsets, lengths, contiguous=True)):
            for name in NAMES:
                queue(t, name, b, ARGS, 3)
            same({name: fetch(t, name) for name in NAMES}, *want)
    with ctx(capi.MODE_PAIR, n_slots=2, words=1 << 18, reads=1 << 12) as t:
        ba, bb = t.host_batch(*capi.pack_reads(reads)), t.host_batch(*capi.pack_reads(other))
        for name in NAMES:
            with pytest.raises(capi.TrewHipError, match="no trew_hip_%s" % name):
                fetch(t, name)
        for name in NAMES:  # the two slots overlap; the mates are two reads
            queue(t, name, ba, ARGS, 3, slot=0)
            queue(t, name, bb, (2, 20, 2, 12), 2, slot=1)
        same({name: fetch(t, name, 1) for name in NAMES}, *want_other)
        same({name: fetch(t, name, 0) for name in NAMES}, *want)
        # a plain and a resolved call alternating on one slot: the last call is what results returns, and fetching twice changes nothing
        for name in NAMES:
            getattr(t, name)(ba, *ARGS, *ROOM[name], slot=0)
            same({name: fetch(t, name)}, *plain)
            queue(t, name, ba, ARGS, 3)
            queue(t, name, ba, ARGS, 3)  # repeated
            same({name: fetch(t, name)}, *want)
            same({name: fetch(t, name)}, *want)
            getattr(t, name)(ba, *ARGS, *ROOM[name], slot=0)
            same({name: fetch(t, name)}, *plain)
        for c in (0, 5):
            for name in NAMES:
                with pytest.raises(capi.TrewHipError, match="resolve: 1 <= candidates <= 4 is required"):
                    queue(t, name, ba, ARGS, c)
        with pytest.raises(capi.TrewHipError, match="periods: 1 <= min_period <= max_period <= 32 is required"):
            queue(t, "tandems", ba, (0, 32, 3, 24), 5)
        with pytest.raises(capi.TrewHipError, match="max_rows must be at least 1"):
            queue(t, "dissect", ba, ARGS, 5, (4, 4, 0))
        queue(t, "dissect", t.host_batch(*capi.pack_reads([])), ARGS, 3)  # no reads: nothing found, no kernel
        assert t.dissect_results()[3:] == (0, 0, 0)


def test_device_resident_batches():
    """generator long reads with the longest read unknown, and a uniform 150-base batch, against the host definitions"""
    buf, st, nd = capi.synth_long_ascii(20250218, 0, 24)
    full = [buf[s:e + 1] for s, e in zip(st, nd)]
    with ctx(capi.MODE_LONG, reads=64, words=1 << 12) as t:
        b, ptrs, _ = t.synth_long_device(20250218, 0, 24)
        b.max_length = 0
        for name in NAMES:
            queue(t, name, b, ARGS, 3)
        got = {name: fetch(t, name) for name in NAMES}
        for p in ptrs:
            t.free(p)
    want = host(full, 3)
    assert want[0][3] > 0
    same(got, *want)
    n, L = 4000, 150
    buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
    short = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = host(short, 3)
    assert want[0][3] >= 20
    with ctx(reads=n, words=1 << 12) as t:
        d = t.malloc(n * 3 * ((L + 31) // 32) * 4 + 64)
        t.synth_short_device(20250218, 0, n, L, d)
        b = t.device_uniform_batch(d, n, L)
        for name in NAMES:
            queue(t, name, b, ARGS, 3)
        got = {name: fetch(t, name) for name in NAMES}
        t.free(d)
    same(got, *want)


def test_many_reads_and_pieces_per_wave_on_one_cu():
    """one CU's grid: 32 waves take a few thousand reads, many each, every piece with 0 .. 4 candidates one after the other -- the
    bins, the best-so-far word and the stack do not leak from piece to piece or from read to read"""
    reads = VC.mixed_reads(7, 3000) + [VC.SHORT_REPAIRED, "", TC.WEAK_FIRST, "A"] * 8
    want = host(reads, 4)
    few = reads[:160] + reads[-8:]  # the yardstick itself against the reference, on some of them
    same(dict(zip(("dissect", "decompose"), host(few, 4))), *ref(few, 4))
    packed = capi.pack_reads(reads)
    with ctx(capi.MODE_LONG, words=len(packed[0]) + 64, reads=len(reads), flags=capi.FLAG_DEBUG_ONE_CU) as t:
        assert t.debug_measure_grid(len(reads)) == 8
        b = t.host_batch(*packed)
        for _ in range(2):  # repeated calls
            for name in NAMES:
                queue(t, name, b, ARGS, 4)
            same({name: fetch(t, name) for name in NAMES}, *want)


def test_the_other_measures_are_unchanged_by_resolved_calls_in_between():
    buf, st, nd = capi.synth_short_ascii(20250218, 0, 6000, 150)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    a, b = reads[:3500], reads[3500:]

    def fresh():
        return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 20, max_batch_reads=1 << 15, table_log2_slots=18)

    def others(t, ba):
        t.refine(ba)
        out = [t.refine_results()]
        t.resolve(ba)
        out.append(t.resolve_results())
        return out

    with fresh() as t:  # without any resolved call
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        alone = others(t, ba)
        plain = {}
        for name in NAMES:
            getattr(t, name)(ba, *ARGS, *ROOM[name])
            plain[name] = fetch(t, name)
        t.submit(ba, slot=0)
        t.submit(bb, slot=1)
        alone_tables = t.collect()
    with fresh() as t:  # resolved calls in between, on both slots; nothing collected until the end
        ba, bb = t.host_batch(*capi.pack_reads(a)), t.host_batch(*capi.pack_reads(b))
        t.submit(ba, slot=0)
        for name in NAMES:
            queue(t, name, bb, ARGS, 3, slot=1)
        t.refine(ba)
        t.resolve(ba)
        for name in NAMES:
            queue(t, name, ba, ARGS, 4, slot=0)
        t.submit(bb, slot=1)
        got = [t.refine_results(), t.resolve_results()]
        resolved_b = {name: fetch(t, name, 1) for name in NAMES}
        again = {}
        for name in NAMES:
            getattr(t, name)(ba, *ARGS, *ROOM[name])
            again[name] = fetch(t, name)
        tables = t.collect()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, alone))
    identical(again, plain)
    same(resolved_b, *host(b, 3))
    assert tables == alone_tables == O.run_short(O.OracleParams(), reads)
    assert sum(len(v) for v in tables.values()) > 0


# ---- the three commands, end to end
def write_fastq(path, reads):
    data = b"".join(b"@r%d\n" % i + r.encode() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads))
    with open(path, "wb") as f:
        f.write(data)


def run_cli(*args):
    r = subprocess.run([TREW, *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_cli_candidates(tmp_path):
    reads = [r for r, _ in RC.long_unit_set()][:4] + RC.child_reads(VC.SHORT_REPAIRED)[:2] + [VC.SHORT_REPAIRED, TC.WEAK_FIRST, TC.TWO_PERFECT] + VC.mixed_reads(3, 40)
    path = str(tmp_path / "resolved.fastq")
    write_fastq(path, reads)
    want_x, want_d = ref(reads, 3)
    t_rows, t_tail = tandem_ref.cli_lines(path, reads, want_x[0], 3)
    assert run_cli("tandems", path, "--candidates", "3", "-t", "2") == t_rows + t_tail
    d_rows, d_tail = decompose_ref.cli_lines(path, reads, want_d, 3)
    assert run_cli("decompose", path, "--candidates", "3", "-t", "3") == d_rows + d_tail
    i_rows, i_tail = decompose_ref.cli_lines(path, reads, want_d, 3, per_item=True)
    assert run_cli("decompose", path, "--candidates", "3", "--items") == i_rows + i_tail
    x_rows, x_tail = dissect_ref.cli_lines(path, reads, want_x, 3)
    assert run_cli("dissect", path, "--candidates", "3", "-t", "2") == x_rows + x_tail
    xi_rows, xi_tail = dissect_ref.cli_lines(path, reads, want_x, 3, per_item=True)
    assert run_cli("dissect", path, "--candidates", "3", "--items") == xi_rows + xi_tail
    for command in NAMES:  # one candidate is the plain command, byte for byte, and differs from three on these reads
        plain = subprocess.run([TREW, command, path], capture_output=True, timeout=600)
        one = subprocess.run([TREW, command, path, "--candidates", "1"], capture_output=True, timeout=600)
        assert plain.returncode == 0 and one.returncode == 0 and plain.stdout == one.stdout and len(plain.stdout) > 1000
        assert plain.stdout.decode().splitlines() != {"tandems": t_rows + t_tail, "decompose": d_rows + d_tail, "dissect": x_rows + x_tail}[command]
