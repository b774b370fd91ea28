"""The prefilter's drain of the reads its uniform path sets aside (reads with an N in a half, reads passing a 4-bucket test):
filter_deferred_uni judges them in one joint k loop with per-lane window masks.  Where the k loop is each half's own
[kmin, kmax] (short and pair mode at 5..32) it flags exactly the reads the general path (TREW_FLAG_DEBUG_NO_UNI_DRAIN) flags,
so the worklists are the same multiset; every read the oracle records must be among them, and the tables equal the oracle's."""
import random
from collections import Counter

import numpy as np
import pytest

import oracle as O
import trew_amd as T
from trew_amd import capi
from helpers import mutate, periodic

FLAGS = (0, T.FLAG_DEBUG_NO_UNI_DRAIN)
TELO = "TTAGGG"


def _acgt(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def _put_n(s, positions):
    s = list(s)
    for p in positions:
        s[p] = "N"
    return "".join(s)


def _n_reads(rnd, count, n):
    """Reads of length n with Ns where they are awkward for per-lane window masks: 1-3 Ns in one half, at base 0, at n-1, on
    either side of the half boundary, adjacent Ns, Ns in both halves, an all-N half; over random, telomeric, homopolymer and
    noisy-periodic reads (and some without an N, so that the 4-bucket passers are in the drain as well)."""
    h = n // 2  # first base of the right half is n - (n + 1) // 2 == h
    out = []
    for i in range(count):
        kind = rnd.random()
        if kind < 0.3:
            s = periodic(TELO, n, rnd.randint(0, 5))
            s = mutate(s, rnd, p_sub=rnd.choice([0, 0.01, 0.04, 0.1]))
        elif kind < 0.4:
            s = rnd.choice("ACGT") * n
        elif kind < 0.7:
            unit = _acgt(rnd, rnd.randint(1, 24))
            s = mutate(periodic(unit, n, rnd.randint(0, 7)), rnd, p_sub=rnd.choice([0, 0.02, 0.08, 0.2]))
        else:
            s = _acgt(rnd, n)
        s = (s + _acgt(rnd, n))[:n]  # periodic() of a short unit at a late phase comes out short
        pat = i % 12
        if pat == 0:
            pos = [rnd.randrange(n)]
        elif pat == 1:
            pos = rnd.sample(range(h), 2)
        elif pat == 2:
            pos = rnd.sample(range(h, n), 3)
        elif pat == 3:
            pos = [0]
        elif pat == 4:
            pos = [n - 1]
        elif pat == 5:
            pos = [h - 1]
        elif pat == 6:
            pos = [h]
        elif pat == 7:
            p = rnd.randrange(n - 3)
            pos = [p, p + 1, p + 2][: rnd.randint(2, 3)]
        elif pat == 8:
            pos = [rnd.randrange(h), rnd.randrange(h, n)]
        elif pat == 9:
            pos = list(range(h)) if rnd.random() < 0.5 else list(range(h, n))
        elif pat == 10:
            pos = []
        else:
            pos = [rnd.randrange(n) for _ in range(rnd.randint(1, 3))]
        out.append(_put_n(s, pos).encode())
    return out


def _run(mode, words, n_units, n, flags):
    stride = 3 * ((n + 31) // 32)
    with T.TrewHip(mode=mode, max_batch_reads=n_units + 8, max_batch_words=1 << 20, flags=flags) as t:
        b = capi.Batch(words.ctypes.data, len(words), None, None, n, stride, n_units, 0, 0)  # uniform batch: the fast path
        t.submit(b, 0)
        t.wait(0)
        wl = Counter(int(x) for x in t.debug_worklist(0))
        return wl, t.collect()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [150, 151])
def test_uniform_drain_reads_with_n(n):
    rnd = random.Random(5100 + n)
    reads = _n_reads(rnd, 2400, n)
    p = O.OracleParams()
    passing = {i for i, r in enumerate(reads) if any(len(tb) for tb in O.run_short(p, [r]).values())}
    assert len(passing) > 200
    want = O.run_short(p, reads)
    words, _, _ = capi.pack_reads(reads)
    got = {f: _run(T.MODE_SHORT, words, len(reads), n, f) for f in FLAGS}
    for f in FLAGS:
        wl, tables = got[f]
        assert max(wl.values()) == 1  # no unit twice
        missing = passing - set(wl)
        assert not missing, ("a read with a passing (segment, k) was dropped by the prefilter", f, sorted(missing)[:5])
        assert tables == want
    assert got[0][0] == got[T.FLAG_DEBUG_NO_UNI_DRAIN][0]


@pytest.mark.gpu
def test_uniform_drain_config2_prefix_worklist_is_unchanged():
    """2 M reads of the benchmark's workload (device-generated, seed 20250218): the same worklist as the general path's."""
    n, L = 2_000_000, 150
    stride = 3 * ((L + 31) // 32)
    res = {}
    for f in FLAGS:
        with T.TrewHip(mode=T.MODE_SHORT, max_batch_reads=n, max_batch_words=16, table_log2_slots=20, flags=f) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(20250218, 0, n, L, d)
            t.submit(t.device_uniform_batch(d, n, L))
            t.wait()
            wl = np.sort(t.debug_worklist(0))
            res[f] = (wl, t.collect())
            t.free(d)
    assert len(res[0][0]) > 10_000
    assert np.array_equal(res[0][0], res[T.FLAG_DEBUG_NO_UNI_DRAIN][0])
    assert res[0][1] == res[T.FLAG_DEBUG_NO_UNI_DRAIN][1]


@pytest.mark.gpu
def test_uniform_drain_pairs_worklist_is_unchanged():
    """Pair mode (two joint pairs of halves per unit) on device-generated pairs: the same worklist and tables."""
    npairs, L = 200_000, 150
    stride = 3 * ((L + 31) // 32)
    res = {}
    for f in FLAGS:
        with T.TrewHip(mode=T.MODE_PAIR, max_batch_reads=2 * npairs, max_batch_words=16, table_log2_slots=20, flags=f) as t:
            d = t.malloc(2 * npairs * stride * 4 + 64)
            t.synth_pair_device(20250218, 0, npairs, L, d)
            t.submit(t.device_uniform_batch(d, 2 * npairs, L))
            t.wait()
            wl = np.sort(t.debug_worklist(0))
            res[f] = (wl, t.collect())
            t.free(d)
    assert len(res[0][0]) > 1000
    assert np.array_equal(res[0][0], res[T.FLAG_DEBUG_NO_UNI_DRAIN][0])
    assert res[0][1] == res[T.FLAG_DEBUG_NO_UNI_DRAIN][1]
