"""The persistent loop of the wave-per-read kernels: `for (r = wave; r < B.n_reads; r += n_waves)`.  launch_wave_per_read starts
min(ceil(n_reads / 4), 8 n_cu) blocks of four waves, 8192 waves on 256 CUs, so a wave sees a second read only in a batch of more
than 8192 reads -- every production batch, and next to no batch of the other GPU tests.  What a wave carries from one read to
the next (the LDS consensus bins, variants' bins, the block of direction bytes of trace, decompose and dissect, whatever the
compiler hoists out of the read loop) is pinned here: with TREW_FLAG_DEBUG_ONE_CU the grid is that of a one-CU device, 32 waves,
and the 4640 reads of persist_cases.schedule(32, 145) take every wave through every ordered pair (previous read, next read) of
the twelve kinds of read of persist_cases.py; without the flag a batch of two and a half trips of the device's own grid does
the same over its waves.  Every part of every result is compared with the host definition (capi.*_host, tiled from the kinds:
tests/test_persist_cpu.py), integer for integer."""
import pytest

import persist_cases as P
from measure_slots import DE_NOVO, DEFAULT, LOGGED, ORDER, Setting, Tiled, fetch, queue
from trew_amd import capi

pytestmark = pytest.mark.gpu

FLAGS = capi.FLAG_DEBUG_ONE_CU | capi.FLAG_DEBUG_ANNOT_GENERAL  # the second: annotate takes its wave-per-read kernel
MOTIF_LISTS = {name: P.MOTIFS for name in ORDER if name not in DE_NOVO}
WAVES, TRIPS = 32, P.K * P.K + 1
WITH_ROWS = ["trace", "decompose", "dissect"]
# test_other_parameters: the de novo measures with other periods, penalty and min_score, satellites also over all its periods;
# the motif measures with the list reversed and penalty 1, trace also with another min_score
OTHER = Setting(2, 12, 5, 10)
OTHER_MOTIF = Setting(1, None, 1, 10)


def context(e, flags, n_slots=1):
    return capi.TrewHip(mode=capi.MODE_SHORT, n_slots=n_slots, max_batch_words=len(e.packed[0]) + 64, max_batch_reads=e.n + 64, table_log2_slots=12,
                        flags=flags)


@pytest.fixture(scope="module")
def e():
    """the 4640-read batch and its expected results"""
    reads, sched = P.batch(WAVES, TRIPS)
    assert len(reads) == WAVES * TRIPS == 4640
    return Tiled(P.kinds(), sched, MOTIF_LISTS)


@pytest.fixture(scope="module")
def t(e):
    with context(e, FLAGS) as ctx:
        yield ctx


def room(e, name, motifs=None, setting=DEFAULT):
    """roomy capacities for a queue call of `name`: twice what the host definition counts (chain's log holds events, of which the
    host counts none: sixteen an item)"""
    out = {}
    if name in LOGGED:
        out["cap"] = (16 if name == "chain" else 2) * e.found(name, motifs, setting) + 64
    if name in WITH_ROWS:
        out["rows"] = 2 * (e.trace_rows(motifs, setting) if name == "trace" else e.rows(name, setting)) + 64
    if name == "dissect":
        out["records"] = 2 * e.dissect_records(setting) + 64
    return out


def test_grid_is_small_under_the_flag(t, e):
    assert t.debug_measure_grid(e.n) == 8 == t.debug_measure_grid(1 << 40) and 4 * 8 == WAVES
    assert t.debug_measure_grid(0) == 0 and t.debug_measure_grid(5) == 2
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 12, max_batch_reads=16, table_log2_slots=12) as plain:
        blocks, full = plain.debug_measure_grid(e.n), plain.debug_measure_grid(1 << 40)
    assert full % 8 == 0 and full > 8  # eight blocks a CU, more than one CU
    assert (e.n + 3) // 4 == 1160 and blocks == min(1160, full) and blocks > 8


@pytest.mark.parametrize("name", ORDER)
def test_every_ordered_pair_of_reads_in_every_wave(t, e, name):
    """every wave of the 32 works through all 144 ordered pairs of kinds (test_persist_cpu.py); twice on the same slot"""
    assert 4 * t.debug_measure_grid(e.n) == WAVES and e.n == WAVES * TRIPS
    for _ in range(2):
        queue(t, name, e, **room(e, name))
        fetch(t, name, e)


# the last case, satellites over all its periods, is what DEFAULT gives satellites (max_period None is its 256): it adds no new
# parameters to test_every_ordered_pair_of_reads_in_every_wave[satellites] and stands here, written out, beside the narrow range
OTHER_CASES = [(name, OTHER if name in DE_NOVO else OTHER_MOTIF) for name in ORDER] + [("satellites", Setting(1, 256, 3, 24))]


@pytest.mark.parametrize("name,setting", OTHER_CASES, ids=["%s-%s" % (name, "-".join(str(x) for x in s)) for name, s in OTHER_CASES])
def test_other_parameters(t, e, name, setting):
    motifs = None if name in DE_NOVO else P.MOTIFS[::-1]
    if name in ("repeats", "tandems", "trace"):  # the other setting finds other things
        assert e.found(name, motifs, setting) != e.found(name)
    queue(t, name, e, motifs, setting=setting, **room(e, name, motifs, setting))
    fetch(t, name, e, motifs, setting=setting)


SHORT = [(name, "cap") for name in LOGGED] + [("dissect", "records")] + [(name, "rows") for name in WITH_ROWS]


@pytest.mark.parametrize("name,short", SHORT, ids=["%s-%s" % (n, {"cap": "log"}.get(c, c)) for n, c in SHORT])
def test_logs_and_workspace_run_out_in_mid_wave(t, e, name, short):
    """one capacity at half of what the host definition counts, the others roomy: inside every wave's sequence of reads there
    are tracts that still fit and tracts that do not, in an order nobody controls.  The overflow contract holds (counts and
    numbers found exact -- for a row workspace that ran out through the recomputed rows of wrap_walk -- and what is copied is what
    trew_hip.h says); then the call again with exactly the reported numbers gives the full result."""
    caps = room(e, name)
    full = {"cap": e.found(name), "records": e.dissect_records(), "rows": e.trace_rows() if name == "trace" else e.rows(name)}[short]
    assert full >= 2 * e.n // P.K  # several a wave
    caps[short] = full // 2
    queue(t, name, e, **caps)
    got = fetch(t, name, e, overflowed=True, log_cap=caps[short])
    if name == "trace" or name == "decompose":
        exact = {"cap": got[3], "rows": got[4]}
    elif name == "dissect":
        exact = {"records": got[3], "cap": got[4], "rows": got[5]}
    else:
        exact = {"cap": got[3] if name == "chain" else got[2]}  # chain: the events
    queue(t, name, e, **exact)
    fetch(t, name, e)


@pytest.fixture(scope="module")
def production():
    """a context without TREW_FLAG_DEBUG_ONE_CU and a batch of two and a half trips of its own grid: on 256 CUs 8192 waves,
    20480 reads, 3.5 Mbases"""
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 12, max_batch_reads=16, table_log2_slots=12) as probe:
        waves = 4 * probe.debug_measure_grid(1 << 40)
    reads, sched = P.batch(waves, 3, cut=waves // 2)
    big = Tiled(P.kinds(), sched, MOTIF_LISTS)
    with context(big, capi.FLAG_DEBUG_ANNOT_GENERAL) as ctx:
        yield ctx, big, waves


@pytest.mark.parametrize("name", ORDER)
def test_production_grid_loops(production, name):
    """the device's own grid: every wave takes a second read and half of them a third, all 144 ordered pairs over the waves"""
    ctx, big, waves = production
    assert 4 * ctx.debug_measure_grid(big.n) == waves and big.n > 2 * waves
    pairs = P.pairs_per_wave(big.sched.tolist(), waves)
    assert all(pairs) and len(set().union(*pairs)) == P.K * P.K
    caps = room(big, name)
    if name in WITH_ROWS:  # the workspace from the host's count: trace has 64 bytes a row
        caps["rows"] = big.trace_rows() if name == "trace" else big.rows(name)
    queue(ctx, name, big, **caps)
    fetch(ctx, name, big)


def test_two_slots_under_the_flag(e):
    """tandems on slot 0 and trace on slot 1, queued without a wait between them: both as on a slot alone"""
    with context(e, FLAGS, n_slots=2) as ctx:
        queue(ctx, "tandems", e, slot=0, **room(e, "tandems"))
        queue(ctx, "trace", e, slot=1, **room(e, "trace"))
        fetch(ctx, "trace", e, slot=1)
        fetch(ctx, "tandems", e, slot=0)
