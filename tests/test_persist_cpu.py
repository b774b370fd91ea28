"""The reads and the schedule of tests/test_gpu_persist.py (persist_cases.py), checked on the host: the de Bruijn sequence, the
pairs of kinds every wave works through, the property every kind of read was built for (with the host definitions, capi.*_host,
at penalty 3, min_score 24, periods 1 to 32 and persist_cases.MOTIFS), and the tiling of the per-kind host results into the
expected results of a batch.

Host cost: the fourteen host definitions over the 4640-read batch (0.9 Mbases) take 29 s on one core here -- trace 9.5 s, align
4.8 s, dissect 3.4 s, decompose 3.1 s, tandems 2.2 s, refine 1.0 s, the other eight 1.5 s together.  So the expected results
of that batch and of the production-grid batch are TILED: the host definition of every kind as a batch of one read, repeated by
the schedule with the read index rewritten (measure_slots.Tiled; trew_hip.h: a read's output does not depend on the rest of the
batch).  test_tiling_equals_the_host_definition_of_the_whole_batch checks the tiling itself against the direct computation for
the nine measures that take a second or less, every shape of result among them."""
import numpy as np
import pytest

import persist_cases as P
from measure_slots import DEFAULT, Expected, Tiled, same
from trew_amd import capi

MOTIF_LISTS = {name: P.MOTIFS for name in ("annotate", "tracts", "intervals", "variants", "chain", "align", "trace")}


@pytest.fixture(scope="module")
def res():
    """{measure: host definition over the twelve kinds as one batch}"""
    packed = capi.pack_reads(list(P.kinds()))
    return {name: P.host(name, packed) for name in P.MEASURES}


def of_read(recs, r):
    return recs[recs["read"] == r]


def test_debruijn():
    for k in (1, 2, 3, 5, P.K):
        P.check_debruijn(P.debruijn(k), k)
    assert P.debruijn(2) == [0, 0, 1, 1]
    with pytest.raises(AssertionError):
        P.check_debruijn(list(range(P.K)) * P.K, P.K)  # the check is no tautology: this one misses (a, a)


def test_every_wave_of_the_small_grid_works_through_every_ordered_pair():
    reads, sched = P.batch(32, P.K * P.K + 1)
    assert len(reads) == 4640 and 850000 < sum(len(r) for r in reads) < 950000
    assert sched[5 * 32 + 7] == P.debruijn(P.K)[(5 + 7) % 144]
    every = {(a, b) for a in range(P.K) for b in range(P.K)}
    per_wave = P.pairs_per_wave(sched, 32)
    assert len(per_wave) == 32 and all(pairs == every for pairs in per_wave)


def test_the_production_grid_works_through_every_ordered_pair_over_its_waves():
    waves = 8192
    reads, sched = P.batch(waves, 3, cut=waves // 2)
    assert len(reads) == 20480 and max(len(r) for r in P.kinds()) <= 550
    per_wave = P.pairs_per_wave(sched, waves)
    assert all(len(pairs) >= 1 for pairs in per_wave) and all(len(pairs) == 2 for pairs in per_wave[:waves // 2])  # second and third read
    assert set().union(*per_wave) == {(a, b) for a in range(P.K) for b in range(P.K)}


def test_the_reads_are_the_same_on_a_second_build():
    first = P.kinds()
    P.kinds.cache_clear()
    second = P.kinds()
    assert first == second and len(first) == P.K
    assert [len(r) for r in first[:4]] == [0, 1, 70, 150] and first[2] == b"N" * 70


def test_kinds_without_a_record(res):
    """kinds 0 to 3: the empty read, one base, 70 N and 150 random bases -- no measure says anything (persist_cases.has_record)"""
    for kind in range(4):
        for name in P.MEASURES:
            assert not P.has_record(name, res[name], kind), (kind, name)
    for kind in (0, 2):  # not even a score
        assert not any(res["align"][kind][f].any() for f in capi.ALIGN_DTYPE.names)


def test_kinds_of_the_trace_blocks(res):
    """kind 4: one LDS block of direction bytes (fewer than 64 rows); kind 5: three (more than 128 rows) and all of period
    32's consensus bins; kind 6: strand rev alone; kind 7: both strands"""
    a = res["trace"][2]
    tel, u32 = a[:, 0], a[:, 2]
    assert P.MIN_SCORE <= tel[4]["score_fwd"] < 2 * P.MIN_SCORE and tel[4]["score_rev"] < P.MIN_SCORE
    assert 0 < tel[4]["end_fwd"] - tel[4]["start_fwd"] < 64 and res["trace"][1][4, 0, 0] > 0
    assert not (a[4]["score_fwd"][1:] >= P.MIN_SCORE).any() and not (a[4]["score_rev"][1:] >= P.MIN_SCORE).any()  # TTAGGG alone is traced
    assert u32[5]["score_fwd"] >= P.MIN_SCORE and u32[5]["end_fwd"] - u32[5]["start_fwd"] > 128 and res["trace"][1][5, 2, 0] > 0
    p = res["periods"][5]
    assert (p["period"], p["scored_period"]) == (32, 32) and p["end"] - p["start"] >= 4 * 32  # every one of the 4 x 32 bins gets votes
    assert tel[6]["score_rev"] >= P.MIN_SCORE > tel[6]["score_fwd"] and res["trace"][1][6, 0].tolist()[0] == 0 < res["trace"][1][6, 0, 1]
    assert tel[7]["score_fwd"] >= P.MIN_SCORE and tel[7]["score_rev"] >= P.MIN_SCORE and (res["trace"][1][7, 0] > 0).all()


def test_kind_with_edits(res):
    """kind 8: refine re-votes the unit; trace and decompose have an edited item with an insertion and one with a deletion"""
    assert res["refine"][8]["changed"] > 0
    for name in ("trace", "decompose"):
        items = of_read(res[name][0], 8)
        assert (items["insertions"] > 0).any() and (items["deletions"] > 0).any(), name


def test_kinds_of_the_piece_walk(res):
    """kind 9: two records; kind 10: depth 3 and more, and the best tract has tracts on both sides (the longer piece is pushed,
    the shorter walked, the pushed one popped); kind 11: period 171 for satellites alone"""
    for name in ("repeats", "tandems"):
        assert len(of_read(res[name][0], 9)) == 2 and res[name][1][9] == 2, name
        recs = of_read(res[name][0], 10)
        assert recs["depth"].max() >= 3 and len(recs) >= 6, name
        top = recs[recs["depth"] == 0]
        assert len(top) == 1 and (recs["end"] <= top[0]["start"]).any() and (recs["start"] >= top[0]["end"]).any(), name
    assert res["dissect"][2][9].tolist()[0] == 2 and len(of_read(res["dissect"][0], 9)) == 2
    assert res["dissect"][2][10, 0] >= 6
    sat = of_read(res["satellites"][0], 11)
    assert len(sat) == 1 and sat[0]["period"] == 171 and (sat[0]["start"], sat[0]["end"]) == (0, 513)
    for name in ("periods", "repeats", "refine", "tandems", "decompose", "dissect"):
        assert not P.has_record(name, res[name], 11), name


def test_every_measure_has_kinds_with_a_record_and_kinds_without(res):
    """so that both orders -- a record behind none, none behind a record -- are in every wave's sequence for every measure"""
    assert len(P.MEASURES) == 14
    for name in P.MEASURES:
        have = [P.has_record(name, res[name], kind) for kind in range(P.K)]
        assert sum(have) >= 4 and have.count(False) >= 3, (name, have)


QUICK = ["annotate", "tracts", "intervals", "variants", "periods", "chain", "repeats", "satellites", "refine"]  # a second or less on the 4640 reads


@pytest.mark.parametrize("name", QUICK)
def test_tiling_equals_the_host_definition_of_the_whole_batch(name):
    """the expected results of the GPU tests are tiled from the kinds (see the head of this file): for the measures whose host
    definition is quick -- arrays per read, per (read, motif), the three logs' records, the counts, the totals, the two
    histograms -- the tiled result is the host definition of the whole batch, byte for byte"""
    reads, sched = P.batch(32, P.K * P.K + 1)
    direct = Expected(reads, MOTIF_LISTS, eager=False).host(name)
    tiled = Tiled(P.kinds(), sched, MOTIF_LISTS).host(name)
    if isinstance(direct, np.ndarray):
        direct, tiled = (direct,), (tiled,)
    assert len(direct) == len(tiled)
    for i, (d, t) in enumerate(zip(direct, tiled)):
        if isinstance(d, np.ndarray):
            same(t, d, "%s part %d" % (name, i))
        else:
            assert t == d and d > 0, (name, i)


def test_tiled_totals_of_the_slow_measures():
    """for the five measures that are tiled because they are slow, on a short schedule: the tiled result is the direct one"""
    sched = P.schedule(5, 30)
    reads = [P.kinds()[k] for k in sched]
    direct, tiled = Expected(reads, MOTIF_LISTS, eager=False), Tiled(P.kinds(), sched, MOTIF_LISTS)
    for name in ("align", "tandems", "trace", "decompose", "dissect"):
        d, t = direct.host(name), tiled.host(name)
        for i, (x, y) in enumerate(zip((d,) if isinstance(d, np.ndarray) else d, (t,) if isinstance(t, np.ndarray) else t)):
            if isinstance(x, np.ndarray):
                same(y, x, "%s part %d" % (name, i))
            else:
                assert x == y and x > 0, (name, i)
    assert tiled.rows("decompose") == direct.rows("decompose") > 0 and tiled.trace_rows() == direct.trace_rows() > 0
    assert DEFAULT.args("satellites") == (1, 256, 3, 24) and DEFAULT.args("trace") == (3, 24)
