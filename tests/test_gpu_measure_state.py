"""The per-measure state of a slot (trew_capi.cpp: MeasureState, stage_motifs, grow, the log counters): the fourteen per-read
measures queued back to back on one slot, each with a motif list (or none) and a batch of its own, keep their results apart;
the pattern tables are restaged exactly when they have to be; every buffer grows when a larger batch comes and carries nothing
over to the next call; a log that overflowed leaves nothing behind for the next call; a results call without its queue call
fails; two slots do not share any of it.  Every result is compared with the CPU definition (capi.*_host), integer for integer."""
import numpy as np
import pytest

from measure_cases import K32, make_reads
from measure_slots import LOGGED, ORDER, ROOMY, ROOMY_ROWS, Expected, fetch, queue, same  # the queue / fetch / compare machinery, shared with test_gpu_persist.py
from trew_amd import capi

pytestmark = pytest.mark.gpu

# lists of 1, 2, 8 and 3 motifs with k = 3, 6 and 32 among them.  stage_motifs skips a list that is a prefix of what the slot
# holds, so no list here is a prefix of the one queued in front of it (annotate follows trace in the rounds of the grow
# test): every call restages, variants with fewer motifs than are staged.  test_pattern_tables_are_restaged_when_they_must_be
# takes the other path on purpose
MOTIFS = {
    "annotate": ["TTAGGG"],
    "tracts": ["TTG", K32],
    "intervals": ["TTAGGG", "TTG", K32, "TTAGG", "TTTAGGG", "TCAGGG", "GGGTTA", "TTAGGGTTTAGGG"],
    "variants": [K32, "TTG", "TTAGGG"],
    "chain": ["TTAGGG", "TTG"],
    "align": [K32],
    "trace": ["TTG", "TTAGGG"],
}
# the lists of the second sequence: other lengths, other motifs, k = 3 and k = 32 again
MOTIFS_B = {
    "annotate": [K32, "TTAGGG", "CCCTAA"],
    "tracts": ["TTAGGG"],
    "intervals": ["TTG", "TTAGGG"],
    "variants": ["TTAGGG", "TCAGGG", "TTG", K32, "GGGTTA"],
    "chain": [K32],
    "align": ["TTG", "TTAGGG", "TTAGG", "AATGG"],
    "trace": ["TTAGGG", K32],
}
WITH_MOTIFS = [name for name in ORDER if name in MOTIFS]  # ORDER: of the queue calls in sequence_a
READS = make_reads()
SMALL = [READS[i] for i in (23, 29, 17, 11)]  # 65, 2017, 33 and 6 bases


@pytest.fixture(scope="module")
def expected():
    return {"small": Expected(SMALL, MOTIFS), "full": Expected(READS, MOTIFS)}


@pytest.fixture(scope="module")
def t():
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 14, max_batch_reads=64, table_log2_slots=12) as ctx:
        yield ctx


def sequence_a(t, e):
    """the fourteen measures queued back to back on slot 0, fetched in reverse order; returns the variants histograms"""
    found = e.intervals[2]
    for name in ORDER:
        queue(t, name, e, cap=max(found, 1) if name == "intervals" else ROOMY)
    got = {name: fetch(t, name, e) for name in reversed(ORDER)}
    v, hist, reads_with = got["variants"]
    same(v, e.variants[0], "variants")
    same(hist, e.variants[1], "hist")
    same(reads_with, e.variants[2], "reads_with")
    iv, counts, n = got["intervals"]
    assert n == found
    same(iv, e.intervals[0], "intervals")
    same(counts, e.intervals[1], "interval counts")
    same(got["tracts"], e.tracts, "tracts")
    same(got["annotate"], e.annotate, "annotate")
    return hist, reads_with


def test_results_call_without_its_queue_call_fails():
    """first in the file: needs a context of its own on which nothing was queued"""
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 12, max_batch_reads=16, table_log2_slots=12) as fresh:
        fetch = {name: getattr(fresh, name + "_results") for name in ORDER}
        assert len(fetch) == 14
        for name, f in fetch.items():
            with pytest.raises(capi.TrewHipError, match="no trew_hip_%s on this slot yet" % name):
                f()
        fresh.annotate(fresh.host_batch(*capi.pack_reads(SMALL)), MOTIFS["annotate"])
        assert fresh.annotate_results().shape == (len(SMALL), 1)
        for name in ORDER[1:]:
            with pytest.raises(capi.TrewHipError, match="no trew_hip_%s on this slot yet" % name):
                fetch[name]()


def test_the_expected_results_are_not_trivial(expected):
    e = expected["full"]
    assert len(READS) == 40 and e.intervals[2] > len(READS)
    assert WITH_MOTIFS[-1] == "trace" and set(MOTIFS) == set(MOTIFS_B) == set(WITH_MOTIFS)
    for lists in (MOTIFS, MOTIFS_B):
        for i, name in enumerate(WITH_MOTIFS):  # no list is a prefix of the one staged in front of it, round after round
            assert lists[WITH_MOTIFS[i - 1]][:len(lists[name])] != lists[name], name
    assert e.annotate["windows_fwd"].sum() > 1000 and e.annotate["windows_rev"].sum() > 1000
    assert all((e.tracts["head_len_fwd"][:, m] > 0).any() for m in range(2))
    assert all(e.variants[1][m].sum() > 0 for m in range(3))
    assert all((e.intervals[1][:, m] > 0).any() for m in range(4))
    # the eight newer measures: records on both batches, and more than the one record (chain: event) of the overflow test's log
    for key in ("small", "full"):
        x = expected[key]
        assert (x.host("periods")["period"] > 0).sum() >= 2 and (x.host("refine")["period"] > 0).sum() >= 2
        for name in LOGGED:
            assert 2 * x.n // 5 < x.found(name) < ROOMY // 8, (key, name)
        assert x.found("tandems") > 1 and x.found("trace") > 1
        assert 1 < x.trace_rows() and max(x.trace_rows(), x.trace_rows(MOTIFS_B["trace"])) < ROOMY_ROWS // 2
        # decompose and dissect: more than the one item, record or row of the overflow tests, and the rows below the workspace
        assert x.found("decompose") > 1 and x.found("dissect") > 1 and 1 < x.dissect_records() < ROOMY // 8
        assert 1 < x.rows("decompose") < ROOMY_ROWS // 2 and 1 < x.rows("dissect") < ROOMY_ROWS // 2
        assert x.dissect_records() == len(x.host("dissect")[0]) == x.found("tandems") and x.found("dissect") == len(x.host("dissect")[1])
        assert all((x.host("chain")[1][:, m] > 0).any() for m in range(2))
    assert e.dissect_records() > e.n * 4 // 5 and e.found("dissect") > e.found("decompose") and e.rows("dissect") > e.rows("decompose")  # tracts beside the best one
    assert (e.host("align")["score_fwd"] > 24).any() and (e.host("align")["score_rev"] > 24).any()
    assert len({r["period"] for r in e.host("satellites")[0]}) >= 3 and len({r["period"] for r in e.host("repeats")[0]}) >= 3
    for lists in (MOTIFS, MOTIFS_B):
        assert {3, 32} <= {len(m) for ms in lists.values() for m in ms}
    assert all(MOTIFS[name] != MOTIFS_B[name] for name in MOTIFS)


def test_four_measures_back_to_back_on_one_slot(t, expected):
    """(all fourteen since the ten newer ones came; the name is the one the test has always had)"""
    sequence_a(t, expected["full"])


def test_alternating_batches_and_other_motif_lists(t, expected):
    """consecutive calls use different batches (the small and the full one in turn) and the lists of MOTIFS_B; nothing is
    fetched until all fourteen are queued, then in the order of the queue calls"""
    batch = {name: expected["small" if i % 2 == 0 else "full"] for i, name in enumerate(ORDER)}
    for name in ORDER:
        queue(t, name, batch[name], MOTIFS_B.get(name))
    for name in ORDER:
        fetch(t, name, batch[name], MOTIFS_B.get(name))
    # and the other way round, fetched in reverse
    batch = {name: expected["full" if i % 2 == 0 else "small"] for i, name in enumerate(ORDER)}
    for name in ORDER:
        queue(t, name, batch[name], MOTIFS_B.get(name))
    for name in reversed(ORDER):
        fetch(t, name, batch[name], MOTIFS_B.get(name))


def test_pattern_tables_are_restaged_when_they_must_be(expected):
    """stage_motifs keeps the slot's tables when the list is a prefix of what the slot holds, and only then.  After a call with
    eight motifs: its first one, its first three and all eight (none restages); the eight with another last motif (same
    number as staged); three with another last motif; four, one more than staged then, whose first three are the staged
    ones.  Nothing is fetched in between; a context of its own, so that what is staged is what this test staged."""
    e = expected["full"]
    eight = MOTIFS["intervals"]
    assert len(eight) == 8 and (len(eight[0]), len(eight[1]), len(eight[2])) == (6, 3, 32)
    other_last = eight[:7] + ["TTAGGC"]
    three = eight[:2] + ["TGAGGG"]
    four = three + ["CCCTAA"]
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 14, max_batch_reads=64, table_log2_slots=12) as ctx:
        calls = [("intervals", eight), ("align", eight[:1]), ("chain", eight[:3]), ("tracts", eight), ("annotate", other_last), ("variants", three)]
        for name, motifs in calls:
            queue(ctx, name, e, motifs)
        fetch(ctx, "align", e, eight[:1])
        queue(ctx, "align", e, four)
        for name, motifs in calls[:1] + calls[2:] + [("align", four)]:
            fetch(ctx, name, e, motifs)
        # back to a prefix of a longer list that is no longer staged: the first motif of `four` is staged, the eighth of `eight` is not
        queue(ctx, "tracts", e, eight)
        queue(ctx, "annotate", e, four[:1])
        fetch(ctx, "annotate", e, four[:1])
        fetch(ctx, "tracts", e, eight)
    assert not np.array_equal(e.host("annotate", other_last)[:, 7], e.host("annotate", eight)[:, 7])  # the last motif matters


@pytest.mark.parametrize("name", LOGGED)
def test_a_log_that_overflowed_leaves_nothing_behind(t, expected, name):
    """a call whose log holds one record, another measure's call, then the same call with room: the counts and the numbers
    found are exact both times, the records complete the second time; on the small and on the full batch"""
    other = "periods" if name != "repeats" else "annotate"
    for key in ("full", "small", "full"):
        e = expected[key]
        queue(t, name, e, cap=1)
        fetch(t, name, e, overflowed=True)
        queue(t, other, e)
        queue(t, name, e, cap=e.found(name) if name != "chain" else ROOMY)
        fetch(t, name, e)
        fetch(t, other, e)
    # queued back to back without a fetch in between: the second call's counter starts at zero
    queue(t, name, expected["full"], cap=1)
    queue(t, name, expected["small"])
    fetch(t, name, expected["small"])


def test_a_trace_workspace_that_overflowed_leaves_nothing_behind(t, expected):
    """the overflow test once more for trace's second counter: a log with room and a workspace of one row, another measure's
    call, then room for both -- exactly the rows the first call reported"""
    for key in ("full", "small", "full"):
        e = expected[key]
        queue(t, "trace", e, rows=1)
        fetch(t, "trace", e, overflowed=True)
        queue(t, "align", e)
        queue(t, "trace", e, cap=e.found("trace"), rows=e.trace_rows())
        fetch(t, "trace", e)
        fetch(t, "align", e)
    queue(t, "trace", expected["full"], rows=1)
    queue(t, "trace", expected["small"])
    fetch(t, "trace", expected["small"])


FURTHER = [("decompose", "rows"), ("dissect", "records"), ("dissect", "cap"), ("dissect", "rows")]


@pytest.mark.parametrize("name,short", FURTHER, ids=["%s-%s" % (n, "items" if c == "cap" else c) for n, c in FURTHER])
def test_a_further_counter_that_overflowed_leaves_nothing_behind(t, expected, name, short):
    """the overflow test once more for the counters beside the first: decompose's workspace, and each of dissect's three
    capacities -- records, items, rows -- at 1 alone with the other two roomy.  The call is refused; then a call of a measure
    that runs the same kernels' code on a state of its own (refine behind decompose, tandems behind dissect); then the refused
    call again with exactly the numbers it reported"""
    other = "refine" if name == "decompose" else "tandems"
    for key in ("full", "small", "full"):
        e = expected[key]
        queue(t, name, e, **{short: 1})
        got = fetch(t, name, e, overflowed=True)
        queue(t, other, e)
        if name == "decompose":
            queue(t, name, e, cap=got[3], rows=got[4])
        else:
            queue(t, name, e, records=got[3], cap=got[4], rows=got[5])
        fetch(t, name, e)
        fetch(t, other, e)
    # queued back to back without a fetch in between: every counter of the second call starts at zero
    queue(t, name, expected["full"], **{short: 1})
    queue(t, name, expected["small"])
    fetch(t, name, expected["small"])


def test_buffers_grow_and_nothing_accumulates(expected):
    """a context of its own, so that the first round is the first use of every buffer and the second grows each of them"""
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 14, max_batch_reads=64, table_log2_slots=12) as ctx:
        first = sequence_a(ctx, expected["small"])
        sequence_a(ctx, expected["full"])
        third = sequence_a(ctx, expected["small"])
    same(third[0], first[0], "hist of the third round")
    same(third[1], first[1], "reads_with of the third round")


def test_two_slots_interleaved(expected):
    """the fourteen measures on slots 0 and 1, interleaved call by call with different batches and motif lists; slot 1 is fetched
    first, in reverse order"""
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=2, max_batch_words=1 << 14, max_batch_reads=64, table_log2_slots=12) as ctx:
        for name in ORDER:
            queue(ctx, name, expected["full"], slot=0)
            queue(ctx, name, expected["small"], MOTIFS_B.get(name), slot=1)
        for name in reversed(ORDER):
            fetch(ctx, name, expected["small"], MOTIFS_B.get(name), slot=1)
        for name in ORDER:
            fetch(ctx, name, expected["full"], slot=0)
