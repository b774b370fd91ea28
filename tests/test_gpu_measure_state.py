"""The per-measure state of a slot (trew_capi.cpp: MeasureState): the four per-read motif measures queued back to back on
one slot, each with a motif list of its own, keep their results apart; every buffer grows when a larger batch comes and
carries nothing over to the next call; a results call without its queue call fails.  Every result is compared with the
CPU definition (capi.*_host), integer for integer."""
import numpy as np
import pytest

from measure_cases import K32, make_reads
from trew_amd import capi

pytestmark = pytest.mark.gpu

# lists of 1, 2, 8 and 3 motifs with k = 3, 6 and 32 among them.  stage_motifs skips a list that is a prefix of what the slot
# holds, so no list here is a prefix of the one queued in front of it (annotate follows variants in the rounds of the grow
# test): every call restages, variants with fewer motifs than are staged
MOTIFS = {
    "annotate": ["TTAGGG"],
    "tracts": ["TTG", K32],
    "intervals": ["TTAGGG", "TTG", K32, "TTAGG", "TTTAGGG", "TCAGGG", "GGGTTA", "TTAGGGTTTAGGG"],
    "variants": [K32, "TTG", "TTAGGG"],
}
ORDER = ["annotate", "tracts", "intervals", "variants"]  # of the queue calls in sequence_a
READS = make_reads()
SMALL = [READS[i] for i in (23, 29, 17, 11)]  # 65, 2017, 33 and 6 bases


class Expected:
    """the CPU definitions of one batch, computed once"""

    def __init__(self, reads):
        self.packed = capi.pack_reads(reads)
        self.annotate = capi.annotate_host(self.packed, MOTIFS["annotate"])
        self.tracts = capi.tracts_host(self.packed, MOTIFS["tracts"], 3)
        self.intervals = capi.intervals_host(self.packed, MOTIFS["intervals"])
        self.variants = capi.variants_host(self.packed, MOTIFS["variants"])


@pytest.fixture(scope="module")
def expected():
    return {"small": Expected(SMALL), "full": Expected(READS)}


@pytest.fixture(scope="module")
def t():
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 14, max_batch_reads=64, table_log2_slots=12) as ctx:
        yield ctx


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), "%s differs at %s" % (what, np.argwhere(got != want)[:1].tolist())


def sequence_a(t, e):
    """the four measures queued back to back on slot 0, fetched in reverse order; returns the variants histograms"""
    b = t.host_batch(*e.packed)
    found = e.intervals[2]
    t.annotate(b, MOTIFS["annotate"])
    t.tracts(b, MOTIFS["tracts"], 3)
    t.intervals(b, MOTIFS["intervals"], max_intervals=max(found, 1))
    t.variants(b, MOTIFS["variants"])
    v, hist, reads_with = t.variants_results()
    same(v, e.variants[0], "variants")
    same(hist, e.variants[1], "hist")
    same(reads_with, e.variants[2], "reads_with")
    iv, counts, n = t.intervals_results()
    assert n == found
    same(iv, e.intervals[0], "intervals")
    same(counts, e.intervals[1], "interval counts")
    same(t.tracts_results(), e.tracts, "tracts")
    same(t.annotate_results(), e.annotate, "annotate")
    return hist, reads_with


def test_results_call_without_its_queue_call_fails():
    """first in the file: needs a context of its own on which nothing was queued"""
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 12, max_batch_reads=16, table_log2_slots=12) as fresh:
        fetch = {"annotate": fresh.annotate_results, "tracts": fresh.tracts_results, "intervals": fresh.intervals_results, "variants": fresh.variants_results}
        for name, f in fetch.items():
            with pytest.raises(capi.TrewHipError, match="no trew_hip_%s on this slot yet" % name):
                f()
        fresh.annotate(fresh.host_batch(*capi.pack_reads(SMALL)), MOTIFS["annotate"])
        assert fresh.annotate_results().shape == (len(SMALL), 1)
        for name in ("tracts", "intervals", "variants"):
            with pytest.raises(capi.TrewHipError, match="no trew_hip_%s on this slot yet" % name):
                fetch[name]()


def test_the_expected_results_are_not_trivial(expected):
    e = expected["full"]
    assert len(READS) == 40 and e.intervals[2] > len(READS)
    for i, name in enumerate(ORDER):  # no list is a prefix of the one staged in front of it, round after round
        assert MOTIFS[ORDER[i - 1]][:len(MOTIFS[name])] != MOTIFS[name], name
    assert e.annotate["windows_fwd"].sum() > 1000 and e.annotate["windows_rev"].sum() > 1000
    assert all((e.tracts["head_len_fwd"][:, m] > 0).any() for m in range(2))
    assert all(e.variants[1][m].sum() > 0 for m in range(3))
    assert all((e.intervals[1][:, m] > 0).any() for m in range(4))


def test_four_measures_back_to_back_on_one_slot(t, expected):
    sequence_a(t, expected["full"])


def test_buffers_grow_and_nothing_accumulates(expected):
    """a context of its own, so that the first round is the first use of every buffer and the second grows each of them"""
    with capi.TrewHip(mode=capi.MODE_SHORT, n_slots=1, max_batch_words=1 << 14, max_batch_reads=64, table_log2_slots=12) as ctx:
        first = sequence_a(ctx, expected["small"])
        sequence_a(ctx, expected["full"])
        third = sequence_a(ctx, expected["small"])
    same(third[0], first[0], "hist of the third round")
    same(third[1], first[1], "reads_with of the third round")
