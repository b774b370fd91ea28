"""The queue / fetch / compare machinery of the fourteen per-read measures on a slot, shared by tests/test_gpu_measure_state.py
and tests/test_gpu_persist.py: Expected holds the CPU definitions (capi.*_host) of one batch, queue makes one queue call, fetch
the results call and compares every part of it with the host definition, integer for integer.  Tiled is an Expected whose batch
is a sequence of a few kinds of read: it computes the host definitions on the kinds and tiles them by the sequence."""
import collections

import numpy as np

from trew_amd import capi

ORDER = ["annotate", "tracts", "intervals", "variants", "periods", "chain", "repeats", "satellites", "align", "refine", "tandems", "trace", "decompose",
         "dissect"]
LOGGED = ["intervals", "chain", "repeats", "satellites", "tandems", "trace", "decompose", "dissect"]  # the measures with an append log and a counter
DE_NOVO = ["periods", "repeats", "satellites", "refine", "tandems", "decompose", "dissect"]  # no motif list: (min_period, max_period, penalty, min_score)
ROOMY = 1 << 16  # a log no batch of test_gpu_measure_state.py fills
ROOMY_ROWS = 1 << 18  # a trace workspace (64 bytes a row; decompose, dissect: 32) no batch of that file fills


class Setting(collections.namedtuple("Setting", "min_period max_period penalty min_score")):
    """the numbers of a queue call beside its motif list: the de novo measures take all four (max_period None: the measure's own
    default, 256 for satellites and 32 for the others), tracts and align the penalty, trace the penalty and min_score, the others
    none"""

    def args(self, name):
        if name in DE_NOVO:
            return (self.min_period, self.max_period or (256 if name == "satellites" else 32), self.penalty, self.min_score)
        return {"tracts": (self.penalty,), "align": (self.penalty,), "trace": (self.penalty, self.min_score)}.get(name, ())


DEFAULT = Setting(1, None, 3, 24)


class Expected:
    """the CPU definitions of one batch, computed once per (measure, motif list, setting); motif_lists: {measure: its motif list
    where a call names none}"""

    def __init__(self, reads, motif_lists, eager=True):
        self.packed = capi.pack_reads(reads)
        self.n = len(reads)
        self.motif_lists = motif_lists
        self._host = {}
        if eager:
            self.annotate = self.host("annotate")
            self.tracts = self.host("tracts")
            self.intervals = self.host("intervals")
            self.variants = self.host("variants")

    def compute(self, name, motifs, setting):
        f = getattr(capi, name + "_host")
        return f(self.packed, *(() if motifs is None else (motifs,)), *setting.args(name))

    def host(self, name, motifs=None, setting=DEFAULT):
        motifs = self.motif_lists.get(name) if motifs is None else motifs
        key = (name, tuple(motifs or ()), setting)
        if key not in self._host:
            self._host[key] = self.compute(name, motifs, setting)
        return self._host[key]

    def found(self, name, motifs=None, setting=DEFAULT):
        """the records (chain, trace, decompose, dissect: items) of a logged measure, as its host definition counts them"""
        return self.host(name, motifs, setting)[{"trace": 3, "decompose": 3, "dissect": 4}.get(name, 2)]

    def dissect_records(self, setting=DEFAULT):
        """the records of dissect's second log"""
        return self.host("dissect", None, setting)[3]

    def rows(self, name, setting=DEFAULT):
        """the workspace rows decompose and dissect claim, a row per base of a traced tract: decompose's from its refined
        records, dissect's as its host definition counts them"""
        if name == "dissect":
            return self.host("dissect", None, setting)[5]
        r = self.host("decompose", None, setting)[2]
        traced = (r["period"] > 0) & (r["score"] >= setting.min_score)
        return int((r["end"].astype(np.int64) - r["start"].astype(np.int64))[traced].sum())

    def trace_rows(self, motifs=None, setting=DEFAULT):
        """the workspace rows trace claims: for every (read, motif) with a strand whose score reaches min_score, the bases
        from the first start to the last end of those strands"""
        a = self.host("trace", motifs, setting)[2].astype([(f, "<i8") for f in capi.ALIGN_DTYPE.names])
        fwd, rev = a["score_fwd"] >= setting.min_score, a["score_rev"] >= setting.min_score
        lo = np.minimum(np.where(fwd, a["start_fwd"], 1 << 40), np.where(rev, a["start_rev"], 1 << 40))
        hi = np.maximum(np.where(fwd, a["end_fwd"], 0), np.where(rev, a["end_rev"], 0))
        return int((hi - lo)[fwd | rev].sum())


def tile_log(per_kind, sched):
    """the sorted log of a batch whose read r is kind sched[r], from the logs of the kinds taken each as a batch of one read (read
    index 0): every read's records in their order, the read index rewritten"""
    sched = np.asarray(sched)
    parts = []
    for k, recs in enumerate(per_kind):
        mine = np.flatnonzero(sched == k)
        if len(recs) == 0 or len(mine) == 0:
            continue
        assert not recs["read"].any()
        block = np.tile(recs, len(mine))
        block["read"] = np.repeat(mine, len(recs)).astype(block["read"].dtype)
        parts.append(block)
    if not parts:
        return per_kind[0][:0].copy()
    out = np.concatenate(parts)
    return out[np.argsort(out["read"], kind="stable")]  # a read's records stay in the order its kind has them in


class Tiled(Expected):
    """Expected for the batch [kinds[k] for k in sched], from the host definitions of the kinds, each taken as a batch of one read,
    tiled by sched.  trew_hip.h: a read's output does not depend on the rest of the batch; the batch totals (found, rows, the two
    histograms of variants) are sums over the reads."""

    def __init__(self, kinds, sched, motif_lists):
        Expected.__init__(self, [kinds[k] for k in sched], motif_lists, eager=False)
        self.sched = np.asarray(sched, dtype=np.int64)
        self.times = np.bincount(self.sched, minlength=len(kinds))  # reads of every kind
        self.one = [Expected([kind], motif_lists, eager=False) for kind in kinds]

    def compute(self, name, motifs, setting):
        per = [one.compute(name, motifs, setting) for one in self.one]
        if name in ("annotate", "tracts", "align", "periods", "refine"):
            return np.concatenate(per)[self.sched]

        def total(i):
            return sum(int(n) * p[i] for n, p in zip(self.times, per))

        def per_read(i):
            return np.concatenate([p[i] for p in per])[self.sched]

        def log(i):
            return tile_log([p[i] for p in per], self.sched)

        if name == "variants":
            return per_read(0), total(1).astype(np.uint64), total(2).astype(np.uint64)
        if name in ("trace", "decompose"):
            return log(0), per_read(1), per_read(2), total(3)
        if name == "dissect":
            return log(0), log(1), per_read(2), total(3), total(4), total(5)
        return log(0), per_read(1), total(2)


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), "%s differs at %s" % (what, np.argwhere(got != want)[:1].tolist())


def queue(t, name, e, motifs=None, cap=ROOMY, slot=0, rows=ROOMY_ROWS, records=ROOMY, setting=DEFAULT):
    """one queue call of measure `name` for the batch of `e`; cap: the log of the eight logged measures (trace, decompose,
    dissect: the item log); rows: the workspace of trace, decompose and dissect; records: dissect's second log"""
    b = t.host_batch(*e.packed)
    motifs = e.motif_lists.get(name) if motifs is None else motifs
    args = setting.args(name)
    if name == "intervals":
        t.intervals(b, motifs, max_intervals=cap, slot=slot)
    elif name == "chain":
        t.chain(b, motifs, max_events=cap, slot=slot)
    elif name in ("repeats", "satellites", "tandems"):
        getattr(t, name)(b, *args, max_records=cap, slot=slot)
    elif name in ("periods", "refine"):
        getattr(t, name)(b, *args, slot=slot)
    elif name == "trace":
        t.trace(b, motifs, *args, max_items=cap, max_rows=rows, slot=slot)
    elif name == "decompose":
        t.decompose(b, *args, max_items=cap, max_rows=rows, slot=slot)
    elif name == "dissect":
        t.dissect(b, *args, max_records=records, max_items=cap, max_rows=rows, slot=slot)
    else:  # annotate, variants; tracts and align with their penalty
        getattr(t, name)(b, motifs, *args, slot=slot)


def fetch(t, name, e, motifs=None, slot=0, overflowed=False, setting=DEFAULT, log_cap=1):
    """the results call of `name`, compared with the host definition of the batch of `e`.  overflowed: the log was too small --
    the counts and the numbers found are exact all the same; intervals keeps as many records as the log held (log_cap, each of
    them a record of the batch), the other five
    none (trace: its log or its workspace was too small; its alignment records and its rows are exact as well; decompose:
    likewise, with its refined records; dissect: any of its three capacities was too small -- no records and no items, the
    counts and the three numbers exact)"""
    want = e.host(name, motifs, setting)
    what = "%s (slot %d)" % (name, slot)
    got = getattr(t, name + "_results")(slot=slot)
    if name in ("annotate", "tracts", "align", "periods", "refine"):
        same(got, want, what)
    elif name == "variants":
        for g, w, part in zip(got, want, ("records", "hist", "reads_with")):
            same(g, w, what + " " + part)
    elif name == "decompose":
        items, counts, refined, n_items, n_rows = got
        assert (n_items, n_rows) == (e.found(name, None, setting), e.rows(name, setting)), what
        same(counts, want[1], what + " counts")
        same(refined, want[2], what + " refined records")
        if overflowed:
            assert len(items) == 0, what
        else:
            same(items, want[0], what + " items")
    elif name == "dissect":
        recs, items, counts, n_records, n_items, n_rows = got
        assert (n_records, n_items, n_rows) == (e.dissect_records(setting), e.found(name, None, setting), e.rows(name, setting)) == want[3:], what
        same(counts, want[2], what + " counts")
        if overflowed:
            assert len(recs) == 0 and len(items) == 0, what
        else:
            same(recs, want[0], what + " tandem records")
            same(items, want[1], what + " items")
    else:
        recs, counts = got[:2]
        found = got[3 if name == "trace" else 2]
        assert found == e.found(name, motifs, setting), what
        same(counts, want[1], what + " counts")
        if name == "trace":
            same(got[2], want[2], what + " alignment records")
            assert got[4] == e.trace_rows(motifs, setting), what
        if name == "chain":
            assert got[3] >= found, what  # an item takes at least one event
        if not overflowed:
            same(recs, want[0], what + " records")
        elif name == "intervals":
            known = {r.tobytes() for r in want[0]}
            assert len(recs) == log_cap and all(r.tobytes() in known for r in recs), what
        else:
            assert len(recs) == 0, what
    return got
