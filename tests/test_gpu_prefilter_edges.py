"""Soundness of the prefilter, and exactness of the exact kernel, at reads on the pass/fail edge -- on every production path.

edge_cases.py walks a periodic read towards failure one substitution at a time and keeps the last unit the oracle records
something for together with the first it records nothing for.  One batch per (mode, parameter set, length) holds every such
twin and 1000 random units, and runs as a uniform batch (with the joint halves loop and the uniform drain each switched on
and off), as a ragged batch (the general path; the only form of unequal mates and of long reads), and with the exact
kernel's group pass switched off.  In every configuration

  soundness    the worklist (trew_hip_debug_worklist) holds no unit twice and every unit the oracle records something for;
  exactness    the tables equal the oracle's: a `>` written for `>=`, a wrong rounding of LOW * COUNT, a tie resolved the
               wrong way or a recorded first-failing twin all show here;
  selectivity  at `5 32 0.5 0.8` and lengths 150 and 151 the flagged random units the oracle records nothing for stay under
               a cap (a prefilter that flags everything is sound, too).

The candidate masks (trew_hip_filter_masks, which switches the joint loop and the uniform drain off) are checked per
(segment, k) at the same reads.  Contexts are made once per (mode, parameters, flags) and fed the lengths one after another."""
import pytest

import trew_amd as T
from trew_amd import capi
import edge_cases as E
from test_gpu_parity import _table_diff

pytestmark = pytest.mark.gpu

NO_JOINT, NO_DRAIN, NO_GROUP = T.FLAG_DEBUG_NO_JOINT, T.FLAG_DEBUG_NO_UNI_DRAIN, T.FLAG_DEBUG_NO_GROUP
UNIFORM, RAGGED = "uniform", "ragged"
CONFIGS = [(UNIFORM, 0), (UNIFORM, NO_JOINT), (UNIFORM, NO_DRAIN), (UNIFORM, NO_JOINT | NO_DRAIN), (UNIFORM, NO_GROUP),
           (RAGGED, 0), (RAGGED, NO_GROUP)]
LONG_CONFIGS = [(RAGGED, 0), (RAGGED, NO_GROUP)]

# Flagged random units the oracle records nothing for, among the 1000 of a cell.  The project's bound on random sequence is 4
# candidate masks among 4000 random 75-base segments (test_filter_is_sound), i.e. 2 among the 2000 halves of 1000 reads and 4
# among the 4000 halves of 1000 pairs.  The cap is the larger of that and twice the count measured on an MI355X at the commit
# before this file, for the same seed (a handful of events scatters from seed to seed): (default flags,
# DEBUG_NO_JOINT | DEBUG_NO_UNI_DRAIN).  No random unit was flagged there in any configuration, so the scaled bound is the cap.
SELECTIVITY_MEASURED = {(E.SHORT, 150): (0, 0), (E.SHORT, 151): (0, 0), (E.PAIR, 150): (0, 0), (E.PAIR, 151): (0, 0)}
SELECTIVITY_BOUND = {E.SHORT: 2, E.PAIR: 4}


def _selectivity_cap(mode, n):
    return max(2 * max(SELECTIVITY_MEASURED[(mode, n)]), SELECTIVITY_BOUND[mode])


def _ids(v):
    if isinstance(v, tuple) and len(v) == 4:
        return "%d-%d-%.3g-%.3g" % v
    if isinstance(v, tuple):
        return "%s-%d" % v
    return str(v)


@pytest.fixture(scope="module")
def short_cells():
    return E.build_cells(E.SHORT)


@pytest.fixture(scope="module")
def pair_cells():
    return E.build_cells(E.PAIR)


@pytest.fixture(scope="module")
def long_cells():
    return E.build_cells(E.LONG)


def _packed(cell):
    if not hasattr(cell, "packed"):
        cell.packed = capi.pack_reads(cell.reads)
    return cell.packed


def _batch(t, cell, form):
    words, offs, lens = _packed(cell)
    if form == RAGGED:
        return t.host_batch(words, offs, lens)
    n = cell.n
    stride = 3 * ((n + 31) // 32)
    assert len(words) == len(cell.reads) * stride
    b = capi.Batch(words.ctypes.data, len(words), None, None, n, stride, len(cell.reads), 0, n)  # no offsets: the uniform path
    b._keep = (words,)
    return b


def _context(mode, ps, flags, sl=150):
    mn, mx, low, high = ps
    return T.TrewHip(mode={E.SHORT: T.MODE_SHORT, E.PAIR: T.MODE_PAIR, E.LONG: T.MODE_LONG}[mode], min_mer=mn, max_mer=mx, low=low,
                     high=high, slice_length=sl, max_batch_reads=4096, max_batch_words=1 << 19, flags=flags)


def _check(t, cell, form, flags):
    """The three assertions for one batch in one configuration."""
    where = "%r, %s batch, flags %d" % (cell, form, flags)
    assert len(cell.pairs) >= 30, where  # never pass on an empty set (test_edges_cpu.py holds the generator to this)
    t.reset_tables()
    t.submit(_batch(t, cell, form), 0)
    t.wait(0)
    wl = [int(x) for x in t.debug_worklist(0)]
    flagged = set(wl)
    assert len(flagged) == len(wl), "a unit is in the worklist twice: " + where
    missing = sorted(cell.passing - flagged)
    assert not missing, "the prefilter dropped %d units the oracle records something for: %s; the first: %s" % (
        len(missing), where, [(i, cell.units[i]) for i in missing[:3]])
    got = t.collect()
    assert got == cell.want, "tables differ from the oracle's: %s: %s" % (where, _table_diff(got, cell.want))
    if cell.ps == E.PARAM_SETS[0] and cell.n2 is None and cell.n in (150, 151) and cell.mode != E.LONG:
        idle = sum(1 for u in flagged if u >= cell.first_random and u not in cell.passing)
        print("selectivity: %s: %d of %d random units flagged and not recorded" % (where, idle, E.N_RANDOM))
        assert idle <= _selectivity_cap(cell.mode, cell.n), where


@pytest.mark.parametrize("config", CONFIGS, ids=_ids)
@pytest.mark.parametrize("ps", E.PARAM_SETS, ids=_ids)
def test_short_edges(short_cells, ps, config):
    form, flags = config
    with _context(E.SHORT, ps, flags) as t:
        for n in E.LENGTHS:
            _check(t, short_cells[(ps, n, None, 150)], form, flags)


@pytest.mark.parametrize("config", CONFIGS, ids=_ids)
@pytest.mark.parametrize("ps", E.PARAM_SETS, ids=_ids)
def test_pair_edges(pair_cells, ps, config):
    form, flags = config
    with _context(E.PAIR, ps, flags) as t:
        for n in E.LENGTHS:
            _check(t, pair_cells[(ps, n, None, 150)], form, flags)
        if form == RAGGED:  # mates of unequal length exist only with offsets and lengths
            for n, n2 in E.UNEQUAL_MATES:
                _check(t, pair_cells[(ps, n, n2, 150)], form, flags)


@pytest.mark.parametrize("config", LONG_CONFIGS, ids=_ids)
@pytest.mark.parametrize("ps_sl", [(ps, sl) for ps in E.LONG_PARAM_SETS for sl in E.slice_lengths(ps)],
                         ids=lambda v: "%s-slice%d" % (_ids(v[0]), v[1]))
def test_long_edges(long_cells, ps_sl, config):
    """Long reads: the repeat fills the first or the last slice, the only ones the prefilter looks at."""
    (ps, sl), (form, flags) = ps_sl, config
    with _context(E.LONG, ps, flags, sl) as t:
        for n in E.long_lengths(sl):
            _check(t, long_cells[(ps, n, None, sl)], form, flags)


def _check_masks(t, cell, form, slots):
    """Every k of every segment of every edge unit whose exact MAX / COUNT reaches LOW is a candidate."""
    if not hasattr(cell, "stats"):
        cell.stats = [E.segment_stats(cell.mode, cell.ps, u) for u in cell.units[:cell.first_random]]
    cand = t.filter_masks(_batch(t, cell, form), slots)
    low = cell.ps[2]
    n_pass, bad = 0, []
    for i, st in enumerate(cell.stats):
        for (slot, k), (cnt, mx) in st.items():
            if cnt and mx / cnt >= low:
                n_pass += 1
                if not (int(cand[i, slot]) >> (k - 1)) & 1:
                    bad.append((i, slot, k, cnt, mx, cell.units[i]))
    assert not bad, "%d passing (segment, k) are no candidates: %r, %s batch: %s" % (len(bad), cell, form, bad[:3])
    assert n_pass >= len(cell.pairs), (cell, n_pass)  # every last-passing unit has a passing (segment, k)


@pytest.mark.parametrize("ps", E.PARAM_SETS, ids=_ids)
def test_short_edge_masks(short_cells, ps):
    """test_uniform_fast_path_is_sound at the edge reads of every parameter set, on uniform and ragged batches."""
    with _context(E.SHORT, ps, 0) as t:
        for n in E.LENGTHS:
            for form in (UNIFORM, RAGGED):
                _check_masks(t, short_cells[(ps, n, None, 150)], form, 3)


@pytest.mark.parametrize("ps", E.PARAM_SETS, ids=_ids)
def test_pair_edge_masks(pair_cells, ps):
    """The same in pair mode: six segments per pair."""
    with _context(E.PAIR, ps, 0) as t:
        for n in E.LENGTHS:
            for form in (UNIFORM, RAGGED):
                _check_masks(t, pair_cells[(ps, n, None, 150)], form, 6)
        for n, n2 in E.UNEQUAL_MATES:
            _check_masks(t, pair_cells[(ps, n, n2, 150)], RAGGED, 6)
