"""The edge-read generator of edge_cases.py, held to its floors on the oracle alone: test_gpu_prefilter_edges.py must never
pass on an empty or a harmless set."""
import random

import pytest

import edge_cases as E

MODES = [E.SHORT, E.PAIR, E.LONG]


@pytest.fixture(scope="module")
def cells():
    """Every cell the GPU tests use (edge pairs only), each built when a test first asks for it."""
    return {mode: E.build_cells(mode, batch=False) for mode in MODES}


def _one_base_apart(a, b):
    return len(a) == len(b) and sum(x != y for x, y in zip(a, b)) == 1


@pytest.mark.parametrize("mode", MODES)
def test_generator_is_deterministic(mode, cells):
    ps, n, n2, sl = E.cell_keys(mode)[-1]  # a cell of LOW = 0.51 (short, pair) or LOW = 1 (long): quick ones
    again = E.edge_pairs(mode, ps, n, n2, sl)
    assert again == cells[mode][(ps, n, n2, sl)].pairs
    assert E.edge_pairs(mode, ps, n, n2, sl, seed=1) != again
    assert E.random_units(mode, n, n2, count=20) == E.random_units(mode, n, n2, count=20)


@pytest.mark.parametrize("mode", MODES)
def test_every_pair_flips_the_verdict_with_one_base(mode, cells):
    for key in E.cell_keys(mode):
        cell = cells[mode][key]
        for a, b in cell.pairs:
            assert _one_base_apart(a[0], b[0]) and a[1:] == b[1:], (cell, a, b)
            assert E.records(mode, cell.p, a) and not E.records(mode, cell.p, b), (cell, a, b)
            assert len(a[0]) == cell.n and (mode != E.PAIR or len(a[1]) == (cell.n if cell.n2 is None else cell.n2))


@pytest.mark.parametrize("mode", MODES)
def test_every_cell_yields_30_edge_pairs(mode, cells):
    every = [cells[mode][key] for key in E.cell_keys(mode)]
    short = {repr(cell): len(cell.pairs) for cell in every if len(cell.pairs) < 30}
    assert not short, short
    assert len(every) >= 42


def test_half_baseline_cells_hold_exact_ties(cells):
    """LOW = 1/2 in short mode: at least 10 edge reads per cell have a (segment, k) with exactly 2 MAX == COUNT, where `>` for
    `>=` and a threshold one too high both change the verdict."""
    seen = 0
    for ps, n, n2, sl in E.cell_keys(E.SHORT):
        if ps[2] == 0.5:
            cell = cells[E.SHORT][(ps, n, n2, sl)]
            ties = E.exact_ties(E.SHORT, ps, [u for pr in cell.pairs for u in pr])
            assert len(ties) >= 10, (cell, len(ties))
            seen += 1
    assert seen == 3 * len(E.LENGTHS)


@pytest.mark.parametrize("mode", [E.SHORT, E.PAIR])
def test_cells_hold_units_a_threshold_one_too_high_would_drop(mode, cells):
    """The exact ties above count any (segment, k); what a prefilter threshold one count too high (or `>` for `>=`) loses is a
    last-passing unit ALL of whose passing (segment, k) pass with the smallest count that can (or all sit exactly on LOW = 1/2).
    Every cell holds such a unit, every (mode, parameter set) at least 20 of them over its lengths, and at LOW = 1/2 at
    least 5 held by ties alone."""
    by_ps = {}
    for ps, n, n2, sl in E.cell_keys(mode):
        cell = cells[mode][(ps, n, n2, sl)]
        last = [a for a, _ in cell.pairs]
        held = E.held_by_the_smallest_count(mode, ps, last)
        assert len(held) >= 1, cell
        tot = by_ps.setdefault(ps, [0, 0])
        tot[0] += len(held)
        tot[1] += len(E.held_by_a_tie(mode, ps, last)) if ps[2] == 0.5 else 0
    assert len(by_ps) == len(E.PARAM_SETS)
    for ps, (held, ties) in by_ps.items():
        assert held >= 20, (mode, ps, held)
        assert ps[2] != 0.5 or ties >= 5, (mode, ps, ties)


@pytest.mark.parametrize("mode", [E.SHORT, E.PAIR])
def test_unit_baseline_cells_are_decided_by_one_base(mode, cells):
    """LOW = 1: the passing twin has a (segment, k) all of whose windows fall into one class, and the one substituted base of
    the failing twin is what breaks it."""
    seen = 0
    for ps, n, n2, sl in E.cell_keys(mode):
        if ps[2] == 1.0:
            cell = cells[mode][(ps, n, n2, sl)]
            assert len(E.decided_by_one_base(mode, ps, cell.pairs)) >= 10, cell
            seen += 1
    assert seen >= len(E.LENGTHS)


def test_segments_follow_the_drivers_geometry():
    """The (slot, k range) table the mask checks go by, at the lengths where it changes shape."""
    assert E.segments(E.SHORT, 150, 150, 5, 32) == [(0, 0, 0, 75, 5, 32), (1, 0, 75, 75, 5, 32)]
    assert E.segments(E.SHORT, 151, 151, 5, 32) == [(0, 0, 0, 75, 5, 32), (1, 0, 75, 76, 5, 32)]
    assert E.segments(E.SHORT, 100, 100, 5, 32) == [(0, 0, 0, 50, 5, 25), (1, 0, 50, 50, 5, 25), (2, 0, 0, 100, 26, 32)]
    assert E.segments(E.SHORT, 64, 64, 3, 12) == [(0, 0, 0, 32, 3, 12), (1, 0, 32, 32, 3, 12)]
    assert E.segments(E.PAIR, 150, 100, 5, 32) == [(0, 0, 0, 75, 5, 25), (1, 0, 75, 75, 5, 25), (2, 1, 50, 50, 5, 25),
                                                   (3, 1, 0, 50, 5, 25), (4, 0, 0, 150, 26, 32), (5, 1, 0, 100, 26, 32)]


def test_recording_finds_the_units_that_record():
    rnd = random.Random(3)
    units = [(E._acgt(rnd, 150).encode(),) for _ in range(40)]
    units[7] = (b"TTAGGG" * 25,)
    units[31] = (b"ACGTC" * 30,)
    p = E.params(E.PARAM_SETS[0])
    assert E.recording(E.SHORT, p, units, 100) == {100 + i for i, u in enumerate(units) if E.records(E.SHORT, p, u)} == {107, 131}
