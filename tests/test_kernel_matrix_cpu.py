"""The kernel-variant matrix (kernel_matrix.py) on the CPU: every cell sits on the edge of the class it is meant for, and is
worth running -- conditions on what the oracle records, not measurements.  The GPU side is test_gpu_kernel_matrix.py."""
import os
import subprocess

import pytest

import kernel_matrix as M
import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECS = M.cell_specs()


def _id(spec):
    return "%s-nw%d-%s-%d" % spec


def test_the_matrix_is_complete():
    """All 32 combinations of mode x class x width, both edges of each (class 3: the small cell and 95), 64 cells."""
    assert {s[:3] for s in SPECS} == {(m, c, w) for m in M.MODES for c in M.CLASSES for w in M.WIDTHS}
    assert len(SPECS) == len(set(SPECS)) == 64
    for mode, cls, width in {s[:3] for s in SPECS}:
        edges = [s[3] for s in SPECS if s[:3] == (mode, cls, width)]
        assert len(edges) == 2 and all(M.class_of(e) == cls for e in edges)
        limits = dict(M.CLASS_LIMITS)
        if cls:
            assert max(edges) == limits[cls]
        if cls != 3:
            assert min(edges) == {5: 96, 10: 160, 0: 320}[cls]
    # the accepted SLICE_LENGTH range (200, 512]: 319, 320 and 512 with narrow and with wide words
    for width in M.WIDTHS:
        assert {319, 320, 512} <= {s[3] for s in SPECS if s[0] == M.LONG and s[2] == width}
    assert M.class_of(95) == 3 and M.class_of(96) == 5 and M.class_of(159) == 5 and M.class_of(160) == 10
    assert M.class_of(319) == 10 and M.class_of(320) == 0 and M.class_of(M.MAX_SEGMENT) == 0


def test_lengths_come_from_the_geometry():
    """The examples of the geometry: halves n / 2 and (n + 1) / 2, the whole read below 4 MAX_MER."""
    assert M.unit_lengths(M.SHORT, M.NARROW, 159) == [(317,), (318,)]
    assert M.unit_lengths(M.SHORT, M.NARROW, 160) == [(319,), (320,)]
    assert M.unit_lengths(M.SHORT, M.NARROW, 96) == [(96,), (191,), (192,)]
    assert M.longest_segment(M.SHORT, M.NARROW, (127,)) == 127 and M.longest_segment(M.SHORT, M.NARROW, (128,)) == 64
    assert M.unit_lengths(M.SHORT, M.WIDE, 96) == [(96,)]  # a 191-base read has a whole-read segment up to 255 bases
    assert M.longest_segment(M.SHORT, M.WIDE, (255,)) == 255 and M.longest_segment(M.SHORT, M.WIDE, (256,)) == 128
    assert M.unit_lengths(M.SHORT, M.WIDE, 500) == [(999,), (1000,)]
    assert (318, 212) in M.unit_lengths(M.PAIR, M.NARROW, 159) and (63, 95) in M.unit_lengths(M.PAIR, M.NARROW, 95)
    assert M.longest_segment(M.LONG, M.NARROW, (5 * 512 - 1,), 512) == 1023 == M.MAX_SEGMENT
    assert [s[2] for s in M.segments(M.LONG, M.NARROW, (3 * 150 + 7,), 150)] == [150, 157, 150]


def test_generator_is_deterministic():
    for spec in (SPECS[0], SPECS[21], SPECS[-1]):
        a, b = M.cell(*spec), M.Cell(*spec, SPECS.index(spec))
        assert a.units == b.units and a.kinds == b.kinds and a.uniform == b.uniform


@pytest.mark.parametrize("spec", SPECS, ids=_id)
def test_cell_sits_on_its_edge(spec):
    mode, cls, width, edge = spec
    c = M.cell(*spec)
    assert (c.ps[1] > 32) == (width == M.WIDE_W)
    if mode == M.LONG:
        assert c.sl == edge and M.class_of(c.sl) == cls and 2 * c.ps[1] <= c.sl <= M.MAX_SLICE
        assert min(len(u[0]) for u in c.units) == c.sl  # no read the reader would drop
        # every slice but the middle one has SLICE_LENGTH bases; the longest middle slice is at the limit
        assert c.longest() == 2 * c.sl - 1
        assert all(s[2] == c.sl or s[2] <= 2 * c.sl - 1 for i in range(len(c.units)) for s in M.segments(mode, c.ps, c.unit_lens(i), c.sl))
    else:
        assert c.longest() == edge and M.class_of(c.longest()) == cls
        lens = {c.unit_lens(i) for i in range(len(c.units))}
        assert any(M.longest_segment(mode, c.ps, ln) < edge for ln in lens)  # shorter reads beside the edge-length ones
        if mode == M.PAIR:
            assert any(a > b for a, b in lens if M.longest_segment(mode, c.ps, (a, b)) == edge)  # unequal mates, the longer one
            assert any(a < b for a, b in lens if M.longest_segment(mode, c.ps, (a, b)) == edge)  # sets the class, either way round
    if mode in (M.SHORT, M.PAIR):
        assert c.uniform
        for n, units in c.uniform.items():
            assert all(len(r) == n for u in units for r in u)
            assert M.longest_segment(mode, c.ps, (n,) * len(units[0])) == edge
    else:
        assert not c.uniform
    assert 200 <= len(c.units) <= 300
    for kind in M.KINDS:
        assert sum(1 for i, k in enumerate(c.kinds) if k == kind and c.is_edge_unit(i)) >= (1 if mode == M.LONG else 3), kind


@pytest.mark.parametrize("spec", SPECS, ids=_id)
def test_cell_is_not_trivial(spec):
    mode, cls, width, edge = spec
    c = M.cell(*spec)
    per_unit = [c.tables([u]) for u in c.units]
    # the tables are sums over the units (nothing in a batch depends on its neighbours): the oracle runs once per unit here, and
    # once more on the whole batch where that is cheap
    want = {n: {} for n in O.TABLE_NAMES}
    for t in per_unit:
        for n in O.TABLE_NAMES:
            for key, cnt in t[n].items():
                want[n][key] = want[n].get(key, 0) + cnt
    if cls in (3, 5):
        assert want == c.want
    high = [n for n in O.TABLE_NAMES if n.endswith("high") and want[n]]
    low = [n for n in O.TABLE_NAMES if n.endswith("low") and want[n]]
    assert high and low, (high, low)
    records = [any(t[n] for n in O.TABLE_NAMES) for t in per_unit]
    assert sum(records) >= 20 and len(records) - sum(records) >= 20, sum(records)
    assert sum(1 for i, r in enumerate(records) if r and c.is_edge_unit(i)) >= 10
    if width == M.WIDE_W:
        assert any(k > 32 for n in O.TABLE_NAMES for (k, _) in want[n])
        assert any(k <= 32 for n in O.TABLE_NAMES for (k, _) in want[n])
    if mode == M.LONG and cls != 3:
        for side in ("both", "forward", "backward"):
            assert any(t[side + "_high"] or t[side + "_low"] for t in per_unit), side
    if mode in (M.SHORT, M.PAIR):
        assert all(want[n] for n in O.TABLE_NAMES), [n for n in O.TABLE_NAMES if not want[n]]
        for n in c.uniform:
            assert sum(len(v) for v in c.want_uniform(n).values()) > 0


def test_slice_length_limit_needs_no_device():
    """trew_hip_init refuses SLICE_LENGTH = 513 before it looks for a device (512 passes that check: with no device the failure
    is the missing device; on a GPU the context opens, test_gpu_kernel_matrix.py)."""
    import trew_amd as T

    with pytest.raises(T.TrewHipError, match="SLICE_LENGTH must be at most 512 on the HIP path."):
        T.TrewHip(mode=T.MODE_LONG, slice_length=513)
    try:
        T.TrewHip(mode=T.MODE_LONG, slice_length=512).close()
    except T.TrewHipError as e:
        assert "SLICE_LENGTH" not in str(e)
