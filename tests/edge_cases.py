"""Reads on the pass/fail edge of k_mer_check, found with the oracle alone (plain Python, no GPU).

A chain starts from a unit the oracle records something for -- a periodic read of a random motif -- and substitutes one base
at a time, at positions in a seeded random order, until the oracle records nothing.  The last passing unit and the first
failing one differ in a single base: somewhere MAX / COUNT sits on a threshold, which is the only place a wrong rounding of
LOW * COUNT, a `>` written for `>=` or an off-by-one in a threshold row can show.

A unit is a tuple of reads (bytes): (read,) in short and long mode, (mate 1, mate 2) in pair mode.  A cell is one
(mode, parameter set, length) -- in long mode (mode, parameter set, slice length, read length)."""
import random

import oracle as O
from helpers import periodic

SHORT, PAIR, LONG = "short", "pair", "long"

# (MIN_MER, MAX_MER, LOW, HIGH): the defaults, a small k range, a low and a non-dyadic baseline (2/3 has no exact float or
# double), 128-bit words, LOW = 1 (one wrong base decides), and a baseline next to 1/2 that no binary format holds
PARAM_SETS = [(5, 32, 0.5, 0.8), (3, 12, 0.5, 0.8), (5, 32, 0.3, 0.6), (5, 32, 2 / 3, 0.9), (5, 64, 0.5, 0.8), (5, 32, 1.0, 1.0),
              (5, 32, 0.51, 0.8)]
LONG_PARAM_SETS = PARAM_SETS[:6]  # 0.51 only where the prefilter has threshold tables of its own: long mode has no uniform path
# 150: equal halves (the joint loop); 151: the joint threshold row of odd lengths; 100: a whole-read segment exists;
# 64: the smallest length; 126 and 190: the 5-word kernel
LENGTHS = [150, 151, 100, 64, 126, 190]
UNEQUAL_MATES = [(150, 100), (101, 151)]  # pair mode, ragged batches only
N_RANDOM = 1000


def params(ps, slice_len=150):
    mn, mx, low, high = ps
    return O.OracleParams(min_mer=mn, max_mer=mx, low=low, high=high, slice_len=slice_len)


def budget(mode, ps):
    """(chains at most, edge pairs wanted) of a cell.  Every cell has to keep at least 30 pairs; chains stop once 32 are
    kept, and 200 chains are enough where the yield is lowest (a low baseline survives many substitutions, so that more
    chains run out of positions before they fail).  The short cells at LOW = 1/2 also have to hold 10 exact ties
    2 MAX == COUNT, which about one pair in five has: they run all their chains, more of them with 128-bit words."""
    if mode == SHORT and ps[2] == 0.5:
        return (200 if ps[1] > 32 else 120), None
    return 200, 32


def slice_lengths(ps):
    """Slice lengths of long mode legal for the parameter set (SLICE_LENGTH >= 2 MAX_MER)."""
    out = []
    for sl in (150, 100, 2 * ps[1] + 7):
        if sl >= 2 * ps[1] and sl not in out:
            out.append(sl)
    return out


def long_lengths(sl):
    out = []
    for n in (sl, sl + 1, 2 * sl - 1, 2 * sl, 3 * sl + 7, 1000):
        if n not in out:
            out.append(n)
    return out


def records(mode, p, unit):
    """True when the oracle records anything for this one unit."""
    if mode == SHORT:
        t = O.run_short(p, [unit[0]])
    elif mode == PAIR:
        t = O.run_pair(p, [unit[0]], [unit[1]])
    else:
        t = O.run_long(p, [unit[0]])
    return any(len(tb) for tb in t.values())


def run(mode, p, units):
    """The oracle's tables of a list of units."""
    if mode == SHORT:
        return O.run_short(p, [u[0] for u in units])
    if mode == PAIR:
        return O.run_pair(p, [u[0] for u in units], [u[1] for u in units])
    return O.run_long(p, [u[0] for u in units])


def segments(mode, n1, n2, mn, mx):
    """(slot, mate, start, length, kmin, kmax) of every segment buffer_task (kmer.cpp:115-171) or buffer_task_pair
    (kmer.cpp:333-340, 467-480) may hand to k_mer_check, in the slot order of trew_hip_filter_masks.  This mirrors get_segment
    (trew_amd/csrc/trew_common.hpp) for short and pair mode: a change to the geometry there is made here as well
    (test_segments_follow_the_drivers_geometry pins it by hand values)."""
    n = n1 if mode == SHORT else min(n1, n2)
    out = []
    if 2 * mn > n:
        return out
    if 4 * mn <= n:
        kr = (mn, min(n // 4, mx))
        out.append((0, 0, 0, n1 // 2) + kr)
        out.append((1, 0, n1 - (n1 + 1) // 2, (n1 + 1) // 2) + kr)
        if mode == PAIR:
            out.append((2, 1, n2 - (n2 + 1) // 2, (n2 + 1) // 2) + kr)
            out.append((3, 1, 0, n2 // 2) + kr)
    if 4 * mx > n:
        kr = (max(n // 4 + 1, mn), min(n // 2, mx))
        if kr[0] <= kr[1]:
            if mode == SHORT:
                out.append((2, 0, 0, n1) + kr)
            else:
                out.append((4, 0, 0, n1) + kr)
                out.append((5, 1, 0, n2) + kr)
    return out


def segment_stats(mode, ps, unit):
    """{(slot, k): (COUNT, MAX)} over every segment of a short or pair unit, from the oracle's class counts."""
    mn, mx = ps[0], ps[1]
    out = {}
    for slot, mate, start, ln, kmin, kmax in segments(mode, len(unit[0]), len(unit[-1]), mn, mx):
        for k, (cnt, m, _) in O.segment_stats(params(ps), unit[mate][start:start + ln], kmin, kmax).items():
            out[(slot, k)] = (cnt, m)
    return out


def _acgt(rnd, n):
    return "".join(rnd.choices("ACGT", k=n))


def _start(rnd, mode, ps, n, n2, sl):
    """A periodic starting unit and the positions of its mutable read that the chain may substitute."""
    mx = ps[1]
    if mode == LONG:
        snum = n // sl
        mid, bonus = (snum + 1) // 2, n % sl
        first = rnd.random() < 0.5
        ln = sl + (bonus if (1 if first else snum) == mid else 0)  # the first / last slice of buffer_task_long (kmer.cpp:790-798)
        a = 0 if first else n - ln
        unit_len = rnd.randint(1, min(mx, ln // 2))
        rep = periodic(_acgt(rnd, unit_len), ln, rnd.randrange(unit_len))
        body = _acgt(rnd, n)
        return (body[:a] + rep + body[a + ln:],), list(range(a, a + ln))
    unit_len = rnd.randint(1, min(mx, n // 2))
    motif = _acgt(rnd, unit_len)
    phase = rnd.randrange(unit_len)
    if rnd.random() < 1 / 3:  # the repeat fills one half, the rest is random
        h = n // 2
        if rnd.random() < 0.5:
            read = periodic(motif, h, phase) + _acgt(rnd, n - h)
        else:
            read = _acgt(rnd, n - h) + periodic(motif, h, phase)
    else:
        read = periodic(motif, n, phase)
    pos = list(range(n))
    if mode == PAIR:
        return (read, _acgt(rnd, n2)), pos
    return (read,), pos


def chain(rnd, mode, ps, n, n2=None, sl=150):
    """One chain: (last passing unit, first failing unit), or None when the start records nothing or no substitution fails."""
    p = params(ps, sl)
    start, pos = _start(rnd, mode, ps, n, n if n2 is None else n2, sl)
    unit = tuple(r.encode() for r in start)
    if not records(mode, p, unit):
        return None
    rnd.shuffle(pos)
    for i in pos:
        read = unit[0]
        other = rnd.choice([c for c in b"ACGTN" if c != read[i]])
        nxt = (read[:i] + bytes([other]) + read[i + 1:],) + unit[1:]
        if not records(mode, p, nxt):
            return unit, nxt
        unit = nxt
    return None


def edge_pairs(mode, ps, n, n2=None, sl=150, seed=0):
    """The edge pairs of one cell: deterministic for (cell, seed)."""
    rnd = random.Random("edge|%s|%r|%d|%r|%d|%d" % (mode, ps, n, n2, sl, seed))
    chains, want = budget(mode, ps)
    out = []
    for _ in range(chains):
        pr = chain(rnd, mode, ps, n, n2, sl)
        if pr is not None:
            out.append(pr)
            if want is not None and len(out) >= want:
                break
    return out


def random_units(mode, n, n2=None, count=N_RANDOM, seed=0):
    rnd = random.Random("random|%s|%d|%r|%d" % (mode, n, n2, seed))
    if mode == PAIR:
        return [(_acgt(rnd, n).encode(), _acgt(rnd, n if n2 is None else n2).encode()) for _ in range(count)]
    return [(_acgt(rnd, n).encode(),) for _ in range(count)]


def recording(mode, p, units, base=0, tables=None):
    """Indices (from `base`) of the units the oracle records something for: tables add up over units, so a stretch whose
    tables (`tables`, when the caller has them) are empty holds none, and random reads almost never do."""
    if tables is None:
        tables = run(mode, p, units) if units else {}
    if not any(len(tb) for tb in tables.values()):
        return set()
    if len(units) == 1:
        return {base}
    h = len(units) // 2
    return recording(mode, p, units[:h], base) | recording(mode, p, units[h:], base + h)


def add_tables(a, b):
    out = {name: dict(tb) for name, tb in a.items()}
    for name, tb in b.items():
        for key, c in tb.items():
            out[name][key] = out[name].get(key, 0) + c
    return out


class Cell:
    """The batch of one cell: every last-passing unit, every first-failing unit, N_RANDOM random units; the indices of the
    units the oracle records something for, and the oracle's tables of the whole batch."""

    def __init__(self, mode, ps, n, n2=None, sl=150, batch=True):
        self.mode, self.ps, self.n, self.n2, self.sl = mode, ps, n, n2, sl
        self.p = params(ps, sl)
        self.pairs = edge_pairs(mode, ps, n, n2, sl)
        if batch:
            self.fill_batch()

    def fill_batch(self):
        mode, n, n2 = self.mode, self.n, self.n2
        k = len(self.pairs)
        rand = random_units(mode, n, n2)
        self.units = [a for a, _ in self.pairs] + [b for _, b in self.pairs] + rand
        self.first_random = 2 * k
        of_random = run(mode, self.p, rand)
        self.passing = set(range(k)) | recording(mode, self.p, rand, 2 * k, of_random)
        self.want = add_tables(run(mode, self.p, self.units[:2 * k]), of_random)
        self.reads = [r for u in self.units for r in u]

    def __repr__(self):
        return "%s %r n=%d%s%s" % (self.mode, self.ps, self.n, "" if self.n2 is None else "/%d" % self.n2,
                                   " slice %d" % self.sl if self.mode == LONG else "")


def cell_keys(mode):
    """(ps, n, n2, sl) of every cell of a mode."""
    out = []
    for ps in (LONG_PARAM_SETS if mode == LONG else PARAM_SETS):
        if mode == LONG:
            out += [(ps, n, None, sl) for sl in slice_lengths(ps) for n in long_lengths(sl)]
        else:
            out += [(ps, n, None, 150) for n in LENGTHS]
            if mode == PAIR:
                out += [(ps, n, n2, 150) for n, n2 in UNEQUAL_MATES]
    return out


class Cells(dict):
    """{(ps, n, n2, sl): Cell} of a mode.  A cell is built when it is first asked for, so that a test pays for its own cells only."""

    def __init__(self, mode, batch=True):
        super().__init__()
        self.mode, self.batch, self.legal = mode, batch, set(cell_keys(mode))

    def __missing__(self, key):
        assert key in self.legal, key
        cell = self[key] = Cell(self.mode, key[0], key[1], key[2], key[3], self.batch)
        return cell


def build_cells(mode, batch=True):
    return Cells(mode, batch)


def exact_ties(mode, ps, units):
    """The short or pair units some (segment, k) of which has exactly 2 MAX == COUNT."""
    return [u for u in units if any(c and 2 * m == c for c, m in segment_stats(mode, ps, u).values())]


def held_by_the_smallest_count(mode, ps, units):
    """The short or pair units every (segment, k) of which that reaches LOW does so with the smallest MAX that can:
    (MAX - 1) / COUNT < LOW <= MAX / COUNT.  A threshold one count too high leaves such a unit no (segment, k) at all."""
    low, out = ps[2], []
    for u in units:
        reach = [(c, m) for c, m in segment_stats(mode, ps, u).values() if c and m / c >= low]
        if reach and all((m - 1) / c < low for c, m in reach):
            out.append(u)
    return out


def held_by_a_tie(mode, ps, units):
    """Those of them where each such (segment, k) sits exactly on LOW = 1/2: 2 MAX == COUNT, where `>` for `>=` decides, too."""
    out = []
    for u in units:
        reach = [(c, m) for c, m in segment_stats(mode, ps, u).values() if c and m / c >= ps[2]]
        if reach and all(2 * m == c for c, m in reach):
            out.append(u)
    return out


def decided_by_one_base(mode, ps, pairs):
    """The short or pair edge pairs whose passing twin has a (segment, k) with MAX == COUNT that the failing twin's one base breaks."""
    out = []
    for a, b in pairs:
        sa, sb = segment_stats(mode, ps, a), segment_stats(mode, ps, b)
        if any(c and m == c and sb[key][1] < sb[key][0] for key, (c, m) in sa.items()):
            out.append((a, b))
    return out
