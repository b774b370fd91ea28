"""The kernel-variant matrix: one cell per (mode, mask-word class, word width, edge) -- shared generator, no test of its own.

The host picks the compiled kernel of a batch from the longest segment the batch stages: pick_nw() in
trew_amd/csrc/trew_kernels.hip maps it to 3 / 5 / 10 / 32 mask words for launch_filter, and launch_exact takes
exact_kernel<NW, MODE, WT> with NW in {3, 5, 10, 0} (0: no lane bounds) and WT = u64 or u128 (MAX_MER > 32).  In long mode
launch_exact goes by SLICE_LENGTH alone (bound_len); the middle slice, which carries the remainder and has up to
2 SLICE_LENGTH - 1 bases, is always decided by decide<0>.  A batch built here has its longest segment exactly on the smallest
or the largest value of its class, next to shorter reads, so every variant is compared with the oracle at both of its edges.

The lengths are not guessed: unit_lengths() searches the oracle's geometry (segments(), a restatement of
oracle/trew_oracle.c: halves n/2 and (n+1)/2, the whole read below 4 MAX_MER, slices with the remainder in the middle one) for
the read lengths whose longest segment is the edge.

All 32 combinations of mode x class x width exist.  Two need other parameters than (5, 32) / (5, 64), none is left out:
  * long mode, class 3, wide words: SLICE_LENGTH >= 2 MAX_MER must stay <= 95, so MAX_MER = 40 (still 128-bit words); the
    same holds for SLICE_LENGTH = 96, the small edge of class 5;
  * the small cell of class 3 ("near 4 MIN_MER") with wide words: a row with k > 32 needs a segment of 66 bases, so the wide
    small cells run at (17, 64) with a longest segment of 70 bases.  In long mode the smallest legal slice, 2 MAX_MER, is the
    small cell (64 bases narrow, 80 at MAX_MER = 40).
"""
import random

import oracle as O
from helpers import mutate, periodic

SEGMENT, SHORT, PAIR, LONG = "segment", "short", "pair", "long"
MODES = (SEGMENT, SHORT, PAIR, LONG)
NARROW_W, WIDE_W = "narrow", "wide"
WIDTHS = (NARROW_W, WIDE_W)
CLASSES = (3, 5, 10, 0)

# pick_nw() (trew_kernels.hip): a longest segment of <= 95 / <= 159 / <= 319 bases runs the 3- / 5- / 10-word kernels, anything
# longer filter_kernel<32> and exact_kernel<0>.  launch_exact: in long mode the class comes from SLICE_LENGTH (bound_len), not
# from the middle slice.  A change of those limits belongs here too.
CLASS_LIMITS = ((3, 95), (5, 159), (10, 319))
MAX_SEGMENT = 1023  # kMaxSegBases
MAX_SHORT_READ = 1000  # short and pair mode refuse longer reads
MAX_SLICE = 512  # "SLICE_LENGTH must be at most 512 on the HIP path.": 2 * 512 - 1 = MAX_SEGMENT

LOW, HIGH = 0.5, 0.8
NARROW, WIDE, WIDE40, WIDE_SMALL = (5, 32), (5, 64), (5, 40), (17, 64)
SMALL_NARROW, SMALL_WIDE = 23, 70  # class 3's small cell: just above 4 MIN_MER = 20 / 68

N_UNITS = 240  # units of a ragged batch: 60 % of an edge length, 40 % shorter
N_UNIFORM = 96  # units of a uniform batch (short and pair mode), per edge length
N_LONG = 210  # reads of a long cell


def class_of(longest):
    for cls, limit in CLASS_LIMITS:
        if longest <= limit:
            return cls
    return 0


def class_edges(mode, cls, width):
    """The smallest and the largest longest-segment (long mode: SLICE_LENGTH) of a class, class 3 with its small cell."""
    if cls == 3:
        if mode == LONG:
            return (2 * (NARROW if width == NARROW_W else WIDE40)[1], 95)
        return (SMALL_NARROW if width == NARROW_W else SMALL_WIDE, 95)
    if cls == 5:
        return (96, 159)
    if cls == 10:
        return (160, 319)
    return (320, {SEGMENT: MAX_SEGMENT, SHORT: MAX_SHORT_READ // 2, PAIR: MAX_SHORT_READ // 2, LONG: MAX_SLICE}[mode])


def cell_params(mode, width, edge):
    if width == NARROW_W:
        return NARROW
    if mode == LONG:
        return WIDE if edge >= 2 * WIDE[1] else WIDE40
    return WIDE_SMALL if edge == SMALL_WIDE else WIDE


# ------------------------------------------------------------------ the oracle's geometry
def segments(mode, ps, lens, sl=None):
    """Every segment the oracle may check of one unit: (mate, start, length, kmin, kmax).  lens: the unit's read lengths."""
    mn, mx = ps
    out = []
    if mode == SEGMENT:
        if lens[0] > 0:
            out.append((0, 0, lens[0], mn, mx))
    elif mode in (SHORT, PAIR):
        n = min(lens)
        if 2 * mn <= n:
            for mate, a in enumerate(lens):
                if 4 * mn <= n:
                    out.append((mate, 0, a // 2, mn, min(n // 4, mx)))
                    out.append((mate, a - (a + 1) // 2, (a + 1) // 2, mn, min(n // 4, mx)))
                if 4 * mx > n and max(n // 4 + 1, mn) <= min(n // 2, mx):
                    out.append((mate, 0, a, max(n // 4 + 1, mn), min(n // 2, mx)))
    else:
        n = lens[0]
        snum, bonus = n // sl, n % sl
        mid = (snum + 1) // 2
        pos = 0
        for t in range(1, snum + 1):
            ln = sl + (bonus if t == mid else 0)
            out.append((0, pos, ln, mn, mx))
            pos += ln
    return out


def longest_segment(mode, ps, lens, sl=None):
    return max((s[2] for s in segments(mode, ps, lens, sl)), default=0)


def unit_lengths(mode, ps, edge):
    """Read lengths (a tuple per unit: one read, or two mates) whose longest segment has exactly `edge` bases."""
    if mode == SEGMENT:
        return [(edge,)]
    single = [n for n in range(1, MAX_SHORT_READ + 1) if longest_segment(SHORT, ps, (n,)) == edge]
    if mode == SHORT:
        return [(n,) for n in single]
    out = [(n, n) for n in single]
    for n in single:  # unequal mates: the longer one sets the class
        m = next(m for m in range(2 * n // 3, n) if longest_segment(PAIR, ps, (n, m)) == edge)
        out += [(n, m), (m, n)]
    return out


def shorter_lengths(mode, ps, edge):
    """Read lengths whose longest segment stays below `edge` (what sits beside the edge-length reads in a ragged batch)."""
    if mode == SEGMENT:
        return [(n,) for n in range(1, edge)]
    return [(n,) if mode == SHORT else (n, n) for n in range(1, MAX_SHORT_READ + 1) if longest_segment(SHORT, ps, (n,)) < edge]


def long_lengths(sl):
    """SL, SL + 1, 2 SL - 1, 2 SL, 3 SL + 7, a middle slice of 2 SL - 1 bases among four slices, and two longer reads for chains
    of several slices in either direction."""
    return [sl, sl + 1, 2 * sl - 1, 2 * sl, 3 * sl + 7, 5 * sl - 1, 7 * sl + 3, 9 * sl + sl // 2]


# ------------------------------------------------------------------ content
KINDS = ("kmin", "kmax", "kmax+1", "sub1", "sub5", "n1", "n_first", "n_last", "junction", "at_only", "homopolymer", "random",
         "random", "phase", "big_unit")
LAYOUTS = ("whole", "whole", "head", "tail", "both_ends")


def _rand(rnd, n, alphabet="ACGT"):
    return "".join(rnd.choice(alphabet) for _ in range(n))


def _unit_k(rnd, kind, kmin, kmax, kbig):
    """Period of the repeat a unit of this kind is made of.  kmin .. kmax: the k range of the unit's halves (or of its only
    segment); kbig: the largest k any of its segments is checked at."""
    if kind == "kmin":
        return kmin
    if kind == "kmax":
        return kmax
    if kind == "kmax+1":
        return kmax + 1
    if kind == "big_unit":  # wide cells: longer than 32; narrow cells: the upper half of the range
        lo = min(33, kbig) if kbig > 32 else max(kmin, (kmin + kbig) // 2)
        return rnd.randint(lo, kbig)
    return rnd.randint(kmin, kmax)


def _repeat(rnd, kind, n, kmin, kmax, kbig):
    """n bases of a unit of the given kind (N at fixed positions is put in afterwards)."""
    if kind == "random":
        return _rand(rnd, n)
    if kind == "at_only":
        return _rand(rnd, n, "AT")
    if kind == "homopolymer":
        return rnd.choice("ACGT") * n
    k = max(1, _unit_k(rnd, kind, kmin, kmax, kbig))
    s = periodic(_rand(rnd, k), n, rnd.randint(0, k - 1) if kind == "phase" else 0)
    if kind == "sub1":
        s = mutate(s, rnd, p_sub=0.01)
    elif kind == "sub5":
        s = mutate(s, rnd, p_sub=0.05)
    elif kind == "n1":
        s = mutate(s, rnd, p_n=0.01)
    elif kind == "junction":
        cut = rnd.choice([n // 2, rnd.randint(0, n)])
        s = s[:cut] + periodic(_rand(rnd, rnd.randint(kmin, kmax)), n - cut)
    return s


_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return s.translate(_COMP)[::-1]


def _k_ranges(mode, ps, lens, sl):
    segs = segments(mode, ps, lens, sl)
    if not segs:
        return ps[0], ps[0], ps[0]
    return segs[0][3], max(segs[0][3], segs[0][4]), max(s[4] for s in segs)


def _poke_n(reads, mode, ps, lens, sl, last):
    """N in the first or the last base of the unit's longest segment (the later one when two are as long)."""
    segs = segments(mode, ps, lens, sl)
    if not segs:
        return reads
    mate, start, ln = max(segs, key=lambda s: (s[2], s[0], s[1]))[:3]
    at = start + (ln - 1 if last else 0)
    r = reads[mate]
    reads = list(reads)
    reads[mate] = r[:at] + "N" + r[at + 1:]
    return reads


def make_unit(rnd, mode, ps, lens, kind, sl=None):
    """One unit (a tuple of bytes: a segment, a read, or two mates) of the given read lengths and kind."""
    kmin, kmax, kbig = _k_ranges(mode, ps, lens, sl)
    if mode == PAIR:
        n1, n2 = lens
        frag = _repeat(rnd, kind, n1 + n2, kmin, kmax, kbig)
        how = rnd.random()
        a, b = frag[:n1], frag[n1:]
        if how < 0.7:  # a fragment read from both ends: the second mate is the reverse complement of its far end
            b = revcomp(b.encode()).decode()
        elif how < 0.85:  # the repeat on one mate only
            b = _rand(rnd, n2)
        reads = [a, b]
    elif mode == LONG:
        n = lens[0]
        layout = rnd.choice(LAYOUTS)
        rep = _repeat(rnd, kind, n, kmin, kmax, kbig)
        t = min(n, rnd.randint(sl // 2, 3 * sl))
        if layout == "whole" or kind == "random":
            body = rep
        elif layout == "head":
            body = rep[:t] + _rand(rnd, n - t)
        elif layout == "tail":
            body = _rand(rnd, n - t) + rep[:t]
        else:
            t = min(t, n // 2)
            body = rep[:t] + _rand(rnd, n - 2 * t) + _repeat(rnd, "kmin", t, kmin, kmax, kbig)
        reads = [body]
    else:
        s = _repeat(rnd, kind, lens[0], kmin, kmax, kbig)
        how = rnd.random()
        if mode == SHORT and how < 0.2:  # the repeat in one half only: forward_* / backward_* rows
            h = lens[0] // 2
            s = s[:h] + _rand(rnd, lens[0] - h) if how < 0.1 else _rand(rnd, h) + s[h:]
        reads = [s]
    if kind in ("n_first", "n_last"):
        reads = _poke_n(reads, mode, ps, lens, sl, kind == "n_last")
    assert tuple(len(r) for r in reads) == tuple(lens)
    return tuple(r.encode() for r in reads)


# ------------------------------------------------------------------ cells
class Cell:
    """mode, cls, width, edge (longest segment; long mode: SLICE_LENGTH), ps = (MIN_MER, MAX_MER), sl; units: the ragged batch,
    kinds[i] the kind of unit i; uniform: {read length: units} (short and pair mode)."""

    def __init__(self, mode, cls, width, edge, index):
        self.mode, self.cls, self.width, self.edge = mode, cls, width, edge
        self.ps = cell_params(mode, width, edge)
        self.sl = edge if mode == LONG else None
        self.seed = 52000 + index
        rnd = random.Random(self.seed)
        self.units, self.kinds, self.uniform = [], [], {}
        if mode == LONG:
            lengths = long_lengths(edge)
            for i in range(N_LONG):
                self._add(rnd, (lengths[i % len(lengths)],), KINDS[i % len(KINDS)])
        else:
            at_edge = unit_lengths(mode, self.ps, edge)
            shorter = shorter_lengths(mode, self.ps, edge)
            for i in range(N_UNITS):
                if i % 5 < 3:
                    lens = at_edge[(i // 5) % len(at_edge)]
                else:  # shorter units, half of them close to the edge
                    lens = rnd.choice(shorter[len(shorter) // 2:] if i % 2 else shorter)
                    if mode == PAIR and rnd.random() < 0.3:  # unequal mates (a short mate can make the long one a whole-read segment)
                        other = (lens[0], rnd.choice(shorter)[0])
                        lens = other if longest_segment(mode, self.ps, other) < edge else lens
                self._add(rnd, lens, KINDS[(i // 5 * 3 + i % 5) % len(KINDS)] if i % 5 < 3 else rnd.choice(KINDS))
            if mode in (SHORT, PAIR):
                for lens in at_edge:
                    if len(set(lens)) == 1:
                        self.uniform[lens[0]] = [make_unit(rnd, mode, self.ps, lens, KINDS[i % len(KINDS)]) for i in range(N_UNIFORM)]

    def _add(self, rnd, lens, kind):
        self.units.append(make_unit(rnd, self.mode, self.ps, lens, kind, self.sl))
        self.kinds.append(kind)

    @property
    def name(self):
        return "%s-nw%d-%s-%d" % (self.mode, self.cls, self.width, self.edge)

    def __repr__(self):
        return "Cell(%s, MIN_MER %d, MAX_MER %d)" % (self.name, self.ps[0], self.ps[1])

    def params(self):
        return O.OracleParams(min_mer=self.ps[0], max_mer=self.ps[1], low=LOW, high=HIGH, slice_len=self.sl or 150)

    def unit_lens(self, i):
        return tuple(len(r) for r in self.units[i])

    def longest(self, units=None):
        """Longest segment over a batch, from the oracle's geometry (long mode: the middle slices included)."""
        return max(longest_segment(self.mode, self.ps, tuple(len(r) for r in u), self.sl) for u in (self.units if units is None else units))

    def is_edge_unit(self, i):
        """The unit has a segment of the edge length (long mode: its middle slice is at the limit, 2 SLICE_LENGTH - 1 bases)."""
        return longest_segment(self.mode, self.ps, self.unit_lens(i), self.sl) == (2 * self.sl - 1 if self.mode == LONG else self.edge)

    def tables(self, units=None):
        """The oracle's tables of a batch of units (segment mode: the two histograms, as forward_high / forward_low)."""
        return oracle_tables(self.mode, self.params(), self.units if units is None else units)

    @property
    def want(self):
        if not hasattr(self, "_want"):
            self._want = self.tables()
        return self._want

    def want_uniform(self, n):
        if not hasattr(self, "_want_uni"):
            self._want_uni = {}
        if n not in self._want_uni:
            self._want_uni[n] = self.tables(self.uniform[n])
        return self._want_uni[n]

    @property
    def segment_results(self):
        """segment mode: the oracle's segment_check of every unit"""
        if not hasattr(self, "_seg"):
            self._seg = [O.segment_check(self.params(), u[0]) for u in self.units]
        return self._seg


def flat(units):
    """The reads of a batch in submission order (pair mode: reads 2 i and 2 i + 1 are mates)."""
    return [r for u in units for r in u]


def oracle_tables(mode, p, units):
    if mode == SHORT:
        return O.run_short(p, flat(units))
    if mode == PAIR:
        return O.run_pair(p, [u[0] for u in units], [u[1] for u in units])
    if mode == LONG:
        return O.run_long(p, flat(units))
    out = {name: {} for name in O.TABLE_NAMES}
    for u in units:
        e = O.segment_check(p, u[0])
        for name, hist in (("forward_high", e["hist_high"]), ("forward_low", e["hist_low"])):
            for key, c in hist.items():
                out[name][key] = out[name].get(key, 0) + c
    return out


def long_walk(p, read, sl):
    """The lengths of the slices buffer_task_long checks of one read, in the order it checks them: the forward chain, then
    the backward chain unless every slice chained (oracle/trew_oracle.c, trew_oracle_add_long; the chains go by k alone)."""
    n = len(read)
    snum, bonus = n // sl, n % sl
    mid = (snum + 1) // 2
    out = []

    def check(t, start):
        ln = sl + (bonus if t == mid else 0)
        if start < 0:
            start += n - ln + 1  # a slice that ends at base n + start
        out.append(ln)
        e = O.segment_check(p, read[start:start + ln])
        return ln, (e["k_high"], e["k_low"])

    si, kmer, rend, pos, t = [1, 1], [0, 0], [False, False], 0, 1
    while t <= snum and not (rend[0] and rend[1]):
        ln, tk = check(t, pos)
        for b in (0, 1):
            if not rend[b] and tk[b] > 0 and (kmer[b] == tk[b] or t == 1):
                si[b], kmer[b] = si[b] + 1, tk[b]
            else:
                rend[b] = True
        pos, t = pos + ln, t + 1
    if si[0] <= snum or si[1] <= snum:
        sj, kmer, rend, end, t = [snum, snum], [0, 0], [False, False], n, snum
        while t >= 1 and not (rend[0] and rend[1]):
            ln, tk = check(t, end - n - 1)
            for b in (0, 1):
                if sj[b] >= si[b] and not rend[b] and tk[b] > 0 and (kmer[b] == tk[b] or t == snum):
                    sj[b], kmer[b] = sj[b] - 1, tk[b]
                else:
                    rend[b] = True
            end, t = end - ln, t - 1
    return out


def cell_specs():
    """(mode, cls, width, edge) of every cell, in a fixed order."""
    return [(mode, cls, width, edge) for mode in MODES for cls in CLASSES for width in WIDTHS for edge in class_edges(mode, cls, width)]


_cells = {}


def cell(mode, cls, width, edge):
    key = (mode, cls, width, edge)
    if key not in _cells:
        _cells[key] = Cell(mode, cls, width, edge, cell_specs().index(key))
    return _cells[key]


def has_group_path(mode, cls, width):
    """Variants with a group pass of their own: short reads in the 3- and 5-word kernels (run_short_group), long reads in the
    5-word kernel (run_long_groups), 64-bit words only.  (The pair driver's group pass does not depend on the class.)"""
    return width == NARROW_W and ((mode == SHORT and cls in (3, 5)) or (mode == LONG and cls == 5))
