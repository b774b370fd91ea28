"""Every kernel variant at both edges of its mask-word class against the oracle, through the C ABI.  GPU only.

The cells come from kernel_matrix.py (test_kernel_matrix_cpu.py holds them to their class and to being worth running): per
(mode, class, word width) the batches whose longest segment is the smallest and the largest of the class, so the host picks
filter_kernel<3|5|10|32> and exact_kernel<3|5|10|0, MODE, u64|u128> on purpose.  Configurations:
  ragged    flags 0, reads of the edge length beside shorter ones (offsets and lengths: the general prefilter);
  uniform   flags 0, every read of one edge length, no offsets (short and pair mode: the uniform fast path of the 3- and 5-word
            prefilter, the general loop of the others);
  nofilter  TREW_FLAG_NO_FILTER: every unit reaches the exact kernel, which the host then builds without lane bounds --
            the same reads through decide<0>;
  nogroup   TREW_FLAG_DEBUG_NO_GROUP where a group pass exists: a wave per segment / per slice.
Tables must equal the oracle's integer for integer; in segment mode so must k_high, k_low and both MAX_SEQ words per segment.
"""
import pytest

import kernel_matrix as M
import oracle as O
import trew_amd as T
from trew_amd import capi
from test_gpu_parity import _table_diff

pytestmark = pytest.mark.gpu

RAGGED, UNIFORM, NOFILTER, NOGROUP = "ragged", "uniform", "nofilter", "nogroup"
FLAGS = {RAGGED: 0, UNIFORM: 0, NOFILTER: T.FLAG_NO_FILTER, NOGROUP: T.FLAG_DEBUG_NO_GROUP}
MODE_ID = {M.SEGMENT: T.MODE_SEGMENT, M.SHORT: T.MODE_SHORT, M.PAIR: T.MODE_PAIR, M.LONG: T.MODE_LONG}


def _configs(mode, cls, width):
    out = [RAGGED]
    if mode in (M.SHORT, M.PAIR):
        out.append(UNIFORM)
    out.append(NOFILTER)
    if M.has_group_path(mode, cls, width) or (mode == M.PAIR and width == M.NARROW_W):
        out.append(NOGROUP)
    return out


# ordered so that neighbouring tests share a context: mode, width, configuration, then the classes
CASES = [(mode, width, config, cls) for mode in M.MODES for width in M.WIDTHS for config in (RAGGED, UNIFORM, NOFILTER, NOGROUP)
         for cls in M.CLASSES if config in _configs(mode, cls, width)]


class _Contexts:
    """One context per (mode, parameters, slice length, flags), reused across cells with reset_tables(); the last few stay open."""

    def __init__(self, keep=3):
        self.keep, self.open = keep, {}

    def get(self, mode, ps, sl, flags):
        key = (mode, ps, sl, flags)
        if key not in self.open:
            while len(self.open) >= self.keep:
                self.open.pop(next(iter(self.open))).close()
            self.open[key] = T.TrewHip(mode=MODE_ID[mode], min_mer=ps[0], max_mer=ps[1], low=M.LOW, high=M.HIGH, slice_length=sl or 150,
                                       n_slots=1, max_batch_reads=1024, max_batch_words=1 << 18, flags=flags)
        return self.open[key]

    def close(self):
        for t in self.open.values():
            t.close()
        self.open = {}


@pytest.fixture(scope="module")
def contexts():
    c = _Contexts()
    yield c
    c.close()


def _uniform_batch(units, n):
    words, _, _ = capi.pack_reads(M.flat(units))
    stride = 3 * ((n + 31) // 32)
    n_reads = sum(len(u) for u in units)
    assert len(words) == n_reads * stride
    b = capi.Batch(words.ctypes.data, len(words), None, None, n, stride, n_reads, 0, n)  # no offsets: the uniform path
    b._keep = (words,)
    return b


def _same_tables(got, want, where):
    assert got == want, "tables differ from the oracle's: %s: %s" % (where, _table_diff(got, want))


def _check_segments(t, c, where):
    kh, kl, sh, sl = t.segment_results(len(c.units))
    bad = []
    for i, e in enumerate(c.segment_results):
        got = (int(kh[i]), int(kl[i]), int(sh[i]), int(sl[i]))
        want = (e["k_high"], e["k_low"], e["seq_high"], e["seq_low"])
        if got != want:
            bad.append((i, c.kinds[i], c.units[i][0], got, want))
    assert not bad, (where, len(bad), bad[:3])


def _check_group_pass_ran(t, c, counters, where):
    """The default run must not hand everything back to the wave-per-segment code, else a "group pass" cell tests the fall-back:
    group_punt + group_routed stays below the number of flagged units.

    In long mode group_punt counts slices, not reads, and it counts every slice longer than 159 bases: those never enter the
    5-word group pass (run_long_groups: `fits`), and the read lengths of a cell are chosen to have them -- SL + 1, 2 SL - 1 and
    every read with a remainder at SLICE_LENGTH = 159.  The slices the walk of each flagged read checks are known from the oracle
    (kernel_matrix.long_walk); the ones above 159 bases are taken off the count first, and must all be in it.  (Measured on an
    MI355X: SLICE_LENGTH 96: 167 reads flagged, group_punt 104, 52 of them slices above 159 bases; SLICE_LENGTH 159: 161 reads
    flagged, group_punt 168 -- more than there are reads -- 110 of them slices above 159 bases.  Short mode, where the counters
    count units: 0 + 55 of 198, 14 + 29 of 190, 15 + 33 of 191, 28 + 34 of 187.)"""
    worklist = [int(u) for u in t.debug_worklist(0)]
    flagged = len(worklist)
    assert flagged == t.last_timing(0)[2] == len(set(worklist)) > 0, where
    forced = 0
    if c.mode == M.LONG:
        group_limit = dict(M.CLASS_LIMITS)[5]
        walks = [M.long_walk(c.params(), c.units[u][0], c.sl) for u in worklist]
        forced = sum(1 for w in walks for ln in w if ln > group_limit)
        assert sum(len(w) for w in walks) - forced >= flagged, where  # slices the group pass can take: at least one per read
    groups = {k: v for k, v in counters.items() if k.startswith("group")}
    print("group pass: %s: %d units flagged, %d slices too long for the group pass, %r" % (where, flagged, forced, groups))
    assert forced <= counters["group_punt"], (where, forced, groups)
    assert counters["group_punt"] - forced + counters["group_routed"] < flagged, (where, flagged, forced, groups)


@pytest.mark.parametrize("mode,width,config,cls", CASES, ids=lambda v: str(v))
def test_variant_at_its_edges(contexts, mode, width, config, cls):
    flags = FLAGS[config]
    for edge in M.class_edges(mode, cls, width):
        c = M.cell(mode, cls, width, edge)
        t = contexts.get(mode, c.ps, c.sl, flags)
        where = "%r, %s" % (c, config)
        if config == UNIFORM:
            for n, units in c.uniform.items():
                t.reset_tables()
                t.submit(_uniform_batch(units, n))
                t.wait()
                _same_tables(t.collect(), c.want_uniform(n), "%s, every read %d bases" % (where, n))
            continue
        t.reset_tables()
        t.submit_reads(M.flat(c.units))
        t.wait()
        _same_tables(t.collect(), c.want, where)
        if mode == M.SEGMENT:
            _check_segments(t, c, where)
        counters = t.debug_counters()
        if config == RAGGED and M.has_group_path(mode, cls, width):
            _check_group_pass_ran(t, c, counters, where)
        if config == NOGROUP:
            assert counters["group_punt"] == counters["group_routed"] == counters["group_target"] == 0, (where, counters)


@pytest.mark.parametrize("sl", [320, 512])
def test_long_device_resident_wide_slices(sl):
    """Device-generated, device-resident long reads at SLICE_LENGTH 320 and 512 (exact_kernel<0, LONG>, middle slices of up to
    1023 bases): with the exact max_length hint, and with none (max_length = 0: kernels sized for the limit)."""
    n, seed = 300, 52000 + sl
    buf, st, nd = capi.synth_long_ascii(seed, 0, n)
    reads = [buf[s:e + 1] for s, e in zip(st, nd)]
    want = O.run_long(O.OracleParams(min_mer=5, max_mer=32, low=M.LOW, high=M.HIGH, slice_len=sl), reads)
    assert sum(len(v) for v in want.values()) > 0 and sum(1 for r in reads if len(r) >= sl) > n // 2
    with T.TrewHip(mode=T.MODE_LONG, low=M.LOW, high=M.HIGH, slice_length=sl, n_slots=1, max_batch_reads=n, max_batch_words=16) as t:
        b, ptrs, _ = t.synth_long_device(seed, 0, n)
        assert b.max_length == max(len(r) for r in reads)
        for hint in (b.max_length, 0):
            b.max_length = hint
            t.reset_tables()
            t.submit(b)
            t.wait()
            _same_tables(t.collect(), want, "SLICE_LENGTH %d, max_length %d" % (sl, hint))
        for p in ptrs:
            t.free(p)


def test_slice_length_limit():
    """SLICE_LENGTH up to 512 (a middle slice of 1023 bases, the longest segment any kernel takes) and no further."""
    with pytest.raises(T.TrewHipError, match="SLICE_LENGTH must be at most 512 on the HIP path."):
        T.TrewHip(mode=T.MODE_LONG, slice_length=513)
    with T.TrewHip(mode=T.MODE_LONG, slice_length=512, max_batch_reads=8, max_batch_words=1 << 12) as t:
        read = (b"TTAGGG" * 600)[:5 * 512 - 1]
        t.submit_reads([read])
        t.wait()
        assert t.collect() == O.run_long(O.OracleParams(slice_len=512), [read])


def test_cli_long_slice_400(tmp_path):
    """`trew long 5 32 -s 400` on the reads of a long cell (some shorter than the slice: the reader drops them), byte for byte."""
    from test_gpu_cli import expected, run, write_fastq

    reads = M.flat(M.cell(M.LONG, 0, M.NARROW_W, 320).units)
    assert any(len(r) < 400 for r in reads) and any(len(r) % 400 > 200 and len(r) >= 800 for r in reads)
    a = str(tmp_path / "matrix_long.fastq")
    write_fastq(a, reads)
    want = expected([(a, O.run_long(O.OracleParams(slice_len=400), reads))], 5)
    assert len(want) > 6
    assert run("long", "5", "32", a, "-s", "400", "-t", "2") == want
