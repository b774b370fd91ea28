"""ctypes binding of include/trew_hip.h (libtrew_hip.so).

This is plumbing for tests and bench.py; the product is the HIP library.  There
is no CPU fallback here: if the library is missing or no GPU is present, the
compute entry points raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TREW_HIP_LIB") or os.path.join(_HERE, "lib", "libtrew_hip.so")  # TREW_HIP_LIB: alternative build (tools/phase_profile.py)

MODE_SHORT, MODE_PAIR, MODE_LONG, MODE_SEGMENT = 0, 1, 2, 3
FLAG_NO_FILTER = 1
FLAG_DEBUG_POISON_LDS = 32  # the exact kernel starts from garbage-filled LDS (tests)
FLAG_NO_TIMING = 64  # no HIP events per submit (last_timing unavailable)
FLAG_COMPAT_G1 = 512  # pair mode, one slot: the reference's 64-bit pair branch as written (un-cleared temp_result_left)
FLAG_TRACK_PRESSURE = 256  # the fill counters come back with every batch; table_pressure asks no device
FLAG_DEBUG_NO_JOINT = 2048  # tests: the prefilter's uniform path without the joint k loop of both halves
FLAG_DEBUG_NO_UNI_DRAIN = 4096  # tests / A-B: the prefilter's set-aside reads judged by the general path (not filter_deferred_uni)
FLAG_DEBUG_NO_GROUP = 1024  # tests / A-B: every segment decided by a wave of its own (no decide_group)
FLAG_DEBUG_ANNOT_GENERAL = 8192  # tests: annotate gives every batch a wave per read (the lane-per-read kernel is never picked)
FLAG_DEBUG_SMALL_BOUNDS = 16384  # tests: the bounds pass hands over 64 worklist entries only (stored bounds and row bounds in one small batch)
FLAG_DEBUG_NO_LIVE_LIST = 32768  # tests, A/B runs: the bounds pass sharpens no bound and drops no entry; the exact kernel reads the prefilter's worklist
FLAG_DEBUG_ONE_CU = 65536  # tests: the wave-per-read kernels of the per-read measures get a one-CU grid (8 blocks, 32 waves): every wave loops over many reads
FLAG_DEBUG_WIDE_NO_WAIT = 128  # tests: the wide table never waits for a slot's ready bit (forces its time-out path)
TABLE_NAMES = ("forward_high", "forward_low", "backward_high", "backward_low", "both_high", "both_low")

# every symbol include/trew_hip.h declares
EXPORTED_SYMBOLS = (
    "trew_hip_init", "trew_hip_destroy", "trew_hip_last_error", "trew_hip_submit", "trew_hip_wait",
    "trew_hip_collect", "trew_hip_reset_tables", "trew_hip_add_rows", "trew_hip_segment_results",
    "trew_hip_filter_masks", "trew_hip_last_timing", "trew_pack_words", "trew_pack_reads",
    "trew_synth_short_ascii", "trew_synth_short_device", "trew_synth_pair_ascii", "trew_synth_pair_device",
    "trew_hip_malloc", "trew_hip_free", "trew_hip_memcpy_h2d", "trew_hip_memcpy_d2h", "trew_hip_abi_version",
    "trew_pack_pairs", "trew_hip_host_alloc", "trew_hip_host_free", "trew_hip_device_count",
    "trew_synth_long_lengths", "trew_synth_long_ascii", "trew_synth_long_device",
    "trew_hip_collect_device", "trew_hip_add_rows_device", "trew_hip_merge", "trew_hip_table_pressure",
    "trew_hip_add_gathered_device", "trew_hip_collect_slice_device", "trew_hip_debug_counters", "trew_hip_debug_worklist", "trew_hip_debug_live_list", "trew_hip_debug_measure_grid", "trew_hip_submit_ascii", "trew_hip_pack_ascii",
    "trew_motif_parse", "trew_hip_annotate", "trew_hip_annotate_results", "trew_annotate_host",
    "trew_hip_tracts", "trew_hip_tracts_results", "trew_tracts_host",
    "trew_hip_intervals", "trew_hip_intervals_results", "trew_intervals_host",
    "trew_hip_variants", "trew_hip_variants_results", "trew_variants_host",
    "trew_hip_periods", "trew_hip_periods_results", "trew_periods_host",
    "trew_hip_chain", "trew_hip_chain_results", "trew_chain_host",
    "trew_hip_repeats", "trew_hip_repeats_results", "trew_repeats_host",
    "trew_hip_satellites", "trew_hip_satellites_results", "trew_satellites_host",
    "trew_hip_align", "trew_hip_align_results", "trew_align_host",
    "trew_hip_refine", "trew_hip_refine_results", "trew_refine_host",
    "trew_hip_tandems", "trew_hip_tandems_results", "trew_tandems_host",
    "trew_hip_trace", "trew_hip_trace_results", "trew_trace_host",
    "trew_hip_decompose", "trew_hip_decompose_results", "trew_decompose_host",
    "trew_hip_dissect", "trew_hip_dissect_results", "trew_dissect_host",
    "trew_hip_resolve", "trew_hip_resolve_results", "trew_resolve_host",
    "trew_hip_tandems_resolved", "trew_tandems_resolved_host", "trew_hip_decompose_resolved", "trew_decompose_resolved_host",
    "trew_hip_dissect_resolved", "trew_dissect_resolved_host",
    "trew_monomer_parse", "trew_hip_monomers", "trew_hip_monomers_results", "trew_monomers_host",
    "trew_hip_copies", "trew_hip_copies_results", "trew_copies_host",
    "trew_hip_polish", "trew_hip_polish_results", "trew_polish_host",
)
DEBUG_COUNTERS = ("strict_rerun", "windows_fallback", "wide_spin_timeout", "inserted", "inserted_wide", "group_punt", "group_routed", "group_target",
                  "half_drain", "unit_drain", "dead_entries")


class Params(C.Structure):
    _fields_ = [
        ("min_mer", C.c_int32), ("max_mer", C.c_int32),
        ("low_baseline", C.c_double), ("high_baseline", C.c_double),
        ("slice_length", C.c_int32), ("mode", C.c_int32), ("device", C.c_int32), ("n_slots", C.c_int32),
        ("max_batch_words", C.c_uint64), ("max_batch_reads", C.c_uint64),
        ("table_log2_slots", C.c_uint32), ("flags", C.c_uint32),
        ("max_batch_ascii_bytes", C.c_uint64),
    ]


class Batch(C.Structure):
    _fields_ = [
        ("words", C.c_void_p), ("n_words", C.c_uint64),
        ("offsets", C.c_void_p), ("lengths", C.c_void_p),
        ("uniform_length", C.c_uint32), ("uniform_stride", C.c_uint32),
        ("n_reads", C.c_uint64), ("on_device", C.c_int32), ("max_length", C.c_int32),
    ]


class AsciiBatch(C.Structure):
    _fields_ = [
        ("bases", C.c_void_p), ("n_bytes", C.c_uint64),
        ("byte_offsets", C.c_void_p), ("lengths", C.c_void_p), ("word_offsets", C.c_void_p),
        ("uniform_length", C.c_uint32), ("reserved", C.c_uint32), ("n_reads", C.c_uint64),
    ]


class Row(C.Structure):
    _fields_ = [("k", C.c_int32), ("table", C.c_int32), ("word_lo", C.c_uint64), ("word_hi", C.c_uint64),
                ("count", C.c_uint64)]


class Motif(C.Structure):
    _fields_ = [("k", C.c_int32), ("reserved", C.c_int32), ("word", C.c_uint64)]


class Annot(C.Structure):
    _fields_ = [("windows_fwd", C.c_uint32), ("windows_rev", C.c_uint32), ("tract_start_fwd", C.c_uint32),
                ("tract_len_fwd", C.c_uint32), ("tract_start_rev", C.c_uint32), ("tract_len_rev", C.c_uint32)]


ANNOT_DTYPE = np.dtype([(name, "<u4") for name, _ in Annot._fields_])
assert ANNOT_DTYPE.itemsize == C.sizeof(Annot)
MAX_MOTIFS = 8


class Tract(C.Structure):
    _fields_ = [(name + sfx, C.c_uint32) for sfx in ("_fwd", "_rev")
                for name in ("covered", "head_len", "head_cov", "tail_len", "tail_cov")]


TRACT_DTYPE = np.dtype([(name, "<u4") for name, _ in Tract._fields_])
assert TRACT_DTYPE.itemsize == C.sizeof(Tract) == 40


class IntervalRule(C.Structure):
    _fields_ = [("max_gap", C.c_uint32), ("min_len", C.c_uint32)]


class Interval(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("read", "motif", "strand", "start", "end", "covered")]


INTERVAL_DTYPE = np.dtype([(name, "<u4") for name, _ in Interval._fields_])
assert INTERVAL_DTYPE.itemsize == C.sizeof(Interval) == 24 and C.sizeof(IntervalRule) == 8


class Variant(C.Structure):
    _fields_ = [(name + s, C.c_uint32) for s in ("_fwd", "_rev") for name in ("units", "variants", "distinct", "top", "top_count")]


VARIANT_DTYPE = np.dtype([(name, "<u4") for name, _ in Variant._fields_])
assert VARIANT_DTYPE.itemsize == C.sizeof(Variant) == 40
VARIANT_BINS = 128
VARIANT_NONE = 0xFFFFFFFF


class Period(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("period", "scored_period", "score", "start", "end", "matches", "support", "reserved")] + [("unit", C.c_uint64)]


PERIOD_DTYPE = np.dtype([(name, "<u8" if name == "unit" else "<u4") for name, _ in Period._fields_])
assert PERIOD_DTYPE.itemsize == C.sizeof(Period) == 40



class ChainItem(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("read", "motif", "strand", "start", "count", "bin")]


CHAIN_DTYPE = np.dtype([(name, "<u4") for name, _ in ChainItem._fields_])
assert CHAIN_DTYPE.itemsize == C.sizeof(ChainItem) == 24


class Repeat(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("read", "depth", "period", "scored_period", "score", "start", "end", "matches", "support",
                                                "reserved")] + [("unit", C.c_uint64)]


REPEAT_DTYPE = np.dtype([(name, "<u8" if name == "unit" else "<u4") for name, _ in Repeat._fields_])
assert REPEAT_DTYPE.itemsize == C.sizeof(Repeat) == 48

SATELLITE_MAX_PERIOD = 256  # TREW_SATELLITE_MAX_PERIOD


class Satellite(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("read", "depth", "period", "scored_period", "score", "start", "end", "matches", "support",
                                                "reserved")] + [("unit", C.c_uint32 * 16)]


SATELLITE_DTYPE = np.dtype([(name, "<u4", (16,)) if name == "unit" else (name, "<u4") for name, _ in Satellite._fields_])
assert SATELLITE_DTYPE.itemsize == C.sizeof(Satellite) == 104


class Alignment(C.Structure):
    _fields_ = [(name + sfx, C.c_uint32) for sfx in ("_fwd", "_rev") for name in ("score", "start", "end", "consumed", "matches")]


ALIGN_DTYPE = np.dtype([(name, "<u4") for name, _ in Alignment._fields_])
assert ALIGN_DTYPE.itemsize == C.sizeof(Alignment) == 40

MONOMER_MAX = 256  # TREW_MONOMER_MAX
MONOMERS_MAX = 8   # TREW_MONOMERS_MAX


class Monomer(C.Structure):
    _fields_ = [("k", C.c_int32), ("reserved", C.c_int32), ("unit", C.c_uint32 * 16)]


assert C.sizeof(Monomer) == 72


class TraceItem(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("read", "motif", "strand", "start", "bases", "count", "phase", "consumed", "mismatches",
                                                "insertions", "deletions", "reserved")]


TRACE_DTYPE = np.dtype([(name, "<u4") for name, _ in TraceItem._fields_])
assert TRACE_DTYPE.itemsize == C.sizeof(TraceItem) == 48


class Refined(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("period", "seed_period", "scored_period", "changed", "score", "start", "end", "consumed", "matches",
                                                "seed_score", "support", "reserved")] + [("unit", C.c_uint64), ("seed_unit", C.c_uint64)]


REFINE_DTYPE = np.dtype([(name, "<u8" if name in ("unit", "seed_unit") else "<u4") for name, _ in Refined._fields_])
assert REFINE_DTYPE.itemsize == C.sizeof(Refined) == 64


POLISH_MAX_PERIOD = 256  # TREW_POLISH_MAX_PERIOD


class Polished(C.Structure):
    _fields_ = list(Refined._fields_[:12]) + [("unit", C.c_uint32 * 16), ("seed_unit", C.c_uint32 * 16)]


POLISH_DTYPE = np.dtype([(name, "<u4") for name, _ in Refined._fields_[:12]] + [("unit", "<u4", (16,)), ("seed_unit", "<u4", (16,))])
assert POLISH_DTYPE.itemsize == C.sizeof(Polished) == 176


class Resolved(C.Structure):
    _fields_ = list(Refined._fields_) + [(name, C.c_uint32) for name in ("candidates", "rank", "first_period", "first_score")]


RESOLVE_DTYPE = np.dtype([(name, "<u8" if name in ("unit", "seed_unit") else "<u4") for name, _ in Resolved._fields_])
assert RESOLVE_DTYPE.itemsize == C.sizeof(Resolved) == 80
RESOLVE_MAX_CANDIDATES = 4


class Tandem(C.Structure):
    _fields_ = [("read", C.c_uint32), ("depth", C.c_uint32)] + list(Refined._fields_)


TANDEM_DTYPE = np.dtype([(name, "<u8" if name in ("unit", "seed_unit") else "<u4") for name, _ in Tandem._fields_])
assert TANDEM_DTYPE.itemsize == C.sizeof(Tandem) == 72

ROW_DTYPE = np.dtype([("k", "<i4"), ("table", "<i4"), ("word_lo", "<u8"), ("word_hi", "<u8"), ("count", "<u8")])
assert ROW_DTYPE.itemsize == C.sizeof(Row)

_lib = None


def rows_to_tables(rows):
    """Structured row array -> {name: {(k, word): count}}."""
    out = {name: {} for name in TABLE_NAMES}
    if len(rows) == 0:
        return out
    for t, k, lo, hi, c in zip(rows["table"].tolist(), rows["k"].tolist(), rows["word_lo"].tolist(),
                               rows["word_hi"].tolist(), rows["count"].tolist()):
        out[TABLE_NAMES[t]][(k, (hi << 64) | lo)] = c
    return out


def tables_to_rows(tables):
    items = [(k, t, w & 0xFFFFFFFFFFFFFFFF, w >> 64, c)
             for t, name in enumerate(TABLE_NAMES) for (k, w), c in tables.get(name, {}).items()]
    return np.array(items, dtype=ROW_DTYPE) if items else np.zeros(0, dtype=ROW_DTYPE)


def load():
    """Load libtrew_hip.so (raises OSError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("libtrew_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = C.CDLL(LIB_PATH)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    lib.trew_hip_abi_version.restype = i32
    lib.trew_hip_init.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    lib.trew_hip_destroy.argtypes = [vp]
    lib.trew_hip_destroy.restype = None
    lib.trew_hip_last_error.argtypes = [vp]
    lib.trew_hip_last_error.restype = C.c_char_p
    lib.trew_hip_submit.argtypes = [vp, C.POINTER(Batch), i32]
    lib.trew_hip_wait.argtypes = [vp, i32]
    lib.trew_hip_submit_ascii.argtypes = [vp, C.POINTER(AsciiBatch), i32]
    lib.trew_hip_pack_ascii.argtypes = [vp, C.POINTER(AsciiBatch), vp, u64, C.POINTER(u64)]
    lib.trew_hip_collect.argtypes = [vp, i32, C.POINTER(Row), u64, C.POINTER(u64)]
    lib.trew_hip_reset_tables.argtypes = [vp]
    lib.trew_hip_add_rows.argtypes = [vp, C.POINTER(Row), u64]
    lib.trew_hip_collect_device.argtypes = [vp, vp, u64, C.POINTER(u64)]
    lib.trew_hip_add_rows_device.argtypes = [vp, vp, u64]
    lib.trew_hip_merge.argtypes = [vp, vp]
    lib.trew_hip_add_gathered_device.argtypes = [vp, vp, C.c_uint32, C.c_uint32, u64, vp, C.POINTER(u64)]
    lib.trew_hip_collect_slice_device.argtypes = [vp, vp, u64, vp, C.POINTER(u64)]
    lib.trew_hip_debug_counters.argtypes = [vp, C.POINTER(u64), i32]
    lib.trew_hip_debug_worklist.argtypes = [vp, i32, vp, u64, C.POINTER(u64)]
    lib.trew_hip_debug_live_list.argtypes = [vp, i32, vp, u64, C.POINTER(u64)]
    lib.trew_hip_debug_measure_grid.restype = i32
    lib.trew_hip_debug_measure_grid.argtypes = [vp, u64, C.POINTER(C.c_uint32)]
    lib.trew_hip_table_pressure.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
    lib.trew_hip_segment_results.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, u64]
    lib.trew_hip_filter_masks.argtypes = [vp, C.POINTER(Batch), vp, i32]
    lib.trew_hip_last_timing.argtypes = [vp, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(u64)]
    lib.trew_motif_parse.argtypes = [C.c_char_p, C.POINTER(Motif)]
    lib.trew_hip_annotate.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Motif), i32]
    lib.trew_hip_annotate_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), C.POINTER(C.c_float)]
    lib.trew_annotate_host.argtypes = [vp, vp, vp, u64, C.POINTER(Motif), i32, vp]
    lib.trew_hip_tracts.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Motif), i32, i32]
    lib.trew_hip_tracts_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), C.POINTER(C.c_float)]
    lib.trew_tracts_host.argtypes = [vp, vp, vp, u64, C.POINTER(Motif), i32, i32, vp]
    lib.trew_hip_intervals.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Motif), C.POINTER(IntervalRule), i32, u64]
    lib.trew_hip_intervals_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), vp, C.POINTER(C.c_float)]
    lib.trew_intervals_host.argtypes = [vp, vp, vp, u64, C.POINTER(Motif), C.POINTER(IntervalRule), i32, vp, u64, C.POINTER(u64), vp]
    lib.trew_hip_variants.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Motif), i32]
    lib.trew_hip_variants_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), vp, vp, C.POINTER(C.c_float)]
    lib.trew_variants_host.argtypes = [vp, vp, vp, u64, C.POINTER(Motif), i32, vp, vp, vp]
    lib.trew_hip_periods.argtypes = [vp, C.POINTER(Batch), i32, i32, i32, i32, C.c_uint32]
    lib.trew_hip_periods_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), C.POINTER(C.c_float)]
    lib.trew_periods_host.argtypes = [vp, vp, vp, u64, i32, i32, i32, C.c_uint32, vp]
    lib.trew_hip_chain.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Motif), i32, u64]
    lib.trew_hip_chain_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), C.POINTER(u64), vp, C.POINTER(C.c_float)]
    lib.trew_chain_host.argtypes = [vp, vp, vp, u64, C.POINTER(Motif), i32, vp, u64, C.POINTER(u64), vp]
    lib.trew_hip_repeats.argtypes = [vp, C.POINTER(Batch), i32, i32, i32, i32, C.c_uint32, u64]
    lib.trew_hip_repeats_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), vp, C.POINTER(C.c_float)]
    lib.trew_repeats_host.argtypes = [vp, vp, vp, u64, i32, i32, i32, C.c_uint32, vp, u64, C.POINTER(u64), vp]
    lib.trew_hip_satellites.argtypes = lib.trew_hip_repeats.argtypes
    lib.trew_hip_satellites_results.argtypes = lib.trew_hip_repeats_results.argtypes
    lib.trew_satellites_host.argtypes = lib.trew_repeats_host.argtypes
    lib.trew_hip_align.argtypes = lib.trew_hip_tracts.argtypes
    lib.trew_hip_align_results.argtypes = lib.trew_hip_tracts_results.argtypes
    lib.trew_align_host.argtypes = lib.trew_tracts_host.argtypes
    lib.trew_monomer_parse.argtypes = [C.c_char_p, C.POINTER(Monomer)]
    lib.trew_hip_monomers.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Monomer), i32, i32]
    lib.trew_hip_monomers_results.argtypes = lib.trew_hip_tracts_results.argtypes
    lib.trew_monomers_host.argtypes = [vp, vp, vp, u64, C.POINTER(Monomer), i32, i32, vp]
    lib.trew_hip_trace.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Motif), i32, i32, C.c_uint32, u64, u64]
    lib.trew_hip_trace_results.argtypes = [vp, i32, vp, u64, C.POINTER(u64), C.POINTER(u64), vp, vp, C.POINTER(C.c_float)]
    lib.trew_trace_host.argtypes = [vp, vp, vp, u64, C.POINTER(Motif), i32, i32, C.c_uint32, vp, u64, C.POINTER(u64), vp, vp]
    lib.trew_hip_decompose.argtypes = [vp, C.POINTER(Batch), i32, i32, i32, i32, C.c_uint32, u64, u64]
    lib.trew_hip_copies.argtypes = [vp, C.POINTER(Batch), i32, C.POINTER(Monomer), i32, i32, C.c_uint32, u64, u64]
    lib.trew_hip_copies_results.argtypes = lib.trew_hip_trace_results.argtypes
    lib.trew_copies_host.argtypes = [vp, vp, vp, u64, C.POINTER(Monomer), i32, i32, C.c_uint32, vp, u64, C.POINTER(u64), C.POINTER(u64), vp, vp]
    lib.trew_hip_decompose_results.argtypes = lib.trew_hip_trace_results.argtypes
    lib.trew_decompose_host.argtypes = [vp, vp, vp, u64, i32, i32, i32, C.c_uint32, vp, u64, C.POINTER(u64), vp, vp]
    lib.trew_hip_dissect.argtypes = [vp, C.POINTER(Batch), i32, i32, i32, i32, C.c_uint32, u64, u64, u64]
    lib.trew_hip_dissect_results.argtypes = [vp, i32, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp, C.POINTER(C.c_float)]
    lib.trew_dissect_host.argtypes = [vp, vp, vp, u64, i32, i32, i32, C.c_uint32, vp, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp]
    lib.trew_hip_refine.argtypes = lib.trew_hip_periods.argtypes
    lib.trew_hip_refine_results.argtypes = lib.trew_hip_periods_results.argtypes
    lib.trew_refine_host.argtypes = lib.trew_periods_host.argtypes
    lib.trew_hip_polish.argtypes = lib.trew_hip_periods.argtypes
    lib.trew_hip_polish_results.argtypes = lib.trew_hip_periods_results.argtypes
    lib.trew_polish_host.argtypes = lib.trew_periods_host.argtypes
    lib.trew_hip_resolve.argtypes = lib.trew_hip_periods.argtypes + [i32]
    lib.trew_hip_resolve_results.argtypes = lib.trew_hip_periods_results.argtypes
    lib.trew_resolve_host.argtypes = lib.trew_periods_host.argtypes[:-1] + [i32, vp]
    lib.trew_hip_tandems.argtypes = lib.trew_hip_repeats.argtypes
    lib.trew_hip_tandems_results.argtypes = lib.trew_hip_repeats_results.argtypes
    lib.trew_tandems_host.argtypes = lib.trew_repeats_host.argtypes
    # the resolved forms: `candidates` behind min_score, the rest as the plain entry point's

    def with_candidates(argtypes):
        at = argtypes.index(C.c_uint32) + 1
        return argtypes[:at] + [i32] + argtypes[at:]

    for name in ("tandems", "decompose", "dissect"):
        getattr(lib, "trew_hip_%s_resolved" % name).argtypes = with_candidates(getattr(lib, "trew_hip_%s" % name).argtypes)
        getattr(lib, "trew_%s_resolved_host" % name).argtypes = with_candidates(getattr(lib, "trew_%s_host" % name).argtypes)
    lib.trew_pack_words.argtypes = [u64]
    lib.trew_pack_words.restype = u64
    lib.trew_pack_reads.argtypes = [C.c_char_p, vp, vp, u64, vp, u64, vp, vp]
    lib.trew_pack_reads.restype = u64
    lib.trew_synth_short_ascii.argtypes = [u64, u64, u64, C.c_uint32, vp]
    lib.trew_synth_short_device.argtypes = [vp, u64, u64, u64, C.c_uint32, vp]
    lib.trew_synth_pair_ascii.argtypes = [u64, u64, u64, C.c_uint32, vp, vp]
    lib.trew_synth_pair_device.argtypes = [vp, u64, u64, u64, C.c_uint32, vp]
    lib.trew_synth_long_lengths.argtypes = [u64, u64, u64, vp]
    lib.trew_synth_long_ascii.argtypes = [u64, u64, u64, vp, vp]
    lib.trew_synth_long_device.argtypes = [vp, u64, u64, u64, vp, vp]
    lib.trew_hip_malloc.argtypes = [vp, u64, C.POINTER(vp)]
    lib.trew_hip_free.argtypes = [vp, vp]
    lib.trew_hip_memcpy_h2d.argtypes = [vp, vp, vp, u64]
    lib.trew_hip_memcpy_d2h.argtypes = [vp, vp, vp, u64]
    _lib = lib
    return lib


class TrewHipError(RuntimeError):
    pass


def pack_reads(reads):
    """codes[] (kmer.cpp:14-31) applied on the host: list of byte strings -> (words, offsets, lengths)."""
    lib = load()
    reads = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
    n = len(reads)
    st = np.zeros(n, dtype=np.int64)
    nd = np.zeros(n, dtype=np.int64)
    pos = 0
    for i, r in enumerate(reads):
        st[i] = pos
        nd[i] = pos + len(r) - 1
        pos += len(r) + 1
    buf = b"\n".join(reads) + b"\n"
    cap = int(sum(lib.trew_pack_words(len(r)) for r in reads)) + 8
    words = np.zeros(cap, dtype=np.uint32)
    offsets = np.zeros(max(n, 1), dtype=np.uint32)
    lengths = np.zeros(max(n, 1), dtype=np.uint32)
    w = lib.trew_pack_reads(buf, st.ctypes.data, nd.ctypes.data, n, words.ctypes.data, cap, offsets.ctypes.data,
                            lengths.ctypes.data)
    if w == 2 ** 64 - 1:
        raise TrewHipError("trew_pack_reads: buffer too small")
    return words[: int(w)], offsets[:n], lengths[:n]


def motif(text):
    """'TTAGGG' (str or bytes, either case) -> Motif; raises TrewHipError for other characters or a length outside [3, 32]."""
    lib = load()
    if isinstance(text, Motif):
        return text
    m = Motif()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    if lib.trew_motif_parse(raw, C.byref(m)) != 0:
        raise TrewHipError("trew_motif_parse failed: %s" % lib.trew_hip_last_error(None).decode())
    return m


def _motif_array(motifs):
    ms = [motif(m) for m in motifs]
    return (Motif * max(len(ms), 1))(*ms), len(ms)


def _packed(reads_or_packed):
    """A list of reads (bytes / str), or the (words, offsets, lengths) of pack_reads -> the three arrays, contiguous uint32."""
    if isinstance(reads_or_packed, tuple) and len(reads_or_packed) == 3 and isinstance(reads_or_packed[0], np.ndarray):
        words, offsets, lengths = reads_or_packed
    else:
        words, offsets, lengths = pack_reads(reads_or_packed)
    return tuple(np.ascontiguousarray(a, dtype=np.uint32) for a in (words, offsets, lengths))


def annotate_host(reads_or_packed, motifs):
    """trew_annotate_host: the annotation computed on the host, window by window.  reads_or_packed: a list of reads (bytes /
    str) or the (words, offsets, lengths) of pack_reads.  Returns ANNOT_DTYPE records of shape (n_reads, n_motifs)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _motif_array(motifs)
    out = np.zeros((len(offsets), max(nm, 1)), dtype=ANNOT_DTYPE)
    if lib.trew_annotate_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, out.ctypes.data) != 0:
        raise TrewHipError("trew_annotate_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out[:, :nm]


def tracts_host(reads_or_packed, motifs, penalty=3):
    """trew_tracts_host: the error-tolerant terminal tracts computed on the host, base by base from the definition.
    reads_or_packed as for annotate_host.  Returns TRACT_DTYPE records of shape (n_reads, n_motifs)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _motif_array(motifs)
    out = np.zeros((len(offsets), max(nm, 1)), dtype=TRACT_DTYPE)
    if lib.trew_tracts_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, int(penalty), out.ctypes.data) != 0:
        raise TrewHipError("trew_tracts_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out[:, :nm]


def align_host(reads_or_packed, motifs, penalty=3):
    """trew_align_host: the indel-aware motif tract of every read (wraparound alignment) computed on the host, cell by cell
    from the definition.  reads_or_packed as for annotate_host.  Returns ALIGN_DTYPE records of shape (n_reads, n_motifs)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _motif_array(motifs)
    out = np.zeros((len(offsets), max(nm, 1)), dtype=ALIGN_DTYPE)
    if lib.trew_align_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, int(penalty), out.ctypes.data) != 0:
        raise TrewHipError("trew_align_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out[:, :nm]


def monomer(text):
    """'ACGT...' (str or bytes, either case, 3 to 256 bases) -> Monomer; raises TrewHipError for other characters or lengths."""
    lib = load()
    if isinstance(text, Monomer):
        return text
    m = Monomer()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    if lib.trew_monomer_parse(raw, C.byref(m)) != 0:
        raise TrewHipError("trew_monomer_parse failed: %s" % lib.trew_hip_last_error(None).decode())
    return m


def _monomer_array(monomers):
    ms = [monomer(m) for m in monomers]
    return (Monomer * max(len(ms), 1))(*ms), len(ms)


def monomers_host(reads_or_packed, monomers, penalty=3):
    """trew_monomers_host: align_host for units of 3 to 256 bases (texts or Monomer, at most 8), computed on the host from the
    definition.  reads_or_packed as for annotate_host.  Returns ALIGN_DTYPE records of shape (n_reads, n_monomers); align_columns
    serves them with k = the monomer's length."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _monomer_array(monomers)
    out = np.zeros((len(offsets), max(nm, 1)), dtype=ALIGN_DTYPE)
    if lib.trew_monomers_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, int(penalty), out.ctypes.data) != 0:
        raise TrewHipError("trew_monomers_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out[:, :nm]


def align_columns(record, k, penalty):
    """What follows exactly from an ALIGN_DTYPE record (or an array of them), the motif's length k and the penalty: a dict of
    copies, mismatches, insertions and deletions with the keys name_fwd and name_rev."""
    out = {}
    for sfx in ("_fwd", "_rev"):
        score, start, end, consumed, matches = (np.asarray(record[f + sfx]).astype(np.int64) for f in ("score", "start", "end", "consumed", "matches"))
        errors = (matches - score) // int(penalty)
        out["copies" + sfx] = consumed // int(k)
        out["insertions" + sfx] = errors - (consumed - matches)
        out["deletions" + sfx] = errors - (end - start - matches)
        out["mismatches" + sfx] = end - start - matches - out["insertions" + sfx]
    return out


def periods_host(reads_or_packed, min_period=1, max_period=32, penalty=3, min_score=24):
    """trew_periods_host: the de novo repeat period and unit of every read computed on the host, position by position from
    the definition.  reads_or_packed as for annotate_host.  Returns PERIOD_DTYPE records of shape (n_reads,)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    out = np.zeros(len(offsets), dtype=PERIOD_DTYPE)
    if lib.trew_periods_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), int(min_period), int(max_period),
                             int(penalty), int(min_score), out.ctypes.data) != 0:
        raise TrewHipError("trew_periods_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out


def variants_host(reads_or_packed, motifs):
    """trew_variants_host: the in-phase variant units computed on the host, window by window from the definition.
    reads_or_packed as for annotate_host.  Returns (VARIANT_DTYPE records of shape (n_reads, n_motifs), hist, reads_with),
    the two histograms uint64 of shape (n_motifs, 2, VARIANT_BINS)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _motif_array(motifs)
    out = np.zeros((len(offsets), max(nm, 1)), dtype=VARIANT_DTYPE)
    hist = np.zeros((max(nm, 1), 2, VARIANT_BINS), dtype=np.uint64)
    reads_with = np.zeros_like(hist)
    if lib.trew_variants_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, out.ctypes.data,
                              hist.ctypes.data, reads_with.ctypes.data) != 0:
        raise TrewHipError("trew_variants_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out[:, :nm], hist[:nm], reads_with[:nm]


def _rule_array(arr, nm, max_gap, min_len):
    """(IntervalRule * 8): max_gap / min_len are an int, a per-motif list or None (the defaults 3 k and 4 k of each motif)."""
    def per_motif(v, name, factor):
        if v is None:
            return [factor * int(arr[m].k) for m in range(nm)]
        if isinstance(v, (int, np.integer)):
            return [int(v)] * nm
        v = [int(x) for x in v]
        if len(v) != nm:
            raise TrewHipError("%s: %d values for %d motifs" % (name, len(v), nm))
        return v
    gaps, lens = per_motif(max_gap, "max_gap", 3), per_motif(min_len, "min_len", 4)
    rules = (IntervalRule * MAX_MOTIFS)()
    for m in range(min(nm, MAX_MOTIFS)):
        if not (0 <= gaps[m] < 1 << 32 and 0 <= lens[m] < 1 << 32):
            raise TrewHipError("max_gap and min_len must fit in 32 bits")
        rules[m] = IntervalRule(gaps[m], lens[m])
    return rules


def _sized_call(call, dtype, cap):
    """The log of a host definition: call(ptr, room, n) fills the buffer at `ptr` (None: no buffer) with up to `room` records and
    sets n (a c_uint64) to the number found.  With `cap` one call into a `dtype` buffer of that size; without, a first call that
    only counts and a second one into a buffer of exactly that size.  Returns (the records in the buffer, found)."""
    n = C.c_uint64(0)
    out = np.zeros(0 if cap is None else int(cap), dtype=dtype)
    call(out.ctypes.data if len(out) else None, len(out), n)
    if cap is None and n.value:
        out = np.zeros(int(n.value), dtype=dtype)
        call(out.ctypes.data, len(out), n)
    return out[:min(len(out), int(n.value))], int(n.value)


def _host_fail(what):
    raise TrewHipError("%s failed: %s" % (what, load().trew_hip_last_error(None).decode()))


def intervals_host(reads_or_packed, motifs, max_gap=None, min_len=None, cap=None):
    """trew_intervals_host: the gap-tolerant motif intervals computed on the host, base by base from the definition.
    reads_or_packed as for annotate_host; max_gap / min_len as for TrewHip.intervals.  Returns (INTERVAL_DTYPE records sorted
    by (read, motif, strand, start), counts of shape (n_reads, n_motifs, 2), found); with `cap` at most that many records."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _motif_array(motifs)
    rules = _rule_array(arr, min(max(nm, 0), MAX_MOTIFS), max_gap, min_len)
    counts = np.zeros((len(offsets), max(nm, 1), 2), dtype=np.uint32)

    def call(ptr, room, n):
        if lib.trew_intervals_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, rules, nm,
                                   ptr, room, C.byref(n), counts.ctypes.data) != 0:
            _host_fail("trew_intervals_host")

    out, found = _sized_call(call, INTERVAL_DTYPE, cap)
    return out, counts[:, :nm], found


def chain_host(reads_or_packed, motifs, cap=None):
    """trew_chain_host: the ordered unit chain computed on the host, window by window from the definition.  reads_or_packed
    as for annotate_host.  Returns (CHAIN_DTYPE items sorted by (read, motif, strand, start), counts of shape (n_reads,
    n_motifs, 2, 2) = [read][motif][strand]{runs, variants}, n_items); with `cap` at most that many items."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _motif_array(motifs)
    counts = np.zeros((len(offsets), max(nm, 1), 2, 2), dtype=np.uint32)

    def call(ptr, room, n):
        if lib.trew_chain_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm,
                               ptr, room, C.byref(n), counts.ctypes.data) != 0:
            _host_fail("trew_chain_host")

    out, found = _sized_call(call, CHAIN_DTYPE, cap)
    return out, counts[:, :nm], found


def trace_host(reads_or_packed, motifs, penalty=3, min_score=24, cap=None):
    """trew_trace_host: the traceback of the wraparound alignment, cut into copies of the motif, computed on the host with the
    full table.  reads_or_packed as for annotate_host.  Returns (TRACE_DTYPE items sorted by (read, motif, strand, start),
    counts of shape (n_reads, n_motifs, 2), ALIGN_DTYPE records of shape (n_reads, n_motifs), n_items); with `cap` at most
    that many items."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _motif_array(motifs)
    counts = np.zeros((len(offsets), max(nm, 1), 2), dtype=np.uint32)
    records = np.zeros((len(offsets), max(nm, 1)), dtype=ALIGN_DTYPE)

    def call(ptr, room, n):
        if lib.trew_trace_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, int(penalty), int(min_score),
                               ptr, room, C.byref(n), counts.ctypes.data,
                               records.ctypes.data) != 0:
            _host_fail("trew_trace_host")

    out, found = _sized_call(call, TRACE_DTYPE, cap)
    return out, counts[:, :nm], records[:, :nm], found


def copies_host(reads_or_packed, monomers, penalty=3, min_score=24, cap=None):
    """trew_copies_host: trace_host for units of 3 to 256 bases (texts or Monomer, at most 8), computed on the host with one
    direction byte a cell of the traced tract.  reads_or_packed as for annotate_host.  Returns (TRACE_DTYPE items sorted by
    (read, monomer, strand, start), counts of shape (n_reads, n_monomers, 2), ALIGN_DTYPE records of shape (n_reads,
    n_monomers), n_items, n_rows); with `cap` at most that many items."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    arr, nm = _monomer_array(monomers)
    counts = np.zeros((len(offsets), max(nm, 1), 2), dtype=np.uint32)
    records = np.zeros((len(offsets), max(nm, 1)), dtype=ALIGN_DTYPE)
    n_rows = C.c_uint64(0)

    def call(ptr, room, n):
        if lib.trew_copies_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), arr, nm, int(penalty), int(min_score),
                                ptr, room, C.byref(n), C.byref(n_rows), counts.ctypes.data, records.ctypes.data) != 0:
            _host_fail("trew_copies_host")

    out, found = _sized_call(call, TRACE_DTYPE, cap)
    return out, counts[:, :nm], records[:, :nm], found, int(n_rows.value)


def _resolved_call(lib, name, candidates):
    """(entry point, the arguments that follow min_score): `name` itself with candidates = 1, its _resolved form otherwise"""
    if int(candidates) == 1:
        return getattr(lib, name), ()
    stem, host = (name[:-5], "_host") if name.endswith("_host") else (name, "")
    return getattr(lib, stem + "_resolved" + host), (int(candidates),)


def decompose_host(reads_or_packed, min_period=1, max_period=32, penalty=3, min_score=24, cap=None, candidates=1):
    """trew_decompose_host: refine_host's record of every read, its unit turned to its smallest rotation (the record's
    `reserved` word is the anchor, the offset of that rotation in the unit) and the traceback of the read's forward strand
    against it, computed on the host with the full table.  reads_or_packed as for annotate_host.  Returns (TRACE_DTYPE items
    sorted by (read, start), motif = strand = 0, counts of shape (n_reads,), REFINE_DTYPE records of shape (n_reads,), n_items);
    with `cap` at most that many items.  candidates > 1: trew_decompose_resolved_host, resolve_host's record in refine_host's place."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    counts = np.zeros(len(offsets), dtype=np.uint32)
    records = np.zeros(len(offsets), dtype=REFINE_DTYPE)
    f, cand = _resolved_call(lib, "trew_decompose_host", candidates)

    def call(ptr, room, n):
        if f(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), int(min_period), int(max_period),
             int(penalty), int(min_score), *cand, ptr, room, C.byref(n), counts.ctypes.data, records.ctypes.data) != 0:
            _host_fail(f.__name__)

    out, found = _sized_call(call, TRACE_DTYPE, cap)
    return out, counts, records, found


def dissect_host(reads_or_packed, min_period=1, max_period=32, penalty=3, min_score=24, rec_cap=None, item_cap=None, candidates=1):
    """trew_dissect_host: tandems_host's records of every read, each with its unit's anchor in `reserved`, and for every record
    decompose_host's items of its piece taken as a read of its own, in read coordinates, computed on the host.  reads_or_packed
    as for annotate_host.  Returns (TANDEM_DTYPE records sorted by (read, start), TRACE_DTYPE items sorted by (read, start) with
    motif = the index of the item's tract among its read's records and strand = 0, counts of shape (n_reads, 2) = (tracts,
    items), n_records, n_items, n_rows); with rec_cap / item_cap at most that many records / items.  candidates > 1:
    trew_dissect_resolved_host, resolve_host's record of every piece in refine_host's place."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    counts = np.zeros((len(offsets), 2), dtype=np.uint32)
    nr, ni, nw = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    f, cand = _resolved_call(lib, "trew_dissect_host", candidates)

    def call(recs, items):
        if f(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), int(min_period), int(max_period),
             int(penalty), int(min_score), *cand, recs.ctypes.data if len(recs) else None, len(recs),
             items.ctypes.data if len(items) else None, len(items), C.byref(nr), C.byref(ni), C.byref(nw), counts.ctypes.data) != 0:
            _host_fail(f.__name__)

    recs = np.zeros(0 if rec_cap is None else int(rec_cap), dtype=TANDEM_DTYPE)
    items = np.zeros(0 if item_cap is None else int(item_cap), dtype=TRACE_DTYPE)
    call(recs, items)
    if (rec_cap is None and nr.value) or (item_cap is None and ni.value):
        if rec_cap is None:
            recs = np.zeros(int(nr.value), dtype=TANDEM_DTYPE)
        if item_cap is None:
            items = np.zeros(int(ni.value), dtype=TRACE_DTYPE)
        call(recs, items)
    return recs[:min(len(recs), int(nr.value))], items[:min(len(items), int(ni.value))], counts, int(nr.value), int(ni.value), int(nw.value)


def decompose_anchor(record):
    """The anchored unit M of a REFINE_DTYPE record of decompose as a packed word: rotation `reserved` of `unit`, M[j] = U[(j +
    anchor) mod period], first base most significant."""
    k, unit, sh = int(record["period"]), int(record["unit"]), 2 * int(record["reserved"])
    return ((unit << sh) | (unit >> (2 * k - sh))) & ((1 << (2 * k)) - 1) if k else 0


_TRACE_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def trace_signature(items, read, k):
    """(units, edited, signature) as `trew trace` prints them for the TRACE_DTYPE items of one (read, motif, strand), given in
    start order, `read` the read's text and k the motif's length: `=r` for a run of r complete exact copies, a complete copy with
    errors as its read bases in upper case, an end piece (consumed < k) as its read bases in lower case; on strand rev the bases
    of an item are reverse-complemented (motif orientation).  units: the copies of the items with consumed = k count; edited:
    the items with an error."""
    if isinstance(read, (bytes, bytearray)):
        read = read.decode("latin-1")
    units = edited = 0
    tokens = []
    for it in items:
        count, consumed = int(it["count"]), int(it["consumed"])
        errors = int(it["mismatches"]) + int(it["insertions"]) + int(it["deletions"])
        units += count if consumed == k * count else 0
        edited += errors > 0
        if consumed == k * count and int(it["phase"]) == 0 and not errors:
            tokens.append("=%d" % count)
            continue
        text = read[int(it["start"]):int(it["start"]) + int(it["bases"])].upper()
        if int(it["strand"]):
            text = "".join(_TRACE_COMP.get(c, "N") for c in reversed(text))
        tokens.append(text if consumed == k else text.lower())
    return units, edited, " ".join(tokens)


def copies_signature(items, read, k, bases=False):
    """(units, edited, signature) as `trew copies` prints them for the TRACE_DTYPE items of one (read, monomer, strand), given
    in start order.  For k <= 32, or with bases, trace_signature's text.  Above 32 an item that is no run of complete exact
    copies prints as `bases:mismatches.insertions.deletions`, an end piece (consumed < k) in parentheses: `=3 172:28.2.1 =1
    (40:0.0.0)`."""
    if k <= 32 or bases:
        return trace_signature(items, read, k)
    units = edited = 0
    tokens = []
    for it in items:
        count, consumed = int(it["count"]), int(it["consumed"])
        errors = int(it["mismatches"]) + int(it["insertions"]) + int(it["deletions"])
        units += count if consumed == k * count else 0
        edited += errors > 0
        if consumed == k * count and int(it["phase"]) == 0 and not errors:
            tokens.append("=%d" % count)
            continue
        text = "%d:%d.%d.%d" % (int(it["bases"]), int(it["mismatches"]), int(it["insertions"]), int(it["deletions"]))
        tokens.append(text if consumed == k else "(" + text + ")")
    return units, edited, " ".join(tokens)


def _tracts_host(name, dtype, reads_or_packed, min_period, max_period, penalty, min_score, cap, candidates=1):
    """trew_repeats_host, trew_satellites_host and trew_tandems_host, which differ in the record only (candidates: tandems alone)"""
    f, cand = _resolved_call(load(), name, candidates)
    words, offsets, lengths = _packed(reads_or_packed)
    counts = np.zeros(len(offsets), dtype=np.uint32)

    def call(ptr, room, n):
        if f(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), int(min_period), int(max_period), int(penalty), int(min_score),
             *cand, ptr, room, C.byref(n), counts.ctypes.data) != 0:
            _host_fail(f.__name__)

    out, found = _sized_call(call, dtype, cap)
    return out, counts, found


def repeats_host(reads_or_packed, min_period=1, max_period=32, penalty=3, min_score=24, cap=None):
    """trew_repeats_host: every de novo repeat tract of every read computed on the host, piece by piece from the definition.
    reads_or_packed as for annotate_host.  Returns (REPEAT_DTYPE records sorted by (read, start), counts of shape (n_reads,),
    found); with `cap` at most that many records."""
    return _tracts_host("trew_repeats_host", REPEAT_DTYPE, reads_or_packed, min_period, max_period, penalty, min_score, cap)


def refine_host(reads_or_packed, min_period=1, max_period=32, penalty=3, min_score=24):
    """trew_refine_host: the refined de novo repeat of every read (the period and tract of `periods`, a seed unit from the
    longest run, wraparound alignment, re-voted unit) computed on the host, step by step from the definition.
    reads_or_packed as for annotate_host.  Returns REFINE_DTYPE records of shape (n_reads,)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    out = np.zeros(len(offsets), dtype=REFINE_DTYPE)
    if lib.trew_refine_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), int(min_period), int(max_period),
                            int(penalty), int(min_score), out.ctypes.data) != 0:
        raise TrewHipError("trew_refine_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out


def polish_host(reads_or_packed, min_period=1, max_period=POLISH_MAX_PERIOD, penalty=3, min_score=24):
    """trew_polish_host: refine_host for periods up to 256 (step 1 is the depth-0 record of `satellites`, the recurrence is
    that of `monomers`) computed on the host, step by step from the definition.  reads_or_packed as for annotate_host.
    Returns POLISH_DTYPE records of shape (n_reads,): refine's twelve words, then unit and seed_unit as sixteen words each
    (satellite_unit_text turns either into text; refine_columns takes the records as they are)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    out = np.zeros(len(offsets), dtype=POLISH_DTYPE)
    if lib.trew_polish_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), int(min_period), int(max_period),
                            int(penalty), int(min_score), out.ctypes.data) != 0:
        raise TrewHipError("trew_polish_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out


def resolve_host(reads_or_packed, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3):
    """trew_resolve_host: refine's unit with the period chosen by alignment, computed on the host step by step from the
    definition: the `candidates` (1 .. 4) best-scoring periods of `periods`' score each refined as refine_host refines its one,
    the record with the largest final score kept.  reads_or_packed as for annotate_host.  Returns RESOLVE_DTYPE records of
    shape (n_reads,); their first sixteen words are a REFINE_DTYPE record (refine_columns takes them as they are)."""
    lib = load()
    words, offsets, lengths = _packed(reads_or_packed)
    out = np.zeros(len(offsets), dtype=RESOLVE_DTYPE)
    if lib.trew_resolve_host(words.ctypes.data, offsets.ctypes.data, lengths.ctypes.data, len(offsets), int(min_period), int(max_period),
                             int(penalty), int(min_score), int(candidates), out.ctypes.data) != 0:
        raise TrewHipError("trew_resolve_host failed: %s" % lib.trew_hip_last_error(None).decode())
    return out


def tandems_host(reads_or_packed, min_period=1, max_period=32, penalty=3, min_score=24, cap=None, candidates=1):
    """trew_tandems_host: every de novo repeat tract of every read under indels computed on the host, piece by piece from the
    definition (the refined record of a piece, then what lies in front of its tract and behind it).  reads_or_packed as for
    annotate_host.  Returns (TANDEM_DTYPE records sorted by (read, start), counts of shape (n_reads,), found); with `cap` at most
    that many records.  candidates > 1: trew_tandems_resolved_host, resolve_host's record of every piece in refine_host's place."""
    return _tracts_host("trew_tandems_host", TANDEM_DTYPE, reads_or_packed, min_period, max_period, penalty, min_score, cap, candidates)


def refine_columns(record, penalty):
    """What follows exactly from a REFINE_DTYPE record (or an array of them) and the penalty: a dict of copies, mismatches,
    insertions and deletions, as align_columns with k = period (all zero for a zero record)."""
    period, score, start, end, consumed, matches = (np.asarray(record[f]).astype(np.int64)
                                                    for f in ("period", "score", "start", "end", "consumed", "matches"))
    errors = (matches - score) // int(penalty)
    insertions = errors - (consumed - matches)
    return {"copies": consumed // np.maximum(period, 1), "mismatches": end - start - matches - insertions, "insertions": insertions,
            "deletions": errors - (end - start - matches)}


def tandem_columns(record, penalty):
    """refine_columns for a TANDEM_DTYPE record (or an array of them): copies, mismatches, insertions and deletions."""
    return refine_columns(record, penalty)


def satellites_host(reads_or_packed, min_period=1, max_period=SATELLITE_MAX_PERIOD, penalty=3, min_score=24, cap=None):
    """trew_satellites_host: repeats_host with periods up to 256 and SATELLITE_DTYPE records (unit: sixteen words, see
    satellite_unit_text).  Returns (records sorted by (read, start), counts of shape (n_reads,), found); with `cap` at most that
    many records."""
    return _tracts_host("trew_satellites_host", SATELLITE_DTYPE, reads_or_packed, min_period, max_period, penalty, min_score, cap)


def satellite_unit_text(unit, period):
    """The unit of a SATELLITE_DTYPE record as text: base j (j < period) lies in bits [2 (j & 15), 2 (j & 15) + 2) of
    unit[j >> 4], codes T 0, G 1, C 2, A 3."""
    return "".join("TGCA"[(int(unit[j >> 4]) >> (2 * (j & 15))) & 3] for j in range(int(period)))


def chain_unit_text(motif_text, bin_):
    """A variant's bin as text: the motif as typed (upper case) with base bin // 4 replaced by the bin's base."""
    t = list((motif_text.decode() if isinstance(motif_text, bytes) else motif_text).upper())
    if bin_ // 4 < len(t):
        t[bin_ // 4] = "TGCA"[bin_ & 3]
    return "".join(t)


def chain_signature(items, motif_text):
    """The signature `trew chain` prints for the items of one (read, motif, strand), given in start order: `=r` for a run of
    r exact units, a variant unit as its text in motif orientation, and `+d` / `-d` between two consecutive items a and b
    with d = b.start - (a.start + a.count k) != 0; joined by single spaces."""
    k = len(motif_text)
    tokens, at = [], None
    for it in items:
        start, count, bin_ = int(it["start"]), int(it["count"]), int(it["bin"])
        if at is not None and start != at:
            tokens.append("%+d" % (start - at))
        tokens.append("=%d" % count if bin_ == VARIANT_NONE else chain_unit_text(motif_text, bin_))
        at = start + count * k
    return " ".join(tokens)


def synth_short_ascii(seed, first_read, n_reads, read_len):
    """Host side of the synthetic short-read generator: returns (buf, st, nd)."""
    lib = load()
    out = np.zeros(n_reads * (read_len + 1), dtype=np.uint8)
    lib.trew_synth_short_ascii(seed, first_read, n_reads, read_len, out.ctypes.data)
    st = np.arange(n_reads, dtype=np.int64) * (read_len + 1)
    nd = st + read_len - 1
    return out.tobytes(), st, nd


def synth_pair_ascii(seed, first_pair, n_pairs, read_len):
    lib = load()
    o1 = np.zeros(n_pairs * (read_len + 1), dtype=np.uint8)
    o2 = np.zeros(n_pairs * (read_len + 1), dtype=np.uint8)
    lib.trew_synth_pair_ascii(seed, first_pair, n_pairs, read_len, o1.ctypes.data, o2.ctypes.data)
    st = np.arange(n_pairs, dtype=np.int64) * (read_len + 1)
    nd = st + read_len - 1
    return o1.tobytes(), o2.tobytes(), st, nd


def synth_long_lengths(seed, first_read, n_reads):
    lib = load()
    lens = np.zeros(n_reads, dtype=np.uint32)
    lib.trew_synth_long_lengths(seed, first_read, n_reads, lens.ctypes.data)
    return lens


def synth_long_ascii(seed, first_read, n_reads):
    """Host side of the long-read generator: (buf, st, nd) with one '\\n' after each read."""
    lib = load()
    lens = synth_long_lengths(seed, first_read, n_reads).astype(np.int64)
    st = np.zeros(n_reads, dtype=np.int64)
    st[1:] = np.cumsum(lens[:-1] + 1)
    out = np.zeros(int(st[-1] + lens[-1] + 1) if n_reads else 0, dtype=np.uint8)
    st_u64 = np.ascontiguousarray(st, dtype=np.uint64)  # keep the array alive across the call
    lib.trew_synth_long_ascii(seed, first_read, n_reads, st_u64.ctypes.data, out.ctypes.data)
    return out.tobytes(), st, st + lens - 1


def _copies_room(batch, nm, max_items, max_rows):
    """(max_items, max_rows) of a copies call with the defaults of TrewHip.copies filled in: trace's items, and its rows for
    each strand (a key claims end - start rows of its own)"""
    items, _ = _trace_room(batch, nm, max_items, 1)
    return items, (_trace_room(batch, 2 * nm, 1, None)[1] if max_rows is None else int(max_rows))


def _trace_room(batch, nm, max_items, max_rows):
    """(max_items, max_rows) of a trace call with the defaults of TrewHip.trace filled in"""
    if max_items is None:
        max_items = max(4 * int(batch.n_reads) * nm, 1)
    if max_rows is None:
        n = int(batch.n_reads)
        if not batch.lengths:  # uniform reads
            bases = n * int(batch.uniform_length)
        elif not batch.on_device:
            bases = int(np.ctypeslib.as_array(C.cast(batch.lengths, C.POINTER(C.c_uint32)), shape=(n,)).sum(dtype=np.uint64)) if n else 0
        else:
            bases = 256 * n  # lengths in device memory: a guess, the results say when it was too small
        max_rows = max(bases * nm, 1)
    return int(max_items), int(max_rows)


class TrewHip:
    """One device context: init / submit / wait / collect."""

    def __init__(self, mode=MODE_SHORT, min_mer=5, max_mer=32, low=0.5, high=0.8, slice_length=150, device=0,
                 n_slots=2, max_batch_words=1 << 22, max_batch_reads=1 << 18, table_log2_slots=20, flags=0, max_batch_ascii_bytes=0):
        self.lib = load()
        flags |= int(os.environ.get("TREW_EXTRA_FLAGS", "0"))  # e.g. 32 = FLAG_DEBUG_POISON_LDS for a whole test run
        self.params = Params(min_mer, max_mer, low, high, slice_length, mode, device, n_slots, max_batch_words,
                             max_batch_reads, table_log2_slots, flags, max_batch_ascii_bytes)
        self.ctx = C.c_void_p()
        rc = self.lib.trew_hip_init(C.byref(self.params), C.byref(self.ctx))
        if rc != 0:
            raise TrewHipError("trew_hip_init failed (%d): %s" % (rc, self.lib.trew_hip_last_error(None).decode()))
        self.mode = mode
        self._keep = {}
        self._queued = {}  # (measure, slot) -> the shape of what the measure queued last on the slot

    def close(self):
        if self.ctx:
            self.lib.trew_hip_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc, what):
        if rc != 0:
            raise TrewHipError("%s failed (%d): %s" % (what, rc, self.lib.trew_hip_last_error(self.ctx).decode()))

    # ---- batches ----
    def host_batch(self, words, offsets, lengths, contiguous=False):
        """contiguous: one buffer laid out [offsets][lengths][words], which trew_hip_submit ships with a single copy."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        if contiguous:
            n = len(offsets)
            buf = np.concatenate([offsets, lengths, words])
            b = Batch(buf.ctypes.data + 8 * n, len(words), buf.ctypes.data, buf.ctypes.data + 4 * n, 0, 0, n, 0, 0)
            b._keep = (buf,)
            return b
        b = Batch(words.ctypes.data, len(words), offsets.ctypes.data, lengths.ctypes.data, 0, 0, len(offsets), 0, 0)
        b._keep = (words, offsets, lengths)
        return b

    def device_uniform_batch(self, d_words, n_reads, read_len):
        stride = 3 * ((read_len + 31) // 32)
        return Batch(d_words, n_reads * stride, None, None, read_len, stride, n_reads, 1, read_len)

    def ascii_batch(self, reads, contiguous=True, uniform=None):
        """Text batch of the reads (bytes objects): the sequence bytes back to back + word/byte offsets + lengths, laid out
        [word_offsets][byte_offsets][lengths][bases] in one buffer when contiguous.  uniform=L: no arrays, every read has L bases."""
        reads = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
        n = len(reads)
        text = np.frombuffer(b"".join(reads) + b"\0" * 8, dtype=np.uint8)
        n_bytes = len(text) - 8
        if uniform is not None:
            assert all(len(r) == uniform for r in reads)
            b = AsciiBatch(text.ctypes.data, n_bytes, None, None, None, uniform, 0, n)
            b._keep = (text,)
            return b
        lens = np.array([len(r) for r in reads], dtype=np.uint32)
        boff = np.zeros(n, dtype=np.uint32)
        woff = np.zeros(n, dtype=np.uint32)
        if n:
            boff[1:] = np.cumsum(lens[:-1], dtype=np.uint64).astype(np.uint32)
            woff[1:] = np.cumsum(3 * ((lens[:-1].astype(np.uint64) + 31) // 32)).astype(np.uint32)
        if contiguous:
            buf = np.concatenate([woff.view(np.uint8), boff.view(np.uint8), lens.view(np.uint8), text])
            base = buf.ctypes.data
            b = AsciiBatch(base + 12 * n, n_bytes, base + 4 * n, base + 8 * n, base, 0, 0, n)
            b._keep = (buf,)
            return b
        b = AsciiBatch(text.ctypes.data, n_bytes, boff.ctypes.data, lens.ctypes.data, woff.ctypes.data, 0, 0, n)
        b._keep = (text, boff, lens, woff)
        return b

    def submit_ascii(self, batch, slot=0):
        self._keep[slot] = batch
        self._chk(self.lib.trew_hip_submit_ascii(self.ctx, C.byref(batch), slot), "trew_hip_submit_ascii")

    def pack_ascii(self, batch):
        """The packed words the device makes of a text batch (diagnostic: must equal pack_reads())."""
        n = C.c_uint64(0)
        self._chk(self.lib.trew_hip_pack_ascii(self.ctx, C.byref(batch), None, 0, C.byref(n)), "trew_hip_pack_ascii")
        words = np.zeros(max(int(n.value), 1), dtype=np.uint32)
        self._chk(self.lib.trew_hip_pack_ascii(self.ctx, C.byref(batch), words.ctypes.data, len(words), C.byref(n)), "trew_hip_pack_ascii")
        return words[: int(n.value)]

    def submit(self, batch, slot=0):
        self._keep[slot] = batch
        self._chk(self.lib.trew_hip_submit(self.ctx, C.byref(batch), slot), "trew_hip_submit")

    def wait(self, slot=0):
        self._chk(self.lib.trew_hip_wait(self.ctx, slot), "trew_hip_wait")

    def _queue(self, measure, slot, batch, arr, nm, keep=(), shape=()):
        """Before a measure's queue call: keeps the batch and the argument arrays (`arr`, `keep`) alive, remembers
        (n_reads, n_motifs) + shape."""
        self._keep[(measure, slot)] = (batch, arr) + keep
        self._queued[(measure, slot)] = (int(batch.n_reads), nm) + shape

    def _fetch_records(self, measure, slot, dtype, want_ms, *extra):
        """The fixed-size records of the slot's last `measure`: (out of shape (n_reads, n_motifs),) + extra [+ (kernel ms,)];
        `extra` are arrays the results call fills between the count and the time."""
        n = C.c_uint64(0)
        ms = C.c_float(0)
        n_reads, nm = self._queued.get((measure, slot), (0, 1))
        out = np.zeros((n_reads, nm), dtype=dtype)
        what = "trew_hip_%s_results" % measure
        self._chk(getattr(self.lib, what)(self.ctx, slot, out.ctypes.data, n_reads * nm, C.byref(n), *[x.ctypes.data for x in extra],
                                          C.byref(ms) if want_ms else None), what)
        if int(n.value) != n_reads * nm:
            raise TrewHipError("%s: %d records, expected %d" % (what, n.value, n_reads * nm))
        return (out,) + extra + ((ms.value,) if want_ms else ())

    def _fetch_log(self, measure, slot, dtype, want_ms, counts_shape=lambda n_reads, nm: (n_reads,), partial=False):
        """The append log of the slot's last intervals, repeats, tandems or satellites: (records, counts, found [, kernel ms]).
        The log is read once, into a buffer of exactly what it holds: a first call for `found` and the counts, a second one for the
        records.  found > the call's capacity: no records, or with `partial` (intervals) as many as the log held."""
        n = C.c_uint64(0)
        ms = C.c_float(0)
        n_reads, nm, cap = self._queued.get((measure, slot), (0, 1, 0))
        counts = np.zeros(counts_shape(n_reads, nm), dtype=np.uint32)
        what = "trew_hip_%s_results" % measure
        results = getattr(self.lib, what)
        self._chk(results(self.ctx, slot, None, 0, C.byref(n), counts.ctypes.data, C.byref(ms) if want_ms else None), what)
        found = int(n.value)
        out = np.zeros(found if found <= cap else cap if partial else 0, dtype=dtype)
        if len(out):
            self._chk(results(self.ctx, slot, out.ctypes.data, len(out), C.byref(n), None, None), what)
        return (out, counts, found, ms.value) if want_ms else (out, counts, found)

    def _queue_tracts(self, measure, batch, min_period, max_period, penalty, min_score, max_records, slot, candidates=1):
        """the queue call of repeats, tandems and satellites; max_records: default the batch's read count, at least 1"""
        if max_records is None:
            max_records = max(int(batch.n_reads), 1)
        self._queue(measure, slot, batch, None, 1, shape=(int(max_records),))
        f, cand = _resolved_call(self.lib, "trew_hip_%s" % measure, candidates)
        self._chk(f(self.ctx, C.byref(batch), slot, int(min_period), int(max_period), int(penalty), int(min_score), *cand, int(max_records)), f.__name__)

    def annotate(self, batch, motifs, slot=0):
        """Queue the annotation of every read of `batch` against `motifs` (texts or Motif, at most 8) on the slot's stream."""
        arr, nm = _motif_array(motifs)
        self._queue("annotate", slot, batch, arr, nm)
        self._chk(self.lib.trew_hip_annotate(self.ctx, C.byref(batch), slot, arr, nm), "trew_hip_annotate")

    def annotate_results(self, slot=0, want_ms=False):
        """Records of the slot's last annotate: ANNOT_DTYPE array of shape (n_reads, n_motifs) [, kernel ms]."""
        res = self._fetch_records("annotate", slot, ANNOT_DTYPE, want_ms)
        return res if want_ms else res[0]

    def tracts(self, batch, motifs, penalty=3, slot=0):
        """Queue the error-tolerant terminal tracts of every read of `batch` for `motifs` (texts or Motif, at most 8) on the
        slot's stream."""
        arr, nm = _motif_array(motifs)
        self._queue("tracts", slot, batch, arr, nm)
        self._chk(self.lib.trew_hip_tracts(self.ctx, C.byref(batch), slot, arr, nm, int(penalty)), "trew_hip_tracts")

    def tracts_results(self, slot=0, want_ms=False):
        """Records of the slot's last tracts: TRACT_DTYPE array of shape (n_reads, n_motifs) [, kernel ms]."""
        res = self._fetch_records("tracts", slot, TRACT_DTYPE, want_ms)
        return res if want_ms else res[0]

    def align(self, batch, motifs, penalty=3, slot=0):
        """Queue the indel-aware motif tract (wraparound alignment) of every read of `batch` for `motifs` (texts or Motif, at
        most 8) on the slot's stream."""
        arr, nm = _motif_array(motifs)
        self._queue("align", slot, batch, arr, nm)
        self._chk(self.lib.trew_hip_align(self.ctx, C.byref(batch), slot, arr, nm, int(penalty)), "trew_hip_align")

    def align_results(self, slot=0, want_ms=False):
        """Records of the slot's last align: ALIGN_DTYPE array of shape (n_reads, n_motifs) [, kernel ms]."""
        res = self._fetch_records("align", slot, ALIGN_DTYPE, want_ms)
        return res if want_ms else res[0]

    def monomers(self, batch, monomers, penalty=3, slot=0):
        """Queue `align` for units of 3 to 256 bases: the wraparound alignment of every read of `batch` against `monomers`
        (texts or Monomer, at most 8) on the slot's stream."""
        arr, nm = _monomer_array(monomers)
        self._queue("monomers", slot, batch, arr, nm)
        self._chk(self.lib.trew_hip_monomers(self.ctx, C.byref(batch), slot, arr, nm, int(penalty)), "trew_hip_monomers")

    def monomers_results(self, slot=0, want_ms=False):
        """Records of the slot's last monomers: ALIGN_DTYPE array of shape (n_reads, n_monomers) [, kernel ms]."""
        res = self._fetch_records("monomers", slot, ALIGN_DTYPE, want_ms)
        return res if want_ms else res[0]

    def periods(self, batch, min_period=1, max_period=32, penalty=3, min_score=24, slot=0):
        """Queue the de novo repeat period and unit of every read of `batch` on the slot's stream (no motifs)."""
        self._queue("periods", slot, batch, None, 1)
        self._chk(self.lib.trew_hip_periods(self.ctx, C.byref(batch), slot, int(min_period), int(max_period), int(penalty), int(min_score)),
                  "trew_hip_periods")

    def periods_results(self, slot=0, want_ms=False):
        """Records of the slot's last periods: PERIOD_DTYPE array of shape (n_reads,) [, kernel ms]."""
        res = self._fetch_records("periods", slot, PERIOD_DTYPE, want_ms)
        return (res[0][:, 0], res[1]) if want_ms else res[0][:, 0]

    def refine(self, batch, min_period=1, max_period=32, penalty=3, min_score=24, slot=0):
        """Queue the refined de novo repeat of every read of `batch` on the slot's stream (no motifs)."""
        self._queue("refine", slot, batch, None, 1)
        self._chk(self.lib.trew_hip_refine(self.ctx, C.byref(batch), slot, int(min_period), int(max_period), int(penalty), int(min_score)),
                  "trew_hip_refine")

    def refine_results(self, slot=0, want_ms=False):
        """Records of the slot's last refine: REFINE_DTYPE array of shape (n_reads,) [, kernel ms]."""
        res = self._fetch_records("refine", slot, REFINE_DTYPE, want_ms)
        return (res[0][:, 0], res[1]) if want_ms else res[0][:, 0]

    def polish(self, batch, min_period=1, max_period=POLISH_MAX_PERIOD, penalty=3, min_score=24, slot=0):
        """Queue the refined de novo repeat of every read of `batch` for periods up to 256 on the slot's stream (no motifs)."""
        self._queue("polish", slot, batch, None, 1)
        self._chk(self.lib.trew_hip_polish(self.ctx, C.byref(batch), slot, int(min_period), int(max_period), int(penalty), int(min_score)),
                  "trew_hip_polish")

    def polish_results(self, slot=0, want_ms=False):
        """Records of the slot's last polish: POLISH_DTYPE array of shape (n_reads,) [, kernel ms]."""
        res = self._fetch_records("polish", slot, POLISH_DTYPE, want_ms)
        return (res[0][:, 0], res[1]) if want_ms else res[0][:, 0]

    def resolve(self, batch, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3, slot=0):
        """Queue refine's unit with the period chosen by alignment for every read of `batch` on the slot's stream (no motifs)."""
        self._queue("resolve", slot, batch, None, 1)
        self._chk(self.lib.trew_hip_resolve(self.ctx, C.byref(batch), slot, int(min_period), int(max_period), int(penalty), int(min_score),
                                            int(candidates)), "trew_hip_resolve")

    def resolve_results(self, slot=0, want_ms=False):
        """Records of the slot's last resolve: RESOLVE_DTYPE array of shape (n_reads,) [, kernel ms]."""
        res = self._fetch_records("resolve", slot, RESOLVE_DTYPE, want_ms)
        return (res[0][:, 0], res[1]) if want_ms else res[0][:, 0]

    def variants(self, batch, motifs, slot=0):
        """Queue the in-phase variant units of every read of `batch` for `motifs` (texts or Motif, at most 8, taken as typed)
        on the slot's stream."""
        arr, nm = _motif_array(motifs)
        self._queue("variants", slot, batch, arr, nm)
        self._chk(self.lib.trew_hip_variants(self.ctx, C.byref(batch), slot, arr, nm), "trew_hip_variants")

    def variants_results(self, slot=0, want_ms=False):
        """Results of the slot's last variants: (VARIANT_DTYPE records of shape (n_reads, n_motifs), hist, reads_with
        [, kernel ms]); the two batch histograms are uint64 of shape (n_motifs, 2, VARIANT_BINS)."""
        nm = self._queued.get(("variants", slot), (0, 1))[1]
        hist = np.zeros((nm, 2, VARIANT_BINS), dtype=np.uint64)
        return self._fetch_records("variants", slot, VARIANT_DTYPE, want_ms, hist, np.zeros_like(hist))

    def intervals(self, batch, motifs, max_gap=None, min_len=None, max_intervals=None, slot=0):
        """Queue the gap-tolerant motif intervals of every read of `batch` for `motifs` (texts or Motif, at most 8) on the
        slot's stream.  max_gap / min_len: an int, a per-motif list, or None for the defaults 3 k and 4 k of each motif;
        max_intervals: the capacity of the log for this call (default: the batch's read count, at least 1)."""
        arr, nm = _motif_array(motifs)
        rules = _rule_array(arr, min(max(nm, 0), MAX_MOTIFS), max_gap, min_len)
        if max_intervals is None:
            max_intervals = max(int(batch.n_reads), 1)
        self._queue("intervals", slot, batch, arr, nm, keep=(rules,), shape=(int(max_intervals),))
        self._chk(self.lib.trew_hip_intervals(self.ctx, C.byref(batch), slot, arr, rules, nm, int(max_intervals)), "trew_hip_intervals")

    def intervals_results(self, slot=0, want_ms=False):
        """Results of the slot's last intervals: (INTERVAL_DTYPE records sorted by (read, motif, strand, start), counts of
        shape (n_reads, n_motifs, 2), found [, kernel ms]).  found > max_intervals: the records are a subset (as many as the
        log held), counts and found are exact; repeat the call with max_intervals >= found."""
        return self._fetch_log("intervals", slot, INTERVAL_DTYPE, want_ms, lambda n_reads, nm: (n_reads, nm, 2), partial=True)

    def chain(self, batch, motifs, max_events=None, slot=0):
        """Queue the ordered unit chain of every read of `batch` for `motifs` (texts or Motif, at most 8, taken as typed) on
        the slot's stream.  max_events: the capacity of the event log for this call (default: four per read, at least 1)."""
        arr, nm = _motif_array(motifs)
        if max_events is None:
            max_events = max(4 * int(batch.n_reads), 1)
        self._queue("chain", slot, batch, arr, nm, shape=(int(max_events),))
        self._chk(self.lib.trew_hip_chain(self.ctx, C.byref(batch), slot, arr, nm, int(max_events)), "trew_hip_chain")

    def chain_results(self, slot=0, want_ms=False):
        """Results of the slot's last chain: (CHAIN_DTYPE items sorted by (read, motif, strand, start), counts of shape
        (n_reads, n_motifs, 2, 2) = [read][motif][strand]{runs, variants}, n_items, n_events [, kernel ms]).  n_events >
        max_events: no items (the stored events cannot be paired), counts, n_items and n_events are exact; repeat the call
        with max_events >= n_events."""
        n_items, n_events = C.c_uint64(0), C.c_uint64(0)
        ms = C.c_float(0)
        n_reads, nm, cap = self._queued.get(("chain", slot), (0, 1, 0))
        counts = np.zeros((n_reads, nm, 2, 2), dtype=np.uint32)
        self._chk(self.lib.trew_hip_chain_results(self.ctx, slot, None, 0, C.byref(n_items), C.byref(n_events), counts.ctypes.data,
                                                  C.byref(ms) if want_ms else None), "trew_hip_chain_results")
        items, events = int(n_items.value), int(n_events.value)
        out = np.zeros(items if events <= cap else 0, dtype=CHAIN_DTYPE)
        if len(out):
            self._chk(self.lib.trew_hip_chain_results(self.ctx, slot, out.ctypes.data, len(out), C.byref(n_items), C.byref(n_events), None, None),
                      "trew_hip_chain_results")
        return (out, counts, items, events, ms.value) if want_ms else (out, counts, items, events)

    def trace(self, batch, motifs, penalty=3, min_score=24, max_items=None, max_rows=None, slot=0):
        """Queue the traceback of the wraparound alignment of every read of `batch` for `motifs` (texts or Motif, at most 8) on
        the slot's stream.  max_items: the capacity of the item log for this call (default: four per read and motif, at least
        1); max_rows: the rows of the direction workspace, 64 bytes each.  A row per base and motif always suffices and
        is the default where the lengths are known on the host (256 per read and motif for ragged device-resident batches); a
        tract whose rows do not fit costs time quadratic in its length."""
        arr, nm = _motif_array(motifs)
        max_items, max_rows = _trace_room(batch, nm, max_items, max_rows)
        self._queue("trace", slot, batch, arr, nm, shape=(int(max_items), int(max_rows)))
        self._chk(self.lib.trew_hip_trace(self.ctx, C.byref(batch), slot, arr, nm, int(penalty), int(min_score), int(max_items), int(max_rows)),
                  "trew_hip_trace")

    def trace_results(self, slot=0, want_ms=False):
        """Results of the slot's last trace: (TRACE_DTYPE items sorted by (read, motif, strand, start), counts of shape (n_reads,
        n_motifs, 2), ALIGN_DTYPE records of shape (n_reads, n_motifs), n_items, n_rows [, kernel ms]).  n_items > max_items or
        n_rows > max_rows: no items, everything else is exact; repeat the call with both at least what was reported."""
        n_items, n_rows = C.c_uint64(0), C.c_uint64(0)
        ms = C.c_float(0)
        n_reads, nm, max_items, max_rows = self._queued.get(("trace", slot), (0, 1, 0, 0))
        counts = np.zeros((n_reads, nm, 2), dtype=np.uint32)
        records = np.zeros((n_reads, nm), dtype=ALIGN_DTYPE)
        self._chk(self.lib.trew_hip_trace_results(self.ctx, slot, None, 0, C.byref(n_items), C.byref(n_rows), counts.ctypes.data, records.ctypes.data,
                                                  C.byref(ms) if want_ms else None), "trew_hip_trace_results")
        items, rows = int(n_items.value), int(n_rows.value)
        out = np.zeros(items if items <= max_items and rows <= max_rows else 0, dtype=TRACE_DTYPE)
        if len(out):
            self._chk(self.lib.trew_hip_trace_results(self.ctx, slot, out.ctypes.data, len(out), C.byref(n_items), C.byref(n_rows), None, None, None),
                      "trew_hip_trace_results")
        return (out, counts, records, items, rows, ms.value) if want_ms else (out, counts, records, items, rows)

    def copies(self, batch, monomers, penalty=3, min_score=24, max_items=None, max_rows=None, slot=0):
        """Queue `trace` for units of 3 to 256 bases: the traceback of the `monomers` alignment of every read of `batch` for
        `monomers` (texts or Monomer, at most 8) on the slot's stream.  max_items: as for trace; max_rows: the rows of the
        direction workspace, 64, 128 or 256 bytes each by the largest k of the call.  A key claims end - start rows, so two rows
        per base and monomer always suffice and are the default where the lengths are known on the host."""
        arr, nm = _monomer_array(monomers)
        max_items, max_rows = _copies_room(batch, nm, max_items, max_rows)
        self._queue("copies", slot, batch, arr, nm, shape=(int(max_items), int(max_rows)))
        self._chk(self.lib.trew_hip_copies(self.ctx, C.byref(batch), slot, arr, nm, int(penalty), int(min_score), int(max_items), int(max_rows)),
                  "trew_hip_copies")

    def copies_results(self, slot=0, want_ms=False):
        """Results of the slot's last copies: (TRACE_DTYPE items sorted by (read, monomer, strand, start), counts of shape
        (n_reads, n_monomers, 2), ALIGN_DTYPE records of shape (n_reads, n_monomers), n_items, n_rows [, kernel ms]).  n_items >
        max_items or n_rows > max_rows: no items, everything else is exact; repeat the call with both at least what was reported."""
        n_items, n_rows = C.c_uint64(0), C.c_uint64(0)
        ms = C.c_float(0)
        n_reads, nm, max_items, max_rows = self._queued.get(("copies", slot), (0, 1, 0, 0))
        counts = np.zeros((n_reads, nm, 2), dtype=np.uint32)
        records = np.zeros((n_reads, nm), dtype=ALIGN_DTYPE)
        self._chk(self.lib.trew_hip_copies_results(self.ctx, slot, None, 0, C.byref(n_items), C.byref(n_rows), counts.ctypes.data, records.ctypes.data,
                                                   C.byref(ms) if want_ms else None), "trew_hip_copies_results")
        items, rows = int(n_items.value), int(n_rows.value)
        out = np.zeros(items if items <= max_items and rows <= max_rows else 0, dtype=TRACE_DTYPE)
        if len(out):
            self._chk(self.lib.trew_hip_copies_results(self.ctx, slot, out.ctypes.data, len(out), C.byref(n_items), C.byref(n_rows), None, None, None),
                      "trew_hip_copies_results")
        return (out, counts, records, items, rows, ms.value) if want_ms else (out, counts, records, items, rows)

    def decompose(self, batch, min_period=1, max_period=32, penalty=3, min_score=24, max_items=None, max_rows=None, slot=0, candidates=1):
        """Queue refine's unit of every read of `batch`, anchored at its smallest rotation, and the traceback of the read against
        it on the slot's stream (no motifs).  max_items, max_rows: as for trace with one motif; a row has 32 bytes here.
        candidates > 1: trew_hip_decompose_resolved, resolve's record in refine's place; the results call is the same."""
        max_items, max_rows = _trace_room(batch, 1, max_items, max_rows)
        self._queue("decompose", slot, batch, None, 1, shape=(int(max_items), int(max_rows)))
        f, cand = _resolved_call(self.lib, "trew_hip_decompose", candidates)
        self._chk(f(self.ctx, C.byref(batch), slot, int(min_period), int(max_period), int(penalty), int(min_score), *cand, int(max_items), int(max_rows)),
                  f.__name__)

    def decompose_results(self, slot=0, want_ms=False):
        """Results of the slot's last decompose: (TRACE_DTYPE items sorted by (read, start), counts of shape (n_reads,),
        REFINE_DTYPE records of shape (n_reads,) with reserved = anchor, n_items, n_rows [, kernel ms]).  n_items > max_items or
        n_rows > max_rows: no items, everything else is exact; repeat the call with both at least what was reported."""
        n_items, n_rows = C.c_uint64(0), C.c_uint64(0)
        ms = C.c_float(0)
        n_reads, _, max_items, max_rows = self._queued.get(("decompose", slot), (0, 1, 0, 0))
        counts = np.zeros(n_reads, dtype=np.uint32)
        records = np.zeros(n_reads, dtype=REFINE_DTYPE)
        self._chk(self.lib.trew_hip_decompose_results(self.ctx, slot, None, 0, C.byref(n_items), C.byref(n_rows), counts.ctypes.data, records.ctypes.data,
                                                      C.byref(ms) if want_ms else None), "trew_hip_decompose_results")
        items, rows = int(n_items.value), int(n_rows.value)
        out = np.zeros(items if items <= max_items and rows <= max_rows else 0, dtype=TRACE_DTYPE)
        if len(out):
            self._chk(self.lib.trew_hip_decompose_results(self.ctx, slot, out.ctypes.data, len(out), C.byref(n_items), C.byref(n_rows), None, None, None),
                      "trew_hip_decompose_results")
        return (out, counts, records, items, rows, ms.value) if want_ms else (out, counts, records, items, rows)

    def dissect(self, batch, min_period=1, max_period=32, penalty=3, min_score=24, max_records=None, max_items=None, max_rows=None, slot=0,
                candidates=1):
        """Queue every de novo repeat tract under indels of every read of `batch`, each with its unit anchored and the traceback
        of its piece against it, on the slot's stream (no motifs).  max_records: as for tandems; max_items, max_rows: as for
        decompose.  candidates > 1: trew_hip_dissect_resolved, resolve's record of every piece in refine's place; the results
        call is the same."""
        if max_records is None:
            max_records = max(int(batch.n_reads), 1)
        max_items, max_rows = _trace_room(batch, 1, max_items, max_rows)
        self._queue("dissect", slot, batch, None, 1, shape=(int(max_records), int(max_items), int(max_rows)))
        f, cand = _resolved_call(self.lib, "trew_hip_dissect", candidates)
        self._chk(f(self.ctx, C.byref(batch), slot, int(min_period), int(max_period), int(penalty), int(min_score), *cand, int(max_records),
                    int(max_items), int(max_rows)), f.__name__)

    def dissect_results(self, slot=0, want_ms=False):
        """Results of the slot's last dissect: (TANDEM_DTYPE records sorted by (read, start) with reserved = anchor, TRACE_DTYPE
        items sorted by (read, start) with motif = the index of the item's tract in its read, counts of shape (n_reads, 2) =
        (tracts, items), n_records, n_items, n_rows [, kernel ms]).  Any of the three beyond its capacity: no records and no
        items, everything else is exact; repeat the call with all three at least what was reported."""
        nr, ni, nw = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ms = C.c_float(0)
        n_reads, _, max_records, max_items, max_rows = self._queued.get(("dissect", slot), (0, 1, 0, 0, 0))
        counts = np.zeros((n_reads, 2), dtype=np.uint32)
        self._chk(self.lib.trew_hip_dissect_results(self.ctx, slot, None, 0, None, 0, C.byref(nr), C.byref(ni), C.byref(nw), counts.ctypes.data,
                                                    C.byref(ms) if want_ms else None), "trew_hip_dissect_results")
        found, items, rows = int(nr.value), int(ni.value), int(nw.value)
        fits = found <= max_records and items <= max_items and rows <= max_rows
        recs = np.zeros(found if fits else 0, dtype=TANDEM_DTYPE)
        out = np.zeros(items if fits else 0, dtype=TRACE_DTYPE)
        if len(recs):
            self._chk(self.lib.trew_hip_dissect_results(self.ctx, slot, recs.ctypes.data, len(recs), out.ctypes.data if len(out) else None, len(out),
                                                        C.byref(nr), C.byref(ni), C.byref(nw), None, None), "trew_hip_dissect_results")
        return (recs, out, counts, found, items, rows, ms.value) if want_ms else (recs, out, counts, found, items, rows)

    def repeats(self, batch, min_period=1, max_period=32, penalty=3, min_score=24, max_records=None, slot=0):
        """Queue every de novo repeat tract of every read of `batch` on the slot's stream (no motifs).  max_records: the
        capacity of the log for this call (default: the batch's read count, at least 1)."""
        self._queue_tracts("repeats", batch, min_period, max_period, penalty, min_score, max_records, slot)

    def repeats_results(self, slot=0, want_ms=False):
        """Results of the slot's last repeats: (REPEAT_DTYPE records sorted by (read, start), counts of shape (n_reads,), found
        [, kernel ms]).  found > max_records: no records, counts and found are exact; repeat the call with max_records >=
        found."""
        return self._fetch_log("repeats", slot, REPEAT_DTYPE, want_ms)

    def tandems(self, batch, min_period=1, max_period=32, penalty=3, min_score=24, max_records=None, slot=0, candidates=1):
        """Queue every de novo repeat tract under indels of every read of `batch` on the slot's stream (no motifs).
        max_records: the capacity of the log for this call (default: the batch's read count, at least 1).  candidates > 1:
        trew_hip_tandems_resolved, resolve's record of every piece in refine's place; the results call is the same."""
        self._queue_tracts("tandems", batch, min_period, max_period, penalty, min_score, max_records, slot, candidates)

    def tandems_results(self, slot=0, want_ms=False):
        """Results of the slot's last tandems: (TANDEM_DTYPE records sorted by (read, start), counts of shape (n_reads,), found
        [, kernel ms]).  found > max_records: no records, counts and found are exact; repeat the call with max_records >=
        found."""
        return self._fetch_log("tandems", slot, TANDEM_DTYPE, want_ms)

    def satellites(self, batch, min_period=1, max_period=SATELLITE_MAX_PERIOD, penalty=3, min_score=24, max_records=None, slot=0):
        """Queue every de novo repeat tract with a period of up to 256 of every read of `batch` on the slot's stream (no
        motifs).  max_records: the capacity of the log for this call (default: the batch's read count, at least 1)."""
        self._queue_tracts("satellites", batch, min_period, max_period, penalty, min_score, max_records, slot)

    def satellites_results(self, slot=0, want_ms=False):
        """Results of the slot's last satellites: (SATELLITE_DTYPE records sorted by (read, start), counts of shape (n_reads,),
        found [, kernel ms]).  found > max_records: no records, counts and found are exact; repeat the call with max_records
        >= found."""
        return self._fetch_log("satellites", slot, SATELLITE_DTYPE, want_ms)

    def submit_reads(self, reads, slot=0):
        b = self.host_batch(*pack_reads(reads))
        self.submit(b, slot)
        return b

    # ---- results ----
    def collect_rows(self, table=-1):
        """Rows of one table (or all, table=-1) as a structured numpy array (ROW_DTYPE)."""
        n = C.c_uint64(0)
        cap = getattr(self, "_collect_cap", 1 << 16)
        while True:  # one call when the guess holds; the table tells its size when it does not
            rows = np.zeros(cap, dtype=ROW_DTYPE)
            self._chk(self.lib.trew_hip_collect(self.ctx, table, C.cast(rows.ctypes.data, C.POINTER(Row)), cap,
                                                C.byref(n)), "trew_hip_collect")
            if n.value <= cap:
                return rows[: n.value]
            cap = self._collect_cap = int(n.value) + 1024

    def collect(self):
        """The six tables as {name: {(k, word): count}}."""
        return rows_to_tables(self.collect_rows(-1))

    def reset_tables(self):
        self._chk(self.lib.trew_hip_reset_tables(self.ctx), "trew_hip_reset_tables")

    def add_rows(self, tables):
        rows = tables if isinstance(tables, np.ndarray) else tables_to_rows(tables)
        rows = np.ascontiguousarray(rows, dtype=ROW_DTYPE)
        if len(rows):
            self._chk(self.lib.trew_hip_add_rows(self.ctx, C.cast(rows.ctypes.data, C.POINTER(Row)), len(rows)),
                      "trew_hip_add_rows")

    def collect_device(self, d_rows, cap):
        """Compact every table into the device buffer d_rows (cap rows of ROW_DTYPE.itemsize bytes); returns the row count
        (which may exceed cap: nothing is written past cap then)."""
        n = C.c_uint64(0)
        self._chk(self.lib.trew_hip_collect_device(self.ctx, d_rows, cap, C.byref(n)), "trew_hip_collect_device")
        return int(n.value)

    def collect_slice_device(self, d_slice, slice_rows, consumer_stream=None, want_count=False):
        """Compact every table into rows 1.. of the exchange slice d_slice (1 + slice_rows rows) and write its header row on
        the device; the collective the caller issues on consumer_stream is ordered behind it without a host hop.  Returns the
        row count when want_count (one host synchronisation), else None."""
        n = C.c_uint64(0)
        self._chk(self.lib.trew_hip_collect_slice_device(self.ctx, d_slice, slice_rows, consumer_stream, C.byref(n) if want_count else None),
                  "trew_hip_collect_slice_device")
        return int(n.value) if want_count else None

    def add_rows_device(self, d_rows, n_rows):
        self._chk(self.lib.trew_hip_add_rows_device(self.ctx, d_rows, n_rows), "trew_hip_add_rows_device")

    def add_gathered_device(self, d_buf, n_slices, own_slice, slice_rows, producer_stream=None):
        """One kernel over the gather buffer of the table exchange (n_slices x (1 + slice_rows) rows, headers in row 0 of each
        slice): adds every slice but own_slice.  Returns the largest header count; if it exceeds slice_rows nothing was added."""
        mx = C.c_uint64(0)
        self._chk(self.lib.trew_hip_add_gathered_device(self.ctx, d_buf, n_slices, own_slice, slice_rows, producer_stream, C.byref(mx)),
                  "trew_hip_add_gathered_device")
        return int(mx.value)

    def debug_counters(self):
        """{name: count} of the kernels' rare fall-back paths since the last reset_tables (DEBUG_COUNTERS)."""
        out = (C.c_uint64 * len(DEBUG_COUNTERS))()
        self._chk(self.lib.trew_hip_debug_counters(self.ctx, out, len(DEBUG_COUNTERS)), "trew_hip_debug_counters")
        return dict(zip(DEBUG_COUNTERS, (int(x) for x in out)))

    def _debug_units(self, fn, name, slot):
        n = C.c_uint64(0)
        self._chk(fn(self.ctx, slot, None, 0, C.byref(n)), name)
        out = np.zeros(int(n.value), dtype=np.uint32)
        if len(out):
            self._chk(fn(self.ctx, slot, out.ctypes.data, len(out), C.byref(n)), name)
        return out

    def debug_worklist(self, slot=0):
        """Unit indices the prefilter of the last submit on `slot` flagged (numpy uint32, worklist order)."""
        return self._debug_units(self.lib.trew_hip_debug_worklist, "trew_hip_debug_worklist", slot)

    def debug_live_list(self, slot=0):
        """Unit indices the exact kernel of the last submit on `slot` walked (numpy uint32, its order): the worklist without the
        entries the bounds pass found dead (debug_counters()["dead_entries"])."""
        return self._debug_units(self.lib.trew_hip_debug_live_list, "trew_hip_debug_live_list", slot)

    def debug_measure_grid(self, n_reads):
        """The blocks (four waves each, a wave per read) the per-read measures' launcher starts for a batch of n_reads here."""
        blocks = C.c_uint32(0)
        self._chk(self.lib.trew_hip_debug_measure_grid(self.ctx, n_reads, C.byref(blocks)), "trew_hip_debug_measure_grid")
        return int(blocks.value)

    def merge_from(self, other):
        """Add every row of `other`'s tables (another context, same or another GPU) into this context's tables."""
        self._chk(self.lib.trew_hip_merge(self.ctx, other.ctx), "trew_hip_merge")

    def table_pressure(self):
        """(used_slots, total_slots, spilled_rows, spill_capacity) -- a snapshot."""
        v = [C.c_uint64(0) for _ in range(4)]
        self._chk(self.lib.trew_hip_table_pressure(self.ctx, *[C.byref(x) for x in v]), "trew_hip_table_pressure")
        return tuple(int(x.value) for x in v)

    def segment_results(self, n_reads, slot=0):
        kh = np.zeros(n_reads, dtype=np.int32)
        kl = np.zeros(n_reads, dtype=np.int32)
        sh = np.zeros(n_reads, dtype=np.uint64)
        sl = np.zeros(n_reads, dtype=np.uint64)
        shh = np.zeros(n_reads, dtype=np.uint64)
        slh = np.zeros(n_reads, dtype=np.uint64)
        self._chk(self.lib.trew_hip_segment_results(self.ctx, slot, kh.ctypes.data, kl.ctypes.data, sh.ctypes.data,
                                                    sl.ctypes.data, shh.ctypes.data, slh.ctypes.data, n_reads),
                  "trew_hip_segment_results")
        # words as Python ints (hi << 64 | lo)
        seq_h = [(int(a) << 64) | int(b) for a, b in zip(shh, sh)]
        seq_l = [(int(a) << 64) | int(b) for a, b in zip(slh, sl)]
        return kh, kl, seq_h, seq_l

    def filter_masks(self, batch, slots_per_read):
        units = batch.n_reads // 2 if self.mode == MODE_PAIR else batch.n_reads
        cand = np.zeros(max(1, units * slots_per_read), dtype=np.uint64)
        self._chk(self.lib.trew_hip_filter_masks(self.ctx, C.byref(batch), cand.ctypes.data, slots_per_read),
                  "trew_hip_filter_masks")
        return cand[: units * slots_per_read].reshape(units, slots_per_read)

    def last_timing(self, slot=0, want_flagged=True):
        a, b, n = C.c_float(), C.c_float(), C.c_uint64()
        self._chk(self.lib.trew_hip_last_timing(self.ctx, slot, C.byref(a), C.byref(b), C.byref(n) if want_flagged else None),
                  "trew_hip_last_timing")
        return a.value, b.value, n.value

    # ---- device memory ----
    def malloc(self, nbytes):
        p = C.c_void_p()
        self._chk(self.lib.trew_hip_malloc(self.ctx, nbytes, C.byref(p)), "trew_hip_malloc")
        return p.value

    def free(self, ptr):
        self._chk(self.lib.trew_hip_free(self.ctx, ptr), "trew_hip_free")

    def d2h(self, ptr, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        self._chk(self.lib.trew_hip_memcpy_d2h(self.ctx, out.ctypes.data, ptr, nbytes), "trew_hip_memcpy_d2h")
        return out

    def synth_short_device(self, seed, first_read, n_reads, read_len, d_words):
        self._chk(self.lib.trew_synth_short_device(self.ctx, seed, first_read, n_reads, read_len, d_words),
                  "trew_synth_short_device")

    def synth_long_device(self, seed, first_read, n_reads):
        """Generate long reads on the device: returns (batch, device pointers to free)."""
        lens = synth_long_lengths(seed, first_read, n_reads)
        nw = 3 * ((lens.astype(np.int64) + 31) // 32)
        offs = np.zeros(n_reads, dtype=np.int64)
        offs[1:] = np.cumsum(nw[:-1])
        total = int(offs[-1] + nw[-1]) if n_reads else 0
        if total >= 2 ** 32:
            raise TrewHipError("long batch exceeds 2^32 words")
        offs32 = offs.astype(np.uint32)
        d_words = self.malloc(total * 4 + 64)
        d_offs = self.malloc(n_reads * 4)
        d_lens = self.malloc(n_reads * 4)
        self._chk(self.lib.trew_hip_memcpy_h2d(self.ctx, d_offs, offs32.ctypes.data, n_reads * 4), "h2d")
        self._chk(self.lib.trew_hip_memcpy_h2d(self.ctx, d_lens, lens.ctypes.data, n_reads * 4), "h2d")
        self._chk(self.lib.trew_synth_long_device(self.ctx, seed, first_read, n_reads, d_offs, d_words), "trew_synth_long_device")
        b = Batch(d_words, total, d_offs, d_lens, 0, 0, n_reads, 1, int(lens.max()) if n_reads else 0)
        return b, (d_words, d_offs, d_lens), int(lens.astype(np.int64).sum())

    def synth_pair_device(self, seed, first_pair, n_pairs, read_len, d_words):
        self._chk(self.lib.trew_synth_pair_device(self.ctx, seed, first_pair, n_pairs, read_len, d_words),
                  "trew_synth_pair_device")


def k_mer_check(seq, min_mer=5, max_mer=32, low=0.5, high=0.8, flags=0, device=0):
    """k_mer_check (kmer.h:232-236) on the GPU for one segment; same result shape as the oracle's segment_check."""
    if isinstance(seq, str):
        seq = seq.encode()
    with TrewHip(mode=MODE_SEGMENT, min_mer=min_mer, max_mer=max_mer, low=low, high=high, device=device, n_slots=1,
                 max_batch_words=1 << 12, max_batch_reads=16, table_log2_slots=14, flags=flags) as t:
        t.submit_reads([seq])
        t.wait()
        kh, kl, sh, sl = t.segment_results(1)
        tabs = t.collect()
    return dict(k_high=int(kh[0]), k_low=int(kl[0]), seq_high=int(sh[0]), seq_low=int(sl[0]),
                hist_high=tabs["forward_high"], hist_low=tabs["forward_low"])


def _one_batch(reads, device):
    """(a context sized for `reads`, their batch) of the one-shot wrappers below; the caller closes the context"""
    words, offsets, lengths = pack_reads(reads)
    t = TrewHip(mode=MODE_SEGMENT, device=device, n_slots=1, max_batch_words=max(len(words), 1 << 12),
                max_batch_reads=max(len(offsets), 16), table_log2_slots=12)
    return t, t.host_batch(words, offsets, lengths)


def _fetch_with_retry(queue, fetch, room, found_at):
    """queue(*room) and fetch(); when what the call found -- fetch()[i] for i in found_at, exact also when it did not fit --
    exceeds `room`, once more with the larger of the two, which always suffices.  Returns what the last fetch returned."""
    queue(*room)
    res = fetch()
    need = tuple(res[i] for i in found_at)
    if any(n > r for n, r in zip(need, room)):
        queue(*(max(n, r) for n, r in zip(need, room)))
        res = fetch()
    return res


def annotate(reads, motifs, device=0):
    """Per-read motif annotation on the GPU: for every read (bytes / str) and motif (text) the matching windows and the
    longest tract on each strand, as ANNOT_DTYPE records of shape (n_reads, n_motifs)."""
    t, b = _one_batch(reads, device)
    with t:
        t.annotate(b, motifs)
        return t.annotate_results()


def tracts(reads, motifs, penalty=3, device=0):
    """Error-tolerant terminal motif tracts on the GPU: for every read (bytes / str) and motif (text) the covered bases and
    the head (5') and tail (3') tract on each strand, as TRACT_DTYPE records of shape (n_reads, n_motifs)."""
    t, b = _one_batch(reads, device)
    with t:
        t.tracts(b, motifs, penalty)
        return t.tracts_results()


def align(reads, motifs, penalty=3, device=0):
    """Indel-aware motif tracts on the GPU: for every read (bytes / str) and motif (text) the best local alignment against the
    motif repeated without end on each strand -- score, start, end, motif bases consumed and matches -- as ALIGN_DTYPE records
    of shape (n_reads, n_motifs); align_columns gives the copies, mismatches, insertions and deletions."""
    t, b = _one_batch(reads, device)
    with t:
        t.align(b, motifs, penalty)
        return t.align_results()


def monomers(reads, monomers, penalty=3, device=0):
    """`align` for units of 3 to 256 bases on the GPU (satellite monomers in noisy reads): for every read (bytes / str) and
    monomer (text) the best local alignment against the monomer repeated without end on each strand, as ALIGN_DTYPE records of
    shape (n_reads, n_monomers); align_columns with k = the monomer's length gives the copies and the error split.  Use a
    penalty of 2 or more: at 1 a random read scores over its whole length against a long unit."""
    t, b = _one_batch(reads, device)
    with t:
        t.monomers(b, monomers, penalty)
        return t.monomers_results()


def periods(reads, min_period=1, max_period=32, penalty=3, min_score=24, device=0):
    """De novo repeat period and unit on the GPU: for every read (bytes / str) the period, the consensus unit and the
    position of its best-scoring repeat tract, as PERIOD_DTYPE records of shape (n_reads,); no motif is given."""
    t, b = _one_batch(reads, device)
    with t:
        t.periods(b, min_period, max_period, penalty, min_score)
        return t.periods_results()


def refine(reads, min_period=1, max_period=32, penalty=3, min_score=24, device=0):
    """De novo repeats under indels on the GPU: for every read (bytes / str) the period and tract of `periods`, a seed unit
    taken from the read, the wraparound alignment against it and the unit re-voted from that alignment -- unit, tract, motif
    bases consumed and matches -- as REFINE_DTYPE records of shape (n_reads,); refine_columns gives the copies, mismatches,
    insertions and deletions.  No motif is given."""
    t, b = _one_batch(reads, device)
    with t:
        t.refine(b, min_period, max_period, penalty, min_score)
        return t.refine_results()


def polish(reads, min_period=1, max_period=POLISH_MAX_PERIOD, penalty=3, min_score=24, device=0):
    """`refine` for periods up to 256 on the GPU: for every read (bytes / str) the period and tract of `satellites`' depth-0
    record, a seed unit taken from the read, the wraparound alignment of `monomers` against it and the unit re-voted from that
    alignment, as POLISH_DTYPE records of shape (n_reads,); refine_columns gives the copies, mismatches, insertions and
    deletions, capi.satellite_unit_text the two units.  No motif is given."""
    t, b = _one_batch(reads, device)
    with t:
        t.polish(b, min_period, max_period, penalty, min_score)
        return t.polish_results()


def resolve(reads, min_period=1, max_period=32, penalty=3, min_score=24, candidates=3, device=0):
    """`refine` with the period chosen by alignment on the GPU: for every read (bytes / str) the `candidates` (1 .. 4)
    best-scoring periods of `periods`' score are each refined as `refine` refines its one, and the record with the largest
    final score is kept -- RESOLVE_DTYPE records of shape (n_reads,): a REFINE_DTYPE record, then candidates, rank (0: what
    `refine` reports), first_period and first_score (of `refine`'s record).  No motif is given."""
    t, b = _one_batch(reads, device)
    with t:
        t.resolve(b, min_period, max_period, penalty, min_score, candidates)
        return t.resolve_results()


def variants(reads, motifs, device=0):
    """In-phase variant units on the GPU: for every read (bytes / str) and motif (text, taken as typed) the exact units, the
    anchored units with one substituted base and the commonest substitution on each strand, and the histogram of the
    substitutions over all reads.  Returns (VARIANT_DTYPE records of shape (n_reads, n_motifs), hist, reads_with)."""
    t, b = _one_batch(reads, device)
    with t:
        t.variants(b, motifs)
        return t.variants_results()


def intervals(reads, motifs, max_gap=None, min_len=None, device=0, max_intervals=None):
    """Gap-tolerant motif intervals on the GPU: for every read (bytes / str) and motif (text) the intervals of covered bases
    whose gaps are at most max_gap bases and whose length is at least min_len (defaults: 3 k and 4 k of each motif), on each
    strand.  Returns (INTERVAL_DTYPE records sorted by (read, motif, strand, start), counts of shape (n_reads, n_motifs, 2)).
    The first call's log holds max_intervals records (default: one per read); when more are found the call is repeated once
    with the exact number."""
    t, b = _one_batch(reads, device)
    with t:
        room = (max(int(b.n_reads), 1) if max_intervals is None else int(max_intervals),)
        return _fetch_with_retry(lambda cap: t.intervals(b, motifs, max_gap, min_len, cap), t.intervals_results, room, (2,))[:2]


def chain(reads, motifs, device=0, max_events=None):
    """Ordered unit chain on the GPU: for every read (bytes / str) and motif (text, taken as typed) the maximal in-phase runs
    of exact units and every anchored unit with one substituted base, in place, on each strand.  Returns (CHAIN_DTYPE items
    sorted by (read, motif, strand, start), counts of shape (n_reads, n_motifs, 2, 2) = [read][motif][strand]{runs,
    variants}).  The first call's log holds max_events events (default: four per read); when more are found the call is
    repeated once with the exact number."""
    t, b = _one_batch(reads, device)
    with t:
        room = (max(4 * int(b.n_reads), 1) if max_events is None else int(max_events),)
        return _fetch_with_retry(lambda cap: t.chain(b, motifs, cap), t.chain_results, room, (3,))[:2]


def trace(reads, motifs, penalty=3, min_score=24, device=0, max_items=None, max_rows=None):
    """Units in place under indels on the GPU: for every read (bytes / str) and motif (text) the traceback of `align`'s
    wraparound alignment on each strand whose score reaches min_score, cut into copies of the motif -- runs of complete exact
    copies, copies with their substitutions, insertions and deletions, and the end pieces, in place.  Returns (TRACE_DTYPE items
    sorted by (read, motif, strand, start), counts of shape (n_reads, n_motifs, 2), ALIGN_DTYPE records of shape (n_reads,
    n_motifs)); trace_signature turns a key's items into text.  The first call's log and workspace hold max_items items
    and max_rows rows (defaults: TrewHip.trace's; its max_rows, a row per base and motif, always suffices); when more are found
    the call is repeated once with the exact numbers."""
    t, b = _one_batch(reads, device)
    with t:
        room = _trace_room(b, _motif_array(motifs)[1], max_items, max_rows)
        return _fetch_with_retry(lambda items, rows: t.trace(b, motifs, penalty, min_score, items, rows), t.trace_results, room, (3, 4))[:3]


def copies(reads, monomers, penalty=3, min_score=24, device=0, max_items=None, max_rows=None):
    """`trace` for units of 3 to 256 bases on the GPU (the monomer decomposition of a satellite array): for every read (bytes /
    str) and monomer (text) the traceback of `monomers`' alignment on each strand whose score reaches min_score, cut into copies
    of the monomer.  Returns (TRACE_DTYPE items sorted by (read, monomer, strand, start), counts of shape (n_reads, n_monomers,
    2), ALIGN_DTYPE records of shape (n_reads, n_monomers)); copies_signature turns a key's items into text.  The first
    call's log and workspace hold max_items items and max_rows rows (defaults: TrewHip.copies'); when more are found the call
    is repeated once with the exact numbers."""
    t, b = _one_batch(reads, device)
    with t:
        room = _copies_room(b, _monomer_array(monomers)[1], max_items, max_rows)
        return _fetch_with_retry(lambda items, rows: t.copies(b, monomers, penalty, min_score, items, rows), t.copies_results, room, (3, 4))[:3]


def decompose(reads, min_period=1, max_period=32, penalty=3, min_score=24, device=0, max_items=None, max_rows=None, candidates=1):
    """Units in place with no motif given on the GPU: for every read (bytes / str) `refine`'s record, its unit turned to its
    smallest rotation (the record's `reserved` word is the anchor; decompose_anchor gives the rotation) and, when the score
    reaches min_score, the traceback of the read against it cut into copies -- `trace`'s items for that unit, in read
    orientation.  Returns (TRACE_DTYPE items sorted by (read, start), counts of shape (n_reads,), REFINE_DTYPE records of shape
    (n_reads,)); trace_signature turns a read's items into text with k = period.  The first call's log and workspace hold
    max_items items and max_rows rows (defaults: TrewHip.trace's for one motif); when more are found the call is repeated once
    with the exact numbers.  candidates > 1 (at most 4): `resolve`'s record with that many candidates in `refine`'s place."""
    t, b = _one_batch(reads, device)
    with t:
        room = _trace_room(b, 1, max_items, max_rows)
        return _fetch_with_retry(lambda items, rows: t.decompose(b, min_period, max_period, penalty, min_score, items, rows, candidates=candidates), t.decompose_results, room,
                                 (3, 4))[:3]


def dissect(reads, min_period=1, max_period=32, penalty=3, min_score=24, device=0, max_records=None, max_items=None, max_rows=None, candidates=1):
    """Units in place for every tract of a read with no motif given on the GPU: `tandems`' records of every read (bytes / str),
    each with its unit turned to its smallest rotation (`reserved` is the anchor; decompose_anchor gives the rotation), and for
    every record `decompose`'s items of its piece, in read coordinates.  Returns (TANDEM_DTYPE records sorted by (read, start),
    TRACE_DTYPE items sorted by (read, start) with motif = the index of the item's tract in its read, counts of shape (n_reads,
    2) = (tracts, items)); trace_signature turns a tract's items into text with k = period, tandem_columns gives a record's
    columns.  The first call's logs and workspace hold max_records records, max_items items and max_rows rows (defaults:
    TrewHip.dissect's); when more are found the call is repeated once with the exact numbers.  candidates > 1 (at most 4): every
    piece gets `resolve`'s record with that many candidates in `refine`'s place."""
    t, b = _one_batch(reads, device)
    with t:
        room = (max(int(b.n_reads), 1) if max_records is None else int(max_records),) + _trace_room(b, 1, max_items, max_rows)
        return _fetch_with_retry(lambda recs, items, rows: t.dissect(b, min_period, max_period, penalty, min_score, recs, items, rows, candidates=candidates), t.dissect_results,
                                 room, (3, 4, 5))[:3]


def repeats(reads, min_period=1, max_period=32, penalty=3, min_score=24, device=0, max_records=None):
    """Every de novo repeat tract on the GPU: for every read (bytes / str) the period, the consensus unit and the position of
    its best-scoring tract (depth 0, the record of `periods`) and, in the same way, of what lies in front of it and behind it,
    until nothing scores min_score.  Returns (REPEAT_DTYPE records sorted by (read, start), counts of shape (n_reads,)).  The
    first call's log holds max_records records (default: one per read); when more are found the call is repeated once with
    the exact number."""
    t, b = _one_batch(reads, device)
    with t:
        room = (max(int(b.n_reads), 1) if max_records is None else int(max_records),)
        return _fetch_with_retry(lambda cap: t.repeats(b, min_period, max_period, penalty, min_score, cap), t.repeats_results, room, (2,))[:2]


def tandems(reads, min_period=1, max_period=32, penalty=3, min_score=24, device=0, max_records=None, candidates=1):
    """Every de novo repeat tract under indels on the GPU: for every read (bytes / str) what `refine` gives it (depth 0) and, in
    the same way, what it gives the bases in front of that tract and behind it, each piece a read of its own, until nothing
    repeats; a piece whose refined score stays below min_score gives no record and is searched around its `periods` tract.
    Returns (TANDEM_DTYPE records sorted by (read, start), counts of shape (n_reads,)); tandem_columns gives the copies,
    mismatches, insertions and deletions.  The first call's log holds max_records records (default: one per read); when more
    are found the call is repeated once with the exact number.  candidates > 1 (at most 4): every piece gets `resolve`'s record
    with that many candidates in `refine`'s place (`rank` and `first_period` are not reported here)."""
    t, b = _one_batch(reads, device)
    with t:
        room = (max(int(b.n_reads), 1) if max_records is None else int(max_records),)
        return _fetch_with_retry(lambda cap: t.tandems(b, min_period, max_period, penalty, min_score, cap, candidates=candidates), t.tandems_results, room, (2,))[:2]


def satellites(reads, min_period=1, max_period=SATELLITE_MAX_PERIOD, penalty=3, min_score=24, device=0, max_records=None):
    """`repeats` with periods up to 256 on the GPU: minisatellites and satellite monomers.  Returns (SATELLITE_DTYPE records
    sorted by (read, start), counts of shape (n_reads,)); satellite_unit_text turns a record's unit into text.  The first
    call's log holds max_records records (default: one per read); when more are found the call is repeated once with the
    exact number."""
    t, b = _one_batch(reads, device)
    with t:
        room = (max(int(b.n_reads), 1) if max_records is None else int(max_records),)
        return _fetch_with_retry(lambda cap: t.satellites(b, min_period, max_period, penalty, min_score, cap), t.satellites_results, room, (2,))[:2]
