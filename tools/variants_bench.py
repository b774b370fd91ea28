#!/usr/bin/env python3
"""Timing of trew_hip_variants next to trew_hip_intervals on the same device-resident batches (HIP events, one stream, one
process, the two kernels alternating launch by launch).

    python tools/variants_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 5] [--launches 30] [--out FILE]

Three motif sets: TTAGGG alone, eight motifs (k = 3 .. 32) and one k = 32 motif; intervals under its default rule.  Prints
one JSON object with, per batch (long / short) and motif set (one / eight / k32):
  <batch>_<set>_variants_ms / _intervals_ms     kernel time from ms_kernel, the mean of --launches launches after --warmup
  <batch>_<set>_variants_over_intervals         their ratio
  <batch>_<set>_units / _variants / _bins       exact units, anchored variants (= LDS atomics) and non-zero (read, motif,
                                                strand, bin) entries (= pairs of 64-bit global atomics) of one launch
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import trew_amd as T  # noqa: E402

SEED = 20250218
SETS = {
    "one": ["TTAGGG"],
    "eight": ["AAT", "ACGTT", "TTAGGG", "AAATTT", "TTAGGGC", "TTAGGGTTAGGGTCAG", "ACGTTGCATGCCATGGTTAACCGATCGATTA", "ACGTTGCATGCCATGGTTAACCGATCGATTAG"],
    "k32": ["TTAGGGTTAGGGTTAGGGTTAGGGTTAGGGTT"],
}


def variants_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_variants_results(t.ctx, 0, None, 0, C.byref(n), None, None, C.byref(ms)), "trew_hip_variants_results")
    return ms.value


def intervals_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_intervals_results(t.ctx, 0, None, 0, C.byref(n), None, C.byref(ms)), "trew_hip_intervals_results")
    return ms.value, int(n.value)


def alternate(t, batch, motifs, warmup, launches):
    t.intervals(batch, motifs, None, None, 1)
    cap = max(intervals_ms(t)[1], 1)
    t.variants(batch, motifs)
    rec, hist, reads_with = t.variants_results()
    work = {"units": int(rec["units_fwd"].astype(np.uint64).sum() + rec["units_rev"].astype(np.uint64).sum()), "variants": int(hist.sum()),
            "bins": int(reads_with.sum())}
    del rec
    for _ in range(warmup):
        t.intervals(batch, motifs, None, None, cap)
        t.variants(batch, motifs)
    t.wait(0)
    a = b = 0.0
    for _ in range(launches):
        t.intervals(batch, motifs, None, None, cap)
        a += intervals_ms(t)[0]
        t.variants(batch, motifs)
        b += variants_ms(t)
    return a / launches, b / launches, work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches}

    def record(prefix, iv, va, work):
        res.update({prefix + "_intervals_ms": round(iv, 4), prefix + "_variants_ms": round(va, 4), prefix + "_variants_over_intervals": round(va / iv, 3)})
        res.update({prefix + "_" + k: v for k, v in work.items()})

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            res.update(long_reads=a.long_reads, long_bases=bases)
            for name, motifs in SETS.items():
                record("long_" + name, *alternate(t, b, motifs, a.warmup, a.launches))
            for p in ptrs:
                t.free(p)

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(SEED, 0, n, L, d)
            b = t.device_uniform_batch(d, n, L)
            res.update(short_reads=n, short_len=L)
            for name, motifs in SETS.items():
                record("short_" + name, *alternate(t, b, motifs, a.warmup, a.launches))
            t.free(d)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
