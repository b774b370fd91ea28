#!/usr/bin/env python3
"""Timing of trew_hip_annotate next to the prefilter on the same device-resident batch (HIP events, one stream).

    python tools/annot_bench.py [--reads 10000000] [--len 150] [--warmup 5] [--launches 50] [--long_reads 20000] [--out FILE]

Prints one JSON object:
  prefilter_ms        ms_filter of trew_hip_last_timing on a one-slot context (no other kernel shares the chip)
  annotate_ms         one motif (TTAGGG), lane per read        annotate_over_prefilter = their ratio
  annotate_8_ms       eight motifs (k = 3, 4, 5, 6, 7, 12, 31, 32) on the same batch
  annotate_wave_ms    one motif, the same batch through the wave-per-read kernel (TREW_FLAG_DEBUG_ANNOT_GENERAL)
  long_ms_per_mreads  one motif on --long_reads reads of the long-read generator, ms per million reads, and Gbases/s
Every figure is the mean of --launches launches after --warmup.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trew_amd as T  # noqa: E402

SEED = 20250218
EIGHT = ["AAT", "TGTG", "CCCTA", "TTAGGG", "GGGTTAG", "TTAGGGTTAGGC", "TTTTGCCCTCATCACACCCTCGCCTCCTTCG", "TTTTGCCCTCATCACACCCTCGCCTCCTTCGC"]


def mean_annotate(t, batch, motifs, warmup, launches):
    for _ in range(warmup):
        t.annotate(batch, motifs)
    t.wait(0)
    total = 0.0
    for _ in range(launches):
        t.annotate(batch, motifs)
        total += annotate_ms_only(t)
    return total / launches


def annotate_ms_only(t):
    """kernel time of the slot's last annotate without copying the records back"""
    import ctypes as C

    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_annotate_results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), "trew_hip_annotate_results")
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = a.reads, a.len
    stride = 3 * ((L + 31) // 32)
    res = {"reads": n, "read_len": L, "warmup": a.warmup, "launches": a.launches}

    with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=22) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(SEED, 0, n, L, d)
        b = t.device_uniform_batch(d, n, L)
        for _ in range(a.warmup):
            t.submit(b)
        t.wait()
        t.last_timing(0, want_flagged=False)
        for _ in range(a.launches):
            t.submit(b)
        t.wait()
        ms_f, ms_e, _ = t.last_timing(0, want_flagged=False)
        res["prefilter_ms"] = round(ms_f, 4)
        res["exact_ms"] = round(ms_e, 4)
        res["annotate_ms"] = round(mean_annotate(t, b, ["TTAGGG"], a.warmup, a.launches), 4)
        res["annotate_over_prefilter"] = round(res["annotate_ms"] / res["prefilter_ms"], 3)
        res["annotate_8_ms"] = round(mean_annotate(t, b, EIGHT, a.warmup, a.launches), 4)
        t.free(d)

    with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12,
                   flags=T.FLAG_DEBUG_ANNOT_GENERAL) as t:
        d = t.malloc(n * stride * 4 + 64)
        t.synth_short_device(SEED, 0, n, L, d)
        b = t.device_uniform_batch(d, n, L)
        res["annotate_wave_ms"] = round(mean_annotate(t, b, ["TTAGGG"], a.warmup, a.launches), 4)
        t.free(d)

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            ms = mean_annotate(t, b, ["TTAGGG"], a.warmup, a.launches)
            for p in ptrs:
                t.free(p)
        res["long_reads"] = a.long_reads
        res["long_bases"] = bases
        res["long_ms"] = round(ms, 4)
        res["long_ms_per_mreads"] = round(ms / a.long_reads * 1e6, 3)
        res["long_gbases_per_s"] = round(bases / ms / 1e6, 2)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
