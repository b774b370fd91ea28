#!/usr/bin/env python3
"""Timing of trew_hip_tracts next to its yardstick, annotate's wave-per-read kernel, on the same device-resident batches
(HIP events, one stream, one process, the two kernels alternating launch by launch).

    python tools/tracts_bench.py [--long_reads 20000] [--reads 10000000] [--len 150] [--warmup 5] [--launches 50] [--penalty 3] [--out FILE]

Prints one JSON object:
  long_annotate_wave_ms / long_tracts_ms   one motif (TTAGGG) on --long_reads reads of the long-read generator
  long_tracts_over_annotate                their ratio (the design predicts about 2)
  long_tracts_8_ms / long_annotate_8_ms    eight motifs (k = 3, 4, 5, 6, 7, 12, 31, 32) on the same batch
  short_tracts_ms / short_annotate_wave_ms / short_annotate_lane_ms
                                           --reads uniform reads of --len bases through the same kernels (lanes idle in
                                           the wave-per-read kernels) and through annotate's lane-per-read kernel
Every figure is the mean of --launches launches after --warmup.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trew_amd as T  # noqa: E402

SEED = 20250218
EIGHT = ["AAT", "TGTG", "CCCTA", "TTAGGG", "GGGTTAG", "TTAGGGTTAGGC", "TTTTGCCCTCATCACACCCTCGCCTCCTTCG", "TTTTGCCCTCATCACACCCTCGCCTCCTTCGC"]


def ms_only(t, results):
    """kernel time of the slot's last call without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), "results")
    return ms.value


def alternate(t, batch, motifs, penalty, warmup, launches):
    """(annotate ms, tracts ms): the two kernels take turns on one stream"""
    for _ in range(warmup):
        t.annotate(batch, motifs)
        t.tracts(batch, motifs, penalty)
    t.wait(0)
    a = b = 0.0
    for _ in range(launches):
        t.annotate(batch, motifs)
        a += ms_only(t, t.lib.trew_hip_annotate_results)
        t.tracts(batch, motifs, penalty)
        b += ms_only(t, t.lib.trew_hip_tracts_results)
    return a / launches, b / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty}

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12,
                       flags=T.FLAG_DEBUG_ANNOT_GENERAL) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            an, tr = alternate(t, b, ["TTAGGG"], a.penalty, a.warmup, a.launches)
            an8, tr8 = alternate(t, b, EIGHT, a.penalty, a.warmup, a.launches)
            for p in ptrs:
                t.free(p)
        res.update(long_reads=a.long_reads, long_bases=bases, long_annotate_wave_ms=round(an, 4), long_tracts_ms=round(tr, 4),
                   long_tracts_over_annotate=round(tr / an, 3), long_tracts_gbases_per_s=round(bases / tr / 1e6, 2),
                   long_annotate_8_ms=round(an8, 4), long_tracts_8_ms=round(tr8, 4), long_tracts_8_over_annotate_8=round(tr8 / an8, 3))

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        for name, flags in (("wave", T.FLAG_DEBUG_ANNOT_GENERAL), ("lane", 0)):
            with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12, flags=flags) as t:
                d = t.malloc(n * stride * 4 + 64)
                t.synth_short_device(SEED, 0, n, L, d)
                an, tr = alternate(t, t.device_uniform_batch(d, n, L), ["TTAGGG"], a.penalty, a.warmup, a.launches)
                t.free(d)
            res["short_annotate_%s_ms" % name] = round(an, 4)
            if name == "wave":
                res["short_tracts_ms"] = round(tr, 4)
        res.update(short_reads=n, short_len=L, short_tracts_over_annotate_wave=round(res["short_tracts_ms"] / res["short_annotate_wave_ms"], 3),
                   short_tracts_mreads_per_s=round(n / res["short_tracts_ms"] / 1e3, 1))

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
