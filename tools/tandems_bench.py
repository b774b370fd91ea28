#!/usr/bin/env python3
"""Timing of trew_hip_tandems next to the two kernels it joins, refine_wave_kernel (the work of one piece: what the parent of
this measure costs for depth 0 alone) and repeats_wave_kernel (the same recursion with the periods record per piece), on the
same device-resident batch (HIP events through ms_kernel, one stream, one process, the three kernels alternating launch by
launch).  `tandems` runs refine's work once for the read and once for every piece below it that may hold a periods record.

    python tools/tandems_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3]
                                  [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases):
  <batch>_<kernel>_ms / _spread      mean of --launches launches, (largest - smallest) / mean; kernel: refine, repeats, tandems
  <batch>_tandems_over_refine        tandems / refine
  <batch>_tandems_over_repeats       tandems / repeats
  <batch>_bases                      bases of the batch
  <batch>_refine_records             reads whose refine record reaches the minimum score (the depth-0 records of tandems)
  <batch>_repeats_records, <batch>_tandems_records   records in the two logs
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trew_amd as T  # noqa: E402

SEED = 20250218
MIN_SCORE = 24


def kernel_ms(t, measure, log):
    """kernel time of the slot's last call of `measure` without copying the records back; also the number of records"""
    n, ms = C.c_uint64(0), C.c_float(0)
    what = "trew_hip_%s_results" % measure
    if log:
        t._chk(getattr(t.lib, what)(t.ctx, 0, None, 0, C.byref(n), None, C.byref(ms)), what)
    else:
        t._chk(getattr(t.lib, what)(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), what)
    return ms.value, int(n.value)


def rows(res, name, t, batch, n_reads, bases, a):
    times = {"refine": [], "repeats": [], "tandems": []}
    cap = 4 * n_reads  # the logs: large enough for both here (the counters say so below)
    found = {}
    for i in range(a.warmup + a.launches):
        t.refine(batch, 1, 32, a.penalty, MIN_SCORE)
        ms_f, _ = kernel_ms(t, "refine", False)
        t.repeats(batch, 1, 32, a.penalty, MIN_SCORE, max_records=cap)
        ms_r, found["repeats"] = kernel_ms(t, "repeats", True)
        t.tandems(batch, 1, 32, a.penalty, MIN_SCORE, max_records=cap)
        ms_t, found["tandems"] = kernel_ms(t, "tandems", True)
        if i >= a.warmup:
            times["refine"].append(ms_f)
            times["repeats"].append(ms_r)
            times["tandems"].append(ms_t)
    for k, v in times.items():
        res["%s_%s_ms" % (name, k)] = round(float(np.mean(v)), 4)
        res["%s_%s_spread" % (name, k)] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
    res[name + "_tandems_over_refine"] = round(float(np.mean(times["tandems"])) / float(np.mean(times["refine"])), 3)
    res[name + "_tandems_over_repeats"] = round(float(np.mean(times["tandems"])) / float(np.mean(times["repeats"])), 3)
    res[name + "_bases"] = int(bases)
    res[name + "_refine_records"] = int((t.refine_results()["score"] >= MIN_SCORE).sum())
    for k, v in found.items():
        res["%s_%s_records" % (name, k)] = v
    res[name + "_log_capacity"] = cap


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "min_score": MIN_SCORE}

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            rows(res, "long", t, b, a.long_reads, bases, a)
            for p in ptrs:
                t.free(p)
        res.update(long_reads=a.long_reads)

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(SEED, 0, n, L, d)
            rows(res, "short", t, t.device_uniform_batch(d, n, L), n, n * L, a)
            t.free(d)
        res.update(short_reads=n, short_len=L)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
