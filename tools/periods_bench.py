#!/usr/bin/env python3
"""Timing of trew_hip_periods next to its yardstick, tracts_wave_kernel on TTAGGG, on the same device-resident batches
(HIP events through ms_kernel, one stream, one process, the two kernels alternating launch by launch).

    python tools/periods_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases) and per period range (1 .. 32 and 6 .. 6):
  <batch>_periods_<lo>_<hi>_ms / <batch>_tracts_<lo>_<hi>_ms   the kernel and its yardstick, taking turns
  <batch>_periods_<lo>_<hi>_over_tracts                        their ratio (nothing is predicted: neither has been measured on this work)
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
RANGES = ((1, 32), (6, 6))


def ms_only(t, results):
    """kernel time of the slot's last call without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), "results")
    return ms.value


def alternate(t, batch, lo, hi, penalty, warmup, launches):
    """(tracts ms, periods ms): the two kernels take turns on one stream"""
    for _ in range(warmup):
        t.tracts(batch, ["TTAGGG"], penalty)
        t.periods(batch, lo, hi, penalty)
    t.wait(0)
    a = b = 0.0
    for _ in range(launches):
        t.tracts(batch, ["TTAGGG"], penalty)
        a += ms_only(t, t.lib.trew_hip_tracts_results)
        t.periods(batch, lo, hi, penalty)
        b += ms_only(t, t.lib.trew_hip_periods_results)
    return a / launches, b / launches


def rows(res, name, t, batch, a):
    for lo, hi in RANGES:
        tr, pe = alternate(t, batch, lo, hi, a.penalty, a.warmup, a.launches)
        key = "%s_%%s_%d_%d" % (name, lo, hi)
        res[key % "tracts" + "_ms"] = round(tr, 4)
        res[key % "periods" + "_ms"] = round(pe, 4)
        res[key % "periods" + "_over_tracts"] = round(pe / tr, 2)


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
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty}

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            rows(res, "long", t, b, a)
            for p in ptrs:
                t.free(p)
        res.update(long_reads=a.long_reads, long_bases=bases)

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(SEED, 0, n, L, d)
            rows(res, "short", t, t.device_uniform_batch(d, n, L), a)
            t.free(d)
        res.update(short_reads=n, short_len=L)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
