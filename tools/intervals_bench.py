#!/usr/bin/env python3
"""Timing of trew_hip_intervals next to its yardstick, the tracts kernel, on the same device-resident batches (HIP events,
one stream, one process, the two kernels alternating launch by launch).

    python tools/intervals_bench.py [--long_reads 20000] [--reads 10000000] [--len 150] [--warmup 5] [--launches 50] [--out FILE]

One motif (TTAGGG) under the default rule (max_gap 3 k, min_len 4 k) and penalty 3.  Prints one JSON object:
  long_tracts_ms / long_intervals_ms        --long_reads reads of the long-read generator
  long_intervals_over_tracts                their ratio
  long_intervals_found / long_appends       kept intervals = atomic appends of one launch (every kept interval is one)
  short_tracts_ms / short_intervals_ms ...  --reads uniform reads of --len bases through the same wave-per-read kernels
  *_minlen1_*                               the same batch with min_len 1: every chance interval is kept and appended
Every figure is the mean of --launches launches after --warmup.  The log holds every interval (a first launch measures how
many there are), so no launch overflows.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trew_amd as T  # noqa: E402

SEED = 20250218
MOTIF = ["TTAGGG"]


def tracts_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_tracts_results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), "trew_hip_tracts_results")
    return ms.value


def intervals_ms(t):
    """(kernel ms, intervals found) of the slot's last call without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_intervals_results(t.ctx, 0, None, 0, C.byref(n), None, C.byref(ms)), "trew_hip_intervals_results")
    return ms.value, int(n.value)


def alternate(t, batch, min_len, warmup, launches):
    """(tracts ms, intervals ms, found): the two kernels take turns on one stream"""
    t.intervals(batch, MOTIF, None, min_len, 1)
    cap = max(intervals_ms(t)[1], 1)
    for _ in range(warmup):
        t.tracts(batch, MOTIF, 3)
        t.intervals(batch, MOTIF, None, min_len, cap)
    t.wait(0)
    a = b = 0.0
    found = 0
    for _ in range(launches):
        t.tracts(batch, MOTIF, 3)
        a += tracts_ms(t)
        t.intervals(batch, MOTIF, None, min_len, cap)
        ms, found = intervals_ms(t)
        assert found == cap
        b += ms
    return a / launches, b / launches, found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches}

    def record(prefix, tr, iv, found, units, per):
        res.update({prefix + "_tracts_ms": round(tr, 4), prefix + "_intervals_ms": round(iv, 4), prefix + "_intervals_over_tracts": round(iv / tr, 3),
                    prefix + "_intervals_found": found, prefix + "_appends": found, prefix + "_intervals_" + per: round(units / iv / 1e6, 2)})

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            res.update(long_reads=a.long_reads, long_bases=bases)
            record("long", *alternate(t, b, None, a.warmup, a.launches), bases, "gbases_per_s")
            record("long_minlen1", *alternate(t, b, 1, a.warmup, a.launches), bases, "gbases_per_s")
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
            record("short", *alternate(t, b, None, a.warmup, a.launches), n * 1e3, "mreads_per_s")
            record("short_minlen1", *alternate(t, b, 1, a.warmup, a.launches), n * 1e3, "mreads_per_s")
            t.free(d)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
