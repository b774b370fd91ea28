#!/usr/bin/env python3
"""Timing of trew_hip_repeats next to its yardstick, periods_wave_kernel, on the same device-resident batches (HIP events
through ms_kernel, one stream, one process, the two kernels alternating launch by launch).

    python tools/repeats_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3]
                                  [--min_score 24] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases), at periods 1 .. 32:
  <batch>_periods_ms / <batch>_repeats_ms            the yardstick and the kernel, taking turns: means of --launches launches
  <batch>_periods_spread / <batch>_repeats_spread    (largest - smallest) / mean over those launches
  <batch>_repeats_over_periods                       the ratio of the means
  <batch>_tracts / <batch>_reads_with                tracts found, reads with at least one; <batch>_most: the most in one read
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


def periods_ms(t):
    """kernel time of the slot's last periods without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_periods_results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), "trew_hip_periods_results")
    return ms.value


def repeats_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_repeats_results(t.ctx, 0, None, 0, C.byref(n), None, C.byref(ms)), "trew_hip_repeats_results")
    return ms.value, int(n.value)


def rows(res, name, t, batch, n_reads, a):
    # the log holds every tract: one launch to learn the number, which the timed launches then use
    t.repeats(batch, 1, 32, a.penalty, a.min_score, max_records=max(n_reads, 1))
    _, counts, found = t.repeats_results()
    cap = max(found, 1)
    for _ in range(a.warmup):
        t.periods(batch, 1, 32, a.penalty, a.min_score)
        t.repeats(batch, 1, 32, a.penalty, a.min_score, max_records=cap)
    t.wait(0)
    pe, rp = [], []
    for _ in range(a.launches):
        t.periods(batch, 1, 32, a.penalty, a.min_score)
        pe.append(periods_ms(t))
        t.repeats(batch, 1, 32, a.penalty, a.min_score, max_records=cap)
        ms, n = repeats_ms(t)
        assert n == found
        rp.append(ms)
    pe, rp = np.array(pe), np.array(rp)
    res[name + "_periods_ms"] = round(float(pe.mean()), 4)
    res[name + "_repeats_ms"] = round(float(rp.mean()), 4)
    res[name + "_periods_spread"] = round(float((pe.max() - pe.min()) / pe.mean()), 4)
    res[name + "_repeats_spread"] = round(float((rp.max() - rp.min()) / rp.mean()), 4)
    res[name + "_repeats_over_periods"] = round(float(rp.mean() / pe.mean()), 3)
    res[name + "_tracts"] = found
    res[name + "_reads_with"] = int((counts > 0).sum())
    res[name + "_most"] = int(counts.max()) if len(counts) else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--min_score", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "min_score": a.min_score}

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            rows(res, "long", t, b, a.long_reads, a)
            for p in ptrs:
                t.free(p)
        res.update(long_reads=a.long_reads, long_bases=bases)

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(SEED, 0, n, L, d)
            rows(res, "short", t, t.device_uniform_batch(d, n, L), n, a)
            t.free(d)
        res.update(short_reads=n, short_len=L)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
