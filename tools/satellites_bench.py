#!/usr/bin/env python3
"""Timing of trew_hip_satellites next to its yardstick, repeats_wave_kernel at periods 1 .. 32, on the same device-resident
batches (HIP events through ms_kernel, one stream, one process, the kernels alternating launch by launch).

    python tools/satellites_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3]
                                     [--min_score 24] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases):
  <batch>_repeats_ms / _repeats_spread          the yardstick at (1, 32): mean of --launches launches, (largest - smallest) / mean
  <batch>_sat_1_32_ms, _sat_1_256_ms, _sat_171_171_ms and their _spread: the kernel at the three ranges, taking turns with it
  <batch>_sat_1_32_over_repeats                 the ratio of the means at the range both have
  <batch>_expected_at_most                      1 + the yardstick's spread + one tenth; _within_expectation: ratio <= that
  <batch>_ms_per_further_period                 (sat_1_256_ms - sat_1_32_ms) / 224
  <batch>_tracts_1_32 / _tracts_1_256 / _tracts_171_171   tracts found; at (1, 32) the number `repeats` finds
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
RANGES = ((1, 32), (1, 256), (171, 171))


def repeats_ms(t):
    """kernel time of the slot's last repeats without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_repeats_results(t.ctx, 0, None, 0, C.byref(n), None, C.byref(ms)), "trew_hip_repeats_results")
    return ms.value, int(n.value)


def satellites_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_satellites_results(t.ctx, 0, None, 0, C.byref(n), None, C.byref(ms)), "trew_hip_satellites_results")
    return ms.value, int(n.value)


def rows(res, name, t, batch, n_reads, a):
    # the logs hold every tract: one launch each to learn the numbers, which the timed launches then use
    t.repeats(batch, 1, 32, a.penalty, a.min_score, max_records=max(n_reads, 1))
    rep_found = t.repeats_results()[2]
    found = {}
    for lo, hi in RANGES:
        t.satellites(batch, lo, hi, a.penalty, a.min_score, max_records=max(n_reads, 1))
        found[(lo, hi)] = t.satellites_results()[2]
    assert found[(1, 32)] == rep_found, (found, rep_found)
    times = {"repeats": []}
    times.update({r: [] for r in RANGES})
    for i in range(a.warmup + a.launches):
        t.repeats(batch, 1, 32, a.penalty, a.min_score, max_records=max(rep_found, 1))
        ms, n = repeats_ms(t)
        assert n == rep_found
        mine = {"repeats": ms}
        for lo, hi in RANGES:
            t.satellites(batch, lo, hi, a.penalty, a.min_score, max_records=max(found[(lo, hi)], 1))
            ms, n = satellites_ms(t)
            assert n == found[(lo, hi)]
            mine[(lo, hi)] = ms
        if i >= a.warmup:
            for k, v in mine.items():
                times[k].append(v)
    stat = {k: (float(np.mean(v)), float((np.max(v) - np.min(v)) / np.mean(v))) for k, v in times.items()}
    res[name + "_repeats_ms"] = round(stat["repeats"][0], 4)
    res[name + "_repeats_spread"] = round(stat["repeats"][1], 4)
    for lo, hi in RANGES:
        res["%s_sat_%d_%d_ms" % (name, lo, hi)] = round(stat[(lo, hi)][0], 4)
        res["%s_sat_%d_%d_spread" % (name, lo, hi)] = round(stat[(lo, hi)][1], 4)
        res["%s_tracts_%d_%d" % (name, lo, hi)] = found[(lo, hi)]
    ratio = stat[(1, 32)][0] / stat["repeats"][0]
    res[name + "_sat_1_32_over_repeats"] = round(ratio, 3)
    res[name + "_expected_at_most"] = round(1.0 + stat["repeats"][1] + 0.1, 3)
    res[name + "_within_expectation"] = bool(ratio <= 1.0 + stat["repeats"][1] + 0.1)
    res[name + "_ms_per_further_period"] = round((stat[(1, 256)][0] - stat[(1, 32)][0]) / 224.0, 4)


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
