#!/usr/bin/env python3
"""Timing of trew_hip_resolve next to trew_hip_refine on the same device-resident batch (HIP events through ms_kernel, one
stream, one process, refine_wave_kernel and resolve_wave_kernel with C = 1 and with C = --candidates alternating launch by
launch).  `resolve` runs refine's stage 1 once and refine's steps 2 to 6 for up to C candidates, so C x `refine` bounds it from
above and at C = 1 it is `refine` but for the kernel's own resources.

    python tools/resolve_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3]
                                  [--candidates 3] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases):
  <batch>_<kernel>_ms / _spread      mean of --launches launches, (largest - smallest) / mean; kernel: refine, resolve1, resolveC
  <batch>_resolve1_over_refine       resolve with C = 1 / refine
  <batch>_resolveC_over_refine       resolve with C = --candidates / refine (the bound: C)
  <batch>_bases, <batch>_records     bases of the batch; reads with a record (period > 0)
  <batch>_candidates                 the candidates of all reads with C = --candidates (the bodies that ran, skipped ones included)
  <batch>_repaired                   reads whose winner is not candidate 0
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


def kernel_ms(t, measure):
    """kernel time of the slot's last call of `measure` without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    what = "trew_hip_%s_results" % measure
    t._chk(getattr(t.lib, what)(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), what)
    return ms.value


def rows(res, name, t, batch, bases, a):
    times = {"refine": [], "resolve1": [], "resolveC": []}
    for i in range(a.warmup + a.launches):
        t.refine(batch, 1, 32, a.penalty, 24)
        ms_f = kernel_ms(t, "refine")
        t.resolve(batch, 1, 32, a.penalty, 24, 1)
        ms_1 = kernel_ms(t, "resolve")
        t.resolve(batch, 1, 32, a.penalty, 24, a.candidates)
        ms_c = kernel_ms(t, "resolve")
        if i >= a.warmup:
            times["refine"].append(ms_f)
            times["resolve1"].append(ms_1)
            times["resolveC"].append(ms_c)
    for k, v in times.items():
        res["%s_%s_ms" % (name, k)] = round(float(np.mean(v)), 4)
        res["%s_%s_spread" % (name, k)] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
    refine = float(np.mean(times["refine"]))
    res[name + "_resolve1_over_refine"] = round(float(np.mean(times["resolve1"])) / refine, 3)
    res[name + "_resolveC_over_refine"] = round(float(np.mean(times["resolveC"])) / refine, 3)
    got = t.resolve_results()  # of the last call: C = --candidates
    res[name + "_bases"] = int(bases)
    res[name + "_records"] = int((got["period"] > 0).sum())
    res[name + "_candidates"] = int(got["candidates"].sum())
    res[name + "_repaired"] = int((got["rank"] > 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "candidates": a.candidates}

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            rows(res, "long", t, b, bases, a)
            for p in ptrs:
                t.free(p)
        res.update(long_reads=a.long_reads)

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(SEED, 0, n, L, d)
            rows(res, "short", t, t.device_uniform_batch(d, n, L), n * L, a)
            t.free(d)
        res.update(short_reads=n, short_len=L)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
