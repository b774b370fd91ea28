#!/usr/bin/env python3
"""Timing of trew_hip_align next to a yardstick, tracts_wave_kernel on the same device-resident batch and motif (HIP events
through ms_kernel, one stream, one process, the two kernels alternating launch by launch).  The two kernels do different
work -- the yardstick only says how steady the machine was during the job and what a pass over the same planes costs.

    python tools/align_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3]
                                [--motif TTAGGG] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases):
  <batch>_tracts_ms / _tracts_spread   the yardstick: mean of --launches launches, (largest - smallest) / mean
  <batch>_align_ms / _align_spread     the kernel, taking turns with it
  <batch>_align_over_tracts            the ratio of the means
  <batch>_bases, <batch>_gcells_per_s  bases of the batch; n k cells of both strands per second: 2 * bases * k / align_ms
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
    times = {"tracts": [], "align": []}
    for i in range(a.warmup + a.launches):
        t.tracts(batch, [a.motif], a.penalty)
        ms_t = kernel_ms(t, "tracts")
        t.align(batch, [a.motif], a.penalty)
        ms_a = kernel_ms(t, "align")
        if i >= a.warmup:
            times["tracts"].append(ms_t)
            times["align"].append(ms_a)
    for k, v in times.items():
        res["%s_%s_ms" % (name, k)] = round(float(np.mean(v)), 4)
        res["%s_%s_spread" % (name, k)] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
    res[name + "_align_over_tracts"] = round(float(np.mean(times["align"]) / np.mean(times["tracts"])), 3)
    res[name + "_bases"] = int(bases)
    res[name + "_gcells_per_s"] = round(2.0 * bases * len(a.motif) / (float(np.mean(times["align"])) * 1e-3) / 1e9, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--motif", default="TTAGGG")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "motif": a.motif}

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
