#!/usr/bin/env python3
"""Timing of trew_hip_refine next to the two kernels it is made of, periods_wave_kernel and align_wave_kernel (motif TTAGGG),
on the same device-resident batch (HIP events through ms_kernel, one stream, one process, the three kernels alternating
launch by launch).  `refine` runs the periods stage, one more walk over the eq words, and up to three single-strand passes
of the alignment (the second with the vote's argmax); `align` runs two strands a pass: the sum periods + 1.5 x align is
what the parts cost, for a unit of six bases.

    python tools/refine_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3]
                                 [--motif TTAGGG] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases):
  <batch>_<kernel>_ms / _spread      mean of --launches launches, (largest - smallest) / mean; kernel: periods, align, refine
  <batch>_parts_ms                   periods + 1.5 x align
  <batch>_refine_over_parts          refine / that sum
  <batch>_bases, <batch>_records     bases of the batch; reads with a refine record (period > 0)
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
    times = {"periods": [], "align": [], "refine": []}
    for i in range(a.warmup + a.launches):
        t.periods(batch, 1, 32, a.penalty, 24)
        ms_p = kernel_ms(t, "periods")
        t.align(batch, [a.motif], a.penalty)
        ms_a = kernel_ms(t, "align")
        t.refine(batch, 1, 32, a.penalty, 24)
        ms_r = kernel_ms(t, "refine")
        if i >= a.warmup:
            times["periods"].append(ms_p)
            times["align"].append(ms_a)
            times["refine"].append(ms_r)
    for k, v in times.items():
        res["%s_%s_ms" % (name, k)] = round(float(np.mean(v)), 4)
        res["%s_%s_spread" % (name, k)] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
    parts = float(np.mean(times["periods"])) + 1.5 * float(np.mean(times["align"]))
    res[name + "_parts_ms"] = round(parts, 4)
    res[name + "_refine_over_parts"] = round(float(np.mean(times["refine"])) / parts, 3)
    res[name + "_bases"] = int(bases)
    res[name + "_records"] = int((t.refine_results()["period"] > 0).sum())


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
