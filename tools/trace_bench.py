#!/usr/bin/env python3
"""Timing of trew_hip_trace next to its yardstick, align_wave_kernel on the same batch and motif (HIP events through
ms_kernel, one stream, one process, the two kernels alternating launch by launch).  trace does align's pass and, for the keys
that reach min_score, the second pass over the tract and the walk: on a batch without tracts it should cost what align costs.

    python tools/trace_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--tail_reads 2000] [--warmup 3]
                                [--launches 20] [--penalty 3] [--min_score 24] [--motif TTAGGG] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases; tails: --tail_reads generator long reads cut to at most 6 kb with a planted noisy (TTAGGG)n tail of 0.3 to 2 kb,
so that the second pass and the walk run in every read):
  <batch>_align_ms / _align_spread     the yardstick: mean of --launches launches, (largest - smallest) / mean
  <batch>_trace_ms / _trace_spread     the kernel, taking turns with it
  <batch>_trace_over_align             the ratio of the means
  <batch>_bases, <batch>_reads         the batch
  <batch>_items, <batch>_rows          what a launch found: items, rows of the workspace claimed
  <batch>_workspace_bytes              64 bytes a row
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trew_amd as T  # noqa: E402
from trew_amd import capi  # noqa: E402

SEED = 20250218
MAX_ITEMS, MAX_ROWS = 1 << 22, 1 << 24  # 192 MB of log, 1 GB of workspace: the batches below stay under both


def align_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_align_results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), "trew_hip_align_results")
    return ms.value


def trace_ms(t):
    ni, nr, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_trace_results(t.ctx, 0, None, 0, C.byref(ni), C.byref(nr), None, None, C.byref(ms)), "trew_hip_trace_results")
    if ni.value > MAX_ITEMS or nr.value > MAX_ROWS:
        raise SystemExit("the batch overflows the log or the workspace: %d items, %d rows" % (ni.value, nr.value))
    return ms.value, int(ni.value), int(nr.value)


def rows(res, name, t, batch, n_reads, bases, a):
    times = {"align": [], "trace": []}
    items = nrows = 0
    for i in range(a.warmup + a.launches):
        t.align(batch, [a.motif], a.penalty)
        ms_a = align_ms(t)
        t.trace(batch, [a.motif], a.penalty, a.min_score, MAX_ITEMS, MAX_ROWS)
        ms_t, items, nrows = trace_ms(t)
        if i >= a.warmup:
            times["align"].append(ms_a)
            times["trace"].append(ms_t)
    for k, v in times.items():
        res["%s_%s_ms" % (name, k)] = round(float(np.mean(v)), 4)
        res["%s_%s_spread" % (name, k)] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
    res[name + "_trace_over_align"] = round(float(np.mean(times["trace"]) / np.mean(times["align"])), 4)
    res.update({name + "_reads": int(n_reads), name + "_bases": int(bases), name + "_items": items, name + "_rows": nrows,
                name + "_workspace_bytes": 64 * nrows})


def noisy_tail(rnd, unit, n):
    """n bases of the unit with substitutions at 0.03 and single-base indels at 0.06"""
    out = []
    p = rnd.randrange(len(unit))
    for i in range(n):
        c = unit[(p + i) % len(unit)]
        x = rnd.random()
        if x < 0.03:
            out.append(rnd.choice([y for y in "ACGT" if y != c]))
        elif x < 0.06:
            out.append(c + rnd.choice("ACGT"))
        elif x >= 0.09:
            out.append(c)
    return "".join(out)


def tail_reads(n, motif):
    rnd = random.Random(8)
    buf, st, nd = capi.synth_long_ascii(SEED, 0, n)
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    out = []
    for i, (s, e) in enumerate(zip(st, nd)):
        read = buf[s:e + 1].decode()[:rnd.randint(500, 6000)] + noisy_tail(rnd, motif, rnd.randint(300, 2000))
        if i % 4 == 3:
            read = "".join(comp.get(c, "N") for c in reversed(read.upper()))
        out.append(read.encode())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--tail_reads", type=int, default=2000)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--min_score", type=int, default=24)
    ap.add_argument("--motif", default="TTAGGG")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "min_score": a.min_score, "motif": a.motif}

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            rows(res, "long", t, b, a.long_reads, bases, a)
            for p in ptrs:
                t.free(p)

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(SEED, 0, n, L, d)
            rows(res, "short", t, t.device_uniform_batch(d, n, L), n, n * L, a)
            t.free(d)

    if a.tail_reads:
        reads = tail_reads(a.tail_reads, a.motif)
        words, offsets, lengths = capi.pack_reads(reads)
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=len(words) + 64, max_batch_reads=len(reads), table_log2_slots=12) as t:
            rows(res, "tails", t, t.host_batch(words, offsets, lengths), len(reads), int(lengths.sum()), a)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
