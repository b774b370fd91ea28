#!/usr/bin/env python3
"""Timing of trew_hip_decompose next to its yardstick, refine_wave_kernel on the same batch (HIP events through ms_kernel, one
stream, one process, the two kernels alternating launch by launch).  decompose does refine's work and, for the reads that
reach min_score, the rows of the tract against the anchored unit and the walk: on a batch without tracts it should cost what
refine costs.

    python tools/decompose_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--tail_reads 2000] [--warmup 3]
                                    [--launches 20] [--penalty 3] [--min_score 24] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of
--len bases; tails: --tail_reads generator long reads cut to at most 6 kb with a planted noisy (TTAGGG)n tail of 0.3 to 2 kb,
the batch of tools/trace_bench.py):
  <batch>_refine_ms / _refine_spread         the yardstick: mean of --launches launches, (largest - smallest) / mean
  <batch>_decompose_ms / _decompose_spread   the kernel, taking turns with it
  <batch>_decompose_over_refine              the ratio of the means
  <batch>_bases, <batch>_reads               the batch
  <batch>_items, <batch>_rows                what a launch found: items, rows of the workspace claimed
  <batch>_workspace_bytes                    32 bytes a row
and for the tails batch the existing route to the same items, refine and then trace with each read's anchored unit as a motif
(every distinct unit of three bases or more, eight motifs a launch, every read against every motif on both strands):
  tails_route_ms, tails_route_units, tails_route_launches, tails_route_over_refine
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trew_amd as T  # noqa: E402
from trew_amd import capi  # noqa: E402
from trace_bench import SEED, tail_reads  # noqa: E402

MAX_ITEMS, MAX_ROWS = 1 << 22, 1 << 24  # 192 MB of log, 512 MB of workspace: the batches below stay under both


def refine_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_refine_results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), "trew_hip_refine_results")
    return ms.value


def decompose_ms(t):
    ni, nr, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_decompose_results(t.ctx, 0, None, 0, C.byref(ni), C.byref(nr), None, None, C.byref(ms)), "trew_hip_decompose_results")
    if ni.value > MAX_ITEMS or nr.value > MAX_ROWS:
        raise SystemExit("the batch overflows the log or the workspace: %d items, %d rows" % (ni.value, nr.value))
    return ms.value, int(ni.value), int(nr.value)


def trace_ms(t):
    ni, nr, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_trace_results(t.ctx, 0, None, 0, C.byref(ni), C.byref(nr), None, None, C.byref(ms)), "trew_hip_trace_results")
    return ms.value, ni.value > 2 * MAX_ITEMS or nr.value > 4 * MAX_ROWS


def rows(res, name, t, batch, n_reads, bases, a):
    times = {"refine": [], "decompose": []}
    items = nrows = 0
    for i in range(a.warmup + a.launches):
        t.refine(batch, 1, 32, a.penalty, a.min_score)
        ms_r = refine_ms(t)
        t.decompose(batch, 1, 32, a.penalty, a.min_score, MAX_ITEMS, MAX_ROWS)
        ms_d, items, nrows = decompose_ms(t)
        if i >= a.warmup:
            times["refine"].append(ms_r)
            times["decompose"].append(ms_d)
    for k, v in times.items():
        res["%s_%s_ms" % (name, k)] = round(float(np.mean(v)), 4)
        res["%s_%s_spread" % (name, k)] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
    res[name + "_decompose_over_refine"] = round(float(np.mean(times["decompose"]) / np.mean(times["refine"])), 4)
    res.update({name + "_reads": int(n_reads), name + "_bases": int(bases), name + "_items": items, name + "_rows": nrows,
                name + "_workspace_bytes": 32 * nrows})


def route(res, name, t, batch, a):
    """refine, then trace with every distinct anchored unit of the batch as a motif, eight a launch"""
    t.decompose(batch, 1, 32, a.penalty, a.min_score, MAX_ITEMS, MAX_ROWS)
    _, counts, recs, _, _ = t.decompose_results()
    units = sorted({(int(r["period"]), capi.decompose_anchor(r)) for r, c in zip(recs, counts) if c and int(r["period"]) >= 3})
    motifs = ["".join("TGCA"[(w >> (2 * (k - 1 - j))) & 3] for j in range(k)) for k, w in units]
    groups = [motifs[i:i + 8] for i in range(0, len(motifs), 8)]
    total = []
    overflowed = False  # a trace launch whose rows did not fit recomputes them: its time is then not the route's
    for i in range(a.warmup + a.launches):
        t.refine(batch, 1, 32, a.penalty, a.min_score)
        ms = refine_ms(t)
        for g in groups:
            t.trace(batch, g, a.penalty, a.min_score, 2 * MAX_ITEMS, 4 * MAX_ROWS)
            ms_t, over = trace_ms(t)
            ms += ms_t
            overflowed |= over
        if i >= a.warmup:
            total.append(ms)
    res.update({name + "_route_ms": round(float(np.mean(total)), 4), name + "_route_spread": round(float((np.max(total) - np.min(total)) / np.mean(total)), 4),
                name + "_route_units": len(motifs), name + "_route_launches": 1 + len(groups), name + "_route_overflowed": bool(overflowed),
                name + "_route_over_refine": round(float(np.mean(total)) / res[name + "_refine_ms"], 4)})


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "min_score": a.min_score}

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
        reads = tail_reads(a.tail_reads, "TTAGGG")
        words, offsets, lengths = capi.pack_reads(reads)
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=len(words) + 64, max_batch_reads=len(reads), table_log2_slots=12) as t:
            batch = t.host_batch(words, offsets, lengths)
            rows(res, "tails", t, batch, len(reads), int(lengths.sum()), a)
            route(res, "tails", t, batch, a)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
