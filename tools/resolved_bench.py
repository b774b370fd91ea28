#!/usr/bin/env python3
"""Timing of trew_hip_tandems_resolved, trew_hip_decompose_resolved and trew_hip_dissect_resolved next to their plain kernels on the
same device-resident batch (HIP events through ms_kernel, one slot, one process; per measure the plain kernel, its resolved
instantiation with C = 1 and with C = --candidates alternate launch by launch).  Stage 1 and the trace run once and only the
alignment passes run per candidate, so C x the plain kernel bounds the resolved one from above; at C = 1 it does the plain
kernel's work with its own registers (the command line and Python call the plain kernel at C = 1, so that ratio is a finding).

    python tools/resolved_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 3] [--launches 20] [--penalty 3]
                                   [--candidates 3] [--out FILE]

Prints one JSON object; per batch (long: --long_reads reads of the long-read generator; short: --reads uniform reads of --len
bases) and measure (tandems, decompose, dissect):
  <batch>_<measure>_plain_ms / _c1_ms / _cC_ms and their _spread   mean of --launches launches, (largest - smallest) / mean
  <batch>_<measure>_c1_over_plain, _cC_over_plain                   the ratios of the means (the bound for the second: C)
  <batch>_<measure>_found_plain, _found_cC                          records (decompose: items) a launch found
  <batch>_bases                                                     bases of the batch
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
MAX_RECORDS, MAX_ITEMS, MAX_ROWS = 1 << 22, 1 << 22, 1 << 24  # 288 MB and 192 MB of logs, 512 MB of workspace: tools/dissect_bench.py's
ROOM = {"tandems": (MAX_RECORDS,), "decompose": (MAX_ITEMS, MAX_ROWS), "dissect": (MAX_RECORDS, MAX_ITEMS, MAX_ROWS)}


def kernel_ms(t, measure):
    """(kernel time, what was found) of the slot's last call of `measure`, plain or resolved, without copying anything back"""
    a, b, c, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    what = "trew_hip_%s_results" % measure
    f = getattr(t.lib, what)
    if measure == "tandems":
        t._chk(f(t.ctx, 0, None, 0, C.byref(a), None, C.byref(ms)), what)
        over = a.value > MAX_RECORDS
    elif measure == "decompose":
        t._chk(f(t.ctx, 0, None, 0, C.byref(a), C.byref(b), None, None, C.byref(ms)), what)
        over = a.value > MAX_ITEMS or b.value > MAX_ROWS
    else:
        t._chk(f(t.ctx, 0, None, 0, None, 0, C.byref(a), C.byref(b), C.byref(c), None, C.byref(ms)), what)
        over = a.value > MAX_RECORDS or b.value > MAX_ITEMS or c.value > MAX_ROWS
    if over:
        raise SystemExit("the batch overflows the logs or the workspace of %s" % measure)
    return ms.value, int(a.value)


def launch(t, measure, batch, a, candidates):
    """candidates None: the plain entry point; otherwise the resolved one, for C = 1 as well"""
    t._queue(measure, 0, batch, None, 1, shape=ROOM[measure])
    head = (t.ctx, C.byref(batch), 0, 1, 32, a.penalty, 24)
    if candidates is None:
        what = "trew_hip_%s" % measure
        t._chk(getattr(t.lib, what)(*head, *ROOM[measure]), what)
    else:
        what = "trew_hip_%s_resolved" % measure
        t._chk(getattr(t.lib, what)(*head, candidates, *ROOM[measure]), what)
    return kernel_ms(t, measure)


def rows(res, name, t, batch, bases, a):
    res[name + "_bases"] = int(bases)
    for measure in ("tandems", "decompose", "dissect"):
        times = {"plain": [], "c1": [], "cC": []}
        found = {}
        for i in range(a.warmup + a.launches):
            for key, cand in (("plain", None), ("c1", 1), ("cC", a.candidates)):
                ms, found[key] = launch(t, measure, batch, a, cand)
                if i >= a.warmup:
                    times[key].append(ms)
        stem = "%s_%s_" % (name, measure)
        for k, v in times.items():
            res[stem + k + "_ms"] = round(float(np.mean(v)), 4)
            res[stem + k + "_spread"] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
        plain = float(np.mean(times["plain"]))
        res[stem + "c1_over_plain"] = round(float(np.mean(times["c1"])) / plain, 3)
        res[stem + "cC_over_plain"] = round(float(np.mean(times["cC"])) / plain, 3)
        res[stem + "found_plain"] = found["plain"]
        res[stem + "found_cC"] = found["cC"]


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
