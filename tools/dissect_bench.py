#!/usr/bin/env python3
"""Timing of trew_hip_dissect next to its two yardsticks, tandems_wave_kernel and decompose_wave_kernel, on the same batch (HIP
events through ms_kernel, one slot, one process, the three kernels alternating launch by launch).  dissect does tandems' work
and, for every tract it reports, what decompose adds to refine for the one tract it traces: where few bases lie in tracts it
should cost about what tandems costs.

    python tools/dissect_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--tail_reads 2000] [--two_reads 2000]
                                  [--warmup 3] [--launches 20] [--penalty 3] [--min_score 24] [--out FILE]

Prints one JSON object; per batch (long, short and tails: the batches of tools/decompose_bench.py; two: --two_reads reads with
two noisy tracts of 300 to 700 bases of random primitive units of 2 to 12 bases, 40 to 120 random bases between them):
  <batch>_tandems_ms / _decompose_ms / _dissect_ms and their _spread   mean of --launches launches, (largest - smallest) / mean
  <batch>_dissect_over_tandems, <batch>_dissect_over_decompose         the ratios of the means
  <batch>_reads, <batch>_bases                                         the batch
  <batch>_records, <batch>_items, <batch>_rows                         what a dissect launch found
  <batch>_workspace_bytes                                              32 bytes a row
  <batch>_decompose_items                                              what a decompose launch found, for comparison
and for the two-tract batch the existing route to the same items: tandems, then every tract cut out on the host and decompose
on the cut-out tracts as a second batch (the kernels' times only: the second upload and the host's work are not in it):
  two_route_ms, two_route_spread, two_route_tracts, two_route_items, two_route_over_dissect
"""
import argparse
import ctypes as C
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import trew_amd as T  # noqa: E402
from trew_amd import capi  # noqa: E402
from trace_bench import SEED, tail_reads  # noqa: E402

MAX_RECORDS, MAX_ITEMS, MAX_ROWS = 1 << 22, 1 << 22, 1 << 24  # 288 MB and 192 MB of logs, 512 MB of workspace
TWO_SEED = 20251015


def tandems_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_tandems_results(t.ctx, 0, None, 0, C.byref(n), None, C.byref(ms)), "trew_hip_tandems_results")
    if n.value > MAX_RECORDS:
        raise SystemExit("the batch overflows the tandems log: %d records" % n.value)
    return ms.value, int(n.value)


def decompose_ms(t):
    ni, nr, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_decompose_results(t.ctx, 0, None, 0, C.byref(ni), C.byref(nr), None, None, C.byref(ms)), "trew_hip_decompose_results")
    if ni.value > MAX_ITEMS or nr.value > MAX_ROWS:
        raise SystemExit("the batch overflows decompose's log or workspace: %d items, %d rows" % (ni.value, nr.value))
    return ms.value, int(ni.value)


def dissect_ms(t):
    nr, ni, nw, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_dissect_results(t.ctx, 0, None, 0, None, 0, C.byref(nr), C.byref(ni), C.byref(nw), None, C.byref(ms)), "trew_hip_dissect_results")
    if nr.value > MAX_RECORDS or ni.value > MAX_ITEMS or nw.value > MAX_ROWS:
        raise SystemExit("the batch overflows dissect's logs or workspace: %d records, %d items, %d rows" % (nr.value, ni.value, nw.value))
    return ms.value, int(nr.value), int(ni.value), int(nw.value)


def spread(v):
    return round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)


def rows(res, name, t, batch, n_reads, bases, a):
    times = {"tandems": [], "decompose": [], "dissect": []}
    found = (0, 0, 0)
    d_items = 0
    for i in range(a.warmup + a.launches):
        t.tandems(batch, 1, 32, a.penalty, a.min_score, MAX_RECORDS)
        ms_t, _ = tandems_ms(t)
        t.decompose(batch, 1, 32, a.penalty, a.min_score, MAX_ITEMS, MAX_ROWS)
        ms_d, d_items = decompose_ms(t)
        t.dissect(batch, 1, 32, a.penalty, a.min_score, MAX_RECORDS, MAX_ITEMS, MAX_ROWS)
        ms_x, *found = dissect_ms(t)
        if i >= a.warmup:
            times["tandems"].append(ms_t)
            times["decompose"].append(ms_d)
            times["dissect"].append(ms_x)
    for k, v in times.items():
        res["%s_%s_ms" % (name, k)] = round(float(np.mean(v)), 4)
        res["%s_%s_spread" % (name, k)] = spread(v)
    res[name + "_dissect_over_tandems"] = round(float(np.mean(times["dissect"]) / np.mean(times["tandems"])), 4)
    res[name + "_dissect_over_decompose"] = round(float(np.mean(times["dissect"]) / np.mean(times["decompose"])), 4)
    res.update({name + "_reads": int(n_reads), name + "_bases": int(bases), name + "_records": found[0], name + "_items": found[1], name + "_rows": found[2],
                name + "_workspace_bytes": 32 * found[2], name + "_decompose_items": d_items})


def junk(rnd, n):
    return "".join(rnd.choice("ACGT") for _ in range(n))


def primitive_unit(rnd, k):
    while True:
        u = junk(rnd, k)
        if len({u[q:] + u[:q] for q in range(k)}) == k:
            return u


def noisy(rnd, unit, n, sub, indel):
    """n bases of (unit)n, each base substituted with probability `sub`, followed by an inserted base or deleted with `indel`"""
    out, j = [], 0
    while len(out) < n:
        c = unit[j % len(unit)]
        j += 1
        x = rnd.random()
        if x < indel / 2:
            continue
        if x < indel:
            out += [c, rnd.choice("ACGT")]
            continue
        out.append(rnd.choice([y for y in "ACGT" if y != c]) if rnd.random() < sub else c)
    return "".join(out[:n])


def two_tract_reads(n, seed=TWO_SEED):
    """reads of the shape of the two-tract set of the tests: two noisy tracts of different units, random bases around them"""
    rnd = random.Random(seed)
    reads = []
    for _ in range(n):
        u1 = primitive_unit(rnd, rnd.randint(2, 12))
        u2 = primitive_unit(rnd, rnd.randint(2, 12))
        while len(u1) == len(u2) and u2 in {u1[q:] + u1[:q] for q in range(len(u1))}:
            u2 = primitive_unit(rnd, rnd.randint(2, 12))
        read = junk(rnd, rnd.randint(0, 40))
        for i, u in enumerate((u1, u2)):
            read += noisy(rnd, u, rnd.randint(300, 700), 0.03, 0.06) + junk(rnd, rnd.randint(40, 120) if i == 0 else rnd.randint(0, 40))
        reads.append(read.encode())
    return reads


def route(res, name, t, reads, batch, a):
    """tandems, then decompose on the cut-out tracts as a second batch (cut once, outside the timed launches)"""
    t.tandems(batch, 1, 32, a.penalty, a.min_score, MAX_RECORDS)
    recs = t.tandems_results()[0]
    cut = [reads[int(x["read"])][int(x["start"]):int(x["end"])] for x in recs]
    second = t.host_batch(*capi.pack_reads(cut))  # smaller than `batch`: it fits the same slot
    total, items = [], 0
    for i in range(a.warmup + a.launches):
        t.tandems(batch, 1, 32, a.penalty, a.min_score, MAX_RECORDS)
        ms, _ = tandems_ms(t)
        t.decompose(second, 1, 32, a.penalty, a.min_score, MAX_ITEMS, MAX_ROWS)
        ms_d, items = decompose_ms(t)
        if i >= a.warmup:
            total.append(ms + ms_d)
    res.update({name + "_route_ms": round(float(np.mean(total)), 4), name + "_route_spread": spread(total), name + "_route_tracts": len(cut),
                name + "_route_items": items, name + "_route_over_dissect": round(float(np.mean(total)) / res[name + "_dissect_ms"], 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--tail_reads", type=int, default=2000)
    ap.add_argument("--two_reads", type=int, default=2000)
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

    for name, reads in (("tails", tail_reads(a.tail_reads, "TTAGGG") if a.tail_reads else []), ("two", two_tract_reads(a.two_reads))):
        if not reads:
            continue
        words, offsets, lengths = capi.pack_reads(reads)
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=len(words) + 64, max_batch_reads=8 * len(reads), table_log2_slots=12) as t:
            batch = t.host_batch(words, offsets, lengths)
            rows(res, name, t, batch, len(reads), int(lengths.sum()), a)
            if name == "two":  # the cut-out tracts are a batch of more reads than the slot's first
                route(res, name, t, reads, batch, a)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
