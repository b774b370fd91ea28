#!/usr/bin/env python3
"""Timing of trew_hip_copies next to trew_hip_monomers on the same planes (HIP events through ms_kernel, one stream, one
process), the two kernels taking turns launch by launch, at k = 64, 128, 171 and 256, on two batches:

  long      the device-resident generator long reads of DESIGN 4.7m, where few bases are traced
  arrays    planted arrays of diverged monomers (every copy of a random unit with substitutions and indels of its own, no
            flanks), where most bases are traced

    python tools/copies_bench.py [--long_reads 20000] [--arrays 1000] [--array_bases 8000] [--warmup 3] [--launches 20]
                                 [--penalty 3] [--min_score 24] [--ks 64,128,171,256] [--out FILE]

monomers_wave_kernel<Q> is the library's own: its kDirs = false instantiation of the row step, whose resource rows equal the
parent commit's (profiles/copies/README.md).  Prints one JSON object; per batch and k:
  <batch>_k<K>_monomers_ms / _spread, <batch>_k<K>_copies_ms / _spread    mean of --launches launches, (largest - smallest) / mean
  <batch>_k<K>_copies_over_monomers                                       the ratio of the means
  <batch>_k<K>_items_per_read / _rows_per_read / _traced_fraction         what the kernel found: rows / (2 * bases) is traced
  <batch>_k<K>_workspace_bytes                                            rows claimed * 64 Q
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


def unit_of(k):
    rnd = random.Random(k)
    return "".join(rnd.choice("ACGT") for _ in range(k))


def diverged_array(rnd, unit, n, sub=0.10, indel=0.02):
    """about n bases of copies of the unit, every base substituted at rate sub and deleted or followed by an extra base at rate indel"""
    out = []
    size = 0
    while size < n:
        for c in unit:
            x = rnd.random()
            if x < sub:
                out.append(rnd.choice([b for b in "ACGT" if b != c]))
            elif x < sub + indel / 2:
                continue
            elif x < sub + indel:
                out.append(c + rnd.choice("ACGT"))
            else:
                out.append(c)
        size += len(unit)
    return "".join(out)


def kernel_ms(t, measure):
    """kernel time of the slot's last call of `measure` without copying anything back but the counters"""
    ms = C.c_float(0)
    what = "trew_hip_%s_results" % measure
    if measure == "monomers":
        n = C.c_uint64(0)
        t._chk(t.lib.trew_hip_monomers_results(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), what)
        return ms.value, 0, 0
    ni, nr = C.c_uint64(0), C.c_uint64(0)
    t._chk(t.lib.trew_hip_copies_results(t.ctx, 0, None, 0, C.byref(ni), C.byref(nr), None, None, C.byref(ms)), what)
    return ms.value, int(ni.value), int(nr.value)


def put(res, name, times):
    mean = float(np.mean(times))
    res[name + "_ms"] = round(mean, 4)
    res[name + "_spread"] = round(float((np.max(times) - np.min(times)) / mean), 4)


def run(t, b, n_reads, bases, units, a, res, tag, first_rows=1):
    for k, unit in units:
        q = 1 if k <= 64 else 2 if k <= 128 else 4
        # size the log and the workspace with one call, so that no timed launch overflows (first_rows: where long tracts are
        # expected, room for them at once -- a tract whose rows do not fit is traced at a cost quadratic in its length)
        t.copies(b, [unit], a.penalty, a.min_score, 1, first_rows)
        _, items, rows = kernel_ms(t, "copies")
        room = (max(items, 1), max(rows, 1))
        mo, co = [], []
        for i in range(a.warmup + a.launches):
            t.monomers(b, [unit], a.penalty)
            ms_m = kernel_ms(t, "monomers")[0]
            t.copies(b, [unit], a.penalty, a.min_score, *room)
            ms_c, items2, rows2 = kernel_ms(t, "copies")
            assert (items2, rows2) == (items, rows)
            if i >= a.warmup:
                mo.append(ms_m)
                co.append(ms_c)
        name = "%s_k%d" % (tag, k)
        put(res, name + "_monomers", mo)
        put(res, name + "_copies", co)
        res[name + "_copies_over_monomers"] = round(float(np.mean(co) / np.mean(mo)), 3)
        res[name + "_items_per_read"] = round(items / max(n_reads, 1), 3)
        res[name + "_rows_per_read"] = round(rows / max(n_reads, 1), 1)
        res[name + "_traced_fraction"] = round(rows / max(2 * bases, 1), 4)
        res[name + "_workspace_bytes"] = rows * 64 * q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--arrays", type=int, default=1000)
    ap.add_argument("--array_bases", type=int, default=8000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--min_score", type=int, default=24)
    ap.add_argument("--ks", default="64,128,171,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",") if x]
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "min_score": a.min_score, "long_reads": a.long_reads, "arrays": a.arrays,
           "array_bases": a.array_bases}
    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            res["long_bases"] = int(bases)
            run(t, b, a.long_reads, int(bases), [(k, unit_of(k)) for k in ks], a, res, "long")
            for p in ptrs:
                t.free(p)
    if a.arrays:
        for k in ks:  # a batch per k: the arrays are made of the unit they are aligned against
            rnd = random.Random(1000 + k)
            unit = unit_of(k)
            reads = [diverged_array(rnd, unit, a.array_bases) for _ in range(a.arrays)]
            words, offsets, lengths = capi.pack_reads(reads)
            bases = int(sum(len(r) for r in reads))
            with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=len(words) + 64, max_batch_reads=max(a.arrays, 16), table_log2_slots=12) as t:
                res["arrays_k%d_bases" % k] = bases
                run(t, t.host_batch(words, offsets, lengths), a.arrays, bases, [(k, unit)], a, res, "arrays", first_rows=2 * bases)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
