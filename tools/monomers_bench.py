#!/usr/bin/env python3
"""Timing of trew_hip_monomers next to trew_hip_align on the same device-resident batch of generator long reads (HIP events
through ms_kernel, one stream, one process).  At k = 32 both kernels run the same unit, alternating launch by launch (there
monomers_wave_kernel<1> computes the records of align_wave_kernel; they are compared once before the timing); at the larger
k, which align does not reach, monomers runs alone with the same warm-up and rounds.

    python tools/monomers_bench.py [--long_reads 20000] [--warmup 3] [--launches 20] [--penalty 3] [--ks 64,128,171,256] [--out FILE]

Prints one JSON object:
  bases                                   bases of the batch
  k32_align_ms / _spread / _gcells_per_s  align at k = 32: mean of --launches launches, (largest - smallest) / mean, and
                                          2 * bases * k cells of both strands per second
  k32_monomers_ms / _spread / _gcells_per_s, k32_monomers_over_align   monomers on the same unit, taking turns with it
  k<K>_monomers_ms / _spread / _gcells_per_s   monomers alone at the k of --ks
  k256_rate_over_align_k32                the one comparison: the cell rate at k = 256 against align's at k = 32
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

SEED = 20250218


def kernel_ms(t, measure):
    """kernel time of the slot's last call of `measure` without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    what = "trew_hip_%s_results" % measure
    t._chk(getattr(t.lib, what)(t.ctx, 0, None, 0, C.byref(n), C.byref(ms)), what)
    return ms.value


def unit_of(k):
    rnd = random.Random(k)
    return "".join(rnd.choice("ACGT") for _ in range(k))


def put(res, name, times, bases, k):
    mean = float(np.mean(times))
    res[name + "_ms"] = round(mean, 4)
    res[name + "_spread"] = round(float((np.max(times) - np.min(times)) / mean), 4)
    res[name + "_gcells_per_s"] = round(2.0 * bases * k / (mean * 1e-3) / 1e9, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--ks", default="64,128,171,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",") if x]
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "long_reads": a.long_reads}
    with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
        b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
        res["bases"] = int(bases)
        u32 = unit_of(32)
        t.align(b, [u32], a.penalty)
        t.monomers(b, [u32], a.penalty)
        res["k32_records_equal"] = bool((t.align_results() == t.monomers_results()).all())
        al, mo = [], []
        for i in range(a.warmup + a.launches):
            t.align(b, [u32], a.penalty)
            ms_a = kernel_ms(t, "align")
            t.monomers(b, [u32], a.penalty)
            ms_m = kernel_ms(t, "monomers")
            if i >= a.warmup:
                al.append(ms_a)
                mo.append(ms_m)
        put(res, "k32_align", al, bases, 32)
        put(res, "k32_monomers", mo, bases, 32)
        res["k32_monomers_over_align"] = round(float(np.mean(mo) / np.mean(al)), 3)
        for k in ks:
            unit, times = unit_of(k), []
            for i in range(a.warmup + a.launches):
                t.monomers(b, [unit], a.penalty)
                ms = kernel_ms(t, "monomers")
                if i >= a.warmup:
                    times.append(ms)
            put(res, "k%d_monomers" % k, times, bases, k)
        if 256 in ks:
            res["k256_rate_over_align_k32"] = round(res["k256_monomers_gcells_per_s"] / res["k32_align_gcells_per_s"], 3)
        for p in ptrs:
            t.free(p)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
