#!/usr/bin/env python3
"""Timing of trew_hip_polish next to satellites_wave_kernel (periods 1 .. 256, every tract) and refine_wave_kernel (periods
1 .. 32) on the same device-resident batch of generator long reads (HIP events through ms_kernel, one stream, one process, the
kernels alternating launch by launch).  polish_wave_kernel<Q> runs at max_period 32 and 64 (Q = 1), 128 (Q = 2) and 256
(Q = 4).  The one like-for-like comparison is polish at max_period 32 against refine: the same reads, equal records (checked
here), a whole-wave row and one strand against refine's half-wave row.

    python tools/polish_bench.py [--long_reads 20000] [--warmup 3] [--launches 20] [--penalty 3] [--min_score 24] [--out FILE]

Prints one JSON object:
  <kernel>_ms / _spread        mean of --launches launches, (largest - smallest) / mean; kernel: satellites, refine, polish32,
                               polish64, polish128, polish256
  polish32_over_refine         polish32 / refine, and polish32_equals_refine: the twelve words and both units of every read
  polish<M>_records            reads with a record (period > 0) at max_period M; bases: the bases of the batch
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import trew_amd as T  # noqa: E402
from trew_amd import capi  # noqa: E402

SEED = 20250218
WIDTHS = (32, 64, 128, 256)


def kernel_ms(t, measure, log=False):
    """kernel time of the slot's last call of `measure` without copying the records back"""
    n, ms = C.c_uint64(0), C.c_float(0)
    what = "trew_hip_%s_results" % measure
    args = (t.ctx, 0, None, 0, C.byref(n)) + ((None,) if log else ()) + (C.byref(ms),)
    t._chk(getattr(t.lib, what)(*args), what)
    return ms.value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--penalty", type=int, default=3)
    ap.add_argument("--min_score", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "penalty": a.penalty, "min_score": a.min_score, "long_reads": a.long_reads}
    times = {"satellites": [], "refine": []}
    times.update({"polish%d" % m: [] for m in WIDTHS})
    with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
        b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
        for i in range(a.warmup + a.launches):
            now = {}
            t.satellites(b, 1, 256, a.penalty, a.min_score, max_records=4 * a.long_reads)
            now["satellites"] = kernel_ms(t, "satellites", log=True)
            t.refine(b, 1, 32, a.penalty, a.min_score)
            now["refine"] = kernel_ms(t, "refine")
            for m in WIDTHS:
                t.polish(b, 1, m, a.penalty, a.min_score)
                now["polish%d" % m] = kernel_ms(t, "polish")
                if i == 0:
                    got = t.polish_results()
                    res["polish%d_records" % m] = int((got["period"] > 0).sum())
                    if m == 32:
                        ref = t.refine_results()
                        res["polish32_equals_refine"] = bool(
                            all((got[f] == ref[f]).all() for f in ref.dtype.names[:12])
                            and all(capi.satellite_unit_text(g[u], g[p]) == "".join("TGCA"[(int(x[u]) >> (2 * (int(x[p]) - 1 - j))) & 3] for j in range(int(x[p])))
                                    for g, x in zip(got, ref) for u, p in (("unit", "period"), ("seed_unit", "seed_period"))))
            if i >= a.warmup:
                for k, v in now.items():
                    times[k].append(v)
        for p in ptrs:
            t.free(p)
    for k, v in times.items():
        res[k + "_ms"] = round(float(np.mean(v)), 4)
        res[k + "_spread"] = round(float((np.max(v) - np.min(v)) / np.mean(v)), 4)
    res["polish32_over_refine"] = round(float(np.mean(times["polish32"])) / float(np.mean(times["refine"])), 3)
    res["bases"] = int(bases)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
