#!/usr/bin/env python3
"""Timing of trew_hip_chain next to trew_hip_variants on the same device-resident batches (HIP events, one stream, one
process, the two kernels alternating launch by launch).

    python tools/chain_bench.py [--long_reads 20000] [--reads 1000000] [--len 150] [--warmup 5] [--launches 30] [--out FILE]

One motif, TTAGGG; the chain's log is large enough for every event (the size comes from a first launch with a log of one
entry, whose counter reports the need).  Prints one JSON object with, per batch (long / short):
  <batch>_chain_ms / _variants_ms       kernel time from ms_kernel, the mean of --launches launches after --warmup
  <batch>_chain_over_variants           their ratio
  <batch>_events / _items / _runs / _variants / _events_per_read
                                        what one launch appends (events), what they pair into (items = runs + variants)
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import trew_amd as T  # noqa: E402

SEED = 20250218
MOTIFS = ["TTAGGG"]


def variants_ms(t):
    n, ms = C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_variants_results(t.ctx, 0, None, 0, C.byref(n), None, None, C.byref(ms)), "trew_hip_variants_results")
    return ms.value


def chain_ms(t, counts=None):
    """(kernel ms, items, events) of the slot's last chain, without pairing anything"""
    ni, ne, ms = C.c_uint64(0), C.c_uint64(0), C.c_float(0)
    t._chk(t.lib.trew_hip_chain_results(t.ctx, 0, None, 0, C.byref(ni), C.byref(ne), counts.ctypes.data if counts is not None else None, C.byref(ms)),
           "trew_hip_chain_results")
    return ms.value, int(ni.value), int(ne.value)


def alternate(t, batch, n_reads, warmup, launches):
    t.chain(batch, MOTIFS, 1)
    counts = np.zeros((n_reads, len(MOTIFS), 2, 2), dtype=np.uint32)
    _, items, events = chain_ms(t, counts)
    cap = max(events, 1)
    work = {"events": events, "items": items, "runs": int(counts[..., 0].astype(np.uint64).sum()), "variants": int(counts[..., 1].astype(np.uint64).sum()),
            "events_per_read": round(events / max(n_reads, 1), 3)}
    for _ in range(warmup):
        t.variants(batch, MOTIFS)
        t.chain(batch, MOTIFS, cap)
    t.wait(0)
    a = b = 0.0
    for _ in range(launches):
        t.variants(batch, MOTIFS)
        a += variants_ms(t)
        t.chain(batch, MOTIFS, cap)
        ms, _, ev = chain_ms(t)
        assert ev == events
        b += ms
    return a / launches, b / launches, work


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--len", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--long_reads", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"warmup": a.warmup, "launches": a.launches, "motif": MOTIFS[0]}

    def record(prefix, va, ch, work):
        res.update({prefix + "_variants_ms": round(va, 4), prefix + "_chain_ms": round(ch, 4), prefix + "_chain_over_variants": round(ch / va, 3)})
        res.update({prefix + "_" + k: v for k, v in work.items()})

    if a.long_reads:
        with T.TrewHip(mode=T.MODE_LONG, n_slots=1, max_batch_words=16, max_batch_reads=a.long_reads, table_log2_slots=12) as t:
            b, ptrs, bases = t.synth_long_device(SEED, 0, a.long_reads)
            res.update(long_reads=a.long_reads, long_bases=bases)
            record("long", *alternate(t, b, a.long_reads, a.warmup, a.launches))
            for p in ptrs:
                t.free(p)

    if a.reads:
        n, L = a.reads, a.len
        stride = 3 * ((L + 31) // 32)
        with T.TrewHip(mode=T.MODE_SHORT, n_slots=1, max_batch_words=16, max_batch_reads=n, table_log2_slots=12) as t:
            d = t.malloc(n * stride * 4 + 64)
            t.synth_short_device(SEED, 0, n, L, d)
            b = t.device_uniform_batch(d, n, L)
            res.update(short_reads=n, short_len=L)
            record("short", *alternate(t, b, n, a.warmup, a.launches))
            t.free(d)

    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
