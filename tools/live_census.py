"""What the bounds pass drops: the 10 M reads of the bench workload through one submit; the flagged reads, those of them with an N,
the live list and the dead entries, by what the generator made of the read (profiles/live_list/README.md)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import trew_amd as T
from trew_amd import capi

n, L = 10_000_000, 150
buf, st, nd = capi.synth_short_ascii(20250218, 0, n, L)
arr = np.frombuffer(buf, dtype=np.uint8).reshape(n, L + 1)[:, :L]
with T.TrewHip(mode=T.MODE_SHORT, max_batch_reads=n, max_batch_words=16) as t:
    d = t.malloc(n * 60 + 64)
    t.synth_short_device(20250218, 0, n, L, d)
    t.submit(t.device_uniform_batch(d, n, L), 0)
    t.wait(0)
    wl, live, dead = t.debug_worklist(0).copy(), t.debug_live_list(0).copy(), t.debug_counters()["dead_entries"]
    t.free(d)
sub = arr[wl]
has_n = (sub == ord("N")).any(axis=1)
per6 = (sub[:, :-6] == sub[:, 6:]).sum(axis=1)  # period-6 autocorrelation: what the generator made of the read
kind = np.where(per6 >= 130, "telomeric", np.where(per6 >= 80, "junction", "other"))
is_live = np.isin(wl, live)
print("flagged %d, with an N %d, live %d, dead %d" % (len(wl), int(has_n.sum()), len(live), dead))
for k in ("telomeric", "junction", "other"):
    for hn in (False, True):
        m = (kind == k) & (has_n == hn)
        print("%-10s N=%d  flagged %7d  dead %7d" % (k, hn, int(m.sum()), int((m & ~is_live).sum())))
