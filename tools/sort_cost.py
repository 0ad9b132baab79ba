#!/usr/bin/env python3
"""sort_cost.py -- what the coordinate sorter (mq_sorter) costs, on one MI355X: 2^16 .. 2^22 hit records of a human-like key
distribution (one reference per entry of tools/sim.py's CHM13-like lengths, a reference drawn by its length, r_start uniform inside it, 3 % of the
reads unmapped, ordinals in input order) offered device-resident with mq_sort_add_device (timed by device events) and sorted by
mq_sort_result: the device side between the library's own events (mqdiag_sort_result_ms), the whole call on the host clock, and the same
run's numpy.lexsort of the same arrays on the host beside it.  The order is checked against the lexsort's.  Needs the library and
tools/sim.py only (device memory and events through ctypes on libamdhip64).  One JSON line.
    python tools/sort_cost.py [--min-log2 16] [--max-log2 22] [--steps 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-log2", type=int, default=16)
    ap.add_argument("--max-log2", type=int, default=22)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=2013)
    a = ap.parse_args()
    import mapquik_amd as mq
    from tools import sim
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP call failed: %d" % rc)

    # the sorter reads the index's reference IDS only (r_start is not range-checked): short references stand for the long ones
    full = np.array(sim.CHM13_LIKE, dtype=np.int64)
    g, off, names = sim.make_genome([2000] * full.size, seed=a.seed)
    ix = mq.Index(mq.Params())
    for r in range(len(names)):
        ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])])
    ix.finalize()
    ev = []
    for _ in range(2):
        e = C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e)))
        ev.append(e)
    rng = np.random.default_rng(a.seed)
    rows = []
    for lg in range(a.min_log2, a.max_log2 + 1):
        n = 1 << lg
        hits = np.zeros(n, dtype=mq.hit_dtype)
        hits["ref_id"] = rng.choice(full.size, n, p=full / full.sum())
        hits["r_start"] = (rng.random(n) * full[hits["ref_id"]]).astype(np.uint32)
        hits["status"] = rng.random(n) >= 0.03
        hits["mapq"] = 60
        d_hits = C.c_void_p()
        ok(hip.hipMalloc(C.byref(d_hits), hits.nbytes))
        ok(hip.hipMemcpy(d_hits, hits.ctypes.data, hits.nbytes, 1))
        s = mq.api.Sorter(ix, capacity=n, min_mapq=0)
        add, res, call, host = [], [], [], []
        for step in range(a.warmup + a.steps):
            s.clear()
            ok(hip.hipEventRecord(ev[0], None))
            s.add_device(d_hits.value, n, 0, 0)
            ok(hip.hipEventRecord(ev[1], None))
            ok(hip.hipEventSynchronize(ev[1]))
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]))
            t0 = time.perf_counter()
            order, refs, tot = s.result()
            dt = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            k = np.flatnonzero(hits["status"] == 1)
            want = k[np.lexsort((k, hits["r_start"][k], hits["ref_id"][k]))]
            ht = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(order, want.astype(np.uint32)) and tot["kept"] == k.size and int(refs["count"].sum()) == k.size
            if step >= a.warmup:
                add.append(t.value), res.append(s.result_ms()), call.append(dt), host.append(ht)
        med = lambda v: round(sorted(v)[len(v) // 2], 4)  # noqa: E731
        rows.append(dict(records=n, kept=tot["kept"], passes=s.passes(), add_ms=med(add), result_device_ms=med(res), result_call_ms=med(call), numpy_lexsort_ms=med(host)))
        s.close()
        ok(hip.hipFree(d_hits))
    print(json.dumps(dict(tile_records=int(mq.load_library().mqdiag_sort_tile_records()), steps=a.steps, rows=rows)), flush=True)


if __name__ == "__main__":
    main()
