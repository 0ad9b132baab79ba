#!/usr/bin/env python3
"""depth_cost.py -- what the depth accumulator (mq_depth) costs, on one MI355X: the first --reads reads of the bench's synthetic batch
(tools/sim.py's genome and reads of bench.py's seeds) mapped with mq_ctx_map_batch_device, the launch alone and the launch with
mq_depth_add_device queued behind it on the same stream, alternating and timed by device events; the add alone; and mq_depth_result at
the default window (its three kernels between the library's own events, and the whole call on the host clock).  Needs the library and
tools/sim.py only (device memory and events through ctypes on libamdhip64).  One JSON line.
    python tools/depth_cost.py [--reads 196608] [--genome-scale 1.0] [--steps 10] [--window 1000] [--min-mapq 60]"""
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
    ap.add_argument("--reads", type=int, default=196608)
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=2013)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--min-mapq", type=int, default=60)
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    import mapquik_amd as mq
    from tools import sim
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
    hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
    hip.hipEventSynchronize.argtypes = [C.c_void_p]
    hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP call failed: %d" % rc)

    def to_device(arr):
        p = C.c_void_p()
        ok(hip.hipMalloc(C.byref(p), max(arr.nbytes, 1) + 64))
        ok(hip.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1))
        return p.value

    t0 = time.time()
    lens = [max(40, int(x * a.genome_scale)) for x in sim.CHM13_LIKE]
    g, off, names = sim.make_genome(lens, seed=a.seed, threads=a.threads, repeat_frac=0.05, tandem_frac=0.01, div=0.01)  # bench.py's planted-repeats preset
    ix = mq.Index(mq.Params())
    for r in range(len(names)):
        ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])])
    ix.finalize()
    reads = sim.make_reads(g, off, a.reads, seed=a.seed + 1000, threads=a.threads)  # reads [0, --reads) of the bench's batch
    bases, offs = reads["bases"], np.ascontiguousarray(reads["offsets"], dtype=np.uint64)
    n, total = offs.size - 1, int(offs[-1])
    d_bases, d_offs = to_device(bases), to_device(offs)
    d_out = to_device(np.zeros(n * mq.hit_dtype.itemsize, dtype=np.uint8))
    ctx = ix.context()
    depth = mq.api.Depth(ix, window=a.window, min_mapq=a.min_mapq)
    ev = []
    for _ in range(2):
        e = C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e)))
        ev.append(e)

    def timed(f):
        ok(hip.hipEventRecord(ev[0], None))
        f()
        ok(hip.hipEventRecord(ev[1], None))
        ok(hip.hipEventSynchronize(ev[1]))
        t = C.c_float()
        ok(hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]))
        return t.value

    def launch():
        ctx.map_batch_device(d_bases, d_offs, n, total, d_out, 0)

    def launch_and_add():
        ctx.map_batch_device(d_bases, d_offs, n, total, d_out, 0)
        depth.add_device(d_out, n, 0)

    ms = dict(launch=[], launch_and_add=[], add=[])
    adds = 0
    for step in range(a.warmup + a.steps):  # the two forms alternate: one box, one index, one batch
        for tag, f in (("launch", launch), ("launch_and_add", launch_and_add), ("add", lambda: depth.add_device(d_out, n, 0))):
            t = timed(f)
            adds += tag != "launch"
            if step >= a.warmup:
                ms[tag].append(t)
    L = mq.load_library()
    res_kernels, res_call = [], []
    for step in range(a.warmup + a.steps):
        t = time.perf_counter()
        refs, wb, ws, tot = depth.result()
        dt = (time.perf_counter() - t) * 1e3
        k = C.c_float()
        ok(L.mqdiag_depth_result_ms(depth._h, C.byref(k)))
        if step >= a.warmup:
            res_kernels.append(k.value)
            res_call.append(dt)
    hits = np.zeros(n, dtype=mq.hit_dtype)
    ok(hip.hipMemcpy(hits.ctypes.data, d_out, hits.nbytes, 2))
    counted = int(((hits["status"] == 1) & (hits["mapq"] >= a.min_mapq)).sum())
    # (a mapped hit the rules turn away -- coordinates that find_coords wrapped -- is out_of_range, not counted)
    assert tot["offered"] == adds * n and tot["counted"] + tot["out_of_range"] == adds * counted and tot["counted"] == int(refs["reads"].sum()), (tot, adds, counted)
    assert int(wb.sum()) == int(refs["bases"].sum())

    def stat(v):
        v = sorted(v)
        return dict(ms_median=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4))

    m = {k: stat(v) for k, v in ms.items()}
    print(json.dumps(dict(reads=n, bases=total, hit_bytes=n * 48, genome_scale=a.genome_scale, window=a.window, min_mapq=a.min_mapq, windows=int(wb.size),
                          accumulator_bytes=16 * int(wb.size), result_bytes=12 * int(wb.size), counted=tot["counted"], out_of_range=tot["out_of_range"], adds=adds, zero_windows=int(refs["zero_windows"].sum()),
                          launch=m["launch"], launch_and_add=m["launch_and_add"], add_alone=m["add"],
                          launch_and_add_over_launch=round(m["launch_and_add"]["ms_median"] / m["launch"]["ms_median"], 4),
                          result_kernels=stat(res_kernels), result_call=stat(res_call), setup_s=round(time.time() - t0, 1))), flush=True)


if __name__ == "__main__":
    main()
