#!/usr/bin/env python3
"""chains_cost.py -- what a chains reservation (mq_ctx_reserve_chains) costs a device-resident launch: the first --reads reads of the
bench's synthetic batch (tools/sim.py's genome and reads of bench.py's seeds) mapped with mq_ctx_map_batch_device on two contexts of one
index, one without and one with a reservation, the launches alternating and timed by device events.  Needs the library and tools/sim.py
only (device memory and events through ctypes on libamdhip64).  One JSON line: ms per launch for both, `needed` per read.
    python tools/chains_cost.py [--reads 196608] [--genome-scale 1.0] [--steps 10]"""
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
    P = mq.Params()
    ix = mq.Index(P)
    for r in range(len(names)):
        ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])])
    ix.finalize()
    reads = sim.make_reads(g, off, a.reads, seed=a.seed + 1000, threads=a.threads)  # reads [0, --reads) of the bench's batch
    bases, offs = reads["bases"], np.ascontiguousarray(reads["offsets"], dtype=np.uint64)
    n, total = offs.size - 1, int(offs[-1])
    d_bases, d_offs = to_device(bases), to_device(offs)
    d_out = to_device(np.zeros(n * mq.hit_dtype.itemsize, dtype=np.uint8))
    # a read has no more chains than runs, cannot have more runs than k-min-mers, and has fewer k-min-mers than list entries: bytes x (4 density + 1/512), the bound of
    # the minimizer lists, holds for any batch
    bound = int(total * (4 * P.density + 1.0 / 512)) + 64
    plain, anch = ix.context(), ix.context()
    anch.reserve_chains(n, min(bound, (1 << 32) - 2))
    ev = []
    for _ in range(2):
        e = C.c_void_p()
        ok(hip.hipEventCreate(C.byref(e)))
        ev.append(e)
    ms = dict(plain=[], chains=[])
    for step in range(a.warmup + a.steps):
        for tag, c in (("plain", plain), ("chains", anch)):
            ok(hip.hipEventRecord(ev[0], None))
            c.map_batch_device(d_bases, d_offs, n, total, d_out, 0)
            ok(hip.hipEventRecord(ev[1], None))
            ok(hip.hipEventSynchronize(ev[1]))
            t = C.c_float()
            ok(hip.hipEventElapsedTime(C.byref(t), ev[0], ev[1]))
            if step >= a.warmup:
                ms[tag].append(t.value)
    spans, chains, info = anch.chains()
    hits = np.zeros(n, dtype=mq.hit_dtype)
    ok(hip.hipMemcpy(hits.ctypes.data, d_out, hits.nbytes, 2))
    mapped = int((hits["status"] == 1).sum())  # (a tied read has chains and no hit: more reads with chains than mapped ones)
    assert int((spans["count"] > 0).sum()) >= mapped and info["dropped_reads"] == 0 and int(spans["count"].sum()) == info["needed"]

    def stat(v):
        v = sorted(v)
        return dict(ms_median=round(v[len(v) // 2], 4), ms_min=round(v[0], 4), ms_max=round(v[-1], 4))

    print(json.dumps(dict(reads=n, bases=total, genome_scale=a.genome_scale, plain=stat(ms["plain"]), chains=stat(ms["chains"]),
                          spec=dict(plain=plain.last_map_spec(), chains=anch.last_map_spec()), mapped=mapped, needed=info["needed"],
                          needed_per_read=round(info["needed"] / n, 3), needed_per_mapped_read=round(info["needed"] / max(mapped, 1), 3),
                          reserved=min(bound, (1 << 32) - 2), setup_s=round(time.time() - t0, 1))), flush=True)


if __name__ == "__main__":
    main()
