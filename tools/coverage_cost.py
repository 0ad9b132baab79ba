#!/usr/bin/env python3
"""coverage_cost.py -- what mq_index_coverage costs, on one MI355X: on the bench's synthetic index (tools/sim.py's CHM13-like contigs under
bench.py's seed and planted-repeats preset, every contig resident on the device and indexed from there) or on any --index file, the call
--steps times behind one warm-up with MQ_COVER_TIMING=1, which puts events around every launch (and a wait behind each, so the whole
call is also timed once more without it).  One JSON line: table slots and live entries, bitmap bytes and intervals, the median
milliseconds (and smallest / largest) of the bitmap's clearing and of each kernel, of the whole call (host clock around it, timed and untimed), and from the same
runs count_kernel's pass over the same table -- a plain stream of the table, which the mark pass cannot beat -- with the ratio.
    python tools/coverage_cost.py [--genome-scale 1.0] [--steps 5] [--factor 8] [--index file.mqx]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = ("bitmap_clear", "cover_mark_kernel", "cover_count_kernel", "cover_scan_kernel", "cover_emit_kernel", "count_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=2013)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--factor", type=int, default=8, help="table slots per k-min-mer of the synthetic index (the library's default)")
    ap.add_argument("--index", help="a saved index instead of the synthetic one")
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    import mapquik_amd as mq
    t0 = time.time()
    if a.index:
        ix = mq.Index.load(a.index)
    else:
        from tools import sim
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        lens = [max(40, int(x * a.genome_scale)) for x in sim.CHM13_LIKE]
        g, off, names = sim.make_genome(lens, seed=a.seed, threads=a.threads, repeat_frac=0.05, tandem_frac=0.01, div=0.01)  # bench.py's planted-repeats preset
        d_g = C.c_void_p()
        for rc in (hip.hipMalloc(C.byref(d_g), g.nbytes + 64), hip.hipMemcpy(d_g, g.ctypes.data, g.nbytes, 1)):
            if rc != 0:
                raise RuntimeError("HIP call failed: %d" % rc)
        ix = mq.Index(mq.Params())
        ix.set_table_factor(a.factor)
        for r in range(len(names)):
            ix.add_ref_device(r, names[r], d_g.value + int(off[r]), int(off[r + 1] - off[r]))
        ix.finalize()
    L = mq.load_library()
    st = ix.stats()

    def med(v):
        v = sorted(v)
        return round(v[len(v) // 2], 3)

    ms = {n: [] for n in NAMES}
    call_timed, call_plain = [], []
    out = (C.c_float * 6)()
    for step in range(a.steps + 1):  # (the first round warms up: code objects, the allocator)
        os.environ["MQ_COVER_TIMING"] = "1"
        t = time.perf_counter()
        refs, ivs, oor = ix.coverage()
        dt = (time.perf_counter() - t) * 1e3
        if L.mqdiag_coverage_ms(out) != 0:
            raise RuntimeError("mqdiag_coverage_ms")
        del os.environ["MQ_COVER_TIMING"]
        t = time.perf_counter()
        ix.coverage()
        dp = (time.perf_counter() - t) * 1e3
        if step:
            call_timed.append(dt)
            call_plain.append(dp)
            for n, v in zip(NAMES, out):
                ms[n].append(float(v))
    m = {n: med(v) for n, v in ms.items()}
    words = int(((refs["len"] + 63) // 64).sum())
    print(json.dumps(dict(index=a.index or "synthetic", genome_scale=None if a.index else a.genome_scale, steps=a.steps, table_slots=st["table_slots"], table_bytes=st["table_bytes"],
                          n_keys=st["n_keys"], live_entries=int(refs["live_kminmers"].sum()), n_unique=st["n_unique"], out_of_range=oor, references=int(refs.size),
                          bases=int(refs["len"].sum()), covered_bases=int(refs["covered_bases"].sum()), bitmap_bytes=8 * words, intervals=int(ivs.size), ms=m,
                          ms_min_max={n: [round(min(v), 3), round(max(v), 3)] for n, v in ms.items()},
                          call_ms=med(call_plain), call_ms_with_events=med(call_timed), mark_over_count_kernel=round(m["cover_mark_kernel"] / m["count_kernel"], 2),
                          kernels_over_count_kernel=round(sum(m[n] for n in NAMES[:5]) / m["count_kernel"], 2), setup_s=round(time.time() - t0, 1))), flush=True)


if __name__ == "__main__":
    main()
