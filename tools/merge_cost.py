#!/usr/bin/env python3
"""merge_cost.py -- what merging two finalized indexes costs, on one MI355X: the bench genome (tools/sim.py's CHM13-like contigs under
bench.py's seed and planted-repeats preset) split into two halves by contig, each half built into an index of its own, and then
    merge, table to table     mq_index_merge(A, B) on one device (merge_table_kernel)
    merge, packed slots       the same with MQ_MERGE_PACKED=1 (pack_slots_kernel, a device-to-device copy, merge_slots_kernel)
    merge, file               mq_index_merge_file(A, B.mqx), B.mqx on tmpfs (--tmp, default /dev/shm)
    build, whole              every contig resident on the device, mq_index_add_ref_device of each + mq_index_finalize, for comparison
    resize of the source      mq_index_resize(B) to twice its table and back (retable_kernel: the same stream in, the same random
                              inserts out, into an EMPTY table), for comparison
every call timed on the host around the call (each ends with a read-back that waits for the device), --steps times, the median.  A merge
changes its destination, so each timed merge gets a fresh clone of A in a table of the whole build's size (mq_index_clone_sized, not
timed: the merge is then timed without a growth in front of it).  One JSON line.
    python tools/merge_cost.py [--genome-scale 1.0] [--steps 5] [--factor 8]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=2013)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--factor", type=int, default=8, help="table slots per k-min-mer of every index here (the library's default)")
    ap.add_argument("--tmp", default="/dev/shm")
    ap.add_argument("--threads", type=int, default=min(16, len(os.sched_getaffinity(0))))
    a = ap.parse_args()
    import mapquik_amd as mq
    from tools import sim
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def ok(rc):
        if rc != 0:
            raise RuntimeError("HIP call failed: %d" % rc)

    t0 = time.time()
    lens = [max(40, int(x * a.genome_scale)) for x in sim.CHM13_LIKE]
    g, off, names = sim.make_genome(lens, seed=a.seed, threads=a.threads, repeat_frac=0.05, tandem_frac=0.01, div=0.01)  # bench.py's planted-repeats preset
    n = len(names)
    d_g = C.c_void_p()
    ok(hip.hipMalloc(C.byref(d_g), g.nbytes + 64))
    ok(hip.hipMemcpy(d_g, g.ctypes.data, g.nbytes, 1))
    half_a, half_b = list(range(0, n, 2)), list(range(1, n, 2))  # alternate contigs: two halves of about equal size

    def build(refs):
        ix = mq.Index(mq.Params())
        ix.set_table_factor(a.factor)
        t = time.perf_counter()
        for r in refs:
            ix.add_ref_device(r, names[r], d_g.value + int(off[r]), int(off[r + 1] - off[r]))
        ix.finalize()
        return ix, (time.perf_counter() - t) * 1e3

    def med(v):
        v = sorted(v)
        return dict(ms_median=round(v[len(v) // 2], 3), ms_min=round(v[0], 3), ms_max=round(v[-1], 3))

    A, _ = build(half_a)
    B, _ = build(half_b)
    path = os.path.join(a.tmp, "merge_cost_%d.mqx" % os.getpid())
    B.save(path)
    ms = dict(table=[], packed=[], file=[], build=[], resize=[])
    whole_stats = None
    try:
        for step in range(a.steps + 1):  # (the first round warms up: code objects, the allocator)
            W, t_build = build(range(n))
            whole_stats = W.stats()
            W.close()
            got = {}
            for route in ("table", "packed", "file"):
                D = A.clone(0, table_slots=whole_stats["table_slots"])  # (the whole build's table: the merge itself, no growth in front of it)
                if route == "packed":
                    os.environ["MQ_MERGE_PACKED"] = "1"
                t = time.perf_counter()
                if route == "file":
                    D.merge_file(path, id_base=0)
                else:
                    D.merge(B, id_base=0)
                got[route] = (time.perf_counter() - t) * 1e3
                os.environ.pop("MQ_MERGE_PACKED", None)
                st = D.stats()
                assert all(st[k] == whole_stats[k] for k in ("n_refs", "n_kminmers", "n_keys", "n_unique")), (route, st, whole_stats)
                D.close()
            slots = B.stats()["table_slots"]
            t = time.perf_counter()
            B.resize(table_slots=2 * slots)
            t_up = (time.perf_counter() - t) * 1e3
            B.resize(table_slots=slots)
            if step:
                ms["build"].append(t_build)
                ms["resize"].append(t_up)
                for route in got:
                    ms[route].append(got[route])
    finally:
        os.unlink(path)
    sa, sb = A.stats(), B.stats()
    print(json.dumps(dict(genome_scale=a.genome_scale, genome_bases=int(off[-1]), factor=a.factor, steps=a.steps,
                          a=dict(n_keys=sa["n_keys"], table_slots=sa["table_slots"]), b=dict(n_keys=sb["n_keys"], table_slots=sb["table_slots"]),
                          whole=dict(n_keys=whole_stats["n_keys"], n_unique=whole_stats["n_unique"], table_slots=whole_stats["table_slots"]),
                          merge_table=med(ms["table"]), merge_packed=med(ms["packed"]), merge_file=med(ms["file"]), build_whole=med(ms["build"]),
                          resize_source_x2=med(ms["resize"]), table_over_resize=round(med(ms["table"])["ms_median"] / med(ms["resize"])["ms_median"], 2),
                          setup_s=round(time.time() - t0, 1))), flush=True)


if __name__ == "__main__":
    main()
