#!/usr/bin/env python3
"""redo_cost.py -- what a redo arena (mq_map_reserve_redo) costs a device-resident launch: the bench's batch (bench.py's genome, index and
reads, built the same way) mapped with mq_map_batch_device, timed by device events, at --reads and at its first --small reads; with
--reserve R,L the index's default context holds an arena for R reads of L bases.  One process = one measurement = one JSON line; the
library is the tree's, or another build's through MQ_LIB (the parent commit's, which knows no arena: no --reserve then).
    python tools/redo_cost.py [--reserve 256,65536] [--genome-preset human-like] [--genome-cache DIR]
A/B of three sides (parent library, this library, this library with an arena): five processes a side, alternating, same flags."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cached_genome(make, path):
    """the genome of make() kept as three .npy files under `path` (a run of many processes synthesises it once)"""
    if not path:
        return make()
    f = [os.path.join(path, n) for n in ("genome.npy", "ctg_off.npy", "ctg_names.npy")]
    if all(os.path.exists(x) for x in f):
        return np.load(f[0]), np.load(f[1]), [str(x) for x in np.load(f[2])]
    g, off, names = make()
    os.makedirs(path, exist_ok=True)
    for x, a in zip(f, (g, off, np.array(names))):
        np.save(x + ".tmp.npy", a)
        os.replace(x + ".tmp.npy", x)
    return g, off, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1572864)
    ap.add_argument("--small", type=int, default=49152)
    ap.add_argument("--genome-scale", type=float, default=1.0)
    ap.add_argument("--genome-preset", choices=("planted-repeats", "human-like"), default="planted-repeats")
    ap.add_argument("--seed", type=int, default=2013)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reserve", default="", help="max_reads,max_read_len of the redo arena (default: none)")
    ap.add_argument("--genome-cache", default="", help="directory that keeps the synthesised genome between processes")
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    import torch

    import bench
    import mapquik_amd as mq
    from tools import sim
    t0 = time.time()
    dev = torch.device("cuda", 0)
    ncpu = bench.effective_cpus()
    lens = [max(40, int(x * a.genome_scale)) for x in sim.CHM13_LIKE]
    kw = sim.HUMAN_LIKE if a.genome_preset == "human-like" else dict(repeat_frac=0.05, tandem_frac=0.01, div=0.01)
    cache = os.path.join(a.genome_cache, "%s_%g_%d" % (a.genome_preset, a.genome_scale, a.seed)) if a.genome_cache else ""
    g, off, names = cached_genome(lambda: sim.make_genome(lens, seed=a.seed, threads=ncpu, **kw), cache)
    ix = bench.build_index_device(mq, torch, dev, 0, mq.Params(), g, off, names)[0]
    B = bench.load_batch(torch, dev, sim, g, off, a.reads, a.seed + 1000, ncpu)
    d_out = torch.empty(B.n * mq.hit_dtype.itemsize, dtype=torch.uint8, device=dev)
    ix.reserve(B.n, B.total_bases)
    if a.reserve:
        r, l = (int(x) for x in a.reserve.split(","))
        ix.reserve_redo(r, l)
    st = torch.cuda.current_stream(dev)
    res = dict(tag=a.tag, lib=os.environ.get("MQ_LIB", "tree"), reserve=a.reserve or None, genome_preset=a.genome_preset, genome_scale=a.genome_scale,
               setup_s=round(time.time() - t0, 1))
    for n in (a.reads, min(a.small, a.reads)):
        total = int(B.offsets[n])

        def step():
            ix.map_batch_device(B.d_bases.data_ptr(), B.d_offs.data_ptr(), n, total, d_out.data_ptr(), st.cuda_stream)

        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
        for e0, e1 in ev:
            e0.record(st)
            step()
            e1.record(st)
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        hits = np.frombuffer(d_out[:n * mq.hit_dtype.itemsize].cpu().numpy().tobytes(), dtype=mq.hit_dtype)
        res["n%d" % n] = dict(ms_median=round(ms[len(ms) // 2], 4), ms_min=round(ms[0], 4), ms_max=round(ms[-1], 4), gbases_s=round(total / ms[len(ms) // 2] / 1e6, 1),
                              overflow_reads=int((hits["status"] == 2).sum()), mapped=int((hits["status"] == 1).sum()),
                              redo_counts=list(ix.redo_counts()) if a.reserve else None)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
