"""Data and a model for the index-extension tests (test_index_extend_host.py, test_gpu_index_extend.py).

Six small contigs with planted shared segments, so that at the split 3 | 3 a k-min-mer key occurs in each of the four ways that
matter when references are added to a finalized index: twice inside the first part, twice inside the second, once in each (LIVE
after the first finalize, DEAD after the second), and once in all.  `extend_model` is the expectation that does not come from the
library: the union of two slot sets (tests/mqx.py's slot_dtype) with counts capped at 2 and the first part's payload kept.
"""
import numpy as np

import mqx

LENS = [42000, 31000, 56000, 24000, 47000, 36000]
SPLIT = 3
SEG = 6000
# (from contig, at) -> (to contig, at): inside the first part, inside the second, and two across the split
PLANTS = [((0, 3000), (1, 9000)), ((4, 5000), (5, 20000)), ((2, 11000), (3, 4000)), ((1, 20000), (4, 30000))]

_cache = {}


def contigs(simlib):
    """(genome bytes, offsets, names) of the six contigs with the segments planted"""
    if "g" not in _cache:
        g, off, names = simlib.make_genome(LENS, seed=77, threads=2)
        g = g.copy()
        for (fc, fa), (tc, ta) in PLANTS:
            g[int(off[tc]) + ta:int(off[tc]) + ta + SEG] = g[int(off[fc]) + fa:int(off[fc]) + fa + SEG]
        _cache["g"] = (g, off, names)
    return _cache["g"]


def contig(simlib, r):
    g, off, _ = contigs(simlib)
    return g[int(off[r]):int(off[r + 1])]


def reads(simlib, n=300):
    if "r" not in _cache:
        g, off, _ = contigs(simlib)
        _cache["r"] = simlib.make_reads(g, off, n, seed=3, len_mean=9000, len_sd=2500, err=0.005, threads=2)
    return _cache["r"]


def insertions(oracle, simlib, refs, po=None):
    """every k-min-mer of the contigs `refs`, in insertion order, as mqx.entry_dtype records with count 1"""
    po = po or oracle.params()
    parts = []
    for r in refs:
        km = oracle.kminmers(contig(simlib, r), po)
        a = np.zeros(km.size, dtype=mqx.entry_dtype)
        for f, o in (("key", "hash"), ("start", "start"), ("end", "end"), ("offset", "offset"), ("rc", "rev")):
            a[f] = km[o]
        a["id"] = r
        a["count"] = 1
        parts.append(a)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=mqx.entry_dtype)


def slot_set(ins):
    """the slots a build of these insertions saves: one per key, the first insertion's payload, count 1 or 2"""
    if ins.size == 0:
        return np.zeros(0, dtype=mqx.slot_dtype)
    _, first, cnt = np.unique(ins["key"], return_index=True, return_counts=True)
    e = ins[first]
    s = np.zeros(e.size, dtype=mqx.slot_dtype)
    for f in ("start", "end", "offset", "key"):
        s[f] = e[f]
    s["id_rc"] = (e["id"] << np.uint32(1)) | (e["rc"] & np.uint32(1))
    s["count"] = np.minimum(cnt, 2)
    s["is_key0"] = (e["key"] == 0).astype(np.uint32)
    return s


def extend_model(a, b):
    """Slot set of "a, then b added": the union of the keys; a key of both has count 2 and a's payload."""
    both = np.concatenate([a, b])  # (np.unique returns the FIRST occurrence: a's slot for a key of both)
    _, first, inv = np.unique(both["key"], return_index=True, return_inverse=True)
    out = both[first].copy()
    total = np.zeros(out.size, dtype=np.uint64)
    np.add.at(total, inv.reshape(-1), both["count"].astype(np.uint64))
    out["count"] = np.minimum(total, 2)
    return out


def kinds(a, b):
    """numbers of keys: twice inside a, twice inside b, once in a and once in b, once in all"""
    ka, kb = dict(zip(a["key"].tolist(), a["count"].tolist())), dict(zip(b["key"].tolist(), b["count"].tolist()))
    twice_a = sum(1 for k, c in ka.items() if c >= 2 and k not in kb)
    twice_b = sum(1 for k, c in kb.items() if c >= 2 and k not in ka)
    once_each = sum(1 for k, c in ka.items() if c == 1 and kb.get(k) == 1)
    once = sum(1 for k, c in ka.items() if c == 1 and k not in kb) + sum(1 for k, c in kb.items() if c == 1 and k not in ka)
    return twice_a, twice_b, once_each, once


def sorted_slots(s, dead_payload=False):
    """slots sorted by key; a dead key's payload is whichever insertion claimed the slot, so it is blanked unless asked for"""
    s = s[np.argsort(s["key"], kind="stable")].copy()
    if not dead_payload:
        dead = (s["count"] != 1) | (s["end"] == 0)
        for f in ("start", "end", "offset", "id_rc"):
            s[f][dead] = 0
        s["count"][dead] = 2
    return s
