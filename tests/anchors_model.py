"""The expected anchor list of a read -- the Match runs of its winning pseudo-chain, what Chain::filter_matches_max leaves
(src/chain.rs:123-129) for the reference find_largest_two_chains picks -- worded twice, from different material:

  by_model()   tests/chain_model.py: runs_of() for the runs, stays() for the filter, the winner by map_read()'s rule (strictly largest
               score in first-seen order, a runner-up of the same score: no winner), all on Python ints
  by_oracle()  the oracle's C functions through oracle.lib(): mqo_chain_matches_explicit for the runs, mqo_check_match_compatible against
               the first run of largest count for the filter; the winner here as "the first candidate with the top score, unless two
               candidates have it"

Both take the oracle's k-min-mers and index answers of the read (as chain_model.map_with_oracle does) and return None for a read without a
winner (unmapped, tied, too short), else Expected(ref, rc, runs) with runs = [(q_start, q_end, r_start, r_end, count)] in read order: raw
coordinates, q_end / r_end as the Match holds them (get_match subtracts 1), before find_coords.  The library's mq_anchor holds the low 32
bits of each (as32()).
"""
import collections
import ctypes as C

import numpy as np

import chain_model

Expected = collections.namedtuple("Expected", "ref rc runs")


def _lookups(O, ox, po, seq):
    """(k-min-mers as the oracle lists them, entry array, hit flags)"""
    km = O.kminmers(seq, po)
    ent = np.zeros(km.size, dtype=O.entry_dtype)
    hit = np.zeros(km.size, dtype=np.uint8)
    get = O.lib().mqo_index_get
    for i, h in enumerate(km["hash"].tolist()):
        p = get(ox.h, h)
        if p:
            ent[i] = np.frombuffer((C.c_char * O.entry_dtype.itemsize).from_address(p), dtype=O.entry_dtype)[0]
            hit[i] = 1
    return km, ent, hit


def _tuple(r):
    return (int(r.q_start), int(r.q_end), int(r.r_start), int(r.r_end), int(r.count))


def by_model(O, ox, po, seq):
    if len(seq) < po.l + po.k - 1:
        return None
    km, ent, hit = _lookups(O, ox, po, seq)
    kmers = list(zip(km["start"].tolist(), km["end"].tolist(), (km["rev"] != 0).tolist()))
    entries = [dict(id=int(e["id"]), start=int(e["start"]), end=int(e["end"]), offset=int(e["offset"]), rc=bool(e["rc"])) if h else None
               for e, h in zip(ent, hit.tolist())]
    per_ref = {}
    for r in chain_model.runs_of(kmers, entries):
        per_ref.setdefault(r.ref, []).append(r)
    g = int(po.g)
    cands = []  # (ref, kept, score) in first-seen order
    for ref, rs in per_ref.items():
        kept = rs
        if len(rs) > 1:
            anchor = rs[0]
            for r in rs[1:]:
                if r.count > anchor.count:
                    anchor = r
            kept = [r for r in rs if chain_model.stays(anchor, r, g)]
        if kept:
            cands.append((ref, kept, sum(r.count for r in kept)))
    if not cands:
        return None
    best = 0
    if len(cands) > 1:
        top = top_score = runner_up = 0
        for i, (_, _, sc) in enumerate(cands):
            if sc > top_score:
                runner_up, top, top_score = top_score, i, sc
            elif sc > runner_up:
                runner_up = sc
        if top_score == runner_up:
            return None
        best = top
    ref, kept, _ = cands[best]
    return Expected(int(ref), bool(kept[0].rc), [_tuple(r) for r in kept])


def by_oracle(O, ox, po, seq):
    if len(seq) < po.l + po.k - 1:
        return None
    L = O.lib()
    km, ent, hit = _lookups(O, ox, po, seq)
    n = km.size
    ms = np.zeros(max(n, 1), dtype=O.match_dtype)
    refs = np.zeros(max(n, 1), dtype=np.uint64)
    nm = L.mqo_chain_matches_explicit(km.ctypes.data, ent.ctypes.data, hit.ctypes.data, n, ms.ctypes.data, refs.ctypes.data, max(n, 1)) if n else 0
    ms, refs = ms[:nm], refs[:nm]
    order = []  # references in first-seen order
    for r in refs.tolist():
        if r not in order:
            order.append(r)
    lists, scores = [], []
    for r in order:
        grp = np.ascontiguousarray(ms[refs == r])
        if grp.size > 1:
            anchor = grp[int(np.argmax(grp["count"])):][:1]  # (argmax: the first of the largest)
            keep = [bool(L.mqo_check_match_compatible(anchor.ctypes.data, grp[i:i + 1].ctypes.data, int(po.g))) for i in range(grp.size)]
            grp = grp[np.array(keep)]
        if grp.size:
            lists.append((r, grp))
            scores.append(int(grp["count"].sum()))
    if not lists:
        return None
    top = max(scores)
    if scores.count(top) > 1:
        return None
    ref, grp = lists[scores.index(top)]
    return Expected(int(ref), bool(grp["rc"][0]), [tuple(int(x[f]) for f in ("q_start", "q_end", "r_start", "r_end", "count")) for x in grp])


def as32(runs):
    """the runs as the library's mq_anchor holds them: the low 32 bits of every field"""
    return [tuple(v & 0xFFFFFFFF for v in r) for r in runs]


def ends_candidate(exp, po):
    """chain_model.candidate()'s tuple (rc, q_start, q_end, r_start, r_end, score, mapq) from the list's two ends, its length and its counts
    alone: what get_match (src/chain.rs:147-169) makes of the list"""
    U64 = chain_model.U64
    a, z = exp.runs[0], exp.runs[-1]
    score = sum(r[4] for r in exp.runs)
    c, s = int(po.c), int(po.s)
    mapq = 60 if (c != 0 and s != 0 and (len(exp.runs) >= c or score >= s)) else 0
    if exp.rc and len(exp.runs) > 1:
        r_start, r_end = z[2], (a[3] - 1) & U64
    else:
        r_start, r_end = a[2], (z[3] - 1) & U64
    return exp.rc, a[0], (z[1] - 1) & U64, r_start, r_end, score, mapq


def batch(O, ox, po, bases, offs, word=by_model):
    """the expected value of every read of a batch"""
    return [word(O, ox, po, bases[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]
