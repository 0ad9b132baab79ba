"""The expected chain list of a read -- one candidate pseudo-chain per reference that has a Match run in the read, what find_matches builds
and find_largest_two_chains looks through (src/mers.rs:77-129) -- worded twice, from different material:

  by_model()   tests/chain_model.py: runs_of() for the runs, candidate() for get_match, place() for find_coords, all on Python ints
  by_oracle()  the oracle's C functions through oracle.lib(): mqo_chain_matches_explicit for the runs, mqo_check_match_compatible against
               the first run of largest count for the filter; get_match's ends and find_coords in numpy uint64 arithmetic

Both take the oracle's k-min-mers and index answers of the read and return the list of
    (flags, ref, rc, mapq, q_start64, q_end64, r_start, r_end, score, n_runs)
in the order of each reference's first run in the read ([] for a read without a run or shorter than l + k - 1).  flags = 1 (MQ_CHAIN_TOP)
for every chain with the read's largest score: a read is mapped exactly when one chain has it.  r_start / r_end are the low 32 bits, as
the library's mq_chain (and mq_hit) hold them.

batches() builds, once per process, the inputs the GPU tests use (test_chains_model.py asserts on the CPU that they contain what they are
named after).
"""
import numpy as np

import anchors_model
import chain_model
import directed
import mosaic as M

TOP = 1
M32 = 0xFFFFFFFF


def by_model(O, ox, po, seq):
    if len(seq) < po.l + po.k - 1:
        return []
    km, ent, hit = anchors_model._lookups(O, ox, po, seq)
    kmers = list(zip(km["start"].tolist(), km["end"].tolist(), (km["rev"] != 0).tolist()))
    entries = [dict(id=int(e["id"]), start=int(e["start"]), end=int(e["end"]), offset=int(e["offset"]), rc=bool(e["rc"])) if h else None
               for e, h in zip(ent, hit.tolist())]
    per_ref = {}
    for r in chain_model.runs_of(kmers, entries):
        per_ref.setdefault(r.ref, []).append(r)
    c, s, g = int(po.c), int(po.s), int(po.g)
    out = []
    for ref, rs in per_ref.items():
        cd = chain_model.candidate(rs, c, s, g)
        if cd is None:
            continue
        kept = rs
        if len(rs) > 1:  # n_runs: the list candidate() filtered (find_largest_match: the first run of the largest count)
            anchor = rs[0]
            for r in rs[1:]:
                if r.count > anchor.count:
                    anchor = r
            kept = [r for r in rs if chain_model.stays(anchor, r, g)]
        p = chain_model.place(len(seq), int(ox.ref_len(ref)), cd)
        out.append([0, int(ref), int(p["rc"]), int(p["mapq"]), int(p["q_start"]), int(p["q_end"]), int(p["r_start"]) & M32, int(p["r_end"]) & M32,
                    int(p["score"]), len(kept)])
    top = max((x[8] for x in out), default=0)
    return [tuple([TOP if x[8] == top else 0] + x[1:]) for x in out]


def by_oracle(O, ox, po, seq):
    if len(seq) < po.l + po.k - 1:
        return []
    L = O.lib()
    km, ent, hit = anchors_model._lookups(O, ox, po, seq)
    n = km.size
    ms = np.zeros(max(n, 1), dtype=O.match_dtype)
    refs = np.zeros(max(n, 1), dtype=np.uint64)
    nm = L.mqo_chain_matches_explicit(km.ctypes.data, ent.ctypes.data, hit.ctypes.data, n, ms.ctypes.data, refs.ctypes.data, max(n, 1)) if n else 0
    ms, refs = ms[:nm], refs[:nm]
    order = []
    for r in refs.tolist():
        if r not in order:
            order.append(r)
    u = np.uint64
    one = u(1)
    q_len = u(len(seq))
    c, s = int(po.c), int(po.s)
    out = []
    with np.errstate(over="ignore"):
        for r in order:
            grp = np.ascontiguousarray(ms[refs == r])
            if grp.size > 1:
                anchor = grp[int(np.argmax(grp["count"])):][:1]
                keep = [bool(L.mqo_check_match_compatible(anchor.ctypes.data, grp[i:i + 1].ctypes.data, int(po.g))) for i in range(grp.size)]
                grp = grp[np.array(keep)]
            if not grp.size:
                continue
            a, z = grp[0], grp[-1]
            rc = bool(a["rc"])
            score = int(grp["count"].sum())
            mapq = 60 if (c != 0 and s != 0 and (grp.size >= c or score >= s)) else 0
            # get_match (src/chain.rs:162-168)
            q_start, q_end = u(a["q_start"]), u(z["q_end"]) - one
            if rc and grp.size > 1:
                r_start, r_end = u(z["r_start"]), u(a["r_end"]) - one
            else:
                r_start, r_end = u(a["r_start"]), u(z["r_end"]) - one
            # find_coords (src/mers.rs:131-183)
            r_len = u(int(ox.ref_len(int(r))))
            tail = q_len - q_end - one
            if not rc:
                frs, exc_s = (r_start - q_start, q_start) if r_start >= q_start else (u(0), r_start)
                fre, exc_e = (r_end + tail, tail) if r_end + tail <= r_len - one else (r_len - one, r_len - r_end - one)
            else:
                fre, exc_s = (r_end + q_start, q_start) if r_end + q_start <= r_len - one else (r_len - one, r_len - r_end - one)
                frs, exc_e = (r_start - tail, tail) if r_start >= tail else (u(0), r_start)
            out.append([0, int(r), int(rc), mapq, int(q_start - exc_s), int(q_end + exc_e), int(frs) & M32, int(fre) & M32, score, int(grp.size)])
    top = max((x[8] for x in out), default=0)
    return [tuple([TOP if x[8] == top else 0] + x[1:]) for x in out]


def batch(O, ox, po, bases, offs, word=by_model):
    """the expected value of every read of a batch"""
    return [word(O, ox, po, bases[int(offs[i]):int(offs[i + 1])]) for i in range(offs.size - 1)]


def as_words(ch):
    """a model tuple as the twelve words of the library's mq_chain"""
    f, ref, rc, mapq, qs, qe, rs, re_, score, n = ch
    return (f, ref, rc, mapq, qs & M32, qe & M32, rs, re_, score, n, qs >> 32, qe >> 32)


def n_top(chs):
    return sum(1 for c in chs if c[0] & TOP)


# ------------------------------------------------------------------ the inputs
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 128, 129)
MATCH_CAP = 64  # the MQ_MATCH_CAP the redo tests set: the reads of "counts" with 65 chains and more have more runs than that


def _exact_count_reads(g, off, ox, po, rng):
    """For every N of COUNTS a read with exactly N chains: N slices of N different contigs (a tiny contig whole, 1200 bases of a longer one),
    each of which maps alone to its contig with one run.  A slice inside a read can lose or gain a run at its junctions, so the oracle
    counts the candidates of a few shuffles and the first with exactly N stays."""
    n_ctg = off.size - 1
    slices = []
    for c in range(n_ctg):
        clen = int(off[c + 1] - off[c])
        ln = min(clen, 1200)
        slices.append(M._slice(g, off, c, int(rng.integers(0, clen - ln + 1)), ln, bool(rng.integers(0, 2)))[0])
    b, o = M.concat(slices)
    out, diag = ox.map_batch_diag(b, o, po, threads=4)
    good = [c for c in range(n_ctg) if out["mapped"][c] and int(out["ref_id"][c]) == c and int(diag["n_matches"][c]) == 1]
    reads = {}
    for n in COUNTS:
        assert len(good) >= n, (len(good), n)
        tries = [np.concatenate([slices[int(c)] for c in rng.choice(good, size=n, replace=False)]) for _ in range(12)]
        tb, to = M.concat(tries)
        d = ox.map_batch_diag(tb, to, po, threads=4)[1]
        hit = [i for i in range(len(tries)) if int(d["n_candidates"][i]) == n]
        assert hit, n
        reads[n] = tries[hit[0]]
    return reads


_BATCHES = None


def batches(O, sim):
    """(genome, ctg_off, names, sets) of the mosaic world and sets[name] = (bases, offs) on its default-parameter index:
      counts   a read with exactly N chains for every N of COUNTS, and the read of the mosaic's default leg with the most candidates
      most     (an index of its own: the k = 1 leg's parameters) the read of the whole mosaic with the most candidate references -- which has
               more runs than the default MQ_MATCH_CAP of 2048 as well -- and the two reads behind it
      ties     n-way ties for n = 2, 17, 65 and the near-ties beside them
      below    a tie below a larger winner: the two slices of a 2-way tie in front of 6 kb of a third contig
      strands  the gap ladder at g = 50: forward and reverse-strand chains of one run and of several
    and `wrap` = (genome, off, names, bases, offs, params) of directed.usize_wrap_case: chains whose find_coords wraps (an index of its own)."""
    global _BATCHES
    if _BATCHES is not None:
        return _BATCHES
    g, off, names, sets = M.world(O, sim)
    po = O.params()
    ox = O.Index()
    ox.build_mt(g, off, names, po, 4)
    rng = np.random.default_rng(9100)
    out = {}
    by_n = _exact_count_reads(g, off, ox, po, rng)
    st = sets["default"]
    d = ox.map_batch_diag(st["bases"], st["offs"], po, threads=4)[1]
    most = int(np.argmax(d["n_candidates"]))
    out["counts"] = M.concat([by_n[n] for n in COUNTS] + [st["bases"][int(st["offs"][most]):int(st["offs"][most + 1])]])
    seqs = []
    for n in (2, 17, 65):
        for nm in ("tie_%d" % n, "near_%d" % n):
            t = sets[nm]
            seqs += [t["bases"][int(t["offs"][i]):int(t["offs"][i + 1])] for i in range(t["offs"].size - 1)]
    out["ties"] = M.concat(seqs)
    t = sets["tie_2"]
    big = M.big_contigs(off)
    below = []
    for i in range(min(4, t["offs"].size - 1)):
        tie = t["bases"][int(t["offs"][i]):int(t["offs"][i + 1])]
        half = tie.size // 2
        for c in big[3 * i:3 * i + 3]:
            win = M._slice(g, off, int(c), 1000, 6000, bool(i & 1))[0]
            below.append(np.concatenate([tie[:half], win, tie[half:]]))
    out["below"] = M.concat(below)
    t = sets["gap_50"]
    out["strands"] = M.select(t["bases"], t["offs"], list(range(0, t["offs"].size - 1, 7)))
    wrap = directed.usize_wrap_case(O, sim)
    st = sets["k1"]
    pk, xk = O.params(**st["ps"]), O.Index()
    xk.build_mt(g, off, names, pk, 4)
    d = xk.map_batch_diag(st["bases"], st["offs"], pk, threads=4)[1]
    most = int(np.argmax(d["n_candidates"]))
    n_k1 = st["offs"].size - 1
    out["most"] = (dict(st["ps"]),) + M.select(st["bases"], st["offs"], [most, (most + 1) % n_k1, (most + 2) % n_k1])
    _BATCHES = (g, off, names, out, wrap)
    return _BATCHES
