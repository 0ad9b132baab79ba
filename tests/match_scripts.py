"""Crafted index payloads that walk MapSink::batch_runs (mq_probe.hpp) through every transition of the Match state machine, at every border
of its wave-parallel scan.  No GPU here: the generator, the expected values and the coverage bookkeeping.

Reads are random A C G T with fixed seeds, no genome: their k-min-mer keys (oracle.kminmers) are pairwise distinct, so a table is a free
lookup per position -- position i of read r gets whatever (id, offset, rc, start, end, live / dead / absent) its SCRIPT asks for.  A script
gives every k-min-mer position one of 19 element kinds, relative to the previous element's entry p:
    misses  "absent" (no key), "dead" (count = 2), "born" (an entry born empty: end = 0)
    hits    (srel, same, step): srel = q.rev != r.rc (the entry's rc is q.rev ^ srel, q.rev from the oracle), same: r.id == p.id or the
            decoy reference, step: r.offset - p.offset in {+1, -1, 0, +2}.  A hit behind a miss has no p: its id and offset are free.
Payload coordinates name the position: start / end are the k-min-mer's own q_start / q_end shifted by CF for srel = 0 and mirrored in CR
for srel = 1, so they are distinct per position, start < end <= len, and a run's (q_start, q_end, r_start, r_end, count) names its first and
last element; runs of one strand on one reference keep equal query and reference gaps, so the chain filter drops none of them for its gap.
c = 2 and an s no score reaches: mapq is 60 exactly when at least two runs are kept.

Families (one table per parameter set holds them all):
    P  probes: one read per (border b, state before, kind at b); behind b two elements that continue whatever state b left, then misses
    R  random walks over the 19 kinds, some of hits alone with an exact number of runs (49 / 50, 65 / 66: MAP_LDS_RECS and the chain chunk)
    W  offsets at the `as i32` casts: runs through 0x7FFFFFFE .. 0x80000001 and up to 0xFFFFFFFE, at b = 64 and mid-batch
    C  (dense set) 2047 / 2048 / 2049 runs back to back: the Match window (MQ_MATCH_CAP) exactly; a batch of its own
    N  the scripts of every tenth P and R read on a fresh read with one N far from the border: map_declined_kernel's MapSink
States before b: "miss"; "fwd" / "rev": a run of 5; "fwd_far" / "rev_far": a run that began 75 elements earlier (carried through a whole
lane-batch: the `fl < 0` branch on a carried Match that was itself extended by it; only where b >= 76); "fwd_nc": a forward run whose last
element is the non-constant one (srel = 1, step +1); "fwd_xref": a forward run whose last element lies on the decoy; "nc2" / "nc3": two
and three non-constant elements in a row ending at b - 1.
"""
import numpy as np

import anchors_model as A
import chain_model
import mqx

LANE, CHUNK = 64, 384            # k-min-mers of a lane-batch and of a chunk (lattice.LANE_BATCH, lattice.CHUNK_KMM)
S_NEVER = 1 << 30                # no score reaches it
CF, CR, REF_LEN = 1 << 20, 1 << 22, 1 << 24
REFS = [(0, "r0", REF_LEN), (1, "r1", REF_LEN), (2, "r2", REF_LEN), (3, "decoy", REF_LEN)]
DECOY = 3

MISSES = ("absent", "dead", "born")
HITS = tuple((srel, same, step) for srel in (0, 1) for same in (True, False) for step in (1, -1, 0, 2))
KINDS = MISSES + HITS
F, RV, NC, X = (0, True, 1), (1, True, -1), (1, True, 1), (0, False, 1)
FWD_CONT = tuple(k for k in HITS if k[2] == 1)
FWD_BREAK = tuple(k for k in HITS if k[2] != 1)
REV_BREAK = tuple(k for k in HITS if k != RV)
STATES = {"miss": [], "fwd": [F] * 5, "rev": [RV] * 5, "fwd_far": [F] * 75, "rev_far": [RV] * 75, "fwd_nc": [F] * 4 + [NC],
          "fwd_xref": [F] * 4 + [X], "nc2": [F] * 3 + [NC] * 2, "nc3": [F] * 3 + [NC] * 3}
STATE_NAMES = ("none", "fwd", "rev")   # the model's state before an element

SETS = {
    "default": dict(ps=dict(c=2, s=S_NEVER), K=400, borders=(64, 384), lasts=(), n_walks=12, C=()),
    "dense": dict(ps=dict(k=3, l=12, density=0.05, c=2, s=S_NEVER), K=832, borders=(0, 63, 64, 65, 383, 384, 385, 768), lasts=(769, 831, 832),
                  n_walks=36, C=(2047, 2048, 2049)),
}
C_KMM = 2112                     # k-min-mers of a family C read
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def kind_name(k):
    return k if isinstance(k, str) else "srel%d %s %+d" % (k[0], "same" if k[1] else "other", k[2])


# ------------------------------------------------------------------ reads
def read_with_kminmers(O, po, seed, K, taken, n_far_from=None):
    """A random read with exactly K k-min-mers, none of whose keys is in `taken` (the keys of the reads made before it; this read's are
    added).  n_far_from = b: one N, K / 2 k-min-mers away from position b.
    At l = 12 a k-min-mer of three neighbouring windows spans 14 compressed bases, and a million random k-min-mers repeat some of those:
    a random read is therefore finished by construction -- one base is redrawn inside every k-min-mer whose key is taken, occurs twice
    in the read or is 0, until none is left (at the defaults nothing is redrawn).  Windows over the N are left alone: they hash as 0."""
    rng = np.random.default_rng(seed)
    per = (1.0 / po.density) * (4.0 / 3.0 if po.use_hpc else 1.0)
    s = bytearray(ACGT[rng.integers(0, 4, int(per * (K + po.k + 8) * 1.12) + 40 * int(po.l))].tobytes())
    km = O.kminmers(bytes(s), po)
    assert km.size > K + 2, (seed, km.size, K)
    n_at = None
    if n_far_from is not None:
        n_at = int(km["start"][(n_far_from + K // 2) % K]) + 3
        s[n_at] = ord("N")

    def zone(km, i):
        return n_at is not None and int(km["start"][i]) - 4 * int(po.l) <= n_at <= int(km["end"][i]) + 4 * int(po.l)
    for _ in range(60):
        km = O.kminmers(bytes(s), po)
        assert km.size > K + 2, (seed, km.size, K)
        keys = km["hash"][:K + 6].tolist()   # (what lies behind is cut off below)
        seen, bad = set(), []
        for i, h in enumerate(keys):
            if h in taken or h in seen or h == 0:
                if not zone(km, i):
                    bad.append(i)
                elif h not in seen and h != 0 and not taken[h]:   # next to the N, but the key of an ordinary k-min-mer made before
                    bad.append(i)
            seen.add(h)
        if not bad:
            break
        for i in bad:
            at = int(km["start"][i]) + int(rng.integers(0, max(1, int(km["end"][i]) - int(km["start"][i]))))
            if at != n_at:
                s[at] = int(ACGT[(b"ACGT".index(bytes([s[at]])) + int(rng.integers(1, 4))) % 4])
    else:
        raise AssertionError("keys still taken after 60 rounds (seed %d)" % seed)
    # close one base behind k-min-mer K - 1 and grow base by base (under homopolymer compression `end` cuts the last window short);
    # counted on the read's tail, which opens at a k-min-mer's first base
    t = max(0, K - 48)
    a = int(km["start"][t])
    for cut in range(int(km["end"][K - 1]), min(len(s), int(km["end"][K]) + 8 * int(po.l))):
        if O.kminmers(bytes(s[a:cut]), po).size == K - t:
            out = bytes(s[:cut])
            fin = O.kminmers(out, po)
            assert fin.size == K and np.array_equal(fin["hash"], km["hash"][:K]), (seed, K)
            for i, h in enumerate(fin["hash"].tolist()):   # (taken: key -> made next to an N)
                taken[h] = taken.get(h, True) and zone(fin, i)
            return out
    raise AssertionError("no cut with %d k-min-mers (seed %d)" % (K, seed))


class Read:
    """one read, its script and what the script became: entries (the index answer per position, None for a miss), kinds (the resolved
    kind per scripted position), states (the model's state before every position: 0 none, 1 forward, 2 reverse), records for the table"""

    def __init__(self, family, name, script, K, b=None, state=None, kind=None, base=None, with_n=False):
        self.family, self.name, self.script, self.K, self.b, self.state, self.kind = family, name, script, K, b, state, kind
        self.base = base or {}
        self.with_n = with_n

    def label(self):
        return (self.family, self.b, self.state, kind_name(self.kind) if self.kind is not None else None)


def _coords(srel, qs, qe):
    return (CR - qe, CR - qs) if srel else (CF + qs, CF + qe)


def _other(rid, ref0):
    return DECOY if rid != DECOY else ref0


def realize(rd, ref0):
    """the script on the read's k-min-mers (rd.km, the oracle's): fills rd.entries, rd.kinds, rd.states, rd.records"""
    km = rd.km
    qs, qe, rev = km["start"].tolist(), km["end"].tolist(), (km["rev"] != 0).tolist()
    keys = km["hash"].tolist()
    K = len(qs)
    assert K == rd.K, (rd.name, K, rd.K)
    ent, states, kinds, recs = [None] * K, [0] * K, {}, []
    p, run, last, n_open = None, None, -2, 0
    for i in sorted(rd.script):
        assert 0 <= i < K, (rd.name, i)
        if i != last + 1:
            p, run = None, None
        last = i
        states[i] = 0 if run is None else (2 if run.rc else 1)
        kind = rd.script[i]
        if kind[0] == "cont":
            kind = HITS[kind[1] % 16] if run is None else (RV if run.rc else FWD_CONT[kind[1] % 4])
        elif kind[0] == "break":
            kind = HITS[kind[1] % 16] if run is None else (REV_BREAK[kind[1] % 15] if run.rc else FWD_BREAK[kind[1] % 12])
        kinds[i] = kind
        fresh = rd.base.get(i, 1000000 + 4096 * i)
        if kind in MISSES:
            if kind != "absent":
                a, z = _coords(0, qs[i], qe[i])
                recs.append((keys[i], ref0, a, 0 if kind == "born" else z, fresh, 0, 2 if kind == "dead" else 1))
            p, run = None, None
        else:
            srel, same, step = kind
            if p is None:
                rid, off = (ref0 + n_open) % 3, fresh
                n_open += 1
            else:
                rid, off = (p["id"] if same else _other(p["id"], ref0)), (p["offset"] + step) & 0xFFFFFFFF
            assert off < 2**32 - 1, (rd.name, i)
            a, z = _coords(srel, qs[i], qe[i])
            e = dict(id=rid, start=a, end=z, offset=off, rc=bool(rev[i]) != bool(srel))
            if run is None or not chain_model.extends(run, rev[i], e, p):
                run = chain_model.Run()
                run.rc = rev[i] != e["rc"]
            ent[i], p = e, e
            recs.append((keys[i], rid, a, z, off, int(e["rc"]), 1))
        if i + 1 < K:
            states[i + 1] = 0 if run is None else (2 if run.rc else 1)
    rd.entries, rd.states, rd.kinds, rd.records, rd.ref0 = ent, states, kinds, recs, ref0
    rd.kmers = list(zip(qs, qe, rev))


# ------------------------------------------------------------------ scripts
def probe_script(b, state, kind, K):
    pre = STATES[state]
    s = {b - len(pre) + j: k for j, k in enumerate(pre)}
    s[b] = kind
    for j in (b + 1, b + 2):
        if j < K:
            s[j] = ("cont", 0)
    return s


def probe_specs(cfg):
    """(b, state, kind, K) of every probe read of a parameter set"""
    out = []
    for b, K in [(b, cfg["K"]) for b in cfg["borders"]] + [(K - 1, K) for K in cfg["lasts"]]:
        for state, pre in STATES.items():
            if (b == 0 and state != "miss") or b - len(pre) < 1 and pre:
                continue   # nothing lies before the read's first k-min-mer; a run of 75 does not fit in front of b = 63 .. 65
            for kind in KINDS:
                out.append((b, state, kind, K))
    return out


def walk_script(rng, K, p_cont=None, n_runs=None):
    """n_runs: hits alone, exactly that many runs (each break is a hit that fails check); else a walk that continues with p_cont"""
    if n_runs is not None:
        brk = set(rng.choice(np.arange(1, K), size=n_runs - 1, replace=False).tolist())
        return {i: ("break" if i in brk else "cont", int(rng.integers(0, 1 << 20))) for i in range(K)}
    s = {}
    for i in range(K):
        if rng.random() < p_cont:
            s[i] = ("cont", int(rng.integers(0, 1 << 20)))
        else:
            s[i] = KINDS[int(rng.integers(0, len(KINDS)))]
    return s


def walk_specs(cfg, seed):
    """(p_cont, n_runs) per walk: run lengths from 1 to beyond 100, four reads of hits alone around MAP_LDS_RECS and the chain chunk"""
    exact = [49, 65, 50, 66]
    out = [(None, m) for m in exact[:2 if cfg["n_walks"] < 20 else 4]]
    ps = (0.3, 0.6, 0.8, 0.9, 0.95, 0.98, 0.99)
    return out + [(ps[j % len(ps)], None) for j in range(cfg["n_walks"] - len(out))]


def cast_scripts():
    """family W: (name, script, base offsets).  Each read holds a run across b = 64 (9 elements) and one mid-batch at 100 (7 elements)"""
    out = []

    def run(at, n, kind):
        return {at + j: kind for j in range(n)}
    for name, kind, first64, first100 in (
            ("fwd across 2^31", F, 0x80000000 - 4, 0x80000000 - 3),          # ... 7FFFFFFF at lane 63, 80000000 at lane 0
            ("rev across 2^31", RV, 0x80000000 + 4, 0x80000000 + 3),         # a step of -1 across 2^31 that continues
            ("fwd to the top", F, 0xFFFFFFFE - 8, 0xFFFFFFFE - 6),           # ends on 0xFFFFFFFE, the largest offset a table takes
            ("rev from the top", RV, 0xFFFFFFFE, 0xFFFFFFFE)):
        s = run(60, 9, kind)
        s.update(run(100, 7, kind))
        out.append((name, s, {60: first64, 100: first100}))
    # a forward run that meets a step of -1 across 2^31 (breaks), and a reverse run that meets +1 across it (breaks)
    s = run(60, 4, F)
    s.update({64: (0, True, -1), 65: ("cont", 0), 66: ("cont", 0)})
    s.update(run(100, 3, F))
    s.update({103: (0, True, -1), 104: ("cont", 0)})
    out.append(("fwd meets -1 at 2^31", s, {60: 0x80000000 - 3, 100: 0x80000000 - 2}))
    s = run(60, 4, RV)
    s.update({64: (1, True, 1), 65: ("cont", 0), 66: ("cont", 0)})
    s.update(run(100, 3, RV))
    s.update({103: (1, True, 1), 104: ("cont", 0)})
    out.append(("rev meets +1 at 2^31", s, {60: 0x80000000 + 2, 100: 0x80000000 + 1}))
    return out


# ------------------------------------------------------------------ a parameter set's world
class World:
    pass


_worlds = {}


def world(O, which, variant=0):
    """every read of a parameter set, its table, the oracle twin; variant: mqo_set_variant while the k-min-mers are taken"""
    if (which, variant) in _worlds:
        return _worlds[(which, variant)]
    cfg = SETS[which]
    w = World()
    w.which, w.cfg, w.variant = which, cfg, variant
    w.params = mqx.params(**cfg["ps"])
    w.po = po = O.params(**cfg["ps"])
    reads = []
    for n, (b, state, kind, K) in enumerate(probe_specs(cfg)):
        reads.append(Read("P", "P b=%d %s %s" % (b, state, kind_name(kind)), probe_script(b, state, kind, K), K, b, state, kind))
    n_probes = len(reads)
    walks = walk_specs(cfg, 0)
    for n, (pc, m) in enumerate(walks):
        rng = np.random.default_rng(7000 + n)
        reads.append(Read("R", "R %d %s" % (n, "p=%.2f" % pc if m is None else "%d runs of hits alone" % m), walk_script(rng, cfg["K"], pc, m), cfg["K"]))
        reads[-1].n_runs = m
    for name, s, base in cast_scripts():
        reads.append(Read("W", "W " + name, s, 200, base=base))
    for m in cfg["C"]:
        reads.append(Read("C", "C %d runs" % m, walk_script(np.random.default_rng(9000 + m), C_KMM, None, m), C_KMM))
        reads[-1].n_runs = m
    for src in reads[0:n_probes:10] + reads[n_probes:n_probes + len(walks):10]:
        reads.append(Read("N", "N of " + src.name, src.script, src.K, src.b if src.b is not None else 0, src.state, src.kind, with_n=True))
        reads[-1].n_runs = None   # (the positions next to the N stay unscripted: a walk's copy may have a run more or less)
    O.lib().mqo_set_variant(variant)
    taken = {}
    try:
        for n, rd in enumerate(reads):
            rd.seq = read_with_kminmers(O, po, 100000 + n, rd.K, taken, rd.b if rd.with_n else None)
            rd.km = O.kminmers(rd.seq, po)
    finally:
        O.lib().mqo_set_variant(0)
    # the keys of the whole set: pairwise distinct and not 0 (a seed that fails this fails; nothing is filtered).  The one exception is
    # by construction: a window over an N hashes as 0, so the few k-min-mers made of such windows alone repeat one key inside their read.
    # Those positions stay unscripted (absent from the table), and they lie next to the N, far from the probed border.
    keys = np.concatenate([rd.km["hash"] for rd in reads])
    uniq, cnt = np.unique(keys, return_counts=True)
    shared = uniq[(cnt > 1) | (uniq == 0)]
    for rd in reads:
        bad = np.flatnonzero(np.isin(rd.km["hash"], shared))
        if not rd.with_n:
            assert bad.size == 0, "%s: a k-min-mer key of %r is 0 or occurs twice" % (which, rd.name)
            continue
        at = rd.seq.index(b"N")
        touched = np.flatnonzero((rd.km["start"].astype(np.int64) - 4 * int(po.l) <= at) & (rd.km["end"] + 4 * int(po.l) >= at))
        assert bad.size < touched.size and np.isin(bad, touched).all() and (rd.family != "N" or not bad.size or abs(int(bad[0]) - rd.b) > LANE), rd.name
        rd.script = {i: k for i, k in rd.script.items() if i not in set(bad.tolist())}
        rd.unscripted = bad.size
    for n, rd in enumerate(reads):
        assert (b"N" in rd.seq) == rd.with_n
        realize(rd, n % 3)
    w.reads = reads
    w.main = [i for i, rd in enumerate(reads) if rd.family != "C"]
    w.window = [i for i, rd in enumerate(reads) if rd.family == "C"]
    w.n_keys_of_reads = int(keys.size)
    rec = [r for rd in reads for r in rd.records]
    e = np.zeros(len(rec), dtype=mqx.entry_dtype)
    for j, f in enumerate(("key", "id", "start", "end", "offset", "rc", "count")):
        e[f] = np.array([r[j] for r in rec], dtype=np.uint64)
    w.table = mqx.Table(w.params, mqx.pow2_above(2 * e.size), REFS, e, "match scripts, " + which)
    _worlds[(which, variant)] = w
    return w


def batch_of(w, idx):
    seqs = [w.reads[i].seq for i in idx]
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), offs


def points_of(w, idx):
    """(name, sequence, family) triples, as test_gpu_lattice's helpers take them"""
    return [(w.reads[i].name, w.reads[i].seq, w.reads[i].family) for i in idx]


# ------------------------------------------------------------------ expected values from runs
def outcome(runs, q_len, po):
    """(hit record, anchor list) of a read from its runs: chain_model's filter, candidate, winner and coordinates -- map_read and
    anchors_model.by_model in one pass, so that a changed run list can be judged (test_match_scripts_cases.py ties it to both)"""
    g = int(po.g)
    per_ref = {}
    for r in runs:
        per_ref.setdefault(r.ref, []).append(r)
    cands = []
    for ref, rs in per_ref.items():
        kept = rs
        if len(rs) > 1:
            anchor = rs[0]
            for r in rs[1:]:
                if r.count > anchor.count:
                    anchor = r
            kept = [r for r in rs if chain_model.stays(anchor, r, g)]
        if kept:
            cands.append(A.Expected(int(ref), bool(kept[0].rc), [A._tuple(r) for r in kept]))
    if not cands:
        return None, None
    scores = [sum(x[4] for x in e.runs) for e in cands]
    best, top, second = 0, 0, 0
    for i, sc in enumerate(scores):
        if sc > top:
            second, best, top = top, i, sc
        elif sc > second:
            second = sc
    if len(cands) > 1 and top == second:
        return None, None
    e = cands[best]
    rec = chain_model.place(q_len, REF_LEN, A.ends_candidate(e, po))
    rec["ref_id"] = e.ref
    return rec, e


def runs_flipped(kmers, entries, b):
    """chain_model.runs_of with the decision at element b inverted: a hit that extends the open run opens the next one instead, a hit that
    does not is taken into the run (b = None: runs_of itself, asserted by the CPU proofs)"""
    out, i, n = [], 0, len(kmers)
    while i < n:
        e = entries[i]
        if e is None:
            i += 1
            continue
        r = chain_model.Run()
        r.q_start, r.q_end, r.r_start, r.r_end, r.count = kmers[i][0], kmers[i][1], e["start"], e["end"], 1
        r.rc = kmers[i][2] != e["rc"]
        r.ref = e["id"]
        prev = e
        i += 1
        while i < n:
            h = entries[i]
            if h is None:
                i += 1
                break
            if chain_model.extends(r, kmers[i][2], h, prev) == (i == b):
                break
            if r.rc:
                r.r_start = h["start"]
            else:
                r.r_end = h["end"]
            r.q_end = kmers[i][1]
            r.count += 1
            prev = h
            i += 1
        out.append(r)
    return out


def flipped(rd):
    """the read's runs with the model's decision at rd.b alone inverted: a miss becomes a live hit that continues the open run (on p's
    reference, one offset higher, or lower with srel 1 behind a reverse run), a hit behind a miss becomes a miss, any other hit changes between `continues` and `opens a run`"""
    b, ent = rd.b, list(rd.entries)
    if ent[b] is None:
        p = ent[b - 1] if b > 0 else None
        srel = 1 if rd.states[b] == 2 else 0
        a, z = _coords(srel, rd.kmers[b][0], rd.kmers[b][1])
        ent[b] = dict(id=p["id"] if p else rd.ref0, start=a, end=z, offset=p["offset"] + (-1 if srel else 1) if p else 1000000 + 4096 * b,
                      rc=rd.kmers[b][2] != bool(srel))
        return chain_model.runs_of(rd.kmers, ent)
    if rd.states[b] == 0:
        ent[b] = None
        return chain_model.runs_of(rd.kmers, ent)
    return runs_flipped(rd.kmers, ent, b)


def run_tuples(runs):
    return [(r.ref, bool(r.rc)) + A._tuple(r) for r in runs]


# ------------------------------------------------------------------ coverage
PLACES = ("lane 0", "lane 63", "chunk first", "read last", "mid-batch")


def places_of(i, K):
    out = []
    if i == K - 1:
        out.append("read last")
    if i % LANE == 0 and i > 0:
        out.append("lane 0")
    if i % LANE == LANE - 1:
        out.append("lane 63")
    if i % CHUNK == 0 and i > 0:
        out.append("chunk first")
    if 0 < i % LANE < LANE - 1 and i != K - 1:
        out.append("mid-batch")
    return out


def coverage(reads):
    """{place: {(state before, kind): count}} over every position of the reads"""
    cov = {p: {} for p in PLACES}
    for rd in reads:
        for i in range(rd.K):
            pl = places_of(i, rd.K)
            if pl:
                key = (rd.states[i], rd.kinds.get(i, "absent"))
                for p in pl:
                    cov[p][key] = cov[p].get(key, 0) + 1
    return cov


def coverage_at(reads, b):
    """{(state before, kind)} at position b over the reads"""
    return {(rd.states[b], rd.kinds.get(b, "absent")) for rd in reads if b < rd.K}


ALL_PAIRS = {(s, k) for s in (0, 1, 2) for k in KINDS}


def coverage_table(cov):
    lines = ["%-22s" % "state, kind" + "".join("%13s" % p for p in PLACES)]
    for s in (0, 1, 2):
        for k in KINDS:
            lines.append("%-22s" % ("%s, %s" % (STATE_NAMES[s], kind_name(k))) + "".join("%13d" % cov[p].get((s, k), 0) for p in PLACES))
    return "\n".join(lines)
