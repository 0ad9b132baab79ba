"""Data and a model for the index-merge tests (test_index_merge_host.py, test_gpu_index_merge.py).

Reference sets.  A = three contigs, B = two, C = one, 6-12 kb each, with planted segments so that every way a key can meet a merge occurs:
    S_AB    once in A (contig 0) and once in B (contig 3, lower case there): live in both, must turn dead
    S_AA    twice inside A (contigs 0 and 1): dead in A already
    S_BB    in B on both strands (contig 4, forward in upper case and reverse-complemented in lower case): dead in B already
    S_ABC   once in each of A, B and C: the first merge of a chain of two turns it dead, the second meets it dead
The GPU side gets the mixed-case bytes (its kernels fold the case: MQ_FLAG_FOLD_CASE); the oracle gets them upper-cased, as the
reference's seam does.

The model (`Model`): a dict keyed by key that holds (payload, times) -- what a table is a function of.  Merging a
slot set into it is the rule of the issue restated: a key that is new arrives with its payload, the id moved, and its count capped at 2;
a key that is there keeps its payload and adds the count.  Nothing of it comes from the library.
"""
import numpy as np

import mqx

LENS_A, LENS_B, LENS_C = [12000, 10000, 8000], [11000, 9000], [7000]
LENS = LENS_A + LENS_B + LENS_C
A_IDS, B_IDS, C_IDS = [0, 1, 2], [3, 4], [5]
SEG = 2500
_cache = {}


def _rc(s):
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[a] = b
    return comp[s[::-1]]


def contigs(simlib):
    """(mixed-case genome bytes, offsets, names): what the library is given"""
    if "g" not in _cache:
        g, off, names = simlib.make_genome(LENS, seed=41, threads=2)
        g = g.copy()
        at = lambda c, p: int(off[c]) + p  # noqa: E731
        seg = lambda c, p: g[at(c, p):at(c, p) + SEG].copy()  # noqa: E731
        lower = lambda s: s | np.uint8(0x20)  # noqa: E731
        g[at(3, 1000):at(3, 1000) + SEG] = lower(seg(0, 500))          # S_AB
        g[at(1, 6000):at(1, 6000) + SEG] = seg(0, 4000)                # S_AA
        g[at(4, 5500):at(4, 5500) + SEG] = lower(_rc(seg(4, 500)))     # S_BB
        s_abc = seg(2, 3000)                                           # S_ABC
        g[at(3, 7000):at(3, 7000) + SEG] = s_abc
        g[at(5, 2000):at(5, 2000) + SEG] = lower(s_abc)
        _cache["g"] = (g, off, names)
    return _cache["g"]


def contig(simlib, r, upper=False):
    g, off, _ = contigs(simlib)
    s = g[int(off[r]):int(off[r + 1])]
    return (s & np.uint8(0xDF)) if upper else s


def reads(simlib):
    """240 reads from all six contigs and 60 that lie inside the planted segments' neighbourhood (contig 3, which carries S_AB and S_ABC)"""
    if "r" not in _cache:
        g, off, _ = contigs(simlib)
        up = g & np.uint8(0xDF)
        a = simlib.make_reads(up, off, 240, seed=5, len_mean=4000, len_sd=1200, len_min=600, len_max=9000, err=0.004, threads=2)
        sub_off = np.array([0, int(off[4] - off[3])], dtype=off.dtype)
        b = simlib.make_reads(up[int(off[3]):int(off[4])], sub_off, 60, seed=6, len_mean=3000, len_sd=600, len_min=600, len_max=6000, err=0.004, threads=2)
        b["ctg"] = b["ctg"] + 3
        bases = np.concatenate([a["bases"], b["bases"]])
        offsets = np.concatenate([a["offsets"], b["offsets"][1:] + a["offsets"][-1]])
        r = dict(bases=bases, offsets=offsets)
        for f in ("ctg", "start", "end", "strand"):
            r[f] = np.concatenate([a[f], b[f]])
        _cache["r"] = r
    return _cache["r"]


def insertions(oracle, simlib, refs, po, ids=None):
    """every k-min-mer of the contigs `refs` (under ids[i], default the contig's number), in insertion order, count 1"""
    parts = []
    for j, r in enumerate(refs):
        km = oracle.kminmers(contig(simlib, r, upper=True), po)
        a = np.zeros(km.size, dtype=mqx.entry_dtype)
        for f, o in (("key", "hash"), ("start", "start"), ("end", "end"), ("offset", "offset"), ("rc", "rev")):
            a[f] = km[o]
        a["id"] = r if ids is None else ids[j]
        a["count"] = 1
        parts.append(a)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=mqx.entry_dtype)


# ------------------------------------------------------------------ the model
class Model:
    """key -> [start, end, offset, id_rc, times]; `n_kminmers` counts every insertion"""

    def __init__(self, slots=None, n_kminmers=None):
        self.d = {}
        self.n_kminmers = 0
        if slots is not None:
            self.merge(slots, 0, n_kminmers)

    def merge(self, slots, id_base, n_kminmers=None):
        """a slot set (mqx.slot_dtype: one slot per key) merged in with its ids moved; the three numbers the kernels count come back"""
        claimed = born_dead = turned_dead = 0
        for s in slots.tolist():
            start, end, offset, id_rc, key, count, _ = s
            assert count >= 1
            e = self.d.get(key)
            if e is None:
                self.d[key] = [start, end, offset, (((id_rc >> 1) + id_base) << 1) | (id_rc & 1), min(count, 2)]
                claimed += 1
                born_dead += 1 if (count >= 2 or end == 0) else 0
            else:
                turned_dead += 1 if (e[4] == 1 and e[1] != 0) else 0
                e[4] = 2
        self.n_kminmers += int(slots["count"].astype(np.uint64).sum()) if n_kminmers is None else n_kminmers
        return claimed, born_dead, turned_dead

    def live(self, key):
        e = self.d.get(key)
        return e is not None and e[4] == 1 and e[1] != 0

    def n_keys(self):
        return len(self.d)

    def n_unique(self):
        return sum(1 for e in self.d.values() if e[4] == 1 and e[1] != 0)

    def slots(self):
        s = np.zeros(len(self.d), dtype=mqx.slot_dtype)
        for i, (k, e) in enumerate(self.d.items()):
            s[i] = (e[0], e[1], e[2], e[3], k, e[4], 1 if k == 0 else 0)
        return s


def sorted_slots(s):
    """slots by key with the payload of every dead key blanked and its count 2 (a dead key's payload is unspecified)"""
    s = s[np.argsort(s["key"], kind="stable")].copy()
    dead = (s["count"] != 1) | (s["end"] == 0)
    for f in ("start", "end", "offset", "id_rc"):
        s[f][dead] = 0
    s["count"][dead] = 2
    return s


def place(keys, table_slots):
    """The probe-order model of tests/mqx.py building a table: every key, in this order, into the first empty slot of its walk.  Returns
    slot -> key.  (A table without an empty slot is refused: a miss would walk forever.)"""
    at = {}
    for k in keys:
        for s in mqx.probe_order(int(k), table_slots):
            if s not in at:
                at[s] = int(k)
                break
            assert at[s] != int(k), "a key twice"
        else:
            raise AssertionError("no empty slot on the walk of %x" % int(k))
    return at


def walk_finds(at, key, table_slots):
    """a lookup by the same model: the key's walk up to the first empty slot"""
    for s in mqx.probe_order(int(key), table_slots):
        if s not in at:
            return False
        if at[s] == int(key):
            return True
    return False


# ------------------------------------------------------------------ crafted destination / source pairs (tests/mqx.py writes both files)
def entries(keys, rid, count=1, start0=10):
    e = np.zeros(len(keys), dtype=mqx.entry_dtype)
    e["key"] = np.asarray(keys, dtype=np.uint64)
    e["id"] = rid
    e["start"] = start0 + 3 * np.arange(len(keys), dtype=np.uint32)
    e["end"] = e["start"] + 31
    e["offset"] = np.arange(len(keys), dtype=np.uint32)
    e["rc"] = np.arange(len(keys), dtype=np.uint32) & 1
    e["count"] = count
    return e


def rand_keys(rng, n, taken=()):
    k = np.unique(rng.integers(1, 2**64, size=2 * n + 8, dtype=np.uint64))
    return rng.permutation(k[~np.isin(k, np.asarray(list(taken), dtype=np.uint64))])[:n]


def crafted_cases():
    """(name, dst Table, src Table, id_base, declared (dst, src) n_kminmers or None): see the test's docstring"""
    rng = np.random.default_rng(8)
    P = mqx.params(k=3, l=12, density=0.05)
    refs_d = [(0, "d0", 100000), (1, "d1", 100000)]
    refs_s = [(0, "s0", 100000)]
    cases = []
    # ONE empty slot after the merge: 600 + 423 keys in 1024 slots (the declared insertion counts keep the table from growing)
    kd = rand_keys(rng, 600)
    ks = rand_keys(rng, 423, kd)
    cases.append(("one empty slot", mqx.Table(P, 1024, refs_d, entries(kd, 1)), mqx.Table(P, 512, refs_s, entries(ks, 0)), 2, (60, 40)))
    # a source key homed in the destination's last bucket, both of whose ways and bucket 0's way 0 are taken: it lands behind the wrap
    ts = 1024
    kd = np.array([(7 << 10) | 1022, (9 << 10) | 1023, (11 << 10) | 1022, (5 << 10) | 0], dtype=np.uint64)  # homes 1022, 1023, 1022 (-> bucket 0 way 0), 0 (-> way 1)
    ks = np.array([(13 << 10) | 1023, (15 << 10) | 1022], dtype=np.uint64)
    cases.append(("behind the wrap", mqx.Table(P, ts, refs_d, entries(kd, 0)), mqx.Table(P, 4, refs_s, entries(ks, 0)), 2, None))
    # 2- and 4-slot source tables
    kd = rand_keys(rng, 40)
    cases.append(("2-slot source", mqx.Table(P, 1024, refs_d, entries(kd, 0)), mqx.Table(P, 2, refs_s, entries(rand_keys(rng, 1, kd), 0)), 5, None))
    cases.append(("4-slot source", mqx.Table(P, 1024, refs_d, entries(kd, 0)), mqx.Table(P, 4, refs_s, entries(np.concatenate([rand_keys(rng, 2, kd), kd[:1]]), 0)), 5, None))
    # the key 0: live in the source only, live in both (turning dead), dead in the source
    z = lambda count: entries(np.zeros(1, np.uint64), 0, count=count, start0=77)  # noqa: E731
    other = entries(rand_keys(rng, 5, kd), 0)
    cases.append(("key 0 in the source only", mqx.Table(P, 1024, refs_d, entries(kd, 0)), mqx.Table(P, 16, refs_s, np.concatenate([other, z(1)])), 2, None))
    cases.append(("key 0 live in both", mqx.Table(P, 1024, refs_d, np.concatenate([entries(kd, 0), z(1)])), mqx.Table(P, 16, refs_s, np.concatenate([other, z(1)])), 2, None))
    cases.append(("key 0 dead in the source", mqx.Table(P, 1024, refs_d, np.concatenate([entries(kd, 0), z(1)])), mqx.Table(P, 16, refs_s, np.concatenate([other, z(2)])), 2, None))
    # a source slot with count = 7 (new, and on a live destination key), and one with end == 0 (born dead; and on a live destination key)
    e = entries(np.concatenate([rand_keys(rng, 4, kd), kd[:2]]), 0)
    e["count"][[0, 4]] = 7
    cases.append(("count 7", mqx.Table(P, 1024, refs_d, entries(kd, 0)), mqx.Table(P, 16, refs_s, e), 2, None))
    e = entries(np.concatenate([rand_keys(rng, 4, kd), kd[:2]]), 0)
    e["end"][[1, 5]] = 0
    cases.append(("end 0", mqx.Table(P, 1024, refs_d, entries(kd, 0)), mqx.Table(P, 16, refs_s, e), 2, None))
    # sparse source ids up to 2^24 - 1 - id_base
    base = 3
    top = mqx.MAX_REF_ID - 1 - base
    refs_sparse = [(0, "lo", 100000), (9, "", 100000), (top, "top", 100000)]
    e = entries(rand_keys(rng, 9, kd), 0)
    e["id"] = np.array([0, 9, top] * 3, dtype=np.uint32)
    cases.append(("sparse ids", mqx.Table(P, 1024, refs_d, entries(kd, 1)), mqx.Table(P, 32, refs_sparse, e), base, None))
    return cases
