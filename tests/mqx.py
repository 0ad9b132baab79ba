"""A second implementation of the on-disk index (`MQHIPIX2`), a model of the table's probe order, and crafted tables.

Plain Python + numpy, written from the format's description (DESIGN.md "On disk"; mq_capi_index_io.hpp, SavedSlot in
mq_build_kernels.hpp) and from the comment that states the probe sequence (mq_device.hpp, "Index table") -- not from the kernels
that walk it.  The file is a port through which a test can put ANY set of keys and entries into a table of ANY power-of-two
size: `Table` holds one crafted table once and feeds both sides, the HIP library through a file (`to_file`) and the CPU oracle
through `Index.add` / `set_ref` (`to_oracle`).  Mapping results do not depend on a table's geometry, so what a crafted table
must answer never comes from the code under test.

Layout (little-endian):
    magic "MQHIPIX2"
    mq_params: k u32, l u32, density f64, use_hpc u32, c u32, s u32, g u32, flags u32, 4 bytes of padding   (40 bytes)
    six u64: slot bytes (32), table_slots, n_kminmers, n_keys, n_unique, n_refs
    n_refs x (id u32, name_len u32, len u64, name)
    n_keys x slot (32 bytes): start u32, end u32, offset u32, id_rc u32 (id << 1 | rc), key u64, count u32, is_key0 u32
count = how often the key was inserted (the library writes 1 or 2); a key inserted more than once, or whose entry's end is 0,
is empty for every lookup (the reference's src/index.rs:67-69, 90-104).  The key 0 has is_key0 = 1 and no slot of the table:
it lives in one extra slot behind it.
"""
import struct

import numpy as np

MAGIC = b"MQHIPIX2"
PARAMS_FMT = "<IIdIIIII4x"
PARAM_NAMES = ("k", "l", "density", "use_hpc", "c", "s", "g", "flags")
SLOT_BYTES = 32
slot_dtype = np.dtype([("start", "<u4"), ("end", "<u4"), ("offset", "<u4"), ("id_rc", "<u4"), ("key", "<u8"), ("count", "<u4"),
                       ("is_key0", "<u4")])
assert slot_dtype.itemsize == SLOT_BYTES and struct.calcsize(PARAMS_FMT) == 40
HEADER_NAMES = ("slot_bytes", "table_slots", "n_kminmers", "n_keys", "n_unique", "n_refs")
MAX_REF_ID = 1 << 24  # reference ids stay below this

# one crafted insertion record: `count` insertions of `key`, the first of them with this payload
entry_dtype = np.dtype([("key", "<u8"), ("id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("offset", "<u4"), ("rc", "<u4"), ("count", "<u4")])


def params(k=5, l=31, density=0.01, use_hpc=True, c=4, s=11, g=2000, flags=0):
    return dict(k=k, l=l, density=density, use_hpc=1 if use_hpc else 0, c=c, s=s, g=g, flags=flags)


def header_counts(slots):
    """(n_kminmers, n_keys, n_unique) of a slot array by the reference's rule: a key is one map entry however often it was
    inserted; it is live iff it was inserted exactly once and its end is not 0."""
    if slots.size == 0:
        return 0, 0, 0
    keys, first, inv = np.unique(slots["key"], return_index=True, return_inverse=True)
    times = np.zeros(keys.size, dtype=np.uint64)
    np.add.at(times, inv.reshape(-1), slots["count"].astype(np.uint64))
    live = (times == 1) & (slots["end"][first] != 0)
    return int(slots["count"].astype(np.uint64).sum()), int(keys.size), int(live.sum())


def write(path, p, table_slots, refs, slots, n_kminmers=None, **wrong):
    """refs: (id, name, length) triples; slots: slot_dtype array.  n_keys / n_unique come from the slots (header_counts);
    `wrong` replaces header words on purpose (slot_bytes, n_keys, n_unique, n_refs; table_slots and n_kminmers are written as
    given) for files that must be refused.  Returns the header as written."""
    slots = np.ascontiguousarray(slots, dtype=slot_dtype)
    n_kmm, n_keys, n_unique = header_counts(slots)
    hdr = dict(slot_bytes=SLOT_BYTES, table_slots=int(table_slots), n_kminmers=n_kmm if n_kminmers is None else int(n_kminmers),
               n_keys=n_keys, n_unique=n_unique, n_refs=len(refs))
    for k, v in wrong.items():
        assert k in hdr, k
        hdr[k] = int(v)
    with open(path, "wb") as f:
        f.write(MAGIC)
        f.write(struct.pack(PARAMS_FMT, *[p[n] for n in PARAM_NAMES]))
        f.write(struct.pack("<6Q", *[hdr[n] for n in HEADER_NAMES]))
        for rid, name, length in refs:
            nb = name.encode()
            f.write(struct.pack("<IIQ", rid, len(nb), length) + nb)
        f.write(slots.tobytes())
    return hdr


def read(path):
    """(params, header, refs, slots) of an index file; raises ValueError on anything but a well-formed file."""
    blob = open(path, "rb").read()
    if blob[:8] != MAGIC:
        raise ValueError("bad magic")
    at = 8
    p = dict(zip(PARAM_NAMES, struct.unpack_from(PARAMS_FMT, blob, at)))
    at += 40
    hdr = dict(zip(HEADER_NAMES, struct.unpack_from("<6Q", blob, at)))
    at += 48
    if hdr["slot_bytes"] != SLOT_BYTES:
        raise ValueError("slot size")
    refs = []
    for _ in range(hdr["n_refs"]):
        rid, nl, length = struct.unpack_from("<IIQ", blob, at)
        at += 16
        refs.append((rid, blob[at:at + nl].decode(), length))
        at += nl
    if len(blob) - at != hdr["n_keys"] * SLOT_BYTES:
        raise ValueError("%d bytes of slots for %d keys" % (len(blob) - at, hdr["n_keys"]))
    return p, hdr, refs, np.frombuffer(blob, dtype=slot_dtype, offset=at).copy()


# ------------------------------------------------------------------ the probe order
def probe_order(key, table_slots):
    """The slots a key visits, in order: its home slot (key & mask), the other way of the home bucket, then the following
    buckets, way 0 before way 1, wrapping behind the last bucket.  Slot s = bucket s >> 1, way s & 1.  The key 0 visits the
    one extra slot behind the table (number table_slots) and nothing else."""
    if key == 0:
        return [table_slots]
    nb = table_slots // 2
    s0 = key & (table_slots - 1)
    b = s0 >> 1
    out = [s0, s0 ^ 1]
    for j in range(1, nb):
        bb = (b + j) % nb
        out += [2 * bb, 2 * bb + 1]
    return out


def home_slots(keys, table_slots):
    return np.asarray(keys, dtype=np.uint64) & np.uint64(table_slots - 1)


def home_buckets(keys, table_slots):
    return home_slots(keys, table_slots) >> np.uint64(1)


def pow2_above(n):
    """the smallest power of two above n"""
    p = 2
    while p <= n:
        p *= 2
    return p


# ------------------------------------------------------------------ one crafted table, both sides
class Table:
    def __init__(self, p, table_slots, refs, entries, name=""):
        self.name = name
        self.params = dict(p)
        self.table_slots = int(table_slots)
        self.refs = [(int(i), str(n), int(ln)) for i, n, ln in refs]
        self.entries = np.ascontiguousarray(entries, dtype=entry_dtype)
        assert np.unique(self.entries["key"]).size == self.entries.size, "one record per key"
        lens = {i: ln for i, _, ln in self.refs}
        e = self.entries
        # payloads a build could have produced: no case argues about arithmetic the reference does in usize
        assert all(int(i) in lens for i in np.unique(e["id"])) and (e["id"] < MAX_REF_ID).all()
        born = e["end"] == 0
        assert ((e["start"] < e["end"]) | born).all() and (e["offset"].astype(np.uint64) < 2**32 - 1).all()
        assert (e["end"].astype(np.uint64) <= np.array([lens[int(i)] for i in e["id"]], dtype=np.uint64)).all()

    def slots(self):
        e = self.entries
        s = np.zeros(e.size, dtype=slot_dtype)
        for f in ("start", "end", "offset", "key", "count"):
            s[f] = e[f]
        s["id_rc"] = (e["id"] << np.uint32(1)) | (e["rc"] & np.uint32(1))
        s["is_key0"] = (e["key"] == 0).astype(np.uint32)
        return s

    def header(self):
        n_kmm, n_keys, n_unique = header_counts(self.slots())
        return dict(slot_bytes=SLOT_BYTES, table_slots=self.table_slots, n_kminmers=n_kmm, n_keys=n_keys, n_unique=n_unique,
                    n_refs=len(self.refs))

    def to_file(self, path, slots=None, refs=None, **wrong):
        return write(path, self.params, wrong.pop("table_slots", self.table_slots), self.refs if refs is None else refs,
                     self.slots() if slots is None else slots, **wrong)

    def to_oracle(self, oracle):
        """The oracle's map with the same content: `add` once for a key inserted once, three times at most for one inserted
        more often (a third insertion leaves a dead key dead), `set_ref` for every reference."""
        ox = oracle.Index()
        for i, n, ln in self.refs:
            ox.set_ref(i, n, ln)
        for r in self.entries:
            for _ in range(min(int(r["count"]), 3)):
                ox.add(int(r["key"]), int(r["id"]), int(r["start"]), int(r["end"]), int(r["offset"]), int(r["rc"]))
        return ox

    def live_mask(self):
        return (self.entries["count"] == 1) & (self.entries["end"] != 0)

    def with_entries(self, entries, name=None):
        return Table(self.params, self.table_slots, self.refs, entries, name or self.name)


# ------------------------------------------------------------------ realistic keys: a simulated genome and reads from it
class Source:
    """A genome of a few contigs with repeats, reads from it with errors, and what the oracle says of both: the distinct
    k-min-mer hashes of the genome with the payload of their first insertion and their multiplicity (`entries`), every
    read's k-min-mer hashes (`read_hashes`: all of them in read order; `read_keys`: the distinct ones)."""

    def __init__(self, oracle, simlib, ps, lens, genome_seed, n_reads, reads_seed, len_mean, len_sd):
        self.ps = dict(ps)
        self.po = oracle.params(**ps)
        self.params = params(**ps)
        self.g, self.off, self.names = simlib.make_genome(lens, seed=genome_seed, repeat_frac=0.2, tandem_frac=0.03, threads=4)
        self.reads = simlib.make_reads(self.g, self.off, n_reads, seed=reads_seed, len_mean=len_mean, len_sd=len_sd, err=0.01, threads=4)
        self.refs = [(r, self.names[r], int(self.off[r + 1] - self.off[r])) for r in range(len(lens))]
        parts = []
        for r in range(len(lens)):
            km = oracle.kminmers(self.contig(r), self.po)
            a = np.zeros(km.size, dtype=entry_dtype)
            for f, o in (("key", "hash"), ("start", "start"), ("end", "end"), ("offset", "offset"), ("rc", "rev")):
                a[f] = km[o]
            a["id"] = r
            parts.append(a)
        ins = np.concatenate(parts)
        _, first, cnt = np.unique(ins["key"], return_index=True, return_counts=True)
        self.entries = ins[first].copy()
        self.entries["count"] = cnt
        self.n_insertions = int(ins.size)
        b, o = self.reads["bases"], self.reads["offsets"]
        per = [oracle.kminmers(b[int(o[i]):int(o[i + 1])], self.po)["hash"] for i in range(o.size - 1)
               if int(o[i + 1] - o[i]) >= self.po.l + self.po.k - 1]
        self.read_hashes = np.concatenate(per) if per else np.zeros(0, np.uint64)
        self.read_keys = np.unique(self.read_hashes)

    def contig(self, r):
        return self.g[int(self.off[r]):int(self.off[r + 1])]

    def oracle_index(self, oracle):
        """the oracle's own index of the genome, built from the sequences"""
        ox = oracle.Index()
        for r, n, _ in self.refs:
            ox.add_ref(r, n, self.contig(r), self.po)
        return ox


# The two legs.  `small`: the parameters of the crowded-table test on a genome sized so that `one_empty` stays within 2^16
# slots; `default`: the product's defaults on a genome of a few Mb.  Seeds are fixed; test_mqx_format.py asserts on the CPU
# that they meet every precondition of the tables below.
LEGS = {
    "small": dict(ps=dict(k=3, l=12, density=0.05), lens=[230000, 120000, 50000], genome_seed=24, n_reads=300, reads_seed=4,
                  len_mean=9000, len_sd=3000),
    "default": dict(ps=dict(), lens=[2000000, 1300000, 700000], genome_seed=31, n_reads=200, reads_seed=6, len_mean=20000,
                    len_sd=4000),
}
_sources = {}


def source(oracle, simlib, leg):
    if leg not in _sources:
        _sources[leg] = Source(oracle, simlib, **LEGS[leg])
    return _sources[leg]


FILLER_NAME = "filler"


def rehoused(src, factor=1):
    """The genome's full key set at the smallest power of two of slots above its key count (load between 1/2 and 1), or at
    `factor` times that."""
    return Table(src.params, pow2_above(src.entries.size) * factor, src.refs, src.entries, "rehoused x%d" % factor)


def filler_entries(src, n, seed, ref_id):
    """n live entries under random 64-bit keys that are neither 0, nor a key of the genome, nor a k-min-mer hash of a read"""
    rng = np.random.default_rng(seed)
    taken = np.union1d(src.entries["key"], src.read_keys)
    keys = np.zeros(0, np.uint64)
    while keys.size < n:
        c = rng.integers(1, 2**64, size=n - keys.size + 64, dtype=np.uint64)
        keys = np.unique(np.concatenate([keys, c[~np.isin(c, taken)]]))
    keys = rng.permutation(keys)[:n]
    a = np.zeros(n, dtype=entry_dtype)
    a["key"] = keys
    a["id"] = ref_id
    a["start"] = np.arange(n, dtype=np.uint32)
    a["end"] = a["start"] + 12
    a["offset"] = np.arange(n, dtype=np.uint32)
    a["rc"] = np.arange(n, dtype=np.uint32) & 1
    a["count"] = 1
    return a


def one_empty(src, seed=5):
    """The full key set padded with filler keys (live entries on a reference of their own) up to n_keys = table_slots - 1:
    every miss walks to the table's single empty slot.  The largest table the loader accepts."""
    ts = pow2_above(src.entries.size)
    n_fill = ts - 1 - src.entries.size
    fid = len(src.refs)
    refs = src.refs + [(fid, FILLER_NAME, n_fill + 12)]
    return Table(src.params, ts, refs, np.concatenate([src.entries, filler_entries(src, n_fill, seed, fid)]), "one_empty")


TABLE_END_EDGE = 8  # buckets at either end of the table whose keys are all kept


def table_end(src):
    """A subset chosen by home bucket, in a table of half `rehoused`'s size: every key homed in the last 8 and the first 8
    buckets, and of the rest those of every other block of 32 consecutive k-min-mers of a contig (runs survive, so reads
    still map).  Three keys homed in the last bucket share their walk from the third step on, so one of them sits behind
    the wrap whatever the insertion order: a HIT in bucket 0 or later for a key homed in the last bucket."""
    ts = pow2_above(src.entries.size) // 2
    nb = ts // 2
    hb = home_buckets(src.entries["key"], ts)
    keep = (hb >= nb - TABLE_END_EDGE) | (hb < TABLE_END_EDGE) | ((src.entries["offset"] // 32) % 2 == 0)
    return Table(src.params, ts, src.refs, src.entries[keep], "table_end")


def tiny_tables(src):
    """table_slots 2, 4, 8 with 1 .. table_slots - 1 keys: the first seven distinct live keys of the genome that the reads
    carry, in read order.  One bucket and two buckets: the wrap arithmetic at its smallest."""
    e = src.entries
    live = e[e["count"] == 1]
    order = {int(k): i for i, k in enumerate(live["key"])}
    seen, picked = set(), []
    for h in src.read_hashes:
        h = int(h)
        if h in order and h not in seen:
            seen.add(h)
            picked.append(order[h])
            if len(picked) == 7:
                break
    assert len(picked) == 7, "the reads carry fewer than 7 live keys"
    out = []
    for ts in (2, 4, 8):
        for n in range(1, ts):
            out.append(Table(src.params, ts, src.refs, live[picked[:n]], "tiny %d/%d" % (n, ts)))
    return out


def key0(src, mode):
    """`rehoused` plus an entry under the key 0: "live", "dead" (inserted twice) or "absent"."""
    t = rehoused(src)
    if mode == "absent":
        return t.with_entries(t.entries, "key0 absent")
    z = np.zeros(1, dtype=entry_dtype)
    z["id"], z["start"], z["end"], z["offset"], z["rc"], z["count"] = 1, 17, 40, 5, 1, (1 if mode == "live" else 2)
    return t.with_entries(np.concatenate([t.entries, z]), "key0 " + mode)


def dead(src):
    """`rehoused` with tombstones by every route the format has, put on keys the reads carry (every 5th live one, the four
    kinds in turn): count 2, 3 and 0xFFFFFFFF, and end = 0 with count 1 (an entry born empty)."""
    e = src.entries.copy()
    on = np.flatnonzero((e["count"] == 1) & np.isin(e["key"], src.read_keys))[::5]
    for j, i in enumerate(on):
        kind = j % 4
        if kind == 3:
            e["end"][i] = 0
        else:
            e["count"][i] = (2, 3, 0xFFFFFFFF)[kind]
    t = Table(src.params, pow2_above(e.size), src.refs, e, "dead")
    t.changed = e["key"][on]
    return t


IDS_MAP = (5, MAX_REF_ID - 1, 1000)  # contig r becomes reference IDS_MAP[r]; 1000 has an empty name
IDS_HUGE = (70000, "huge", 2**32 - 1)  # a reference whose length only the reference table knows
IDS_HOLE = 3  # an id below the largest that the table does not have


def ids(src):
    """`rehoused` under sparse reference ids, the largest possible one among them, one reference with an empty name, and
    one of length 2^32 - 1 that owns entries at the top of the 32-bit range."""
    assert len(src.refs) == len(IDS_MAP)
    e = src.entries.copy()
    e["id"] = np.array(IDS_MAP, dtype=np.uint32)[src.entries["id"]]
    refs = [(IDS_MAP[r], "" if IDS_MAP[r] == 1000 else n, ln) for r, n, ln in src.refs] + [IDS_HUGE]
    top = filler_entries(src, 4, 77, IDS_HUGE[0])
    top["start"] = 2**32 - 100 + np.arange(4, dtype=np.uint32)
    top["end"] = 2**32 - 1 - np.arange(4, dtype=np.uint32)
    top["offset"] = 2**32 - 2 - np.arange(4, dtype=np.uint32)
    ent = np.concatenate([e, top])
    return Table(src.params, pow2_above(ent.size), refs, ent, "ids")


# ------------------------------------------------------------------ what a table forces (the preconditions of the plans)
def miss_lookups(table, src):
    """the read lookups (one per k-min-mer of every read) whose key the table does not hold"""
    return src.read_hashes[~np.isin(src.read_hashes, table.entries["key"])]


def certain_steps(table, src):
    """A lower bound of the slots the reads' lookups visit beyond their home slots, from the table's content alone: a slot
    that is some table key's home slot is occupied wherever the keys ended up, so a lookup of an absent key homed there
    steps at least once."""
    k = table.entries["key"]
    occupied_homes = np.unique(home_slots(k[k != 0], table.table_slots))
    return int(np.isin(home_slots(miss_lookups(table, src), table.table_slots), occupied_homes).sum())


def max_misses_at_one_slot(table, src):
    m = miss_lookups(table, src)
    if m.size == 0:
        return 0
    return int(np.unique(home_slots(m, table.table_slots), return_counts=True)[1].max())


def check_table_end(t, src):
    nb = t.table_slots // 2
    n_last = int((home_buckets(t.entries["key"], t.table_slots) == nb - 1).sum())
    assert n_last >= 3, "table_end: %d keys homed in the last bucket" % n_last
    absent = src.read_keys[~np.isin(src.read_keys, t.entries["key"])]
    assert (home_buckets(absent, t.table_slots) == nb - 1).any(), "table_end: no read miss homed in the last bucket"
    assert t.entries.size < t.table_slots


def check_one_empty(t, src):
    assert t.header()["n_keys"] == t.table_slots - 1 and t.table_slots <= 1 << 16
    m = miss_lookups(t, src)
    assert m.size >= 1000, "one_empty: %d read lookups miss" % m.size
    hb = home_buckets(m, t.table_slots)
    nb = t.table_slots // 2
    assert (hb < nb // 2).any() and (hb >= nb // 2).any()
    assert not np.isin(t.entries["key"][t.entries["id"] == len(src.refs)], src.read_keys).any()


def check_rehoused(t):
    assert 2 * t.header()["n_keys"] > t.table_slots > t.header()["n_keys"]


def n_mapped(want):
    return int((want["mapped"] != 0).sum())
