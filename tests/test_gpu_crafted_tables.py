"""GPU: crafted index files -- table wrap, long walks, the key 0, tombstones, sparse reference ids, and save against the oracle.

The library never builds a table above load 1/2, and its own builds reach the table's hard cases only by luck.  The on-disk
index is a port through which any set of keys goes into a table of any power-of-two size (tests/mqx.py writes the file from
the format's description), and the oracle has the same port (`Index.add`, `set_ref`): every table here exists once
(`mqx.Table`) and feeds both sides.  For each table: `stats` and `ref_info` against the file's header, `lookup` of every key
of the table, of every read k-min-mer hash outside it, of 5,000 random absent keys and of the key 0 against
`oracle.Index.get`; `map_batch` against the oracle twin's (and, where the table holds the genome's full key set, byte for
byte against the index the library built from the sequences); the device-resident form on a result buffer filled with 0xFF;
and `save` of the loaded index parsed by `mqx.read` (the same key set, live payloads and dead set).

Reads are mapped with MapSink::probe_all (one 16-byte home-bucket load, then walking rounds shared by the wave), `lookup`
walks with probe_table, the loader inserts with table_insert: three routines with their own wrap arithmetic, all held
against the probe order as mq_device.hpp states it.

The key 0 on the MAP path stays out of reach: it needs a read whose k-min-mer tuple hashes to 0, and no preimage of 0 under
SipHash-1-3 (or under the fast tuple hash with its per-length start value) is at hand.  probe_all's `k == 0` branch is
covered by reading only; the key 0 is covered through insert, count, lookup, save and clone.

No case is skipped or filtered at run time: the preconditions of tests/test_mqx_format.py are asserted again at the top of
each test, and a seed that misses one fails the test.
"""
import numpy as np
import pytest

import mqx
from test_gpu_parity import _cmp_hits, _map_both, mq  # noqa: F401  (mq: the module fixture)
from test_gpu_poison import _assert_all_written, _launch_poisoned

pytestmark = pytest.mark.gpu

_built = {}


def built(mq, oracle, simlib, leg):
    """the leg's source, the index the library builds itself from the sequences, the oracle's, and both sides' hits"""
    if leg not in _built:
        src = mqx.source(oracle, simlib, leg)
        ix, ox, hits, want = _map_both(mq, oracle, src.g, src.off, src.names, src.reads, src.ps)
        _cmp_hits(hits, want)
        st = ix.stats()
        assert (st["n_keys"], st["n_unique"], st["n_kminmers"]) == (src.entries.size, int((src.entries["count"] == 1).sum()), src.n_insertions)
        _built[leg] = dict(src=src, ix=ix, ox=ox, hits=hits, want=want)
    return _built[leg]


def _check_lookups(ix, ox, t, src, seed=1):
    keys = t.entries["key"]
    rng = np.random.default_rng(seed)
    rnd = rng.integers(1, 2**64, size=5000, dtype=np.uint64)
    q = np.concatenate([keys, src.read_keys[~np.isin(src.read_keys, keys)], rnd[~np.isin(rnd, keys)], np.zeros(1, np.uint64)])
    found, ent, ids = ix.lookup(q)
    got = np.stack([found.astype(np.uint64), ids.astype(np.uint64)] + [ent[f].astype(np.uint64) for f in ("start", "end", "offset", "rev")], axis=1)
    want = np.zeros_like(got)
    for i, h in enumerate(q):
        e = ox.get(int(h))
        if e is not None:
            want[i] = (1, e["id"], e["start"], e["end"], e["offset"], e["rc"])
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, (t.name, bad.size, [(hex(int(q[i])), got[i].tolist(), want[i].tolist()) for i in bad[:5]])
    assert np.array_equal(ent["hash"], q)
    assert int(want[:keys.size, 0].sum()) == t.header()["n_unique"]  # every live key of the table was asked for and found


def _check_save(mq, ix, t, path):
    """`save` of the loaded index, parsed by the second implementation: the same key set, the same live payloads, the same
    dead set (a dead key's payload is whichever insertion claimed the slot: key and count >= 2 only), is_key0 exactly on the
    key 0."""
    ix.save(path)
    p, hdr, refs, slots = mqx.read(path)
    assert p == t.params and hdr == t.header() and refs == sorted(t.refs), t.name
    mine = t.slots()
    a, b = slots[np.argsort(slots["key"], kind="stable")], mine[np.argsort(mine["key"], kind="stable")]
    assert np.array_equal(a["key"], b["key"]), t.name
    assert np.array_equal(a["is_key0"], (a["key"] == 0).astype(np.uint32)), t.name
    live = (b["count"] == 1) & (b["end"] != 0)
    assert np.array_equal(a["count"] == 1, live) and (a["count"][~live] >= 2).all(), t.name
    assert a[live].tobytes() == b[live].tobytes(), t.name


def _check_table(mq, oracle, t, src, tmp_path, identical_to=None, full=True):
    """one crafted table through load, stats, ref_info, lookup, host-form map, device-form map on a poisoned buffer, save"""
    p = str(tmp_path / "crafted.mqx")
    hdr = t.to_file(p)
    ix = mq.Index.load(p)
    st = ix.stats()
    assert {k: st[k] for k in mqx.HEADER_NAMES} == hdr, t.name
    for rid, name, ln in t.refs:
        assert ix.ref_info(rid) == (name, ln), (t.name, rid)
    ox = t.to_oracle(oracle)
    _check_lookups(ix, ox, t, src)
    b, o = src.reads["bases"], src.reads["offsets"]
    hits = ix.map_batch(b, o)
    want = ox.map_batch(b, o, src.po, threads=4)
    _cmp_hits(hits, want)
    if identical_to is not None:
        assert np.array_equal(hits.view(np.uint8), identical_to.view(np.uint8)), t.name
    if full:
        dev = _launch_poisoned(mq, ix, b, o)
        _assert_all_written(dev)
        assert np.array_equal(dev.view(np.uint8), hits.view(np.uint8)), t.name
        _check_save(mq, ix, t, str(tmp_path / "saved.mqx"))
    return ix, ox, hits, want


def _check_clone(mq, ix, ox, t, src, hits):
    """a replica (device-to-device copy of a table the build could not have made) looks up and maps like its source"""
    c = ix.clone(0)
    assert c.stats() == ix.stats()
    _check_lookups(c, ox, t, src, seed=2)
    assert np.array_equal(c.map_batch(src.reads["bases"], src.reads["offsets"]).view(np.uint8), hits.view(np.uint8))
    c.close()


LEGS = ("small", "default")


@pytest.mark.parametrize("leg", LEGS)
def test_rehoused(mq, oracle, simlib, tmp_path, leg):
    """The genome's full key set at load between 1/2 and 1 (the smallest power of two above n_keys) and at a quarter of that
    load: the hits of the index the library built itself, byte for byte."""
    B = built(mq, oracle, simlib, leg)
    src = B["src"]
    t = mqx.rehoused(src)
    mqx.check_rehoused(t)
    for tab in (t, mqx.rehoused(src, 4)):
        ix, ox, hits, want = _check_table(mq, oracle, tab, src, tmp_path, identical_to=B["hits"])
        assert mqx.n_mapped(want) >= 0.9 * mqx.n_mapped(B["want"])
        ix.close()


@pytest.mark.parametrize("leg", LEGS)
def test_one_empty(mq, oracle, simlib, tmp_path, leg):
    """n_keys = table_slots - 1, the largest table the loader accepts: every miss walks to the single empty slot -- long
    walks, many lanes of a wave walking together for different distances, about half of them through the wrap."""
    B = built(mq, oracle, simlib, leg)
    src = B["src"]
    t = mqx.one_empty(src)
    mqx.check_one_empty(t, src)
    ix, ox, hits, want = _check_table(mq, oracle, t, src, tmp_path, identical_to=B["hits"])
    assert mqx.n_mapped(want) >= 0.9 * mqx.n_mapped(B["want"])
    _check_clone(mq, ix, ox, t, src, hits)
    ix.close()


def test_table_end(mq, oracle, simlib, tmp_path):
    """A subset with at least three keys homed in the last bucket: a HIT whose slot lies behind the wrap, on the map path
    (the oracle twin holds the same subset), and a read miss homed in the last bucket that walks into bucket 0."""
    B = built(mq, oracle, simlib, "small")
    src = B["src"]
    t = mqx.table_end(src)
    mqx.check_table_end(t, src)
    ix, ox, hits, want = _check_table(mq, oracle, t, src, tmp_path)
    assert mqx.n_mapped(want) >= 20
    ix.close()


def test_tiny(mq, oracle, simlib, tmp_path):
    """table_slots 2, 4, 8 with 1 .. table_slots - 1 keys: one bucket and two buckets, the wrap arithmetic of insert,
    lookup and the map path's walk at its smallest."""
    B = built(mq, oracle, simlib, "small")
    src = B["src"]
    tabs = mqx.tiny_tables(src)
    assert [(t.table_slots, t.entries.size) for t in tabs] == [(s, n) for s in (2, 4, 8) for n in range(1, s)]
    for t in tabs:
        ix, ox, hits, want = _check_table(mq, oracle, t, src, tmp_path)
        ix.close()


@pytest.mark.parametrize("leg,mode", [("small", "live"), ("small", "dead"), ("small", "absent"), ("default", "live")])
def test_key0(mq, oracle, simlib, tmp_path, leg, mode):
    """The key 0 present in a table -- live, dead, and absent: the extra bucket through insert, count, lookup, save and
    clone; n_keys counts it, no slot of the table holds it.  (Not through the map path: see the module's docstring.)"""
    B = built(mq, oracle, simlib, leg)
    src = B["src"]
    t = mqx.key0(src, mode)
    ix, ox, hits, want = _check_table(mq, oracle, t, src, tmp_path, identical_to=B["hits"])
    base = mqx.rehoused(src).header()
    st = ix.stats()
    assert st["n_keys"] == base["n_keys"] + (mode != "absent") and st["n_unique"] == base["n_unique"] + (mode == "live")
    found, ent, ids = ix.lookup(np.zeros(1, np.uint64))
    assert bool(found[0]) == (mode == "live")
    if mode == "live":
        assert (int(ids[0]), int(ent[0]["start"]), int(ent[0]["end"]), int(ent[0]["offset"]), int(ent[0]["rev"])) == (1, 17, 40, 5, 1)
    if mode != "absent":
        _check_clone(mq, ix, ox, t, src, hits)
    ix.close()


def test_dead(mq, oracle, simlib, tmp_path):
    """Tombstones by every route the format has, on keys the reads carry: count 2, 3 and 0xFFFFFFFF, and end = 0 with
    count 1 (an entry born empty, src/index.rs:67-69)."""
    B = built(mq, oracle, simlib, "small")
    src = B["src"]
    t = mqx.dead(src)
    assert t.changed.size >= 40
    ix, ox, hits, want = _check_table(mq, oracle, t, src, tmp_path)
    assert ix.stats()["n_unique"] == mqx.rehoused(src).header()["n_unique"] - t.changed.size
    found, _, _ = ix.lookup(t.changed)
    assert not found.any()
    ix.close()


def test_ids_and_the_hole(mq, oracle, simlib, tmp_path):
    """Sparse reference ids with 2^24 - 1 among them, a reference with an empty name, one of length 2^32 - 1 that only the
    file's table knows: the dense length array and mq_format_paf on the largest id.  The same file with ONE entry moved
    to an id inside a hole of the reference table (below the largest id, not in the table) must be refused: it used to
    load, and reads mapped to a reference that does not exist."""
    B = built(mq, oracle, simlib, "small")
    src = B["src"]
    t = mqx.ids(src)
    ix, ox, hits, want = _check_table(mq, oracle, t, src, tmp_path)
    assert (hits["ref_id"][hits["status"] == 1] == mqx.MAX_REF_ID - 1).any() and (hits["ref_id"][hits["status"] == 1] == 1000).any()
    rn = simlib.read_names(src.reads, src.names)
    lines = ix.paf_lines(rn, src.reads["offsets"], hits)
    assert lines == oracle.paf_lines(ox, rn, want) and len(lines) >= 0.9 * mqx.n_mapped(B["want"])
    ix.close()
    assert mqx.IDS_HOLE not in [r[0] for r in t.refs] and mqx.IDS_HOLE < max(r[0] for r in t.refs)
    s = t.slots()
    s["id_rc"][11] = (mqx.IDS_HOLE << 1) | (int(s["id_rc"][11]) & 1)
    p = str(tmp_path / "hole.mqx")
    t.to_file(p, slots=s)
    with pytest.raises(mq.MapquikError):
        mq.Index.load(p)


def test_files_that_must_be_refused(mq, oracle, simlib, tmp_path):
    """Headers the host refuses before anything is launched (mq_index_load checks the header before it creates the index or
    a table; a table without an empty slot would make a miss walk forever, so that check has to be first), and slots the
    scatter or the count that follows it refuses.  Each raises MapquikError and leaves no device memory behind."""
    from hipmem import hip
    import ctypes as C
    B = built(mq, oracle, simlib, "small")
    src = B["src"]
    t = mqx.rehoused(src)
    ts, h = t.table_slots, t.header()
    p = str(tmp_path / "bad.mqx")

    def free_bytes():
        f, tot = C.c_size_t(), C.c_size_t()
        assert hip().hipMemGetInfo(C.byref(f), C.byref(tot)) == 0
        return f.value

    def refused(slots=None, refs=None, **wrong):
        t.to_file(p, slots=slots, refs=refs, **wrong)
        with pytest.raises(mq.MapquikError):
            mq.Index.load(p)

    def cycle():
        t.to_file(p)
        mq.Index.load(p).close()
        refused(n_unique=h["n_unique"] + 1)

    cycle()
    before = free_bytes()
    # decided on the host, from the header and the reference table
    refused(n_keys=ts)
    refused(n_keys=ts + 1)
    for bad_ts in (0, 1, 3, 2**41):
        refused(table_slots=bad_ts)
    refused(n_unique=h["n_keys"] + 1)
    refused(slot_bytes=64)
    refused(n_refs=2**24 + 1)
    refused(refs=t.refs + [(2**24, "beyond", 1000)])
    # decided on the device
    good = t.slots()
    hdr = dict(n_keys=h["n_keys"], n_unique=h["n_unique"])

    def with_slot(i, **fields):
        s = good.copy()
        for k, v in fields.items():
            s[k][i] = v
        return s

    i = int(np.flatnonzero(good["count"] == 1)[3])
    refused(slots=with_slot(i, count=0), **hdr)
    refused(slots=with_slot(i, key=0), **hdr)                  # the key 0 outside its slot
    refused(slots=with_slot(i, is_key0=1), **hdr)              # a key that is not 0 in the key 0's slot
    refused(slots=with_slot(i, key=0, is_key0=2), **hdr)
    refused(n_unique=h["n_unique"] + 1)
    refused(n_unique=h["n_unique"] - 1)
    dup = good.copy()
    dup[i + 1] = dup[i]                                        # the same key in two slots: the table holds fewer keys than the header says
    refused(slots=dup, **hdr)
    cycle()
    after = free_bytes()
    assert before - after < (64 << 20), (before, after)


def test_load_refused_at_every_section(mq, tmp_path):
    """A valid small file (two references, 40 keys) cut inside the header, inside the reference table, in the middle of a reference
    name, inside the slots and one byte short of its end, and the whole file with one byte behind it: each load is refused with the
    text of its section, and a good file still loads afterwards with the header's numbers."""
    rng = np.random.default_rng(12)
    e = np.zeros(40, dtype=mqx.entry_dtype)
    e["key"] = np.unique(rng.integers(1, 2**64, size=64, dtype=np.uint64))[:40]
    e["id"] = np.arange(40) % 2
    e["start"] = 10 * np.arange(40)
    e["end"] = e["start"] + 31
    e["offset"] = np.arange(40)
    e["rc"] = np.arange(40) & 1
    e["count"] = 1
    t = mqx.Table(mqx.params(), 128, [(0, "alpha", 5000), (1, "beta", 3000)], e, "two refs, 40 keys")
    good = str(tmp_path / "good.mqx")
    hdr = t.to_file(good)
    blob = open(good, "rb").read()
    head = 8 + 40 + 48
    refs_end = head + (16 + len("alpha")) + (16 + len("beta"))
    assert len(blob) == refs_end + 40 * mqx.SLOT_BYTES
    not_an_index = "not a mapquik HIP index (or another layout version): "
    truncated = "truncated or unreadable index file: "
    cases = [("header", blob[:50], not_an_index),
             ("reference table", blob[:head + 16 + len("alpha") + 8], truncated),
             ("reference name", blob[:head + 16 + 2], truncated),
             ("slots", blob[:refs_end + 10 * mqx.SLOT_BYTES + 7], truncated),
             ("one byte short", blob[:-1], truncated),
             ("one byte more", blob + b"\0", "corrupt index file (bytes after the last slot): ")]
    for what, content, text in cases:
        p = str(tmp_path / "cut.mqx")
        with open(p, "wb") as f:
            f.write(content)
        with pytest.raises(mq.MapquikError) as ei:
            mq.Index.load(p)
        print("%s: %s" % (what, ei.value))
        assert str(ei.value) == "mq_index_load: " + text + p, what
    ix = mq.Index.load(good)
    st = ix.stats()
    assert {k: st[k] for k in mqx.HEADER_NAMES} == hdr
    assert [ix.ref_info(r) for r in (0, 1)] == [("alpha", 5000), ("beta", 3000)]
    ix.close()


def test_probe_stats_walks(mq, oracle, simlib, tmp_path, capsys):
    """Slots visited beyond the home slot by the reads' lookups (the instrumented launch).  Lower bounds from the table's
    content and the probe order alone: on `one_empty` every miss steps at least once except those homed at the one empty
    slot (at most the largest number of misses homed at one slot); on any table a miss homed at a slot that is some key's
    home slot steps at least once (that slot is occupied wherever the keys went).  At load above 1/2 a miss visits more than
    one further slot on average, so `rehoused` is held to the first form as well.  And `one_empty` walks more per lookup
    than the library's own factor-2 table of the same genome: two measured values, no constant."""
    from hipmem import DevBuf
    B = built(mq, oracle, simlib, "small")
    src = B["src"]
    b, o = src.reads["bases"], src.reads["offsets"]
    n = o.size - 1
    d_b, d_o, d_h = DevBuf.from_numpy(b), DevBuf.from_numpy(o), DevBuf(n * 48)

    def measure(ix):
        lookups, extra = ix.probe_stats(d_b.ptr, d_o.ptr, n, int(o[-1]), d_h.ptr)
        assert np.array_equal(d_h.to_numpy(mq.hit_dtype, n).view(np.uint8), B["hits"].view(np.uint8))
        assert lookups == src.read_hashes.size
        return lookups, extra

    rates = {}
    for t in (mqx.one_empty(src), mqx.rehoused(src)):
        p = str(tmp_path / "t.mqx")
        t.to_file(p)
        ix = mq.Index.load(p)
        lookups, extra = measure(ix)
        misses = mqx.miss_lookups(t, src).size
        assert misses >= 1000
        rates[t.name] = extra / lookups
        print("probe_stats %s: lookups %d, misses %d, extra steps %d (%.3f per lookup)" % (t.name, lookups, misses, extra, extra / lookups))
        assert extra >= misses - mqx.max_misses_at_one_slot(t, src), t.name
        assert extra >= mqx.certain_steps(t, src), t.name
        ix.close()
    f2 = mq.Index(mq.Params(**src.ps))
    f2.set_table_factor(2)
    for r, name, _ in src.refs:
        f2.add_ref(r, name, src.contig(r))
    f2.finalize()
    st = f2.stats()
    assert st["table_slots"] <= 4 * st["n_kminmers"]
    lookups, extra = measure(f2)
    rates["factor 2"] = extra / lookups
    print("probe_stats factor-2 table (%d slots, %d keys): extra steps %d (%.3f per lookup)" % (st["table_slots"], st["n_keys"], extra, extra / lookups))
    assert rates["one_empty"] > rates["factor 2"]
    f2.close()
    with capsys.disabled():
        print("\n[crafted tables] extra steps per lookup: " + ", ".join("%s %.3f" % kv for kv in rates.items()))
