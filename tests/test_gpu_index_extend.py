"""GPU: a finalized index kept and maintained -- mq_index_reopen + add + finalize, mq_index_resize (retable_kernel),
mq_index_load_sized, mq_index_clone_sized, and the two drivers' --add-reference / --index --table-factor.

What an extended index must be never comes from the extension itself: it is the index built from all references in one go, the
oracle's map of everything (Index.add), and the pure-Python union of two slot sets (tests/extend_data.py, checked against the
oracle on the CPU in tests/test_index_extend_host.py).  What a resized table must answer is what the table answered before, which
test_gpu_crafted_tables.py's _check_lookups holds against the oracle twin of each crafted table.  A dead key's payload is whichever
insertion claimed its slot, so slot sets are compared with dead payloads blanked (extend_data.sorted_slots).
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import extend_data as X
import mqx
from hipmem import DevBuf
from test_gpu_crafted_tables import _check_lookups
from test_gpu_parity import _cmp_hits, mq  # noqa: F401  (mq: the module fixture)

pytestmark = pytest.mark.gpu
N = len(X.LENS)
MQ_EINVAL, MQ_ESTATE = -1, -5


def _add(simlib, ix, refs):
    _, _, names = X.contigs(simlib)
    return sum(ix.add_ref(r, names[r], X.contig(simlib, r)) for r in refs)


def _built(mq, simlib, refs, factor=0, **pk):
    ix = mq.Index(mq.Params(**pk))
    if factor:
        ix.set_table_factor(factor)
    _add(simlib, ix, refs)
    ix.finalize()
    return ix


def _extended(mq, simlib, split, factor=0, **pk):
    ix = _built(mq, simlib, range(split), factor, **pk)
    ix.reopen()
    _add(simlib, ix, range(split, N))
    ix.finalize()
    return ix


def _queries(keys, seed=1):
    rnd = np.random.default_rng(seed).integers(1, 2**64, size=3000, dtype=np.uint64)
    return np.concatenate([np.asarray(keys, np.uint64), rnd[~np.isin(rnd, keys)], np.zeros(1, np.uint64)])


def _answers(ix, q):
    found, ent, ids = ix.lookup(q)
    return found.tobytes() + ent.tobytes() + ids.tobytes()


def _saved(ix, path):
    ix.save(path)
    p, hdr, refs, slots = mqx.read(path)
    return hdr, refs, X.sorted_slots(slots)


def _state(simlib, ix, q, path):
    """everything two equal indexes must agree on"""
    hdr, refs, slots = _saved(ix, path)
    r = X.reads(simlib)
    return dict(stats=ix.stats(), answers=_answers(ix, q), hdr=hdr, refs=refs, slots=slots.tobytes(), hits=ix.map_batch(r["bases"], r["offsets"]).tobytes())


def _assert_same(got, want, what, table_too=True):
    for k in ("stats", "hdr"):
        a, b = dict(got[k]), dict(want[k])
        if not table_too:
            for f in ("table_slots", "table_bytes"):
                a.pop(f, None), b.pop(f, None)
        assert a == b, (what, k, a, b)
    for k in ("answers", "refs", "slots", "hits"):
        assert got[k] == want[k], (what, k)


@pytest.fixture(scope="module")
def whole(mq, oracle, simlib, tmp_path_factory):
    """the index built in one go, the oracle's, the model's slot set and the queries every case uses"""
    tmp = tmp_path_factory.mktemp("whole")
    g, off, names = X.contigs(simlib)
    ix = _built(mq, simlib, range(N))
    ox, po = oracle.Index(), oracle.params()
    for r in range(N):
        ox.add_ref(r, names[r], X.contig(simlib, r), po)
    model = X.slot_set(X.insertions(oracle, simlib, range(N)))
    q = _queries(model["key"])
    st = _state(simlib, ix, q, str(tmp / "w.mqx"))
    assert st["slots"] == X.sorted_slots(model).tobytes() and st["stats"]["n_unique"] == ox.count() and st["stats"]["n_keys"] == ox.keys()
    r = X.reads(simlib)
    want = ox.map_batch(r["bases"], r["offsets"], po, threads=4)
    hits = np.frombuffer(st["hits"], dtype=mq.hit_dtype)
    _cmp_hits(hits, want)
    rn = simlib.read_names(r, names)
    paf = oracle.paf_lines(ox, rn, want)
    assert ix.paf_lines(rn, r["offsets"], hits) == paf and len(paf) >= 100
    return dict(ix=ix, ox=ox, q=q, st=st, rn=rn, paf=paf, model=model)


@pytest.mark.parametrize("split", range(N + 1))
def test_split_build_equals_whole_build(mq, oracle, simlib, tmp_path, whole, split):
    """A = the first `split` contigs, finalize, reopen, add the rest, finalize: the index built in one go (stats with table_slots,
    lookups, saved slot set, hits byte for byte, PAF lines).  Split 0 reopens an empty finalized index, split 6 adds nothing.  At the
    split 3 | 3 the keys that are live after the first finalize and dead after the second exist (asserted from the oracle)."""
    if split == X.SPLIT:
        k = X.kinds(X.slot_set(X.insertions(oracle, simlib, range(split))), X.slot_set(X.insertions(oracle, simlib, range(split, N))))
        assert all(x > 0 for x in k), k
    ix = _extended(mq, simlib, split)
    st = _state(simlib, ix, whole["q"], str(tmp_path / "e.mqx"))
    _assert_same(st, whole["st"], "split %d" % split)
    r = X.reads(simlib)
    assert ix.paf_lines(whole["rn"], r["offsets"], np.frombuffer(st["hits"], dtype=mq.hit_dtype)) == whole["paf"]
    ix.close()


def test_growth_and_no_growth(mq, simlib, tmp_path):
    """Table factor 2.  A = one small contig: adding the rest must at least quadruple the table, up to what the whole build gets.  A =
    all but the last contig, whose addition needs no larger table: table_slots stays."""
    w = _built(mq, simlib, range(N), factor=2)
    ws = w.stats()
    a = _built(mq, simlib, [3], factor=2)
    a_slots = a.stats()["table_slots"]
    assert ws["table_slots"] >= 4 * a_slots, (ws["table_slots"], a_slots)
    a.reopen()
    _add(simlib, a, [0, 1, 2, 4, 5])
    a.finalize()
    assert a.stats() == ws
    q = _queries(mqx.read(str(_save(w, tmp_path / "w.mqx")))[3]["key"])
    assert _answers(a, q) == _answers(w, q)
    b = _built(mq, simlib, range(N - 1), factor=2)
    b_slots = b.stats()["table_slots"]
    assert b_slots == ws["table_slots"], "precondition: the last contig needs no larger table"
    b.reopen()
    _add(simlib, b, [N - 1])
    b.finalize()
    assert b.stats() == ws and _answers(b, q) == _answers(w, q)
    for ix in (w, a, b):
        ix.close()


def _save(ix, path):
    ix.save(str(path))
    return path


@pytest.mark.parametrize("route", ["host", "device", "staged", "staged-lines"])
def test_every_add_route_after_reopen(mq, simlib, tmp_path, whole, route):
    g, off, names = X.contigs(simlib)
    ix = _built(mq, simlib, range(X.SPLIT))
    ix.reopen()
    rest = list(range(X.SPLIT, N))
    if route == "host":
        _add(simlib, ix, rest)
    elif route == "device":
        for r in rest:
            d = DevBuf.from_numpy(X.contig(simlib, r))
            ix.add_ref_device(r, names[r], d.ptr, int(off[r + 1] - off[r]))
            d.free()
    else:
        width = 70
        recs, at = [], 0
        for r in rest:
            s = X.contig(simlib, r).tobytes()
            body = b"".join(s[i:i + width] + b"\n" for i in range(0, len(s), width)) if route == "staged-lines" else s + b"\n"
            hdr = b">" + names[r].encode() + b"\n"
            recs.append((r, at + len(hdr), len(body) if route == "staged-lines" else len(s), hdr + body))
            at += len(hdr) + len(body)
        blob = np.frombuffer(b"".join(x[3] for x in recs), dtype=np.uint8)
        ix.stage_begin(blob.size)
        t = ix.stage_piece(0, blob)
        for r, seq_at, n, _ in recs:
            if route == "staged-lines":
                cnt, joined = ix.add_ref_staged_lines(r, names[r], seq_at, n, t)
                assert joined == int(off[r + 1] - off[r])
            else:
                ix.add_ref_staged(r, names[r], seq_at, n, t)
    ix.finalize()
    _assert_same(_state(simlib, ix, whole["q"], str(tmp_path / "r.mqx")), whole["st"], route)
    ix.close()


def test_contexts_across_a_growth(mq, simlib, whole):
    """Contexts made before the reopen -- a plain one, one after mq_ctx_reserve, one with a redo arena -- map, after a finalize that grew
    and moved the table, what a fresh context maps."""
    L = mq.load_library()
    r = X.reads(simlib)
    b, o = r["bases"], r["offsets"]
    n = o.size - 1
    ix = _built(mq, simlib, [3], factor=2)
    before = ix.stats()["table_slots"]
    plain, reserved, arena = ix.context(), ix.context(), ix.context()
    assert L.mq_ctx_reserve(reserved._h, n, int(o[-1])) == 0
    arena.reserve_redo(16, 30000)
    first = plain.map_batch(b, o).tobytes()
    assert reserved.map_batch(b, o).tobytes() == first
    ix.reopen()
    _add(simlib, ix, [0, 1, 2, 4, 5])
    ix.finalize()
    assert ix.stats()["table_slots"] >= 4 * before
    fresh = ix.context()
    want = fresh.map_batch(b, o).tobytes()
    assert want == whole["st"]["hits"] and want != first
    assert plain.map_batch(b, o).tobytes() == want and reserved.map_batch(b, o).tobytes() == want
    d_b, d_o, d_h = DevBuf.from_numpy(b), DevBuf.from_numpy(o), DevBuf(n * 48)
    arena.map_batch_device(d_b.ptr, d_o.ptr, n, int(o[-1]), d_h.ptr)
    arena.redo_counts()  # (waits for the stream)
    assert d_h.to_numpy(mq.hit_dtype, n).tobytes() == want
    for c in (plain, reserved, arena, fresh):
        c.close()
    ix.close()


def test_state(mq, simlib, whole):
    L = mq.load_library()
    g, off, names = X.contigs(simlib)
    r = X.reads(simlib)
    b, o = r["bases"], r["offsets"]
    n = o.size - 1
    fresh = mq.Index(mq.Params())
    assert L.mq_index_reopen(fresh.handle) == MQ_ESTATE and L.mq_index_resize(fresh.handle, 4096, 0) == MQ_ESTATE
    fresh.close()
    ix = _built(mq, simlib, range(X.SPLIT))
    ctx = ix.context()
    ix.reopen()
    assert L.mq_index_reopen(ix.handle) == MQ_ESTATE
    out = np.zeros(n, dtype=mq.hit_dtype)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    d_b, d_o, d_h = DevBuf.from_numpy(b), DevBuf.from_numpy(o), DevBuf(n * 48)
    assert L.mq_map_batch(ix.handle, p(b), p(o), n, p(out)) == MQ_ESTATE
    assert L.mq_map_batch_device(ix.handle, C.c_void_p(d_b.ptr), C.c_void_p(d_o.ptr), n, int(o[-1]), C.c_void_p(d_h.ptr), None) == MQ_ESTATE
    assert L.mq_ctx_map_batch(ctx._h, p(b), p(o), n, p(out)) == MQ_ESTATE
    assert L.mq_ctx_submit(ctx._h, p(b), p(o), n, p(out)) == MQ_ESTATE
    starts, lens = np.ascontiguousarray(o[:-1]), (o[1:] - o[:-1]).astype(np.uint32)
    assert L.mq_ctx_submit_spans(ctx._h, p(b), b.size, p(starts), p(lens), n, p(out)) == MQ_ESTATE
    fa = np.frombuffer(b">r\nACGTACGTTGCA\n", dtype=np.uint8)
    assert L.mq_ctx_submit_fasta(ctx._h, p(fa), 0, fa.size) == MQ_ESTATE
    for fmt in (0, 1, 2):
        assert L.mq_ctx_submit_fastx(ctx._h, p(fa), 0, fa.size, fmt) == MQ_ESTATE
    assert L.mq_ctx_map_batch_device(ctx._h, C.c_void_p(d_b.ptr), C.c_void_p(d_o.ptr), n, int(o[-1]), C.c_void_p(d_h.ptr), None) == MQ_ESTATE
    q = np.ones(4, dtype=np.uint64)
    f, e, i = np.zeros(4, np.uint8), np.zeros(4, mq.kminmer_dtype), np.zeros(4, np.uint32)
    assert L.mq_index_lookup(ix.handle, p(q), 4, p(f), p(e), p(i)) == MQ_ESTATE
    assert L.mq_index_save(ix.handle, b"/dev/null") == MQ_ESTATE and L.mq_index_resize(ix.handle, 1 << 20, 0) == MQ_ESTATE
    with pytest.raises(mq.MapquikError, match="duplicate ref_id"):
        ix.add_ref(1, "again", X.contig(simlib, 1))
    _add(simlib, ix, range(X.SPLIT, N))  # after the refused calls the index still works
    ix.finalize()
    assert ix.stats() == whole["st"]["stats"] and ctx.map_batch(b, o).tobytes() == whole["st"]["hits"]
    ctx.close()
    ix.close()


# ------------------------------------------------------------------ crafted tables through mq_index_resize
def _crafted(oracle, simlib):
    src = mqx.source(oracle, simlib, "small")
    big = mqx.rehoused(src)
    big = mqx.Table(big.params, 1 << 17, big.refs, big.entries, "2^17 slots")
    assert big.entries.size < 1 << 16
    return src, [mqx.one_empty(src), mqx.table_end(src), mqx.key0(src, "live"), mqx.key0(src, "dead"), mqx.dead(src), mqx.ids(src), big] + mqx.tiny_tables(src)


def _pow2s(lo, hi):
    out = []
    while lo <= hi:
        out.append(lo)
        lo *= 2
    return out


def test_resize_crafted_tables(mq, oracle, simlib, tmp_path):
    """Each crafted table resized to every power of two from the smallest legal size (one empty slot whenever n_keys + 1 is a power of
    two) to 8 times its own, and down again: the same lookups (found flag and payload, every key plus absent keys), the same stats
    but for the table's size, the same saved slot set under the new table_slots.  Sizes from 2 slots to 2^20: tails of the kernel's wave
    and workgroup footprint, and more than one workgroup."""
    L = mq.load_library()
    src, tables = _crafted(oracle, simlib)
    for t in tables:
        p = str(tmp_path / "t.mqx")
        hdr = t.to_file(p)
        ix = mq.Index.load(p)
        ox = t.to_oracle(oracle)
        _check_lookups(ix, ox, t, src)
        q = _queries(np.concatenate([t.entries["key"], src.read_keys[:2000]]))
        want = _answers(ix, q)
        _, _, slots0 = _saved(ix, str(tmp_path / "s0.mqx"))
        n_keys = hdr["n_keys"]
        # refused sizes: the index is untouched
        for ts, f in ((n_keys, 0), (mqx.pow2_above(n_keys) // 2, 0), (3 * 1024, 0), (1 << 41, 0), (1 << 20, 8), (0, 1), (0, 65), (1, 0)):
            if ts == 0 and f == 0:
                continue  # (a table without keys: "as it is", not a refusal)
            assert L.mq_index_resize(ix.handle, ts, f) == MQ_EINVAL, (t.name, ts, f)
        assert ix.stats()["table_slots"] == t.table_slots and _answers(ix, q) == want
        ix.resize()  # both 0: nothing happens
        assert ix.stats()["table_slots"] == t.table_slots
        up = _pow2s(mqx.pow2_above(n_keys), 8 * t.table_slots)
        for ts in up + up[-2::-1]:
            ix.resize(table_slots=ts)
            st = ix.stats()
            assert st["table_slots"] == ts and st["table_bytes"] == (ts // 2 + 1) * 64, (t.name, ts)
            assert {k: st[k] for k in ("n_refs", "n_kminmers", "n_keys", "n_unique")} == {k: hdr[k] for k in ("n_refs", "n_kminmers", "n_keys", "n_unique")}
            assert _answers(ix, q) == want, (t.name, ts)
            h2, _, slots = _saved(ix, str(tmp_path / "s.mqx"))
            assert h2 == dict(hdr, table_slots=ts) and slots.tobytes() == slots0.tobytes(), (t.name, ts)
        _check_lookups(ix, ox, t, src)  # at the smallest legal size
        if hdr["n_kminmers"] < 1 << 20:  # (the `dead` table records 2^32 - 1 insertions of a key: no table for so many is asked for here)
            ix.resize(factor=8)
            assert ix.stats()["table_slots"] == max(1024, mqx.pow2_above(8 * hdr["n_kminmers"] - 1), mqx.pow2_above(n_keys)) and _answers(ix, q) == want
        ix.close()


def test_load_sized_and_clone_sized(mq, oracle, simlib, tmp_path):
    """load_sized(file, S) and clone_sized onto the same device give what load(file) then resize(S) gives (lookups, stats, hits)."""
    src, tables = _crafted(oracle, simlib)
    b, o = src.reads["bases"], src.reads["offsets"]
    for t in tables[:6] + tables[-3:]:
        p = str(tmp_path / "t.mqx")
        t.to_file(p)
        q = _queries(np.concatenate([t.entries["key"], src.read_keys[:2000]]))
        n_keys = t.header()["n_keys"]
        sizes = [dict(table_slots=mqx.pow2_above(n_keys)), dict(table_slots=4 * t.table_slots)]
        if t.header()["n_kminmers"] < 1 << 20:  # (see test_resize_crafted_tables)
            sizes.append(dict(factor=2))
        for kw in sizes:
            a = mq.Index.load(p)
            a.resize(**kw)
            ls = mq.Index.load(p, **kw)
            cs = a.clone(0, **kw)
            plain = mq.Index.load(p).clone(0, table_slots=kw.get("table_slots", 0) or a.stats()["table_slots"])
            want = (a.stats(), _answers(a, q), a.map_batch(b, o).tobytes())
            for what, ix in (("load_sized", ls), ("clone_sized", cs), ("clone_sized of the file's table", plain)):
                assert (ix.stats(), _answers(ix, q), ix.map_batch(b, o).tobytes()) == want, (t.name, kw, what)
                ix.close()
            a.close()
        a = mq.Index.load(p)
        same = a.clone(0)  # both 0 in the sized calls: exactly load / clone
        assert mq.Index.load(p, table_slots=0, factor=0).stats() == a.stats() == same.stats()
        with pytest.raises(mq.MapquikError):
            a.clone(0, table_slots=n_keys if n_keys >= 2 and n_keys & (n_keys - 1) == 0 else 3)
        with pytest.raises(mq.MapquikError):
            a.clone(0, table_slots=1 << 20, factor=2)
        a.close()
        same.close()


def test_load_sized_refuses_what_load_refuses(mq, oracle, simlib, tmp_path):
    """Every file test_gpu_crafted_tables.py expects mq_index_load to refuse, at a legal requested size; and a good file at a size that
    does not exceed its key count, not a power of two, or given twice."""
    src = mqx.source(oracle, simlib, "small")
    t = mqx.rehoused(src)
    ts, h = t.table_slots, t.header()
    p = str(tmp_path / "bad.mqx")
    legal = 4 * ts

    def refused(slots=None, refs=None, **wrong):
        t.to_file(p, slots=slots, refs=refs, **wrong)
        for kw in (dict(table_slots=legal), dict(factor=2)):
            with pytest.raises(mq.MapquikError):
                mq.Index.load(p, **kw)

    refused(n_keys=ts)
    refused(n_keys=ts + 1)
    for bad_ts in (0, 1, 3, 2**41):
        refused(table_slots=bad_ts)
    refused(n_unique=h["n_keys"] + 1)
    refused(slot_bytes=64)
    refused(n_refs=2**24 + 1)
    refused(refs=t.refs + [(2**24, "beyond", 1000)])
    good = t.slots()
    hdr = dict(n_keys=h["n_keys"], n_unique=h["n_unique"])

    def with_slot(i, **fields):
        s = good.copy()
        for k, v in fields.items():
            s[k][i] = v
        return s

    i = int(np.flatnonzero(good["count"] == 1)[3])
    refused(slots=with_slot(i, count=0), **hdr)
    refused(slots=with_slot(i, key=0), **hdr)
    refused(slots=with_slot(i, is_key0=1), **hdr)
    refused(slots=with_slot(i, key=0, is_key0=2), **hdr)
    refused(n_unique=h["n_unique"] + 1)
    refused(n_unique=h["n_unique"] - 1)
    dup = good.copy()
    dup[i + 1] = dup[i]
    refused(slots=dup, **hdr)
    blob_ok = str(tmp_path / "ok.mqx")
    t.to_file(blob_ok)
    with open(p, "wb") as f:
        f.write(open(blob_ok, "rb").read() + b"\0")
    with pytest.raises(mq.MapquikError, match="bytes after the last slot"):
        mq.Index.load(p, table_slots=legal)
    with open(p, "wb") as f:
        f.write(open(blob_ok, "rb").read()[:-1])
    with pytest.raises(mq.MapquikError):
        mq.Index.load(p, table_slots=legal)
    for kw in (dict(table_slots=ts // 2), dict(table_slots=3 * ts), dict(table_slots=2**41), dict(table_slots=legal, factor=2), dict(factor=1), dict(factor=65)):
        with pytest.raises(mq.MapquikError):
            mq.Index.load(blob_ok, **kw)
    assert h["n_keys"] >= ts // 2  # (ts // 2 does not exceed the key count)
    mq.Index.load(blob_ok, table_slots=legal).close()


SIZES = (dict(table_slots=1 << 12), dict(factor=2))


def _refused_with(mq, path, text):
    """both sized forms refuse the file with mq_index_load's own text for it: the same check fires, not the size check ahead of it"""
    for kw in SIZES:
        with pytest.raises(mq.MapquikError) as ei:
            mq.Index.load(path, **kw)
        assert str(ei.value) == "mq_index_load_sized: " + text + path, (kw, str(ei.value))


def test_load_sized_refuses_the_hole_in_the_reference_table(mq, oracle, simlib, tmp_path):
    """test_gpu_crafted_tables.py's file with ONE entry moved to a reference id inside a hole of the (sparse) reference table: the
    refusal that rests on the dense length array uploaded before the scatter, here with the scatter running into a table of another size
    than the file's.  The unchanged file loads at both sizes."""
    src = mqx.source(oracle, simlib, "small")
    t = mqx.ids(src)
    p = str(tmp_path / "hole.mqx")
    t.to_file(p)
    sizes = (dict(table_slots=4 * t.table_slots), dict(factor=2))
    for kw in sizes:
        ix = mq.Index.load(p, **kw)
        assert ix.stats()["n_keys"] == t.header()["n_keys"]
        ix.close()
    assert mqx.IDS_HOLE not in [r[0] for r in t.refs] and mqx.IDS_HOLE < max(r[0] for r in t.refs)
    s = t.slots()
    s["id_rc"][11] = (mqx.IDS_HOLE << 1) | (int(s["id_rc"][11]) & 1)
    t.to_file(p, slots=s)
    for kw in sizes:
        with pytest.raises(mq.MapquikError) as ei:
            mq.Index.load(p, **kw)
        assert str(ei.value) == "mq_index_load_sized: corrupt index file (an entry names a reference the file does not have, or a malformed slot): " + p, kw


def test_load_sized_refused_at_every_section(mq, tmp_path):
    """test_gpu_crafted_tables.py's small file (two references, 40 keys) cut inside the header, inside the reference table, in the middle
    of a reference name, inside the slots, one byte short, and with one byte behind it: refused with the text of its section by both sized
    forms; the good file still loads at both sizes."""
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
        _refused_with(mq, p, text)
    for kw, want_slots in zip(SIZES, (1 << 12, 1024)):
        ix = mq.Index.load(good, **kw)
        st = ix.stats()
        assert {k: st[k] for k in mqx.HEADER_NAMES} == dict(hdr, table_slots=want_slots)
        assert [ix.ref_info(r) for r in (0, 1)] == [("alpha", 5000), ("beta", 3000)]
        ix.close()


def test_a_loaded_index_extended(mq, simlib, tmp_path, whole):
    a = _built(mq, simlib, range(X.SPLIT))
    a.save(str(tmp_path / "a.mqx"))
    a.close()
    ix = mq.Index.load(str(tmp_path / "a.mqx"))
    ix.reopen()
    _add(simlib, ix, range(X.SPLIT, N))
    ix.finalize()
    ix.save(str(tmp_path / "ab.mqx"))
    ix.close()
    back = mq.Index.load(str(tmp_path / "ab.mqx"))
    _assert_same(_state(simlib, back, whole["q"], str(tmp_path / "again.mqx")), whole["st"], "load, reopen, add, finalize, save, load")
    back.close()


@pytest.mark.parametrize("case", ["k7", "fast_kh", "variant4", "variant16", "no_spec"])
def test_other_parameters(mq, simlib, tmp_path, whole, monkeypatch, case):
    """The split 3 | 3 under other seeding parameters (variant 16 carries every minimizer's second position through the build scratch
    that the reopened index allocates anew), and on the run-time kernel pair (MQ_NO_SPEC=1)."""
    pk = dict(k7=dict(k=7), fast_kh=dict(fast_kh=True), variant4=dict(seeding_variant=4), variant16=dict(seeding_variant=16), no_spec=dict())[case]
    if case == "no_spec":
        monkeypatch.setenv("MQ_NO_SPEC", "1")
    w = _built(mq, simlib, range(N), **pk)
    q = _queries(mqx.read(str(_save(w, tmp_path / "w.mqx")))[3]["key"])
    e = _extended(mq, simlib, X.SPLIT, **pk)
    want = _state(simlib, w, q, str(tmp_path / "w2.mqx"))
    assert want["stats"]["n_unique"] > 1000 and want["stats"]["n_keys"] > want["stats"]["n_unique"]
    _assert_same(_state(simlib, e, q, str(tmp_path / "e.mqx")), want, case)
    if case == "no_spec":
        assert want["hits"] == whole["st"]["hits"] and e.last_map_spec() == 0
    w.close()
    e.close()


def _fasta(simlib, path, refs):
    _, _, names = X.contigs(simlib)
    with open(path, "wb") as f:
        for r in refs:
            f.write(b">" + names[r].encode() + b"\n" + X.contig(simlib, r).tobytes() + b"\n")
    return str(path)


@pytest.mark.parametrize("driver", ["native", "python"])
def test_drivers(mq, simlib, tmp_path, whole, driver):
    """--index a.mqx --add-reference b.fa --save-index ab.mqx: the PAF of --reference ab.fa byte for byte, and an ab.mqx with the whole
    build's slot set; --index a8.mqx --table-factor 2: the same PAF from a quarter of the table; --add-reference alone: exit 2."""
    from mapquik_amd import build
    cmd = [build.build_cli()] if driver == "native" else [sys.executable, "-m", "mapquik_amd"]
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = X.reads(simlib)
    rd = tmp_path / "reads.fa"
    with open(rd, "wb") as f:
        for i, n in enumerate(whole["rn"]):
            f.write(b">" + n.encode() + b"\n" + r["bases"][int(r["offsets"][i]):int(r["offsets"][i + 1])].tobytes() + b"\n")
    a, b, ab = (_fasta(simlib, tmp_path / n, refs) for n, refs in (("a.fa", range(X.SPLIT)), ("b.fa", range(X.SPLIT, N)), ("ab.fa", range(N))))
    t = lambda n: str(tmp_path / n)  # noqa: E731

    def run(args, rc=0, says=None):
        res = subprocess.run(cmd + [str(rd)] + args, capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == rc, (args, res.returncode, res.stderr[-2000:])
        assert says is None or says in res.stderr, (args, res.stderr[-2000:])
        return res

    run(["--reference", a, "--save-index", t("a.mqx"), "-p", t("a")])
    run(["--reference", ab, "--save-index", t("w.mqx"), "-p", t("w")])
    res = run(["--index", t("a.mqx"), "--add-reference", b, "--save-index", t("ab.mqx"), "-p", t("x")])
    assert res.stdout.count("Indexed reference ") == N - X.SPLIT
    want_paf = "".join(x + "\n" for x in whole["paf"])
    assert open(t("w.paf")).read() == want_paf and open(t("x.paf")).read() == want_paf
    (_, hw, rw, sw), (_, hx, rx, sx) = mqx.read(t("w.mqx")), mqx.read(t("ab.mqx"))
    assert hx == hw and rx == rw and X.sorted_slots(sx).tobytes() == X.sorted_slots(sw).tobytes() == whole["st"]["slots"]
    run(["--reference", ab, "--save-index", t("a8.mqx"), "--table-factor", "8", "-p", t("w8")])
    run(["--index", t("a8.mqx"), "--table-factor", "2", "-p", t("y")])
    run(["--index", t("a8.mqx"), "-p", t("z")])
    assert open(t("y.paf")).read() == want_paf and open(t("z.paf")).read() == want_paf
    assert mqx.read(t("a8.mqx"))[1]["table_slots"] >= 4 * 1024
    usage = "--add-reference adds to the index given with --index"  # (the flag is known: this check, not the argument parser's)
    run(["--add-reference", b, "-p", t("u")], rc=2, says=usage)
    run(["--reference", a, "--add-reference", b, "-p", t("u")], rc=2, says=usage)
