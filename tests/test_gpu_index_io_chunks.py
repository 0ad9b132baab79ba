"""The chunk borders of the index movers: mq_index_load / mq_index_load_sized / mq_index_merge_file (the file-to-device slot streamer) and
mq_index_save (its own device-to-file loop) with MQ_IX_IO_CHUNK=96 -- three slots per chunk, where the product moves 64 MB.

Files of 0, 1, 3, 4, 6, 7 and 25 slots: no chunk, a partial one, exactly one, one and a slot, exactly two, two and a slot, nine (more than the
loader's eight workers).  tests/mqx.py writes every file and reads every saved one; what an index must answer comes from mqx.Table and the
dict model of merge_data.py, never from the library.  Every route runs a second time with the hook unset and must give the same.

Refusals at a border: a slot with count 0 as the last of the first chunk, the first of the second, and alone in the last; the file cut one
slot short (its last chunk is missing altogether) and with 32 bytes too many.  The cut and the lengthened file hold well-formed slots only:
with a malformed slot as well, the loader (which finds bytes behind the slots after scattering them) and mq_index_merge_file (which holds
the file's size against its header before it reads a slot) answer with different texts, today as before.
"""
import numpy as np
import pytest

import merge_data as M
import mqx
from test_gpu_parity import mq  # noqa: F401  (mq: the module fixture)

pytestmark = pytest.mark.gpu
HOOK, CHUNK = "MQ_IX_IO_CHUNK", "96"  # 3 slots of 32 bytes
P = mqx.params(k=3, l=12, density=0.05)
FILE_REFS = [(1, "f1", 100000), (4, "", 100000)]  # two ids, holes below and between them
DST_REFS = [(0, "d0", 100000)]
ID_BASE = 2
COUNTS = (0, 1, 3, 4, 6, 7, 25)
COUNT_FIELDS = ("n_refs", "n_kminmers", "n_keys", "n_unique")


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("chunks")


def file_table(n):
    """n slots under both reference ids; from three slots on, the second is the key 0's and the last is dead (count 2)"""
    keys = M.rand_keys(np.random.default_rng(100 + n), n)
    if n >= 3:
        keys[1] = 0
    e = M.entries(keys, 1)
    e["id"][1::2] = 4
    if n >= 3:
        e["count"][n - 1] = 2
    return mqx.Table(P, 64, FILE_REFS, e, "file %d" % n)


def dst_table(src):
    """a small destination: five keys of its own, and the file's first and last key (a live one and, from three slots on, the dead one)"""
    own = M.rand_keys(np.random.default_rng(7), 5, src.entries["key"])
    shared = np.unique(src.entries["key"][[0, -1]]) if src.entries.size else np.zeros(0, np.uint64)
    return mqx.Table(P, 1024, DST_REFS, M.entries(np.concatenate([own, shared[shared != 0]]), 0, start0=500), "dst")


def queries(keys):
    absent = M.rand_keys(np.random.default_rng(3), 40, keys)
    q = np.concatenate([np.asarray(keys, np.uint64), absent])
    return q if (q == 0).any() else np.concatenate([q, np.zeros(1, np.uint64)])  # the key 0 is asked for whether it is there or not


def check_lookups(ix, model, what):
    """every key of the model answers as the model says, absent keys miss; returns the raw answer"""
    keys = np.array(list(model.d), dtype=np.uint64)
    q = queries(keys)
    found, ent, ids = ix.lookup(q)
    assert found[:keys.size].tolist() == [1 if model.live(int(k)) else 0 for k in keys], what
    assert not found[keys.size:].any(), what
    for i in np.flatnonzero(found[:keys.size]):
        e = model.d[int(keys[i])]
        assert (int(ent["start"][i]), int(ent["end"][i]), int(ent["offset"][i]), (int(ids[i]) << 1) | int(ent["rev"][i])) == tuple(e[:4]), what
    return found.tobytes() + ent.tobytes() + ids.tobytes()


def counts_of(ix):
    st = ix.stats()
    return {k: st[k] for k in COUNT_FIELDS}


def by_key(slots):
    return slots[np.argsort(slots["key"], kind="stable")]


def routes(mq, tmp, n):
    """the file of n slots through load, load at another size, merge_file and save; everything the library said, for the second run to equal"""
    t = file_table(n)
    path, out = str(tmp / ("f%d.mqx" % n)), {}
    hdr = t.to_file(path)
    model = M.Model(t.slots(), hdr["n_kminmers"])
    want = dict(n_refs=2, n_kminmers=hdr["n_kminmers"], n_keys=hdr["n_keys"], n_unique=hdr["n_unique"])
    assert want["n_keys"] == n and want["n_unique"] == model.n_unique()
    for what, kw, slots in (("load", {}, 64), ("load_sized", dict(table_slots=256), 256)):
        ix = mq.Index.load(path, **kw)
        assert counts_of(ix) == want and ix.stats()["table_slots"] == slots, (what, n)
        out[what] = check_lookups(ix, model, (what, n))
        assert [ix.ref_info(i) for i, _, _ in FILE_REFS] == [(nm, ln) for _, nm, ln in FILE_REFS], (what, n)
        for hole in (0, 2, 3, 5):
            with pytest.raises(mq.MapquikError, match="unknown ref_id"):
                ix.ref_info(hole)
        if what == "load":  # save's own chunk loop: the file comes back, slot for slot
            saved = str(tmp / "saved.mqx")
            ix.save(saved)
            p2, hdr2, refs2, slots2 = mqx.read(saved)
            assert p2 == t.params and hdr2 == hdr and refs2 == t.refs, n
            assert by_key(slots2).tobytes() == by_key(t.slots()).tobytes(), n
            out["saved"] = open(saved, "rb").read()[:8 + 40 + 48]  # (the order of the slots is the packer's, run by run)
        ix.close()
    d = dst_table(t)
    pd = str(tmp / "dst.mqx")
    hd = d.to_file(pd)
    merged = M.Model(d.slots(), hd["n_kminmers"])
    merged.merge(t.slots(), ID_BASE, hdr["n_kminmers"])
    ix = mq.Index.load(pd)
    assert ix.merge_file(path, id_base=ID_BASE) == ID_BASE
    assert counts_of(ix) == dict(n_refs=3, n_kminmers=merged.n_kminmers, n_keys=merged.n_keys(), n_unique=merged.n_unique()), n
    out["merge_file"] = check_lookups(ix, merged, ("merge_file", n))
    assert [ix.ref_info(i + ID_BASE) for i, _, _ in FILE_REFS] == [(nm, ln) for _, nm, ln in FILE_REFS] and ix.ref_info(0) == ("d0", 100000), n
    ix.close()
    return out


@pytest.mark.parametrize("n", COUNTS)
def test_chunk_borders(mq, tmp, monkeypatch, n):
    monkeypatch.setenv(HOOK, CHUNK)
    small = routes(mq, tmp, n)
    monkeypatch.delenv(HOOK)
    assert routes(mq, tmp, n) == small, n


def test_refusals_at_a_border(mq, tmp, monkeypatch):
    monkeypatch.setenv(HOOK, CHUNK)
    t = file_table(7)
    good, bad = str(tmp / "good7.mqx"), str(tmp / "bad7.mqx")
    hdr = t.to_file(good)
    d = dst_table(t)
    pd = str(tmp / "dst7.mqx")
    hd = d.to_file(pd)
    dst = mq.Index.load(pd)
    before = M.Model(d.slots(), hd["n_kminmers"])
    st0, ans0 = dst.stats(), check_lookups(dst, before, "dst")

    def refused(says, what):
        for kw in ({}, dict(table_slots=256)):
            with pytest.raises(mq.MapquikError, match=says):
                mq.Index.load(bad, **kw)
        with pytest.raises(mq.MapquikError, match=says):
            dst.merge_file(bad, id_base=ID_BASE)
        assert dst.stats() == st0 and check_lookups(dst, before, what) == ans0, what

    for at in (2, 3, 6):  # last of the first chunk, first of the second, alone in the last
        s = t.slots()
        s["count"][at] = 0
        mqx.write(bad, P, 64, FILE_REFS, s, n_kminmers=hdr["n_kminmers"], n_keys=hdr["n_keys"], n_unique=hdr["n_unique"])
        refused("a malformed slot", at)
    blob = open(good, "rb").read()
    for content, says in ((blob[:-mqx.SLOT_BYTES], "truncated"), (blob + bytes(32), "bytes after the last slot")):
        with open(bad, "wb") as f:
            f.write(content)
        refused(says, says)
    # and the destination still takes the good file
    assert dst.merge_file(good, id_base=ID_BASE) == ID_BASE
    after = M.Model(d.slots(), hd["n_kminmers"])
    after.merge(t.slots(), ID_BASE, hdr["n_kminmers"])
    assert dst.stats()["n_keys"] == after.n_keys() and dst.stats()["n_unique"] == after.n_unique()
    check_lookups(dst, after, "after the refusals")
    dst.close()
