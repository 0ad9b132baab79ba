"""GPU: a finalized index takes another finished index in -- mq_index_merge (table to table, and the packed-slot route forced with
MQ_MERGE_PACKED=1), mq_index_merge_file, Index.merge / merge_file, and the two drivers' --merge-index.

What a merged index must be never comes from the merge: it is the index built from all references in one go, the oracle's map of
everything (stats, lookups, hits, PAF bytes), and for crafted files the dict model of tests/merge_data.py (checked against the probe-order
model of tests/mqx.py on the CPU in tests/test_index_merge_host.py).  A dead key's payload is whichever insertion claimed its slot, so
slot sets are compared with dead payloads blanked (merge_data.sorted_slots).  Every test here needs the two new symbols.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import extend_data as X
import merge_data as M
import mqx
from test_gpu_parity import _cmp_hits, mq  # noqa: F401  (mq: the module fixture)

pytestmark = pytest.mark.gpu
MQ_EINVAL, MQ_ESTATE = -1, -5
ALL = M.A_IDS + M.B_IDS + M.C_IDS
# the small cousin of the defaults, --nohpc, -k 7, the cheap tuple hash (what the oracle is given: the same without fast_kh)
PARAM_SETS = {"small": dict(k=3, l=9, density=0.15), "nohpc": dict(use_hpc=False), "k7": dict(k=7), "fast_kh": dict(fast_kh=True)}


def _opk(pk):
    return {k: v for k, v in pk.items() if k != "fast_kh"}


def _built(mq, simlib, refs, ids=None, factor=0, **pk):
    _, _, names = M.contigs(simlib)
    ix = mq.Index(mq.Params(fold_case=True, **pk))
    if factor:
        ix.set_table_factor(factor)
    for j, r in enumerate(refs):
        ix.add_ref(r if ids is None else ids[j], names[r], M.contig(simlib, r))
    ix.finalize()
    return ix


def _queries(keys, seed=1):
    rnd = np.random.default_rng(seed).integers(1, 2**64, size=2000, dtype=np.uint64)
    return np.concatenate([np.asarray(keys, np.uint64), rnd[~np.isin(rnd, keys)], np.zeros(1, np.uint64)])


def _answers(ix, q):
    found, ent, ids = ix.lookup(q)
    dead = found == 0  # (a lookup's payload fields are zeroed for a miss)
    assert not ent["end"][dead].any()
    return found.tobytes() + ent.tobytes() + ids.tobytes()


def _saved(ix, path):
    ix.save(str(path))
    p, hdr, refs, slots = mqx.read(str(path))
    return hdr, refs, M.sorted_slots(slots)


def _hits(simlib, ix):
    r = M.reads(simlib)
    return ix.map_batch(r["bases"], r["offsets"])


def _state(simlib, ix, q, path):
    hdr, refs, slots = _saved(ix, path)
    return dict(stats=ix.stats(), answers=_answers(ix, q), hdr=hdr, refs=refs, slots=slots.tobytes(), hits=_hits(simlib, ix).tobytes())


def _assert_same(got, want, what, table_too=False):
    for k in ("stats", "hdr"):
        a, b = dict(got[k]), dict(want[k])
        if not table_too:
            for f in ("table_slots", "table_bytes"):
                a.pop(f, None), b.pop(f, None)
        assert a == b, (what, k, a, b)
    for k in ("answers", "refs", "slots", "hits"):
        assert got[k] == want[k], (what, k)


_whole = {}


def _whole_of(mq, oracle, simlib, tmp, name, refs=ALL):
    """the from-scratch build of `refs` under a parameter set, the oracle's index and PAF, the queries: computed once, shared, left unchanged"""
    key = (name, tuple(refs))
    if key in _whole:
        return _whole[key]
    pk = PARAM_SETS[name]
    _, _, names = M.contigs(simlib)
    ix = _built(mq, simlib, refs, **pk)
    ox, po = oracle.Index(), oracle.params(**_opk(pk))
    for r in refs:
        ox.add_ref(r, names[r], M.contig(simlib, r, upper=True), po)
    hdr, _, slots = _saved(ix, tmp / ("whole_%s_%d.mqx" % (name, len(refs))))
    okeys = np.unique(M.insertions(oracle, simlib, refs, po)["key"])
    q = _queries(np.concatenate([slots["key"], okeys]))
    st = _state(simlib, ix, q, tmp / "w.mqx")
    assert st["stats"]["n_unique"] == ox.count() and st["stats"]["n_keys"] == ox.keys()
    r = M.reads(simlib)
    want = ox.map_batch(r["bases"], r["offsets"], po, threads=4)
    hits = np.frombuffer(st["hits"], dtype=mq.hit_dtype)
    _cmp_hits(hits, want)
    rn = simlib.read_names(r, names)
    paf = oracle.paf_lines(ox, rn, want)
    assert ix.paf_lines(rn, r["offsets"], hits) == paf and len(paf) >= 60, len(paf)
    if "fast_kh" not in pk:  # every oracle key, live or dead, answers as the oracle says
        found, ent, ids = ix.lookup(okeys)
        for i in range(0, okeys.size, 3):
            e = ox.get(int(okeys[i]))
            assert (e is not None) == bool(found[i]), i
            if e is not None:
                assert (int(e["id"]), int(e["rc"]), int(e["start"]), int(e["end"]), int(e["offset"])) == (int(ids[i]), int(ent["rev"][i]), int(ent["start"][i]), int(ent["end"][i]), int(ent["offset"][i]))
    _whole[key] = dict(ix=ix, q=q, st=st, rn=rn, paf=paf, pk=pk)
    return _whole[key]


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("merge")


# ------------------------------------------------------------------ 1. against a from-scratch build and the oracle
@pytest.mark.parametrize("name", list(PARAM_SETS))
def test_merge_equals_whole_build(mq, oracle, simlib, tmp, name):
    """merge(A, B) = build(A u B): stats, lookups of every key and of absent keys, saved slot set, hits byte for byte, PAF bytes = the
    oracle's.  The three classes of key are there (from the oracle's k-min-mers): live in both, dead in A, dead in B."""
    refs = M.A_IDS + M.B_IDS
    w = _whole_of(mq, oracle, simlib, tmp, name, refs)
    po = oracle.params(**_opk(w["pk"]))
    a, b = X.slot_set(M.insertions(oracle, simlib, M.A_IDS, po)), X.slot_set(M.insertions(oracle, simlib, M.B_IDS, po))
    twice_a, twice_b, once_each, once = X.kinds(a, b)
    print(name, "keys dead in A, dead in B, live in both, once in all:", (twice_a, twice_b, once_each, once))
    assert twice_a > 0 and twice_b > 0 and once_each > 0 and once > 0
    A, B = _built(mq, simlib, M.A_IDS, **w["pk"]), _built(mq, simlib, M.B_IDS, ids=[0, 1], **w["pk"])
    sa, sb = A.stats(), B.stats()
    assert A.merge(B) == 3  # (None: behind A's largest id)
    st = A.stats()
    assert st["n_kminmers"] == sa["n_kminmers"] + sb["n_kminmers"] and st["n_refs"] == 5
    got = _state(simlib, A, w["q"], tmp / "m.mqx")
    _assert_same(got, w["st"], name)
    r = M.reads(simlib)
    assert A.paf_lines(w["rn"], r["offsets"], np.frombuffer(got["hits"], dtype=mq.hit_dtype)) == w["paf"]
    assert B.stats() == sb  # the source is only read
    A.close()
    B.close()


# ------------------------------------------------------------------ 2. the three routes agree
def test_three_routes_agree(mq, oracle, simlib, tmp, monkeypatch):
    w = _whole_of(mq, oracle, simlib, tmp, "small", M.A_IDS + M.B_IDS)
    B = _built(mq, simlib, M.B_IDS, **w["pk"])
    B.save(str(tmp / "B.mqx"))
    out = {}
    for route in ("table", "packed", "file"):
        A = _built(mq, simlib, M.A_IDS, **w["pk"])
        if route == "packed":
            monkeypatch.setenv("MQ_MERGE_PACKED", "1")
        if route == "file":
            A.merge_file(str(tmp / "B.mqx"), id_base=0)
        else:
            A.merge(B, id_base=0)
        monkeypatch.delenv("MQ_MERGE_PACKED", raising=False)
        out[route] = _state(simlib, A, w["q"], tmp / ("r_%s.mqx" % route))
        A.close()
    B.close()
    for route in out:
        _assert_same(out[route], w["st"], route)


# ------------------------------------------------------------------ 3. associativity and order
def test_associativity_and_order(mq, oracle, simlib, tmp):
    """(A + B) + C = A + (B + C) = build(A u B u C); S_ABC's keys occur once in each: the second merge meets keys the first turned dead"""
    w = _whole_of(mq, oracle, simlib, tmp, "small")
    pk = w["pk"]
    po = oracle.params(**_opk(pk))
    sets = [set(M.insertions(oracle, simlib, ids, po)["key"].tolist()) for ids in (M.A_IDS, M.B_IDS, M.C_IDS)]
    assert len(sets[0] & sets[1] & sets[2]) > 0
    left = _built(mq, simlib, M.A_IDS, **pk)
    B, Cx = _built(mq, simlib, M.B_IDS, **pk), _built(mq, simlib, M.C_IDS, **pk)
    left.merge(B, id_base=0)
    left.merge(Cx, id_base=0)
    right = _built(mq, simlib, M.A_IDS, **pk)
    B.merge(Cx, id_base=0)
    right.merge(B, id_base=0)
    for what, ix in (("(A+B)+C", left), ("A+(B+C)", right)):
        _assert_same(_state(simlib, ix, w["q"], tmp / "assoc.mqx"), w["st"], what)
        ix.close()
    B.close()
    Cx.close()


# ------------------------------------------------------------------ 4. crafted files
def test_crafted_files(mq, tmp):
    """Crafted destination and source files (tests/mqx.py writes both sides) through mq_index_merge_file: the saved result is the dict model's
    slot set, its header the model's counts, every key answers as the model says and absent keys miss (also where ONE empty slot is left:
    every miss walks to it), and the result loads again."""
    for name, dst, src, id_base, declared in M.crafted_cases():
        pd, ps = str(tmp / "cd.mqx"), str(tmp / "cs.mqx")
        hd = dst.to_file(pd, **({} if declared is None else dict(n_kminmers=declared[0])))
        hs = src.to_file(ps, **({} if declared is None else dict(n_kminmers=declared[1])))
        model = M.Model(dst.slots(), hd["n_kminmers"])
        model.merge(src.slots(), id_base, hs["n_kminmers"])
        ix = mq.Index.load(pd)
        assert ix.merge_file(ps, id_base=id_base) == id_base
        st = ix.stats()
        assert (st["n_kminmers"], st["n_keys"], st["n_unique"], st["n_refs"]) == (model.n_kminmers, model.n_keys(), model.n_unique(), len(dst.refs) + len(src.refs)), name
        if name == "one empty slot":
            assert st["table_slots"] == 1024 and st["n_keys"] == 1023
        hdr, refs, slots = _saved(ix, tmp / "cm.mqx")
        assert slots.tobytes() == M.sorted_slots(model.slots()).tobytes(), name
        assert refs == sorted(dst.refs + [(i + id_base, n, ln) for i, n, ln in src.refs]), name
        keys = np.array(list(model.d), dtype=np.uint64)
        absent = M.rand_keys(np.random.default_rng(3), 500, keys)
        found, ent, ids = ix.lookup(np.concatenate([keys, absent]))
        assert found[:keys.size].tolist() == [1 if model.live(int(k)) else 0 for k in keys], name
        assert not found[keys.size:].any(), name
        for i in np.flatnonzero(found[:keys.size]):
            e = model.d[int(keys[i])]
            assert (int(ent["start"][i]), int(ent["end"][i]), int(ent["offset"][i]), (int(ids[i]) << 1) | int(ent["rev"][i])) == tuple(e[:4]), name
        back = mq.Index.load(str(tmp / "cm.mqx"))
        assert {k: back.stats()[k] for k in ("n_refs", "n_kminmers", "n_keys", "n_unique")} == {k: st[k] for k in ("n_refs", "n_kminmers", "n_keys", "n_unique")}, name
        back.close()
        ix.close()


# ------------------------------------------------------------------ 5. growth
def test_growth_and_contexts(mq, oracle, simlib, tmp):
    """Table factor 2: A alone sits in a table that A u B u C outgrows; the merges grow it to the whole build's size.  Contexts made before
    the merge (a plain one and one with reservations) map afterwards what a fresh one maps."""
    w = _whole_of(mq, oracle, simlib, tmp, "small")
    pk = w["pk"]
    whole2 = _built(mq, simlib, ALL, factor=2, **pk)
    A = _built(mq, simlib, [2], factor=2, **pk)
    rest = _built(mq, simlib, [0, 1, 3, 4, 5], ids=[0, 1, 3, 4, 5], factor=2, **pk)
    before = A.stats()["table_slots"]
    assert whole2.stats()["table_slots"] > before, "precondition: the merged count asks for a larger table"
    r = M.reads(simlib)
    b, o = r["bases"], r["offsets"]
    plain, reserved = A.context(), A.context()
    reserved.reserve_anchors(o.size - 1, 1 << 16)
    first = plain.map_batch(b, o).tobytes()
    A.merge(rest, id_base=0)
    assert A.stats() == whole2.stats() and A.stats()["table_slots"] > before
    # ids: contig 2 stayed 2, the others came under their own numbers: the whole build's hits and lookups
    assert _answers(A, w["q"]) == w["st"]["answers"]
    want = A.context().map_batch(b, o).tobytes()
    assert want == w["st"]["hits"] and want != first
    assert plain.map_batch(b, o).tobytes() == want and reserved.map_batch(b, o).tobytes() == want
    for ix in (A, rest, whole2):
        ix.close()


# ------------------------------------------------------------------ 6. refusals leave dst usable and unchanged
def test_refusals(mq, oracle, simlib, tmp):
    L = mq.load_library()
    w = _whole_of(mq, oracle, simlib, tmp, "small", M.A_IDS + M.B_IDS)
    pk = w["pk"]
    A = _built(mq, simlib, M.A_IDS, **pk)
    q = w["q"]
    st0, ans0, hits0 = A.stats(), _answers(A, q), _hits(simlib, A).tobytes()

    def unchanged(what):
        assert A.stats() == st0 and _answers(A, q) == ans0 and _hits(simlib, A).tobytes() == hits0, what

    def err():
        return (L.mq_last_error() or b"").decode()

    # every differing seeding parameter, one at a time, index to index and through a file
    base = dict(k=3, l=9, density=0.15, use_hpc=True, seeding_variant=0, fast_kh=False)
    for change in (dict(k=4), dict(l=10), dict(density=0.14), dict(use_hpc=False), dict(seeding_variant=32), dict(fast_kh=True)):
        other = _built(mq, simlib, [3], ids=[7], **dict(base, **change))
        assert L.mq_index_merge(A.handle, other.handle, 0) == MQ_EINVAL, change
        e = err()
        assert "same seeding parameters" in e and "-k 3 -l 9 -d 0.15 --seeding-variant 0" in e, e  # this index's set; the other's follows from the change
        for text, key in (("-k 4", "k"), ("-l 10", "l"), ("-d 0.14", "density"), ("--nohpc", "use_hpc"), ("--seeding-variant 32", "seeding_variant"), ("--fast-kh", "fast_kh")):
            assert (text in e) == (key in change), (change, e)
        other.save(str(tmp / "other.mqx"))
        assert L.mq_index_merge_file(A.handle, os.fsencode(str(tmp / "other.mqx")), 0) == MQ_EINVAL and "same seeding parameters" in err(), change
        other.close()
        unchanged(change)
    # mapping-time parameters may differ
    B = _built(mq, simlib, M.B_IDS, ids=[0, 1], **dict(pk, c=2, s=5, g=500))
    # an id collision, an id at 2^24, dst == src, an unfinalized src
    assert L.mq_index_merge(A.handle, B.handle, 2) == MQ_EINVAL and "already an id" in err()
    assert L.mq_index_merge(A.handle, B.handle, 2**24 - 1) == MQ_EINVAL and "2^24" in err()
    assert L.mq_index_merge(A.handle, A.handle, 100) == MQ_EINVAL and "same index" in err()
    raw = mq.Index(mq.Params(fold_case=True, **pk))
    raw.add_ref(0, "x", M.contig(simlib, 3))
    assert L.mq_index_merge(A.handle, raw.handle, 10) == MQ_ESTATE and "not finalized" in err()
    assert L.mq_index_merge(raw.handle, A.handle, 10) == MQ_ESTATE
    raw.close()
    unchanged("index-to-index refusals")
    # a context with a batch in flight
    r = M.reads(simlib)
    ctx = A.context()
    ctx.submit(r["bases"], r["offsets"])
    assert L.mq_index_merge(A.handle, B.handle, 3) == MQ_ESTATE and "submitted batch" in err()
    assert ctx.wait().tobytes() == hits0
    ctx.close()
    unchanged("context in flight")
    # the file: every header refusal of the loader, every per-slot refusal, a cut file, a byte too many
    B.save(str(tmp / "B.mqx"))
    p, hdr, refs, slots = mqx.read(str(tmp / "B.mqx"))
    bad = str(tmp / "bad.mqx")

    def refused(says, slots_=None, refs_=None, **wrong):
        ts = wrong.pop("table_slots", hdr["table_slots"])
        mqx.write(bad, p, ts, refs if refs_ is None else refs_, slots if slots_ is None else slots_, n_kminmers=hdr["n_kminmers"], **wrong)
        assert L.mq_index_merge_file(A.handle, os.fsencode(bad), 3) == MQ_EINVAL, (says, wrong)
        assert says in err(), (says, err())
        unchanged((says, wrong))

    not_index = "not a mapquik HIP index"
    refused(not_index, n_keys=hdr["table_slots"])
    for ts in (0, 1, 3, 2**41):
        refused(not_index, table_slots=ts)
    refused(not_index, n_unique=hdr["n_keys"] + 1)
    refused(not_index, slot_bytes=64)
    refused(not_index, n_refs=2**24 + 1)
    refused("truncated or unreadable", refs_=refs + [(2**24, "beyond", 1000)])
    refused("disagree with its header", n_unique=hdr["n_unique"] - 1)

    def with_slot(i, **fields):
        s = slots.copy()
        for k, v in fields.items():
            s[k][i] = v
        return s

    i = int(np.flatnonzero(slots["count"] == 1)[3])
    keep = dict(n_keys=hdr["n_keys"], n_unique=hdr["n_unique"])
    malformed = "a malformed slot"
    refused(malformed, slots_=with_slot(i, count=0), **keep)
    refused(malformed, slots_=with_slot(i, key=0), **keep)
    refused(malformed, slots_=with_slot(i, is_key0=1), **keep)
    refused(malformed, slots_=with_slot(i, key=0, is_key0=2), **keep)
    refused(malformed, slots_=with_slot(i, id_rc=(2 << 1) | 1), **keep)  # an id above the file's largest (0, 1)
    refused(malformed, slots_=with_slot(i, id_rc=(1 << 1)), refs_=[(0, refs[0][1], refs[0][2]), (4, refs[1][1], refs[1][2])], **keep)  # in a hole of it
    blob = open(str(tmp / "B.mqx"), "rb").read()
    for content, says in ((blob[:-1], "truncated"), (blob + b"\0", "bytes after the last slot"), (blob[:50], not_index), (b"", not_index)):
        with open(bad, "wb") as f:
            f.write(content)
        assert L.mq_index_merge_file(A.handle, os.fsencode(bad), 3) == MQ_EINVAL and says in err(), (says, err())
        unchanged(says)
    assert L.mq_index_merge_file(A.handle, os.fsencode(str(tmp / "none.mqx")), 3) == MQ_EINVAL and "cannot open" in err()
    with pytest.raises(mq.MapquikError, match="already an id"):
        A.merge_file(str(tmp / "B.mqx"), id_base=1)
    unchanged("file refusals")
    # after all of it the index still merges, and ends where the whole build ends (B's own c, s, g did not travel)
    assert A.merge_file(str(tmp / "B.mqx")) == 3
    _assert_same(_state(simlib, A, q, tmp / "after.mqx"), w["st"], "merge after the refusals")
    A.close()
    B.close()


# ------------------------------------------------------------------ 7. drivers
def _fasta(simlib, path, refs):
    _, _, names = M.contigs(simlib)
    with open(path, "wb") as f:
        for r in refs:
            f.write(b">" + names[r].encode() + b"\n" + M.contig(simlib, r).tobytes() + b"\n")
    return str(path)


@pytest.mark.parametrize("driver", ["native", "python"])
def test_drivers(mq, oracle, simlib, tmp, tmp_path, driver):
    """--index A.mqx --merge-index B.mqx --merge-index C.mqx --save-index ABC.mqx: the PAF of --reference ABC.fa byte for byte; ABC.mqx
    loads and maps the same; --reference A.fa --merge-index B.mqx --merge-index C.mqx too; --merge-index alone: exit 2."""
    from mapquik_amd import build
    cmd = [build.build_cli()] if driver == "native" else [sys.executable, "-m", "mapquik_amd"]
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    w = _whole_of(mq, oracle, simlib, tmp, "small")
    r = M.reads(simlib)
    rd = tmp_path / "reads.fa"
    with open(rd, "wb") as f:
        for i, n in enumerate(w["rn"]):
            f.write(b">" + n.encode() + b"\n" + r["bases"][int(r["offsets"][i]):int(r["offsets"][i + 1])].tobytes() + b"\n")
    a, b, c, abc = (_fasta(simlib, tmp_path / n, refs) for n, refs in (("a.fa", M.A_IDS), ("b.fa", M.B_IDS), ("c.fa", M.C_IDS), ("abc.fa", ALL)))
    t = lambda n: str(tmp_path / n)  # noqa: E731
    seeding = ["-k", "3", "-l", "9", "-d", "0.15"]

    def run(args, rc=0, says=None):
        res = subprocess.run(cmd + [str(rd)] + seeding + args, capture_output=True, text=True, timeout=300, env=env)
        assert res.returncode == rc, (args, res.returncode, res.stderr[-2000:])
        assert says is None or says in res.stderr, (args, res.stderr[-2000:])
        return res

    for fa, ix in ((a, "a.mqx"), (b, "b.mqx"), (c, "c.mqx")):
        run(["--reference", fa, "--save-index", t(ix), "-p", t("tmp")])
    run(["--reference", abc, "-p", t("w")])
    res = run(["--index", t("a.mqx"), "--merge-index", t("b.mqx"), "--merge-index", t("c.mqx"), "--save-index", t("abc.mqx"), "-p", t("x")])
    out = res.stdout
    assert "Merged index %s: 2 references" % t("b.mqx") in out and "Merged index %s: 1 references" % t("c.mqx") in out
    assert out.index(t("b.mqx")) < out.index(t("c.mqx")) < out.index("Saved index to")
    want_paf = "".join(x + "\n" for x in w["paf"])
    assert open(t("w.paf")).read() == want_paf and open(t("x.paf")).read() == want_paf
    run(["--index", t("abc.mqx"), "-p", t("y")])
    run(["--reference", a, "--merge-index", t("b.mqx"), "--merge-index", t("c.mqx"), "-p", t("z")])
    assert open(t("y.paf")).read() == want_paf and open(t("z.paf")).read() == want_paf
    _, hx, rx, sx = mqx.read(t("abc.mqx"))
    assert M.sorted_slots(sx).tobytes() == w["st"]["slots"] and [x[0] for x in rx] == ALL
    assert {k: hx[k] for k in ("n_kminmers", "n_keys", "n_unique", "n_refs")} == {k: w["st"]["hdr"][k] for k in ("n_kminmers", "n_keys", "n_unique", "n_refs")}
    run(["--merge-index", t("b.mqx"), "-p", t("u")], rc=2, says="--merge-index merges into the index given with --index or built from --reference")
