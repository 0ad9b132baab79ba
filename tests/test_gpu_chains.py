"""GPU: the chains output (mq_ctx_reserve_chains, include/mapquik_hip.h) -- every candidate chain of every read, ties included.  Every case
compares spans and chains with the model (tests/chains_model.py; test_chains_model.py ties it to the oracle's records and asserts that the
inputs hold the cases they are named after) read for read, and the hits byte for byte with a context WITHOUT a reservation on the same
index.  Spans and pool are filled with 0xFF on the device before the call, and every span of the batch must have been written."""
import numpy as np
import pytest

import anchors_model as A
import chains_model as CM
import hipmem
import mosaic as M

pytestmark = pytest.mark.gpu

MQ_ESTATE, MQ_EINVAL = -5, -1
DROPPED = 0xFFFFFFFF


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture()
def O(oracle):
    yield oracle
    oracle.lib().mqo_set_variant(0)


def _index_both(mq, O, g, off, names, ps, variant=0):
    O.lib().mqo_set_variant(variant)
    P, po = mq.Params(seeding_variant=variant, **ps), O.params(**ps)
    ix, ox = mq.Index(P), O.Index()
    for r in range(off.size - 1):
        s = g[int(off[r]):int(off[r + 1])]
        assert ix.add_ref(r, names[r], s) == ox.add_ref(r, names[r], s, po)
    assert ix.finalize() == ox.count()
    return ix, ox, po


def _poison(c, max_reads, max_chains):
    """the context's device span array and pool filled with 0xFF"""
    sp, ch = c.chains_device()
    assert hipmem.hip().hipMemset(sp, 0xFF, 8 * int(max_reads)) == 0 and hipmem.hip().hipMemset(ch, 0xFF, 48 * int(max_chains)) == 0
    hipmem.device_sync()


def _reserving(ix, max_reads, max_chains):
    c = ix.context()
    c.reserve_chains(max_reads, max_chains)
    _poison(c, max_reads, max_chains)
    return c


def _check(got, exp, cap, hits=None):
    """spans, chains and counters of one batch against the model's lists; returns the reads that were dropped"""
    spans, chains, info = got
    assert spans.size == len(exp)
    assert not ((spans["first"] == DROPPED) & (spans["count"] == DROPPED)).any()  # every span was written
    need = sum(len(e) for e in exp)
    assert int(spans["count"].sum()) == need == info["needed"] and info["stored"] == min(need, cap) == chains.size
    words = chains.view(np.uint32).reshape(-1, 12)
    used, dropped = [], []
    for r, e in enumerate(exp):
        f, c = int(spans["first"][r]), int(spans["count"][r])
        assert c == len(e), r
        if not e:
            assert f == 0, r
            continue
        if f == DROPPED:
            dropped.append(r)
            continue
        assert f + c <= info["stored"], r
        assert [tuple(w) for w in words[f:f + c].tolist()] == [CM.as_words(x) for x in e], r
        used.append((f, f + c))
        if hits is not None:  # the unique top chain is the hit in every word but word 9; a read without one is not mapped
            tops = [j for j in range(c) if e[j][0] & CM.TOP]
            h = hits[r:r + 1].view(np.uint32).reshape(12)
            if len(tops) == 1:
                w = words[f + tops[0]]
                assert int(h[0]) == 1 and [int(x) for x in w[:9]] == [int(x) for x in h[:9]] and [int(x) for x in w[10:]] == [int(x) for x in h[10:]], r
            else:
                assert int(h[0]) == 0 and len(tops) >= 2, r
    used.sort()
    assert all(a[1] <= b[0] for a, b in zip(used, used[1:]))  # stored lists are pairwise disjoint
    assert info["dropped_reads"] == len(dropped)
    if need <= cap:
        assert not dropped
    return dropped


def _run_host(mq, ix, exp, bases, offs, cap=None):
    """map_batch on a reserving context and on a plain one: hits equal byte for byte, chains as the model says"""
    n = offs.size - 1
    need = sum(len(e) for e in exp)
    cap = max(need, 1) if cap is None else cap
    plain = ix.context()
    want = plain.map_batch(bases, offs)
    plain.close()
    c = _reserving(ix, n, cap)
    hits = c.map_batch(bases, offs)
    assert hits.tobytes() == want.tobytes()
    got = c.chains()
    dropped = _check(got, exp, cap, hits)
    c.close()
    return got, dropped


# ------------------------------------------------------------------ contents on the mosaic world
@pytest.fixture(scope="module")
def mos(mq, oracle, simlib):
    g, off, names, sets, wrap = CM.batches(oracle, simlib)
    ix, ox, po = _index_both(mq, oracle, g, off, names, dict())
    yield dict(ix=ix, ox=ox, po=po, sets=sets, wrap=wrap, genome=(g, off, names))
    ix.close()


@pytest.mark.parametrize("name", ["counts", "ties", "below", "strands"])
def test_contents(mq, O, mos, name):
    """counts: 1 .. 5, 63 .. 65, 128, 129 chains and the default leg's most; ties: 2-, 17- and 65-way beside near-ties; below: a tie under a
    larger winner; strands: both strands with one run and with several (g = 50)"""
    bases, offs = mos["sets"][name]
    ix = mos["ix"]
    g = 50 if name == "strands" else 2000
    ix.set_map_params(4, 11, g)
    try:
        exp = CM.batch(O, mos["ox"], O.params(g=g), bases, offs)
        _run_host(mq, ix, exp, bases, offs)
    finally:
        ix.set_map_params(4, 11, 2000)


def test_the_largest_count_through_the_host_redo(mq, O, mos):
    """the mosaic's read with the most candidate references (the k = 1 leg): more than 2048 runs, so its chains come from the host-driven redo"""
    ps, bases, offs = mos["sets"]["most"]
    g, off, names = mos["genome"]
    ix, ox, po = _index_both(mq, O, g, off, names, ps)
    exp = CM.batch(O, ox, po, bases, offs)
    assert len(exp[0]) >= 180
    _run_host(mq, ix, exp, bases, offs)
    ix.close()


def test_wrapping_coordinates(mq, O, mos):
    g, off, names, bases, offs, ps = mos["wrap"]
    ix, ox, po = _index_both(mq, O, g, off, names, ps)
    b, o = M.select(bases, offs, list(range(0, offs.size - 1, 3))[:40])
    exp = CM.batch(O, ox, po, b, o)
    assert sum(1 for chs in exp for c in chs if c[4] >> 32 or c[5] >> 32) >= 3
    _run_host(mq, ix, exp, b, o)
    ix.close()


def test_chain_chunk_4(mq, O, mos, monkeypatch):
    """MQ_CHAIN_CHUNK=4 (read at mq_index_new): 1 .. 5 chains on the chunk's borders, and the long lists through many chunks"""
    monkeypatch.setenv("MQ_CHAIN_CHUNK", "4")
    g, off, names = mos["genome"]
    ix, ox, po = _index_both(mq, O, g, off, names, dict())
    bases, offs = mos["sets"]["counts"]
    _run_host(mq, ix, CM.batch(O, ox, po, bases, offs), bases, offs)
    ix.close()


# ------------------------------------------------------------------ a small plain batch: launch forms, pool edges, lifecycle
@pytest.fixture(scope="module")
def plain(mq, oracle, simlib):
    g, off, names = simlib.make_genome([300000, 200000], seed=77, repeat_frac=0.2)
    reads = simlib.make_reads(g, off, 60, seed=5, len_mean=7000, err=0.02)
    bases, offs = reads["bases"].copy(), reads["offsets"]
    for r in (3, 17, 40):  # reads with an N: the fast seeder declines them (map_declined_kernel)
        bases[int(offs[r]) + 1500] = ord("N")
    ix, ox, po = _index_both(mq, oracle, g, off, names, dict())
    exp = CM.batch(oracle, ox, po, bases, offs)
    assert sum(len(e) >= 1 for e in exp) >= 40 and any(len(e) >= 2 for e in exp)
    c0 = ix.context()
    want = c0.map_batch(bases, offs)
    spec0 = c0.last_map_spec()
    c0.close()
    yield dict(ix=ix, ox=ox, po=po, bases=bases, offs=offs, exp=exp, want=want, need=sum(len(e) for e in exp), spec0=spec0, genome=(g, off, names))
    ix.close()


def _records(bases, offs, fmt):
    seqs = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(offs.size - 1)]
    if fmt == "fasta":
        return b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate(seqs))
    if fmt == "fastq":
        return b"".join(b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))
    return b"".join(b">r%d\n" % i + b"".join(s[j:j + 70] + b"\n" for j in range(0, len(s), 70)) for i, s in enumerate(seqs))


@pytest.mark.parametrize("form", ["host", "submit", "spans", "device", "fasta", "fastq", "lines"])
def test_every_launch_form(mq, plain, form):
    fx = plain
    ix, bases, offs, n, want = fx["ix"], fx["bases"], fx["offs"], fx["offs"].size - 1, fx["want"]
    c = _reserving(ix, n, fx["need"])
    if form == "host":
        hits = c.map_batch(bases, offs)
    elif form == "submit":
        c.submit(bases, offs)
        hits = c.wait()
    elif form == "spans":
        c.submit_spans(bases, offs[:-1], (offs[1:] - offs[:-1]).astype(np.uint32))
        hits = c.wait()
    elif form == "device":
        db, do, dout = hipmem.DevBuf.from_numpy(bases), hipmem.DevBuf.from_numpy(offs), hipmem.DevBuf(n * 48)
        hipmem.memset(dout, 0xFF)
        c.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dout.ptr)
        got = c.chains()  # waits for the call's stream itself
        hits = dout.to_numpy(mq.hit_dtype, n)
        for b in (db, do, dout):
            b.free()
    else:
        buf = np.frombuffer(_records(bases, offs, form), dtype=np.uint8)
        c.submit_fasta(buf, fastq=form == "fastq", lines=form == "lines")
        res = c.wait_fasta_lines() if form == "lines" else c.wait_fasta()
        hits = res[0]
        assert res[-1] == 0
    assert hits.tobytes() == want.tobytes()
    if form != "device":
        got = c.chains()
    assert not _check(got, fx["exp"], fx["need"], hits)
    assert c.last_map_spec() == 0 and fx["spec0"] == 1  # the product path is untouched: the pair of the defaults without a reservation
    c.close()


def test_no_spec_makes_no_difference(mq, O, plain, monkeypatch):
    monkeypatch.setenv("MQ_NO_SPEC", "1")
    g, off, names = plain["genome"]
    ix, ox, po = _index_both(mq, O, g, off, names, dict())
    c = _reserving(ix, plain["offs"].size - 1, plain["need"])
    assert c.map_batch(plain["bases"], plain["offs"]).tobytes() == plain["want"].tobytes()
    assert not _check(c.chains(), plain["exp"], plain["need"]) and c.last_map_spec() == 0
    c.close()
    ix.close()


def test_pool_edges(mq, plain):
    fx = plain
    exp, need = fx["exp"], fx["need"]
    _, d = _run_host(mq, fx["ix"], exp, fx["bases"], fx["offs"], cap=need)
    assert not d
    (spans, chains, info), d = _run_host(mq, fx["ix"], exp, fx["bases"], fx["offs"], cap=need - 1)
    # exactly the reads whose claim ended beyond the pool are dropped: the stored lists fill [0, first dropped claim) without a hole,
    # every dropped read would not have fit behind them, and at least the read that claimed last is among them
    assert len(d) >= 1 and info["needed"] == need and info["dropped_reads"] == len(d)
    # claims are handed out from one cursor and tile [0, need): with room for need - 1 entries only the claim that ends at `need` -- the read
    # that claimed last -- crosses the pool's end.  So exactly one read is dropped, and the stored lists tile [0, need - its count) without a hole
    assert len(d) == 1
    stored = sorted((int(spans["first"][r]), len(exp[r])) for r in range(len(exp)) if exp[r] and r not in d)
    at = 0
    for f, c in stored:
        assert f == at
        at += c
    assert at == need - len(exp[d[0]]) and int(spans["count"][d[0]]) == len(exp[d[0]])
    (spans, chains, info), d = _run_host(mq, fx["ix"], exp, fx["bases"], fx["offs"], cap=1)
    with_chains = [r for r, e in enumerate(exp) if e]
    assert len(d) >= len(with_chains) - 1 and info["stored"] == 1 and info["needed"] == need
    assert all(int(spans["count"][r]) == len(exp[r]) for r in d)


def test_batches_and_reservation_lifecycle(mq, plain):
    fx = plain
    ix, bases, offs, exp, need, want = fx["ix"], fx["bases"], fx["offs"], fx["exp"], fx["need"], fx["want"]
    n = offs.size - 1
    Lb = mq.load_library()
    c = ix.context()
    with pytest.raises(mq.MapquikError):
        c.chains()  # no reservation
    assert Lb.mq_ctx_reserve_chains(c._h, 0, 5) == MQ_EINVAL and Lb.mq_ctx_reserve_chains(c._h, 5, 0) == MQ_EINVAL
    assert Lb.mq_ctx_reserve_chains(c._h, 1 << 30, 5) == MQ_EINVAL and Lb.mq_ctx_reserve_chains(c._h, 5, (1 << 32) - 1) == MQ_EINVAL
    # a batch of max_reads + 1 reads is refused before anything is queued, and the context maps the next batch
    c.reserve_chains(n - 1, need)
    with pytest.raises(mq.MapquikError):
        c.map_batch(bases, offs)
    sub = offs[:n].copy()
    assert c.map_batch(bases[:int(sub[-1])], sub).tobytes() == want[:n - 1].tobytes()
    assert not _check(c.chains(), exp[:n - 1], need)
    # a FASTX piece with more records than spans is refused at the wait
    c.submit_fasta(np.frombuffer(_records(bases, offs, "fasta"), dtype=np.uint8))
    with pytest.raises(mq.MapquikError):
        c.wait_fasta()
    # a submitted batch: MQ_ESTATE
    c.submit(bases[:int(sub[-1])], sub)
    assert Lb.mq_ctx_reserve_chains(c._h, 5, 5) == MQ_ESTATE
    c.wait()
    # re-reserve larger, map; release: the product pair is back; reserve again: two batches in a row, the cursor restarts
    c.reserve_chains(n + 9, need + 100)
    assert c.map_batch(bases, offs).tobytes() == want.tobytes()
    assert not _check(c.chains(), exp, need + 100)
    c.reserve_chains(0, 0)
    assert c.map_batch(bases, offs).tobytes() == want.tobytes() and c.last_map_spec() == fx["spec0"] == 1
    with pytest.raises(mq.MapquikError):
        c.chains()
    c.reserve_chains(n, need)
    spans, chains, info = c.chains()
    assert spans.size == 0 and info == dict(stored=0, needed=0, dropped_reads=0)  # no batch yet
    for _ in range(2):
        _poison(c, n, need)
        assert c.map_batch(bases, offs).tobytes() == want.tobytes()
        assert not _check(c.chains(), exp, need)
    c.close()
    # the index's default context
    ix.reserve_chains(n, need)
    try:
        assert ix.map_batch(bases, offs).tobytes() == want.tobytes()
        assert not _check(ix.chains(), exp, need)
    finally:
        ix.reserve_chains(0, 0)
    assert ix.map_batch(bases, offs).tobytes() == want.tobytes()


def test_split_pipeline_refuses(mq, plain, monkeypatch):
    monkeypatch.setenv("MQ_PIPELINE", "split")
    g, off, names = plain["genome"]
    ix = mq.Index(mq.Params())
    for r in range(off.size - 1):
        ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])])
    ix.finalize()
    c = ix.context()
    assert mq.load_library().mq_ctx_reserve_chains(c._h, 10, 10) == MQ_EINVAL
    assert b"split" in mq.load_library().mq_last_error()
    c.close()
    ix.close()


@pytest.mark.parametrize("variant", [4, 16])
def test_seeding_variants(mq, O, plain, variant):
    g, off, names = plain["genome"]
    ix, ox, po = _index_both(mq, O, g, off, names, dict(), variant=variant)
    exp = CM.batch(O, ox, po, plain["bases"], plain["offs"])
    assert sum(len(e) >= 1 for e in exp) >= 40
    _run_host(mq, ix, exp, plain["bases"], plain["offs"])
    ix.close()


def test_anchors_and_chains_together(mq, O, plain):
    """both reservations on one context: both outputs equal their models, and the anchors are what the anchors pair alone gives"""
    fx = plain
    ix, bases, offs, n = fx["ix"], fx["bases"], fx["offs"], fx["offs"].size - 1
    aexp = A.batch(O, fx["ox"], fx["po"], bases, offs)
    aneed = sum(len(e.runs) for e in aexp if e)
    alone = ix.context()
    alone.reserve_anchors(n, aneed)
    assert alone.map_batch(bases, offs).tobytes() == fx["want"].tobytes()
    sp1, an1, info1 = alone.anchors()
    alone.close()
    c = _reserving(ix, n, fx["need"])
    c.reserve_anchors(n, aneed)
    hits = c.map_batch(bases, offs)
    assert hits.tobytes() == fx["want"].tobytes() and c.last_map_spec() == 0
    assert not _check(c.chains(), fx["exp"], fx["need"], hits)
    sp2, an2, info2 = c.anchors()
    assert info2 == info1 and sp2["count"].tobytes() == sp1["count"].tobytes()
    for r, e in enumerate(aexp):
        f1, f2, k = int(sp1["first"][r]), int(sp2["first"][r]), int(sp1["count"][r])
        assert k == (len(e.runs) if e else 0)
        assert an1[f1:f1 + k].tobytes() == an2[f2:f2 + k].tobytes(), r
        if e:
            assert [tuple(int(v) for v in a) for a in an2[f2:f2 + k].tolist()] == A.as32(e.runs), r
    # the anchors go, the chains stay
    c.reserve_anchors(0, 0)
    _poison(c, n, fx["need"])
    assert c.map_batch(bases, offs).tobytes() == fx["want"].tobytes()
    assert not _check(c.chains(), fx["exp"], fx["need"])
    c.close()


# ------------------------------------------------------------------ redo: more runs than MQ_MATCH_CAP
@pytest.fixture(scope="module")
def over(mq, oracle, simlib):
    """MQ_MATCH_CAP=64 (read when the index works out its launch geometry): the reads of `counts` with 65 chains and more overflow the window"""
    g, off, names, sets, _ = CM.batches(oracle, simlib)
    bases, offs = sets["counts"]
    mp = pytest.MonkeyPatch()
    mp.setenv("MQ_MATCH_CAP", str(CM.MATCH_CAP))
    try:
        ix, ox, po = _index_both(mq, oracle, g, off, names, dict())
        want = ix.map_batch(bases, offs)  # (the first map call: the geometry is fixed here)
    finally:
        mp.undo()
    exp = CM.batch(oracle, ox, po, bases, offs)
    diag = ox.map_batch_diag(bases, offs, po, threads=4)[1]
    n_over = int((diag["n_matches"] > CM.MATCH_CAP).sum())
    assert 3 <= n_over < offs.size - 1
    aexp = A.batch(oracle, ox, po, bases, offs)  # (the anchors of the same batch: test_both_reservations_through_*)
    yield dict(n_over=n_over, ix=ix, bases=bases, offs=offs, exp=exp, want=want, need=sum(len(e) for e in exp), lens=(offs[1:] - offs[:-1]).astype(np.int64),
               aexp=aexp, aneed=sum(len(e.runs) for e in aexp if e), over_mapped=[int(r) for r in np.flatnonzero(diag["n_matches"] > CM.MATCH_CAP) if aexp[r]])
    ix.close()


def test_host_driven_redo_delivers_chains(mq, over):
    fx = over
    _run_host(mq, fx["ix"], fx["exp"], fx["bases"], fx["offs"])


@pytest.mark.parametrize("arena_first", [False, True])
def test_in_stream_redo_delivers_chains(mq, over, arena_first):
    """the device form: without an arena an overflow read leaves with status 2 and span {0, 0}; with one its chains come from the arena's
    launch (whose unclaimed slots write nothing).  arena_first: the arena is reserved before the chains, so the chains reservation brings
    the arena's chain windows; else the arena's own reservation does"""
    fx = over
    ix, bases, offs, exp, need = fx["ix"], fx["bases"], fx["offs"], fx["exp"], fx["need"]
    n = offs.size - 1
    db, do, dout = hipmem.DevBuf.from_numpy(bases), hipmem.DevBuf.from_numpy(offs), hipmem.DevBuf(n * 48)
    c = ix.context()
    if arena_first:
        c.reserve_redo(n + 7, int(fx["lens"].max()))
    c.reserve_chains(n, need)
    _poison(c, n, need)
    if not arena_first:
        c.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dout.ptr)
        got = c.chains()
        hits = dout.to_numpy(mq.hit_dtype, n)
        overflow = hits["status"] == 2
        assert overflow.sum() == fx["n_over"]
        left = [[] if overflow[r] else e for r, e in enumerate(exp)]
        assert hits[~overflow].tobytes() == fx["want"][~overflow].tobytes()
        _check(got, left, need)
        c.reserve_redo(n + 7, int(fx["lens"].max()))
        _poison(c, n, need)
    c.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dout.ptr)
    got = c.chains()
    hits = dout.to_numpy(mq.hit_dtype, n)
    assert hits.tobytes() == fx["want"].tobytes()
    assert c.redo_counts() == (fx["n_over"], 0)
    assert not _check(got, exp, need, hits)
    c.close()
    for b in (db, do, dout):
        b.free()


def _both_reserving(c, fx):
    """the chains and the anchors reservation on c (which may have a redo arena already), spans and pools of both filled with 0xFF"""
    n = fx["offs"].size - 1
    assert fx["over_mapped"]  # a redone read with a winning chain: the redo's one id map places a span of either kind
    c.reserve_chains(n, fx["need"])
    c.reserve_anchors(n, fx["aneed"])
    _poison(c, n, fx["need"])
    sp, an = c.anchors_device()
    assert hipmem.hip().hipMemset(sp, 0xFF, 8 * n) == 0 and hipmem.hip().hipMemset(an, 0xFF, 20 * fx["aneed"]) == 0
    hipmem.device_sync()


def _check_anchors(got, aexp, aneed):
    """spans and anchors against the anchors model, read for read (test_anchors_and_chains_together's comparison)"""
    spans, anchors, info = got
    assert spans.size == len(aexp)
    assert not ((spans["first"] == DROPPED) & (spans["count"] == DROPPED)).any()  # every span was written
    assert info == dict(stored=aneed, needed=aneed, dropped_reads=0) and anchors.size == aneed
    for r, e in enumerate(aexp):
        f, k = int(spans["first"][r]), int(spans["count"][r])
        assert k == (len(e.runs) if e else 0), r
        if e:
            assert f + k <= aneed, r
            assert [tuple(int(v) for v in a) for a in anchors[f:f + k].tolist()] == A.as32(e.runs), r


def test_both_reservations_through_the_host_driven_redo(mq, over):
    """anchors and chains on one context, the overflow reads redone through the host: one list of read numbers places the redo's spans of
    both kinds"""
    fx = over
    c = fx["ix"].context()
    _both_reserving(c, fx)
    hits = c.map_batch(fx["bases"], fx["offs"])
    assert hits.tobytes() == fx["want"].tobytes()
    assert not _check(c.chains(), fx["exp"], fx["need"], hits)
    _check_anchors(c.anchors(), fx["aexp"], fx["aneed"])
    c.close()


@pytest.mark.parametrize("arena_first", [False, True])
def test_both_reservations_through_the_in_stream_redo(mq, over, arena_first):
    """... and redone in stream: the arena's slot-to-read array is the id map of both outputs.  arena_first as in
    test_in_stream_redo_delivers_chains"""
    fx = over
    bases, offs = fx["bases"], fx["offs"]
    n = offs.size - 1
    db, do, dout = hipmem.DevBuf.from_numpy(bases), hipmem.DevBuf.from_numpy(offs), hipmem.DevBuf(n * 48)
    c = fx["ix"].context()
    if arena_first:
        c.reserve_redo(n + 7, int(fx["lens"].max()))
    _both_reserving(c, fx)
    if not arena_first:
        c.reserve_redo(n + 7, int(fx["lens"].max()))
    c.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dout.ptr)
    got = c.chains()
    hits = dout.to_numpy(mq.hit_dtype, n)
    assert hits.tobytes() == fx["want"].tobytes()
    assert c.redo_counts() == (fx["n_over"], 0)
    assert not _check(got, fx["exp"], fx["need"], hits)
    _check_anchors(c.anchors(), fx["aexp"], fx["aneed"])
    c.close()
    for b in (db, do, dout):
        b.free()


def test_format_paf_chain(mq, plain):
    """the twelve columns for any chain; for the unique top chain the bytes of mq_format_paf on the hit"""
    fx = plain
    ix, bases, offs, n = fx["ix"], fx["bases"], fx["offs"], fx["offs"].size - 1
    c = _reserving(ix, n, fx["need"])
    hits = c.map_batch(bases, offs)
    spans, chains, info = c.chains()
    c.close()
    seen = 0
    for r in range(n):
        q_len = int(offs[r + 1] - offs[r])
        for ch in chains[int(spans["first"][r]):int(spans["first"][r]) + int(spans["count"][r])]:
            line = ix.format_paf_chain("r%d" % r, q_len, ch)
            name, r_len = ix.ref_info(int(ch["ref_id"]))[:2]
            qs, qe = (int(ch["q_start_hi"]) << 32) | int(ch["q_start"]), (int(ch["q_end_hi"]) << 32) | int(ch["q_end"])
            assert line == "r%d\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d" % (r, q_len, qs, qe, "-" if ch["rc"] else "+", name, r_len, ch["r_start"],
                                                                           ch["r_end"], ch["score"], r_len, ch["mapq"])
            if ch["flags"] & 1 and hits["status"][r] == 1:
                assert line == ix.format_paf("r%d" % r, q_len, hits[r])
                seen += 1
    assert seen >= 40


# ------------------------------------------------------------------ the two drivers
def _chains_text(rn, names, offs, exp):
    out = []
    for i, chs in enumerate(exp):
        tops = CM.n_top(chs)
        q_len = int(offs[i + 1] - offs[i])
        for c in chs:
            f, ref, rc, mapq, qs, qe, rs, re_, score, n = c
            top = bool(f & CM.TOP)
            out.append("%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\ttp:A:%s\tcn:i:%d%s\n"
                       % (rn[i], q_len, qs, qe, "-" if rc else "+", names[ref][0], names[ref][1], rs, re_, score, names[ref][1], mapq,
                          "P" if top and tops == 1 else "S", n, "\ttie:i:1" if top and tops > 1 else ""))
    return "".join(out)


def test_both_drivers_write_the_chains_file(mq, O, mos, tmp_path, capsys):
    """`--chains` of `python -m mapquik_amd` and of the native `mapquik`, alone and with `--anchors`, on the mosaic contigs with the tie
    reads, the tie below a winner and the chain-count reads: <prefix>.chains is the text formatted from the model (tp:A:P / tp:A:S, cn:i,
    tie:i:1); the .paf is byte-identical with and without the flag"""
    import subprocess

    from mapquik_amd import build, cli
    g, off, names = mos["genome"]
    seqs = []
    for nm in ("ties", "below", "counts"):
        b, o = mos["sets"][nm]
        seqs += [b[int(o[i]):int(o[i + 1])] for i in range(0, o.size - 1, 2 if nm == "ties" else 1)]
    bases, offs = M.concat(seqs)
    rn = ["q%d" % i for i in range(len(seqs))]
    exp = CM.batch(O, mos["ox"], mos["po"], bases, offs)
    assert any(CM.n_top(c) >= 2 for c in exp) and any(CM.n_top(c) == 1 and len(c) >= 3 for c in exp)
    ref_of = {r: (names[r], int(off[r + 1] - off[r])) for r in range(off.size - 1)}
    want = _chains_text(rn, ref_of, offs, exp)
    ref_fa, reads_fa = tmp_path / "ref.fa", tmp_path / "reads.fa"
    ref_fa.write_bytes(b"".join(b">" + names[r].encode() + b"\n" + g[int(off[r]):int(off[r + 1])].tobytes() + b"\n" for r in range(off.size - 1)))
    reads_fa.write_bytes(b"".join(b">" + rn[i].encode() + b"\n" + bases[int(offs[i]):int(offs[i + 1])].tobytes() + b"\n" for i in range(len(rn))))
    exe = build.build_cli()
    for tag, flag in (("0", []), ("1", ["--chains"]), ("2", ["--chains", "--anchors"])):
        r = subprocess.run([exe, str(reads_fa), "--reference", str(ref_fa), "-p", str(tmp_path / ("n" + tag)), "--batch-bases", "300000"] + flag,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert cli.main([str(reads_fa), "--reference", str(ref_fa), "-p", str(tmp_path / ("p" + tag)), "--batch-bases", "300000"] + flag) == 0
    capsys.readouterr()
    for pre in ("n1", "n2", "p1", "p2"):
        assert (tmp_path / (pre + ".chains")).read_text() == want, pre
    assert not (tmp_path / "n0.chains").exists() and not (tmp_path / "p0.chains").exists()
    assert (tmp_path / "n2.anchors").read_bytes() == (tmp_path / "p2.anchors").read_bytes() and (tmp_path / "n2.anchors").stat().st_size > 0
    paf = (tmp_path / "n0.paf").read_bytes()
    assert paf.count(b"\n") == sum(CM.n_top(c) == 1 for c in exp)
    for other in ("n1", "n2", "p0", "p1", "p2"):
        assert (tmp_path / (other + ".paf")).read_bytes() == paf, other
