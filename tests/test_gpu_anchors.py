"""GPU: the anchor output (mq_ctx_reserve_anchors, include/mapquik_hip.h) -- the Match runs of every mapped read's winning chain.  Every
case compares spans and anchors with the model (tests/anchors_model.py; test_anchors_model.py ties it to the pinned PAF columns) read
for read, and the hits byte for byte with a context WITHOUT a reservation on the same index.  The span array is filled with 0xFF on the
device before the call, and every span of the batch must have been written."""
import ctypes as C

import hipmem
import numpy as np
import pytest

import anchors_model as A
import lattice as L
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


def _poison(c, max_reads):
    """the context's device span array filled with 0xFF"""
    sp, _ = c.anchors_device()
    assert hipmem.hip().hipMemset(sp, 0xFF, 8 * int(max_reads)) == 0
    hipmem.device_sync()


def _reserving(ix, max_reads, max_anchors):
    c = ix.context()
    c.reserve_anchors(max_reads, max_anchors)
    _poison(c, max_reads)
    return c


def _check(got, exp, cap):
    """spans, anchors and counters of one batch against the model's lists; returns the number of dropped reads"""
    spans, anchors, info = got
    assert spans.size == len(exp)
    assert not ((spans["first"] == DROPPED) & (spans["count"] == DROPPED)).any()  # every span was written
    need = sum(len(e.runs) for e in exp if e)
    assert info["needed"] == need and info["stored"] == min(need, cap) == anchors.size
    used, dropped = [], 0
    for r, e in enumerate(exp):
        f, c = int(spans["first"][r]), int(spans["count"][r])
        if e is None:
            assert (f, c) == (0, 0), r
            continue
        assert c == len(e.runs), r
        if f == DROPPED:
            dropped += 1
            continue
        assert f + c <= info["stored"], r
        assert [tuple(int(v) for v in a) for a in anchors[f:f + c].tolist()] == A.as32(e.runs), r
        used.append((f, f + c))
    used.sort()
    assert all(a[1] <= b[0] for a, b in zip(used, used[1:]))  # stored lists are pairwise disjoint
    assert info["dropped_reads"] == dropped
    if need <= cap:
        assert dropped == 0
    return dropped


def _check_hits(mq, hits, exp):
    for r, e in enumerate(exp):
        assert (int(hits["status"][r]) == 1) == (e is not None), r
        if e:
            assert int(hits["ref_id"][r]) == e.ref and bool(hits["rc"][r]) == e.rc and int(hits["score"][r]) == sum(x[4] for x in e.runs), r


def _run_host(mq, ix, exp, bases, offs, cap=None):
    """map_batch on a reserving context and on a plain one: hits equal byte for byte, anchors as the model says"""
    n = offs.size - 1
    need = sum(len(e.runs) for e in exp if e)
    cap = max(need, 1) if cap is None else cap
    plain = ix.context()
    want = plain.map_batch(bases, offs)
    plain.close()
    c = _reserving(ix, n, cap)
    hits = c.map_batch(bases, offs)
    assert hits.tobytes() == want.tobytes()
    _check_hits(mq, hits, exp)
    got = c.anchors()
    dropped = _check(got, exp, cap)
    c.close()
    return got, dropped


# ------------------------------------------------------------------ run counts on the chain stage's sizes
@pytest.fixture(scope="module")
def lat(mq, oracle, simlib):
    g, off, names = L.world(simlib)
    ix, ox, po = _index_both(mq, oracle, g, off, names, dict())
    yield dict(g=g, ix=ix, ox=ox, po=po)
    ix.close()


def _run_count_reads(O, lat):
    """reads with exactly 1, 2, 47 / 48 / 49 (MAP_LDS_RECS), 63 / 64 / 65 (CH) Match runs on one reference, forward and reverse-complemented"""
    g, ox, po = lat["g"], lat["ox"], lat["po"]
    km1 = O.kminmers(g, O.params(k=1))
    pts = []
    for strand, f in (("fwd", lambda s: s), ("rc", L.revcomp)):
        for t in range(L.E_RETRIES + 1):
            try:
                read = L.read_with_minimizers(O, g, dict(), L.LANE_BATCH * 18 + po.k, first=60 + 100 * t, km1=km1)[0]
                made = L.reads_with_match_runs(O, ox, f(read), po)
                break
            except L.LatticeError:
                if t == L.E_RETRIES:
                    raise
        pts += [("%s %d" % (strand, m), s, m) for m, s in made.items()]
    return pts


def test_run_counts_on_the_chain_stage_sizes(mq, O, lat):
    pts = _run_count_reads(O, lat)
    bases, offs = L.batch(pts)
    exp = A.batch(O, lat["ox"], lat["po"], bases, offs)
    # the CPU side: the run counts are what the names say, and -- substitutions break runs but move nothing -- every run stays: the kept
    # list of the one reference has 1, 2, 47 .. 49 and 63 .. 65 entries (64 | 65: pass C's rank across a chunk border)
    assert sorted(m for _, _, m in pts) == sorted(L.E_RUNS * 2)
    for (name, s, m), e in zip(pts, exp):
        assert L.n_matches(lat["ox"], s, lat["po"]) == m, name
        assert e is not None and len(e.runs) == m, name
    assert {len(e.runs) for e in exp} >= {1, 64, 65}
    assert sum(e.rc for e in exp) == len(exp) // 2  # reverse-strand chains of up to 65 runs
    _run_host(mq, lat["ix"], exp, bases, offs)


# ------------------------------------------------------------------ chain contents on the mosaic world
@pytest.fixture(scope="module")
def mos(mq, oracle, simlib):
    g, off, names, sets = M.world(oracle, simlib)
    ix, ox, po = _index_both(mq, oracle, g, off, names, dict())
    yield dict(ix=ix, ox=ox, sets=sets)
    ix.close()


def _subset(st, step):
    n = st["offs"].size - 1
    return M.select(st["bases"], st["offs"], list(range(0, n, step)))


@pytest.mark.parametrize("name,step", [("default", 6), ("mixed", 5), ("gap_2000", 3), ("gap_0", 5), ("gap_50", 5), ("late", 1)])
def test_chain_contents(mq, O, mos, name, step):
    """default / mixed: up to hundreds of runs over dozens of references, kept lists that are strict subsets with dropped runs between kept
    ones, both strands; gap_<g>: runs dropped at a gap difference beyond g and kept at g; late: the winner's only run in a later chunk"""
    st = mos["sets"][name]
    ix = mos["ix"]
    g = st["ps"].get("g", 2000)
    ix.set_map_params(4, 11, g)
    try:
        po = O.params(g=g)
        bases, offs = _subset(st, step)
        exp = A.batch(O, mos["ox"], po, bases, offs)
        diag = mos["ox"].map_batch_diag(bases, offs, po, threads=4)[1]
        mapped = [e for e in exp if e]
        assert len(mapped) >= 10
        if name in ("default", "mixed"):
            assert (diag["n_matches"] > 64).any() and any(e.rc and len(e.runs) > 1 for e in mapped) and any(not e.rc and len(e.runs) > 1 for e in mapped)
            assert (diag["filtered_out"] > 0).any()
        if name.startswith("gap_"):
            lens = {len(e.runs) for e in mapped}
            assert len(lens) >= 2  # some jumps keep every segment's run, others drop one
        _run_host(mq, ix, exp, bases, offs)
    finally:
        ix.set_map_params(4, 11, 2000)


@pytest.mark.parametrize("n", [2, 17, 65])
def test_ties_claim_nothing(mq, O, mos, n):
    """n-way ties next to near-ties: a tie has span {0, 0}, and `needed` is the sum of the mapped reads' counts alone (_check)"""
    sets = mos["sets"]
    seqs = []
    for nm in ("tie_%d" % n, "near_%d" % n):
        st = sets[nm]
        seqs += [st["bases"][int(st["offs"][i]):int(st["offs"][i + 1])] for i in range(st["offs"].size - 1)]
    bases, offs = M.concat(seqs)
    po = O.params()
    exp = A.batch(O, mos["ox"], po, bases, offs)
    assert sum(e is None for e in exp) >= 3 and sum(e is not None for e in exp) >= 3
    _run_host(mq, mos["ix"], exp, bases, offs)


def test_more_runs_than_the_match_window_and_the_precedence_quirk(mq, O, simlib):
    """the k = 1 leg at the default MQ_MATCH_CAP: mosaic reads with more than 2048 Match runs deliver their anchors from the redo -- through the
    host, and in stream from the arena on a device-form call; beside them reads in which a forward run was extended onto another
    reference by the Match::check precedence quirk"""
    g, off, names, sets = M.world(O, simlib)
    st = sets["k1"]
    ix, ox, po = _index_both(mq, O, g, off, names, st["ps"])
    out, diag = ox.map_batch_diag(st["bases"], st["offs"], po, threads=4)
    n_all = st["offs"].size - 1
    big = [i for i in range(n_all) if diag["n_matches"][i] > 2048 and out["mapped"][i]][:2]
    quirk = [i for i in range(n_all) if diag["quirk_cross_ref"][i] > 0 and out["mapped"][i] and diag["n_matches"][i] <= 2048][:3]
    assert len(big) == 2 and len(quirk) == 3
    bases, offs = M.select(st["bases"], st["offs"], big + quirk)
    n = offs.size - 1
    exp = A.batch(O, ox, po, bases, offs)
    assert all(e is not None for e in exp) and exp == A.batch(O, ox, po, bases, offs, word=A.by_oracle)
    (spans, anchors, info), _ = _run_host(mq, ix, exp, bases, offs)
    need = info["needed"]
    db, do, dout = hipmem.DevBuf.from_numpy(bases), hipmem.DevBuf.from_numpy(offs), hipmem.DevBuf(n * 48)
    plain = ix.context()
    want = plain.map_batch(bases, offs)
    plain.close()
    c = _reserving(ix, n, need)
    c.reserve_redo(n, int((offs[1:] - offs[:-1]).max()))
    c.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dout.ptr)
    got = c.anchors()
    assert dout.to_numpy(mq.hit_dtype, n).tobytes() == want.tobytes()
    assert c.redo_counts() == (2, 0)
    assert _check(got, exp, need) == 0
    c.close()
    for b in (db, do, dout):
        b.free()
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
    exp = A.batch(oracle, ox, po, bases, offs)
    assert sum(e is not None for e in exp) >= 40 and any(e and len(e.runs) >= 3 for e in exp)
    c0 = ix.context()
    want = c0.map_batch(bases, offs)
    spec0 = c0.last_map_spec()
    c0.close()
    yield dict(ix=ix, ox=ox, po=po, bases=bases, offs=offs, exp=exp, want=want, need=sum(len(e.runs) for e in exp if e), spec0=spec0,
               genome=(g, off, names))
    ix.close()


def _records(bases, offs, fmt):
    seqs = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(offs.size - 1)]
    if fmt == "fasta":
        return b"".join(b">r%d\n" % i + s + b"\n" for i, s in enumerate(seqs))
    if fmt == "fastq":
        return b"".join(b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))
    return b"".join(b">r%d\n" % i + b"".join(s[j:j + 70] + b"\n" for j in range(0, len(s), 70)) for i, s in enumerate(seqs))


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("form", ["host", "submit", "spans", "device", "fasta", "fastq", "lines"])
def test_every_launch_form(mq, plain, form, pool, monkeypatch):
    """pool: MQ_LIST_F16=64 (read at every launch) -- every list outgrows its region and is written again into the pool behind the regions"""
    if pool:
        monkeypatch.setenv("MQ_LIST_F16", "64")
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
        got = c.anchors()  # waits for the call's stream itself
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
        got = c.anchors()
    assert _check(got, fx["exp"], fx["need"]) == 0
    assert c.last_map_spec() == 0 and fx["spec0"] == 1  # the product path is untouched: the pair of the defaults without a reservation
    c.close()


def test_list_overflows_its_region(mq, plain, monkeypatch):
    """MQ_LIST_F16=64: every list outgrows its region and is written again into the pool behind the regions; anchors as before"""
    monkeypatch.setenv("MQ_LIST_F16", "64")
    fx = plain
    _run_host(mq, fx["ix"], fx["exp"], fx["bases"], fx["offs"])


def test_pool_edges(mq, plain):
    fx = plain
    exp, need = fx["exp"], fx["need"]
    _, d = _run_host(mq, fx["ix"], exp, fx["bases"], fx["offs"], cap=need)
    assert d == 0
    (spans, anchors, info), d = _run_host(mq, fx["ix"], exp, fx["bases"], fx["offs"], cap=need - 1)
    assert d >= 1 and info["needed"] == need and info["dropped_reads"] == d
    (spans, anchors, info), d = _run_host(mq, fx["ix"], exp, fx["bases"], fx["offs"], cap=1)
    single = sum(1 for e in exp if e and len(e.runs) == 1)
    assert d >= sum(e is not None for e in exp) - min(single, 1) and info["stored"] == 1 and info["needed"] == need


def test_batches_and_reservation_lifecycle(mq, plain):
    fx = plain
    ix, bases, offs, exp, need, want = fx["ix"], fx["bases"], fx["offs"], fx["exp"], fx["need"], fx["want"]
    n = offs.size - 1
    Lb = mq.load_library()
    c = ix.context()
    with pytest.raises(mq.MapquikError):
        c.anchors()  # no reservation
    assert Lb.mq_ctx_reserve_anchors(c._h, 0, 5) == MQ_EINVAL and Lb.mq_ctx_reserve_anchors(c._h, 5, 0) == MQ_EINVAL
    assert Lb.mq_ctx_reserve_anchors(c._h, 1 << 30, 5) == MQ_EINVAL and Lb.mq_ctx_reserve_anchors(c._h, 5, (1 << 32) - 1) == MQ_EINVAL
    # a batch of max_reads + 1 reads is refused, and the context maps the next batch
    c.reserve_anchors(n - 1, need)
    with pytest.raises(mq.MapquikError):
        c.map_batch(bases, offs)
    sub = offs[:n].copy()
    assert c.map_batch(bases[:int(sub[-1])], sub).tobytes() == want[:n - 1].tobytes()
    assert _check(c.anchors(), exp[:n - 1], need) == 0
    # a submitted batch: MQ_ESTATE
    c.submit(bases[:int(sub[-1])], sub)
    assert Lb.mq_ctx_reserve_anchors(c._h, 5, 5) == MQ_ESTATE
    c.wait()
    # release: the product pair is back; reserve again: two batches in a row, the cursor restarts
    c.reserve_anchors(0, 0)
    assert c.map_batch(bases, offs).tobytes() == want.tobytes() and c.last_map_spec() == fx["spec0"] == 1
    with pytest.raises(mq.MapquikError):
        c.anchors()
    c.reserve_anchors(n, need)
    spans, anchors, info = c.anchors()
    assert spans.size == 0 and info == dict(stored=0, needed=0, dropped_reads=0)  # no batch yet
    for _ in range(2):
        _poison(c, n)
        assert c.map_batch(bases, offs).tobytes() == want.tobytes()
        assert _check(c.anchors(), exp, need) == 0
    c.close()
    # the index's default context
    ix.reserve_anchors(n, need)
    try:
        assert ix.map_batch(bases, offs).tobytes() == want.tobytes()
        assert _check(ix.anchors(), exp, need) == 0
    finally:
        ix.reserve_anchors(0, 0)
    assert ix.map_batch(bases, offs).tobytes() == want.tobytes()


def test_split_pipeline_refuses(mq, plain, monkeypatch):
    monkeypatch.setenv("MQ_PIPELINE", "split")
    g, off, names = plain["genome"]
    ix = mq.Index(mq.Params())
    for r in range(off.size - 1):
        ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])])
    ix.finalize()
    c = ix.context()
    assert mq.load_library().mq_ctx_reserve_anchors(c._h, 10, 10) == MQ_EINVAL
    assert b"split" in mq.load_library().mq_last_error()
    c.close()
    ix.close()


def test_chain_chunk_4(mq, O, plain, monkeypatch):
    """MQ_CHAIN_CHUNK=4 (read at mq_index_new): the plain batch through the multi-chunk path of all three passes"""
    monkeypatch.setenv("MQ_CHAIN_CHUNK", "4")
    g, off, names = plain["genome"]
    ix, ox, po = _index_both(mq, O, g, off, names, dict())
    assert any(e and len(e.runs) > 4 for e in plain["exp"])
    _run_host(mq, ix, plain["exp"], plain["bases"], plain["offs"])
    ix.close()


@pytest.mark.parametrize("variant", [4, 16])
def test_seeding_variants(mq, O, plain, variant):
    """the VAR pairs (variant 16: q_end from the second position list), against the oracle switched alike"""
    g, off, names = plain["genome"]
    ix, ox, po = _index_both(mq, O, g, off, names, dict(), variant=variant)
    exp = A.batch(O, ox, po, plain["bases"], plain["offs"])
    assert sum(e is not None for e in exp) >= 40
    _run_host(mq, ix, exp, plain["bases"], plain["offs"])
    ix.close()


# ------------------------------------------------------------------ redo: more runs than MQ_MATCH_CAP
@pytest.fixture(scope="module")
def over(mq, oracle, simlib):
    """MQ_MATCH_CAP=8 (read when the index works out its launch geometry): of 40 noisy reads several have more Match runs than the window"""
    mp = pytest.MonkeyPatch()
    mp.setenv("MQ_MATCH_CAP", "8")
    try:
        g, off, names = simlib.make_genome([200000], seed=5, repeat_frac=0.3)
        reads = simlib.make_reads(g, off, 40, seed=2, len_mean=9000, err=0.03)
        bases, offs = reads["bases"], reads["offsets"]
        ix, ox, po = _index_both(mq, oracle, g, off, names, dict(k=3, l=15, density=0.03))
        want = ix.map_batch(bases, offs)  # (the first map call: the geometry is fixed here)
    finally:
        mp.undo()
    exp = A.batch(oracle, ox, po, bases, offs)
    diag = ox.map_batch_diag(bases, offs, po, threads=4)[1]
    # (a read whose records all fit the LDS window -- MAP_LDS_RECS -- never looks at the scratch window: those above it overflow)
    n_over = int((diag["n_matches"] > L.MAP_LDS_RECS).sum())
    assert 3 <= n_over < 40
    yield dict(n_over=n_over, ix=ix, bases=bases, offs=offs, exp=exp, want=want, need=sum(len(e.runs) for e in exp if e), lens=(offs[1:] - offs[:-1]).astype(np.int64))
    ix.close()


def test_host_driven_redo_delivers_anchors(mq, over):
    fx = over
    _run_host(mq, fx["ix"], fx["exp"], fx["bases"], fx["offs"])


def test_in_stream_redo_delivers_anchors(mq, over):
    """the device form: without an arena an overflow read leaves with status 2 and span {0, 0}; with one its anchors come from the arena's
    launch (whose unclaimed slots write nothing: every other span stays what the main launch wrote)"""
    fx = over
    ix, bases, offs, exp, need = fx["ix"], fx["bases"], fx["offs"], fx["exp"], fx["need"]
    n = offs.size - 1
    db, do, dout = hipmem.DevBuf.from_numpy(bases), hipmem.DevBuf.from_numpy(offs), hipmem.DevBuf(n * 48)
    c = _reserving(ix, n, need)
    c.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dout.ptr)
    got = c.anchors()
    hits = dout.to_numpy(mq.hit_dtype, n)
    overflow = hits["status"] == 2
    assert overflow.sum() == fx["n_over"]
    left = [None if overflow[r] else e for r, e in enumerate(exp)]
    assert hits[~overflow].tobytes() == fx["want"][~overflow].tobytes()
    spans, anchors, info = got
    _check(got, left, need)
    # an arena with more slots than overflow reads
    c.reserve_redo(n + 7, int(fx["lens"].max()))
    _poison(c, n)
    c.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dout.ptr)
    got = c.anchors()
    hits = dout.to_numpy(mq.hit_dtype, n)
    assert hits.tobytes() == fx["want"].tobytes()
    assert c.redo_counts() == (int(overflow.sum()), 0)
    assert _check(got, exp, need) == 0
    c.close()
    for b in (db, do, dout):
        b.free()


# ------------------------------------------------------------------ the two drivers
def test_both_drivers_write_the_anchors_file(mq, O, simlib, tmp_path, capsys):
    """`--anchors` of `python -m mapquik_amd` and of the native `mapquik` on an e. coli-sized synthetic: <prefix>.anchors is the text
    formatted from the model, reads in input order and runs in read order; the .paf is byte-identical with and without the flag"""
    import subprocess

    from mapquik_amd import build, cli
    g, off, names = simlib.make_genome(simlib.ECOLI_LEN, seed=913)
    reads = simlib.make_reads(g, off, 150, seed=4, len_mean=9000, err=0.02)
    bases, offs = reads["bases"], reads["offsets"]
    rn = simlib.read_names(reads, names)
    po, ox = O.params(), O.Index()
    for r in range(off.size - 1):
        ox.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])], po)
    exp = A.batch(O, ox, po, bases, offs)
    assert sum(e is not None for e in exp) >= 100 and any(e and len(e.runs) >= 3 for e in exp)
    want = "".join("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d\n" % (rn[i], q0, q1, "-" if e.rc else "+", names[e.ref], r0, r1, c)
                   for i, e in enumerate(exp) if e for q0, q1, r0, r1, c in A.as32(e.runs))
    ref_fa, reads_fa = tmp_path / "ref.fa", tmp_path / "reads.fa"
    ref_fa.write_bytes(b"".join(b">" + names[r].encode() + b"\n" + g[int(off[r]):int(off[r + 1])].tobytes() + b"\n" for r in range(off.size - 1)))
    reads_fa.write_bytes(b"".join(b">" + rn[i].encode() + b"\n" + bases[int(offs[i]):int(offs[i + 1])].tobytes() + b"\n" for i in range(len(rn))))
    exe = build.build_cli()
    for tag, flag in (("n0", []), ("n1", ["--anchors"])):
        r = subprocess.run([exe, str(reads_fa), "--reference", str(ref_fa), "-p", str(tmp_path / tag), "--batch-bases", "300000"] + flag,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert cli.main([str(reads_fa), "--reference", str(ref_fa), "-p", str(tmp_path / ("p" + tag[1])), "--batch-bases", "300000"] + flag) == 0
    capsys.readouterr()
    assert (tmp_path / "n1.anchors").read_text() == want and (tmp_path / "p1.anchors").read_text() == want
    assert not (tmp_path / "n0.anchors").exists() and not (tmp_path / "p0.anchors").exists()
    paf = (tmp_path / "n0.paf").read_bytes()
    assert paf.count(b"\n") == sum(e is not None for e in exp)
    for other in ("n1", "p0", "p1"):
        assert (tmp_path / (other + ".paf")).read_bytes() == paf, other
