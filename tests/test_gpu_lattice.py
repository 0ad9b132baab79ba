"""GPU: the boundary lattice of tests/lattice.py -- reads, runs, minimizer counts and Match-run breaks that sit ON the kernels' compile-time
sizes and one element to either side (test_lattice_cases.py proves on the CPU that they do) -- through the HIP path, every comparison
exact: the k-min-mer tuples hash, start, end, offset, rev of Index.kminmers_batch against oracle.kminmers; status, the eight numeric
columns and n_kminmers of every record against oracle.Index.map_batch_diag.  Every family asserts last_map_path_counts(), so that the
reads demonstrably went through the seeder the family is about, and the number of mapped reads comes from the oracle's output: a launch
that answered "unmapped" everywhere cannot pass.

Path counts: a read below l + k - 1 bases is seeded by nobody (src/mers.rs:44); one below 16 bases -- the fast seeder's first 16-byte piece,
seed_fast_eligible -- is the general seeder's by design.  `_expect_paths` states that rule; everything else ACGT-only must be fast."""
import numpy as np
import pytest

import lattice as L

pytestmark = pytest.mark.gpu

FIELDS = ("hash", "start", "end", "offset", "rev")
COLUMNS = ("ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score")


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture(scope="module")
def world(simlib):
    return L.world(simlib)


def _index(mq, oracle, world, ps, variant=0):
    """(HIP index, oracle index, oracle params) of the genome; the environment (MQ_FORCE_GENERAL) is read when the HIP index is made"""
    g, off, names = world
    P, po = mq.Params(seeding_variant=variant, **ps), oracle.params(**ps)
    ix, ox = mq.Index(P), oracle.Index()
    assert ix.add_ref(0, names[0], g) == ox.add_ref(0, names[0], g, po)
    assert ix.finalize() == ox.count()
    return ix, ox, po


def _expect_paths(pts, po, forced=False):
    """(fast, general) the launch must report for these reads"""
    seeded = [p[1] for p in pts if len(p[1]) >= po.l + po.k - 1]
    general = sum(1 for s in seeded if forced or len(s) < 16 or any(c not in b"ACGT" for c in set(s)))
    return len(seeded) - general, general


def _tuples(oracle, ix, po, pts, paths, what):
    bases, offs = L.batch(pts)
    got = ix.kminmers_batch(bases, offs)
    assert ix.last_map_path_counts() == paths, (what, ix.last_map_path_counts(), paths)
    total = 0
    for i, p in enumerate(pts):
        w = L.kminmers_or_none(oracle, p[1], po)
        assert len(got[i]) == len(w), (what, p[0], len(got[i]), len(w))
        for f in FIELDS:
            assert np.array_equal(got[i][f].astype(np.uint64), w[f].astype(np.uint64)), (what, p[0], f)
        total += len(w)
    return got, total


def _same(mq, got, want, diag, what):
    """status, every numeric PAF column and the k-min-mer count of every read against the oracle's (as test_gpu_poison._same)"""
    bad = np.flatnonzero(got["status"] > 2)
    assert bad.size == 0, "%s: %d records never written, first %s" % (what, bad.size, bad[:10].tolist())
    assert np.array_equal(got["n_kminmers"].astype(np.uint64), diag["n_kminmers"].astype(np.uint64)), what
    m = want["mapped"] != 0
    assert np.array_equal(got["status"] == 1, m), what
    for f in COLUMNS:
        assert np.array_equal(mq.hit_column(got, f)[m], want[f][m].astype(np.uint64)), (what, f)


def _hits(mq, ix, ox, po, pts, paths, what, device=True):
    """the host form and (device=True) the device form on a 0xFF-filled result buffer of exactly the batch's bytes; returns the oracle's answer"""
    from test_gpu_poison import _launch_poisoned
    bases, offs = L.batch(pts)
    want, diag = ox.map_batch_diag(bases, offs, po, threads=8)
    hits = ix.map_batch(bases, offs)
    assert ix.last_map_path_counts() == paths, (what, ix.last_map_path_counts(), paths)
    _same(mq, hits, want, diag, what)
    if device:
        dh = _launch_poisoned(mq, ix, bases, offs)
        _same(mq, dh, want, diag, (what, "device form"))
        assert dh.tobytes() == hits.tobytes(), what
        assert ix.last_map_path_counts() == paths
    short = np.array([len(p[1]) < po.l + po.k - 1 for p in pts])
    assert (hits["status"][short] == 0).all() and (hits["n_kminmers"][short] == 0).all(), what
    return want, diag, hits


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("l", L.A_LS + ("dense",))
def test_family_a_raw_lengths(mq, oracle, world, l):
    ps = L.A_DENSE if l == "dense" else L.a_params(l)
    ix, ox, po = _index(mq, oracle, world, ps)
    pts = L.raw_length_points(world[0], po.l)
    paths = _expect_paths(pts, po)
    assert paths[1] == sum(1 for _, s in pts if po.l + po.k - 1 <= len(s) < 16)
    _, n_kmm = _tuples(oracle, ix, po, pts, paths, ("A", ps))
    want, diag, _ = _hits(mq, ix, ox, po, pts, paths, ("A", ps))
    assert n_kmm == int(diag["n_kminmers"].sum()) and n_kmm > len(pts)
    if po.l >= 12:   # error-free reads of a random genome map (at l = 2 and l = 4 the k-min-mers repeat all over the genome: none is unique)
        assert (want["mapped"] != 0).sum() >= sum(1 for _, s in pts if len(s) >= L.SD_SR_RAW - 65)
    ix.close()


# ------------------------------------------------------------------ B
@pytest.mark.parametrize("leg", range(len(L.B_PARAMS) + len(L.B_VARIANTS)))
def test_family_b_runs_on_the_borders(mq, oracle, world, leg):
    ps = L.B_PARAMS[leg] if leg < len(L.B_PARAMS) else dict()
    variant = 0 if leg < len(L.B_PARAMS) else L.B_VARIANTS[leg - len(L.B_PARAMS)]
    oracle.lib().mqo_set_variant(variant)
    try:
        ix, ox, po = _index(mq, oracle, world, ps, variant)
        pts = L.run_border_points(world[0], po.l)
        paths = _expect_paths(pts, po)
        assert paths == (len(pts), 0)
        _, n_kmm = _tuples(oracle, ix, po, pts, paths, ("B", ps, variant))
        want, diag, _ = _hits(mq, ix, ox, po, pts, paths, ("B", ps, variant))
        assert n_kmm == int(diag["n_kminmers"].sum()) and n_kmm > len(pts)
        # the random part of every read with a planted run is several kilobases of the genome: it maps
        planted = np.array([p[2] is not None for p in pts])
        assert planted.sum() > 400 and (want["mapped"][planted] != 0).all()
        ix.close()
    finally:
        oracle.lib().mqo_set_variant(0)


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("ps", L.C_PARAMS, ids=["default", "k3l12"])
def test_family_c_where_a_read_sits(mq, oracle, world, ps):
    from hipmem import DevBuf, device_sync, memset
    g = world[0]
    ix, ox, po = _index(mq, oracle, world, ps)
    reads = L.placement_reads(g)
    alone_hits, alone_tuples = [], []
    for name, s in reads:   # alone in a batch: the expected record
        one = [(name, s)]
        paths = _expect_paths(one, po)
        got, _ = _tuples(oracle, ix, po, one, paths, ("C alone", name))
        _, _, hits = _hits(mq, ix, ox, po, one, paths, ("C alone", name))
        alone_hits.append(hits[0].tobytes())
        alone_tuples.append(got[0].tobytes())
    assert sum(1 for h in alone_hits if np.frombuffer(h, dtype=mq.hit_dtype)["status"][0] == 1) >= 3

    def placed(pts, where, what):
        paths = _expect_paths(pts, po)
        # (the counts below allow the general seeder the reads the rule gives it -- an N of their own, fewer than 16 bases -- and no other:
        # nobody is declined because of a neighbour)
        assert not any(_expect_paths([pts[i]], po)[1] for i in where)
        got, _ = _tuples(oracle, ix, po, pts, paths, what)
        _, _, hits = _hits(mq, ix, ox, po, pts, paths, what)
        for i, (w, _) in where.items():
            assert hits[i].tobytes() == alone_hits[w] and got[i].tobytes() == alone_tuples[w], (what, i, reads[w][0])
    placed(*L.placement_offsets_batch(g, reads), "C (i) every offset mod 64")
    placed(*L.placement_neighbour_batch(g, reads), "C (ii) runs across the read border")
    placed(*L.placement_n_batch(g, reads), "C (iii) N behind")
    # (iv) the read is the last of the batch, the device buffer holds exactly the batch's bytes
    for w, (name, s) in enumerate(reads):
        pts = [("front", L.placement_reads(g, seed=20 + w)[1][1]), (name, s)]
        bases, offs = L.batch(pts)
        db, do, out = DevBuf.from_numpy(bases), DevBuf.from_numpy(offs), DevBuf(2 * mq.hit_dtype.itemsize)
        assert db.nbytes == int(offs[-1])
        memset(out, 0xFF)
        ix.reserve(2, int(offs[-1]))
        ix.map_batch_device(db.ptr, do.ptr, 2, int(offs[-1]), out.ptr)
        device_sync()
        hits = out.to_numpy(mq.hit_dtype, 2)
        assert ix.last_map_path_counts() == _expect_paths(pts, po)
        assert (hits["status"] <= 2).all() and hits[1].tobytes() == alone_hits[w], ("C (iv)", name)
        for b in (db, do, out):
            b.free()
    # (v) a raw FASTQ buffer through Context.submit_spans: the byte in front of every read is a newline
    buf, starts, lens = L.fastq_buffer(reads)
    ctx = ix.context()
    ctx.submit_spans(buf, starts, lens)
    hits = ctx.wait()
    ctx.close()
    for w in range(len(reads)):
        assert hits[w].tobytes() == alone_hits[w], ("C (v)", reads[w][0])
    ix.close()


# ------------------------------------------------------------------ D
@pytest.mark.parametrize("leg", range(len(L.D_PARAMS)))
def test_family_d_minimizer_counts(mq, oracle, world, leg):
    ps = L.D_PARAMS[leg]
    ix, ox, po = _index(mq, oracle, world, ps)
    pts = L.minimizer_count_points(oracle, world[0], ps)
    pts += [(n + " rc", L.revcomp(s)) for n, s in pts]
    paths = _expect_paths(pts, po)
    assert paths == (len(pts), 0)
    got, _ = _tuples(oracle, ix, po, pts, paths, ("D", ps))
    want, diag, _ = _hits(mq, ix, ox, po, pts, paths, ("D", ps))
    counts = L.minimizer_counts(po.k) * 2
    assert [len(x) for x in got] == [max(0, N - po.k + 1) for N in counts]
    assert np.array_equal(diag["n_kminmers"], np.array([max(0, N - po.k + 1) for N in counts], dtype=np.uint64))
    chunked = np.array([N - po.k + 1 > L.CHUNK_KMM for N in counts])
    assert chunked.sum() == 2 * 10 and (want["mapped"][chunked] != 0).all()   # every read longer than one chunk maps
    ix.close()


# ------------------------------------------------------------------ E
@pytest.mark.parametrize("leg", range(len(L.E_PARAMS)))
def test_family_e_where_a_match_run_breaks(mq, oracle, world, leg):
    ps = L.E_PARAMS[leg]
    ix, ox, po = _index(mq, oracle, world, ps)
    pts = L.match_break_points(oracle, ox, world[0], ps)
    paths = _expect_paths(pts, po)
    assert paths == (len(pts), 0)
    _tuples(oracle, ix, po, pts, paths, ("E", ps))
    want, diag, _ = _hits(mq, ix, ox, po, pts, paths, ("E", ps))
    runs = {p[2][1]: int(diag["n_matches"][i]) for i, p in enumerate(pts) if p[2][0] == "runs"}
    assert all(m == n for m, n in runs.items()) and set(runs) == set(L.E_RUNS)
    assert (diag["n_matches"][[i for i, p in enumerate(pts) if p[2][0] != "runs"]] >= 2).all()
    assert (want["mapped"] != 0).all() and (want["rc"] != 0).sum() == len(pts) // 2
    ix.close()


# ------------------------------------------------------------------ F
def _general_points(g, po):
    return [p[:2] for p in L.general_run_points(g) + L.declined_stretch_points(g) + L.dense_step_points(g)]


@pytest.mark.parametrize("leg", range(len(L.F_PARAMS)))
def test_family_f_general_seeder_forced(mq, oracle, world, monkeypatch, leg):
    monkeypatch.setenv("MQ_FORCE_GENERAL", "1")
    g = world[0]
    ps = L.F_PARAMS[leg]
    ix, ox, po = _index(mq, oracle, world, ps)
    pts = _general_points(g, po)
    paths = _expect_paths(pts, po, forced=True)
    assert paths == (0, len(pts))
    _tuples(oracle, ix, po, pts, paths, ("F forced", ps))
    want, diag, _ = _hits(mq, ix, ox, po, pts, paths, ("F forced", ps))
    assert (want["mapped"] != 0).sum() >= len(L.F_RUNS) * len(L.F_RUN_STARTS)   # the reads with a run of A C G or T are sequence but for the run
    ix.close()


@pytest.mark.parametrize("l", L.A_LS)
def test_family_f_general_seeder_lengths(mq, oracle, world, monkeypatch, l):
    monkeypatch.setenv("MQ_FORCE_GENERAL", "1")
    ps = L.a_params(l)
    legs = [ps] + ([dict(ps, use_hpc=True)] if l in (12, 31, 64) else [])
    for ps in legs:
        ix, ox, po = _index(mq, oracle, world, ps)
        pts = L.raw_length_points(world[0], l, bases=L.F_BASES)
        paths = _expect_paths(pts, po, forced=True)
        assert paths[0] == 0 and paths[1] == sum(1 for _, s in pts if len(s) >= po.l + po.k - 1)
        _tuples(oracle, ix, po, pts, paths, ("F lengths", ps))
        want, _, _ = _hits(mq, ix, ox, po, pts, paths, ("F lengths", ps))
        if l >= 12:
            assert (want["mapped"] != 0).sum() >= sum(1 for _, s in pts if len(s) >= 2 * L.GEN_STEP)
        ix.close()


@pytest.mark.parametrize("leg", range(len(L.F_PARAMS)))
def test_family_f_declined_reads(mq, oracle, world, leg):
    """without the switch: the reads with a byte other than A C G T are declined by the fast seeder and seeded stretch by stretch"""
    g = world[0]
    ps = L.F_PARAMS[leg]
    ix, ox, po = _index(mq, oracle, world, ps)
    pts = _general_points(g, po)
    paths = _expect_paths(pts, po)
    n_dirty = sum(1 for _, s in pts if b"N" in s or b"n" in s)
    assert paths == (len(pts) - n_dirty, n_dirty) and n_dirty >= len(L.F_RUNS) * 3 + len(L.F_CLEAN) * 3 + len(L.F_HEADS)
    _tuples(oracle, ix, po, pts, paths, ("F declined", ps))
    want, diag, _ = _hits(mq, ix, ox, po, pts, paths, ("F declined", ps))
    assert (want["mapped"] != 0).sum() >= len(L.F_RUNS) * len(L.F_RUN_STARTS) + len(L.F_CLEAN) * 3
    ix.close()


# ------------------------------------------------------------------ G
@pytest.mark.parametrize("leg", range(len(L.G_PARAMS)))
def test_family_g_the_same_sequences_as_references(mq, oracle, world, leg):
    g = world[0]
    ps = L.G_PARAMS[leg]
    P, po = mq.Params(**ps), oracle.params(**ps)
    ix, ox = mq.Index(P), oracle.Index()
    pts = L.reference_length_points(g, po.l) + [p[:2] for p in L.reference_run_points(g, po.l)]
    hs = []
    for r, (name, s) in enumerate(pts):
        n_gpu, n_cpu = ix.add_ref(r, "ref%d" % r, s), ox.add_ref(r, "ref%d" % r, s, po)
        assert n_gpu == n_cpu, (ps, name, n_gpu, n_cpu)
        hs.append(L.kminmers_or_none(oracle, s, po)["hash"])
    assert ix.finalize() == ox.count()
    st = ix.stats()
    assert st["n_keys"] == ox.keys() and st["n_unique"] == ox.count() and st["n_unique"] > 0
    q = np.unique(np.concatenate(hs))
    found, ent, ids = ix.lookup(q)
    for i, h in enumerate(q):
        e = ox.get(int(h))
        assert bool(found[i]) == (e is not None), (ps, i)
        if e is not None:
            assert (int(ids[i]), int(ent[i]["start"]), int(ent[i]["end"]), int(ent[i]["offset"]), int(ent[i]["rev"])) == \
                   (int(e["id"]), int(e["start"]), int(e["end"]), int(e["offset"]), int(e["rc"])), (ps, i)
    ix.close()
