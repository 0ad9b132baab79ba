"""GPU: the boundary lattice through EVERY map-kernel instantiation.  test_gpu_lattice.py runs the lattice through one kernel pair, the product
pair at the frozen reading; this module runs a core batch of it (lattice.core_points: every size of lattice.py's header exactly and one
element to either side, proved on the CPU by test_lattice_cases.py) plus two families of its own -- H, the list region's capacity, and I,
lower case on the seeders' borders -- through the rest of MAP_KERNELS, MAP_SPECS and the split pipeline.  Every row asserts (a) that the
configuration took effect, (b) k-min-mer tuples equal to the oracle's, (c) records written into a 0xFF-filled buffer, host form and device
form, equal to the oracle's, (d) where the records must not change, byte equality with the baseline: the core batch through the product
pair, itself checked against the oracle.  The oracle's answers are computed once per (batch, oracle variant).

  row                  kernels it runs
  baseline             map_kernel<64,false,false,SpecFixed<5,31,hpc>> + map_declined_kernel of the same (k = 3, l = 12: SpecNone)
  nospec               map_pair<64,false,false> (SpecNone at the default parameters)
  spec2                SpecFixed<7,31,hpc>, against map_pair<64,false,false>
  spec3_fold           SpecFixed<5,31,hpc,fold>, against map_pair<64,false,false> folding at run time
  chunk4               map_pair<4,false,false>
  instrumented         map_pair<64,true,false>
  split                seed_reads_kernel<0>, seed_general_kernel, map_lists_kernel<64,false>
  split_var16          the same three with mz_last[] handed over through mz_base[]
  fast_kh              map_pair<64,false,false> with KhFast in the chunk's lane-batch loop
  v1 .. v63            map_pair<64,false,true>; v4: seed_stage_b32
  v4_chunk4 v16_chunk4 map_pair<4,false,true>
  v16_instrumented     map_pair<64,true,true>
  list_f16             the product pair and map_pair<64,false,true> with 64-entry list regions: seed_read_fast / seed_read_general's move to
                       the pool
  host_redo            the product pair with a one-record Match window, redo_relaunch and the redo arena's launch (f16 = 65536, no pool)
  heavy_off            order_reads_kernel without its front, the product pair

What the core batch leaves out: at k = 3, l = 12 family E's BREAK points (an error-free read misses at some k-min-mers, so the search for
"all hit but one" has nowhere to start: lattice.core_points); its Match-run reads of 47 / 48 / 49 and 63 / 64 / 65 runs are there
(lattice.match_run_points), and the guard on them is asserted for every parameter set.
The list-capacity point at the DEFAULT f16 -- a read whose minimizer count equals its own region -- does not exist in this genome (a
region is 2.6 times the expected list; lattice.read_at_default_cap raises LatticeError, asserted here and on the CPU): family H's points
are the ones at MQ_LIST_F16=1.

Sensitivity of list_f16, checked once on a scratch build and not committed: with seed_read_fast's `cnt > cap` changed to
`cnt >= cap + 2` the row fails at 'H N=65' itself, device form, one record (q_end wrong).  The neighbour's record is unharmed: the first
seeding pass does stop storing at cap, so the 65th entry is never written and the map phase reads the neighbour's first entry in its place.

Timings on an MI355X (pytest --durations=0; none is asserted): the module 17.9 s for 32 tests.  The first test pays for the three core
batches' construction and their oracle answers, 7.7 s (on the CPU the constructors' searches take 9.9 s for the default batch, 11.0 s for
k = 7, 0.2 s for k = 3, l = 12, nearly all of it family E); v4, v8, v63 and split_var16 1.0 s each and the three v4 length lattices
0.85 - 0.95 s each, most of it the oracle's naive minimizer routine under variants 4 / 8 / 16; spec3_fold, fast_kh, v1, v2, v32 and the
k = 3, l = 12 variants 0.2 - 0.3 s; every other row at most 0.12 s.  Nothing exceeded 5 s but the shared construction, so no batch was
cut.  For comparison, test_gpu_lattice.py in the same session: its slowest tests 3.4 s and 2.1 s (family E, which searches with the oracle
per test), 1.6 s twice (family B under variants 8 and 16), each of its other 33 tests below 0.95 s."""
import os

import numpy as np
import pytest

import lattice as L
from test_gpu_lattice import COLUMNS, FIELDS, _expect_paths, _same, _tuples
from test_gpu_poison import _launch_poisoned

pytestmark = pytest.mark.gpu

HOOKS = ("MQ_NO_SPEC", "MQ_CHAIN_CHUNK", "MQ_PIPELINE", "MQ_FORCE_GENERAL", "MQ_LIST_F16", "MQ_MATCH_CAP", "MQ_HEAVY_FIRST")


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture(scope="module")
def world(simlib):
    return L.world(simlib)


class _Kmm:
    """the oracle's k-min-mers of a batch, computed once; stands in for the oracle module in test_gpu_lattice._tuples"""

    def __init__(self, O, pts, po, upper):
        self.kminmer_dtype = O.kminmer_dtype
        self._of = {p[1]: L.kminmers_or_none(O, p[1].upper() if upper else p[1], po) for p in pts}

    def kminmers(self, seq, po):
        return self._of[seq]


class _Answer:
    """a batch and what the oracle says about it under one variant: records (want, diag), tuples (kmm), the index's counts"""


class _World:
    """batches and the oracle's answers, each made on first use and kept for the module"""

    def __init__(self, O, world):
        self.O, self.world, self._pts, self._ans = O, world, {}, {}

    def _oracle_index(self, ps):
        g, off, names = self.world
        po, ox = self.O.params(**ps), self.O.Index()
        n_ref = ox.add_ref(0, names[0], g, po)
        return ox, po, n_ref

    def core(self, which):
        if which not in self._pts:
            ps, families = L.CORE_PARAMS[which]
            ox, po, _ = self._oracle_index(ps)
            self._pts[which] = L.core_points(self.O, ox, self.world[0], ps, families)
        return self._pts[which]

    def answer(self, key, ps, v, pts, upper=False):
        """the oracle on `pts` with mqo_set_variant(v); key names the batch (the cache is per (key, v))"""
        if (key, v) not in self._ans:
            a = _Answer()
            a.pts, a.ps = pts, ps
            a.bases, a.offs = L.batch(pts)
            ub = np.frombuffer(a.bases.tobytes().upper(), dtype=np.uint8) if upper else a.bases   # the reference folds before it seeds (src/closures.rs:63,106)
            self.O.lib().mqo_set_variant(v)
            try:
                ox, a.po, a.n_ref = self._oracle_index(ps)
                a.unique = ox.count()
                a.want, a.diag = ox.map_batch_diag(ub, a.offs, a.po, threads=8)
                a.kmm = _Kmm(self.O, pts, a.po, upper)
            finally:
                self.O.lib().mqo_set_variant(0)
            self._ans[(key, v)] = a
        return self._ans[(key, v)]

    def core_answer(self, which, v=0):
        a = self.answer("core " + which, L.CORE_PARAMS[which][0], v, self.core(which))
        if v == 0:
            # shared guard: every error-free read of a random genome maps at l >= 12, so the oracle maps at least the reads of >= 4,000 bases cut
            # from the genome (families A, D, E).  Observed on the CPU: default 315 mapped of 330 / 126 such reads; k = 3, l = 12: 258 of 270 /
            # 54; k = 7: 315 of 330 / 126
            n_long = sum(1 for p in a.pts if p[2] in "ADE" and len(p[1]) >= 4000)
            assert n_long >= 40 and int((a.want["mapped"] != 0).sum()) >= n_long, (which, n_long)
            for m in L.CORE_RUNS:   # chunk4, instrumented, split and the variants: a read on either side of MAP_LDS_RECS and of the chain chunk
                assert (a.diag["n_matches"] == m).sum() >= 2, (which, "no read with %d Match runs" % m)
        return a


@pytest.fixture(scope="module")
def lat(oracle, world):
    for h in HOOKS:
        assert h not in os.environ, h
    return _World(oracle, world)


def _index(mq, world, a, variant=0, **flags):
    """the HIP index of the genome with the answer's parameters; the environment hooks are read here (MQ_MATCH_CAP: at its first map call)"""
    g, off, names = world
    ix = mq.Index(mq.Params(seeding_variant=variant, **flags, **a.ps))
    assert ix.add_ref(0, names[0], g) == a.n_ref
    assert ix.finalize() == a.unique
    return ix


def _host_poisoned(mq, ix, a):
    """the host-buffer form (mq_map_batch, the default context) into a 0xFF-filled array"""
    import ctypes as C
    n = a.offs.size - 1
    out = np.frombuffer(b"\xff" * (n * mq.hit_dtype.itemsize), dtype=mq.hit_dtype).copy()
    vp = C.c_void_p
    rc = ix._L.mq_map_batch(ix._h, vp(a.bases.ctypes.data), vp(a.offs.ctypes.data), n, vp(out.ctypes.data))
    assert rc == 0, ix._L.mq_last_error()
    return out


def _records(mq, got, a, what):
    """status, the eight columns and n_kminmers of every record against the oracle's: the first read that differs is named, then _same"""
    w, d = a.want, a.diag
    m = w["mapped"] != 0
    bad = (got["status"] > 2) | (got["n_kminmers"].astype(np.uint64) != d["n_kminmers"].astype(np.uint64)) | ((got["status"] == 1) != m)
    for f in COLUMNS:
        bad |= m & (mq.hit_column(got, f) != w[f].astype(np.uint64))
    i = np.flatnonzero(bad)
    assert i.size == 0, "%s: %d records differ from the oracle's, first at %r: %s" % (what, i.size, a.pts[i[0]][0], got[i[0]])
    _same(mq, got, w, d, what)


def _bytes_equal(got, ref, pts, what):
    i = np.flatnonzero(got != ref) if got.shape == ref.shape else np.arange(1)
    assert got.tobytes() == ref.tobytes(), "%s: %d records differ, first at %r: %s != %s" % (what, i.size, pts[i[0]][0], got[i[0]], ref[i[0]])


def _paths_fold(pts, po):
    """_expect_paths where a c g t are sequence too"""
    seeded = [p[1] for p in pts if len(p[1]) >= po.l + po.k - 1]
    general = sum(1 for s in seeded if len(s) < 16 or any(c not in b"ACGTacgt" for c in set(s)))
    return len(seeded) - general, general


def _run(mq, ix, a, what, paths=None, tuples=True, host=True, spec=None):
    """(b) the tuples, (c) the host form and the device form on 0xFF-filled buffers against the oracle's answer `a`; the seeding paths and
    (spec) the kernel pair of every launch.  Returns the device form's records."""
    if paths is None:
        paths = _expect_paths(a.pts, a.po)
    if tuples:
        _tuples(a.kmm, ix, a.po, a.pts, paths, what)
    dev = _launch_poisoned(mq, ix, a.bases, a.offs)
    assert ix.last_map_path_counts() == paths, (what, "device form", ix.last_map_path_counts(), paths)
    if spec is not None:
        assert ix.last_map_spec() == spec, (what, "device form", ix.last_map_spec(), spec)
    _records(mq, dev, a, (what, "device form"))
    if host:
        hh = _host_poisoned(mq, ix, a)
        assert ix.last_map_path_counts() == paths, (what, "host form", ix.last_map_path_counts(), paths)
        if spec is not None:
            assert ix.last_map_spec() == spec, (what, "host form", ix.last_map_spec(), spec)
        _records(mq, hh, a, (what, "host form"))
        _bytes_equal(hh, dev, a.pts, (what, "host form against device form"))
    return dev


@pytest.fixture(scope="module")
def baseline(mq, lat, world):
    """the core batches through the product pair, checked against the oracle exactly: {which: (records of the device form, spec id)}"""
    made = {}

    def get(which):
        if which not in made:
            a = lat.core_answer(which)
            ix = _index(mq, world, a)
            dev = _run(mq, ix, a, ("baseline", which))
            made[which] = (dev, ix.last_map_spec(), ix.last_map_order())
            ix.close()
        return made[which]
    return get


def test_baseline_is_the_product_pair(baseline):
    assert baseline("default")[1] == 1 and baseline("k3l12")[1] == 0 and baseline("k7")[1] == 2
    for which in L.CORE_PARAMS:   # family B's long homopolymer runs are taken for tandem arrays: the launch put reads first
        taken, first = baseline(which)[2]
        assert 0 < first <= taken, (which, taken, first)


def test_nospec(mq, lat, world, baseline, monkeypatch):
    monkeypatch.setenv("MQ_NO_SPEC", "1")
    a = lat.core_answer("default")
    ix = _index(mq, world, a)
    dev = _run(mq, ix, a, "nospec", spec=0)
    _bytes_equal(dev, baseline("default")[0], a.pts, "nospec against the baseline")
    ix.close()


def test_spec2(mq, lat, world, baseline, monkeypatch):
    a = lat.core_answer("k7")
    ix = _index(mq, world, a)
    dev = _run(mq, ix, a, "spec2", spec=2)
    ix.close()
    monkeypatch.setenv("MQ_NO_SPEC", "1")
    ix = _index(mq, world, a)
    own = _run(mq, ix, a, "spec2 with MQ_NO_SPEC=1", tuples=False, spec=0)
    _bytes_equal(dev, own, a.pts, "spec2 against its own nospec run")
    ix.close()


def test_spec3_fold(mq, lat, world, monkeypatch):
    pts = lat.core("default") + L.fold_border_points(world[0])
    a = lat.answer("core default + I, folded", dict(), 0, pts, upper=True)
    paths = _paths_fold(pts, a.po)
    dirty = sum(1 for p in pts if any(c not in b"ACGTacgt" for c in set(p[1])))
    assert paths[1] == dirty + sum(1 for p in pts if a.po.l + a.po.k - 1 <= len(p[1]) < 16) and dirty >= 4 + len(L.F_RUNS) + len(L.F_CLEAN) + len(L.F_HEADS)
    assert sum(1 for p in pts if p[1] != p[1].upper()) >= len(L.I_BYTES) + 7
    ix = _index(mq, world, a, fold_case=True)
    dev = _run(mq, ix, a, "spec3_fold", paths=paths, spec=3)
    ix.close()
    monkeypatch.setenv("MQ_NO_SPEC", "1")
    ix = _index(mq, world, a, fold_case=True)
    own = _run(mq, ix, a, "fold with MQ_NO_SPEC=1", paths=paths, tuples=False, spec=0)
    _bytes_equal(dev, own, pts, "spec3_fold against MQ_NO_SPEC=1 + fold")
    ix.close()


@pytest.mark.parametrize("which", ["default", "k3l12"])
def test_chunk4(mq, lat, world, baseline, monkeypatch, which):
    monkeypatch.setenv("MQ_CHAIN_CHUNK", "4")
    a = lat.core_answer(which)
    ix = _index(mq, world, a)
    dev = _run(mq, ix, a, ("chunk4", which), tuples=False, spec=0)
    _bytes_equal(dev, baseline(which)[0], a.pts, ("chunk4 against the baseline", which))
    ix.close()


def _probe(mq, ix, a, what):
    """the instrumented launch on the device-resident batch, 0xFF-filled result: (records, lookups); every seeded read was timed"""
    from hipmem import DevBuf, device_sync, memset
    n = a.offs.size - 1
    db, do, out = DevBuf.from_numpy(a.bases), DevBuf.from_numpy(a.offs), DevBuf(n * mq.hit_dtype.itemsize)
    memset(out, 0xFF)
    ix.reserve(n, int(a.offs[-1]))
    lookups, _ = ix.probe_stats(db.ptr, do.ptr, n, int(a.offs[-1]), out.ptr)
    device_sync()
    hits = out.to_numpy(mq.hit_dtype, n)
    cyc, _ = ix.last_read_cycles(n)
    for b in (db, do, out):
        b.free()
    seeded = np.array([len(p[1]) >= a.po.l + a.po.k - 1 for p in a.pts])
    i = np.flatnonzero(seeded & (cyc == 0))
    assert i.size == 0, "%s: no cycles for %d seeded reads, first %r" % (what, i.size, a.pts[i[0]][0])
    assert lookups > 0, what
    return hits, lookups


def test_instrumented(mq, lat, world, baseline):
    a = lat.core_answer("default")
    ix = _index(mq, world, a)
    hits, lookups = _probe(mq, ix, a, "instrumented")
    assert lookups >= int(a.diag["n_kminmers"].sum()) // 2
    _bytes_equal(hits, baseline("default")[0], a.pts, "instrumented against the baseline")
    ix.close()


@pytest.mark.parametrize("forced", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("which", ["default", "k3l12"])
def test_split(mq, lat, world, baseline, monkeypatch, which, forced):
    monkeypatch.setenv("MQ_PIPELINE", "split")
    if forced:
        monkeypatch.setenv("MQ_FORCE_GENERAL", "1")
    a = lat.core_answer(which)
    paths = _expect_paths(a.pts, a.po, forced=forced)
    assert paths[1] > 0 and (forced or paths[0] > paths[1])
    ix = _index(mq, world, a)
    dev = _run(mq, ix, a, ("split", which, forced), paths=paths)
    _bytes_equal(dev, baseline(which)[0], a.pts, ("split against the baseline", which, forced))
    ix.close()


def test_split_var16(mq, lat, world, monkeypatch):
    monkeypatch.setenv("MQ_PIPELINE", "split")
    a = lat.core_answer("default", 16)
    ix = _index(mq, world, a, variant=16)
    _run(mq, ix, a, "split_var16")
    ix.close()


def test_fast_kh(mq, lat, world, baseline):
    a, sip = lat.core_answer("default", 64), lat.core_answer("default")
    ix = _index(mq, world, a, fast_kh=True)
    dev = _run(mq, ix, a, "fast_kh", spec=0)
    n = 0
    for p in a.pts:   # the oracle's own two hashes (the tuples above are the oracle's under bit 64): every other field equal, no hash equal
        f, s = a.kmm.kminmers(p[1], a.po), sip.kmm.kminmers(p[1], a.po)
        assert len(f) == len(s) and all(np.array_equal(f[x], s[x]) for x in FIELDS[1:]), ("fast_kh", p[0])
        assert not (f["hash"] == s["hash"]).any(), ("fast_kh: a tuple hash equal to SipHash's", p[0])
        n += len(f)
    assert n > 10000
    _bytes_equal(dev, baseline("default")[0], a.pts, "fast_kh against the baseline")   # a record holds no hash: every field equal
    ix.close()


VARIANT_ROWS = [("default", v) for v in (1, 2, 4, 8, 16, 32, 63)] + [("k3l12", 4), ("k3l12", 16)]


@pytest.mark.parametrize("which,v", VARIANT_ROWS, ids=["v%d%s" % (v, "" if w == "default" else "_" + w) for w, v in VARIANT_ROWS])
def test_variant(mq, lat, world, which, v):
    a = lat.core_answer(which, v)
    ix = _index(mq, world, a, variant=v)
    _run(mq, ix, a, ("v%d" % v, which), spec=0)
    ix.close()


@pytest.mark.parametrize("l", [31, 32, 33])
def test_v4_full_length_lattice(mq, lat, world, l):
    """stage B on two dwords rotates its frame with period 32: family A's FULL length lattice for l around it"""
    ps = L.a_params(l)
    a = lat.answer("A l=%d" % l, ps, 4, L.raw_length_points(world[0], l))
    assert len(a.pts) == len(L.length_lattice(l)) and int(a.diag["n_kminmers"].sum()) > len(a.pts)
    ix = _index(mq, world, a, variant=4)
    _run(mq, ix, a, ("v4 family A", l), spec=0)
    ix.close()


@pytest.mark.parametrize("v", [4, 16])
def test_variant_chunk4(mq, lat, world, monkeypatch, v):
    a = lat.core_answer("default", v)
    ix = _index(mq, world, a, variant=v)
    ref = _run(mq, ix, a, ("v%d" % v, "chunk 64"), tuples=False, host=False)
    ix.close()
    monkeypatch.setenv("MQ_CHAIN_CHUNK", "4")
    ix = _index(mq, world, a, variant=v)
    dev = _run(mq, ix, a, "v%d_chunk4" % v, tuples=False, spec=0)
    _bytes_equal(dev, ref, a.pts, "v%d_chunk4 against the v%d run" % (v, v))
    ix.close()


def test_v16_instrumented(mq, lat, world):
    a = lat.core_answer("default", 16)
    ix = _index(mq, world, a, variant=16)
    ref = _run(mq, ix, a, "v16", tuples=False, host=False)
    hits, _ = _probe(mq, ix, a, "v16_instrumented")
    _bytes_equal(hits, ref, a.pts, "v16_instrumented against the v16 run")
    ix.close()


@pytest.mark.parametrize("v", [0, 16])
def test_list_f16(mq, lat, world, baseline, monkeypatch, v):
    """64-entry list regions (MQ_LIST_F16=1, read at every launch): lists of 63 and 64 entries stay, those of 65 and of a stage R round more
    move to the pool, with a neighbour's region directly behind each; fast reads and reads with an N.  The point at the default f16 does
    not exist for this genome (LatticeError)."""
    g = world[0]
    with pytest.raises(L.LatticeError):
        L.read_at_default_cap(lat.O, g, dict(), lat.O.kminmers(g, lat.O.params(k=1)))
    core = lat.core("default")
    h = L.list_capacity_points(lat.O, g, dict(), default_too=False)
    pts = [("H " + p[0], p[1], p[2]) for p in h] + [p for p in core if p[2] == "D"]
    assert L.regions_adjacent(pts) == [True] * (2 * len(L.H_COUNTS))    # a store at [cap] lands in the neighbour's first entry
    counts = [p[2] for p in h if isinstance(p[2], int)]
    assert min(counts) <= L.LIST_SLACK and max(counts) >= L.LIST_SLACK + 1                # (the CPU proof pins every count)
    a = lat.answer("H + core D", dict(), v, pts)
    n_dirty = sum(1 for p in pts if b"N" in p[1])
    assert n_dirty == len(L.H_COUNTS) and _expect_paths(pts, a.po) == (len(pts) - n_dirty, n_dirty)
    ix = _index(mq, world, a, variant=v)
    plain = _run(mq, ix, a, ("default f16", v), tuples=False, host=False)
    # every neighbour alone: its record and its tuples
    alone = lat.answer("H neighbour", dict(), v, [("neighbour alone", h[1][1], None)])
    rec_alone = _run(mq, ix, alone, ("neighbour alone", v))
    kmm_alone = ix.kminmers_batch(alone.bases, alone.offs)[0]
    monkeypatch.setenv("MQ_LIST_F16", str(L.H_F16))
    dev = _run(mq, ix, a, ("list_f16", v))
    got = ix.kminmers_batch(a.bases, a.offs)
    for i, p in enumerate(pts):
        if p[0].startswith("H neighbour"):
            assert dev[i].tobytes() == rec_alone[0].tobytes(), ("list_f16", v, p[0], dev[i], rec_alone[0])
            assert got[i].tobytes() == kmm_alone.tobytes(), ("list_f16", v, p[0], "tuples")
    assert sum(1 for p in pts if p[0].startswith("H neighbour")) == 2 * len(L.H_COUNTS)
    _bytes_equal(dev, plain, pts, ("list_f16 against the default f16", v))
    if v == 0:
        base = baseline("default")[0]
        at = {p[0]: i for i, p in enumerate(core)}
        for i, p in enumerate(pts):
            if p[2] == "D":
                assert dev[i].tobytes() == base[at[p[0]]].tobytes(), ("list_f16 against the baseline", p[0])
    ix.close()


def test_host_redo(mq, lat, world, monkeypatch):
    """MQ_MATCH_CAP=1 on the core batch: the device form reports MQ_HIT_OVERFLOW for the reads with more Match runs than a one-record window,
    the host form redoes them (f16 = 65536, no pool, worst-case windows on a small grid), an arena does the same in stream"""
    monkeypatch.setenv("MQ_MATCH_CAP", "1")
    a = lat.core_answer("default")
    paths = _expect_paths(a.pts, a.po)
    ix = _index(mq, world, a)
    raw = _launch_poisoned(mq, ix, a.bases, a.offs)
    assert ix.last_map_path_counts() == paths, ("host_redo", ix.last_map_path_counts(), paths)
    over = raw["status"] == 2
    n, n_over = len(a.pts), int(over.sum())
    assert (raw["status"] <= 2).all() and 0 < n_over < n, ("host_redo", n_over, n)
    i = np.flatnonzero(over & (a.diag["n_matches"] <= 1))
    assert i.size == 0, ("host_redo: overflow with at most one Match run", a.pts[i[0]][0] if i.size else None)
    hh = _host_poisoned(mq, ix, a)
    assert not (hh["status"] == 2).any()
    _records(mq, hh, a, "host_redo, host form")
    _bytes_equal(raw[~over], hh[~over], [p for p, o in zip(a.pts, over) if not o], "host_redo: the reads that did not overflow")
    ix.reserve_redo(n, max(len(p[1]) for p in a.pts))
    try:
        dev = _launch_poisoned(mq, ix, a.bases, a.offs)
        assert ix.redo_counts() == (n_over, 0)
        _bytes_equal(dev, hh, a.pts, "host_redo: device form with an arena against the host form")
        assert ix.last_map_path_counts() == paths, ("host_redo with an arena", ix.last_map_path_counts(), paths)   # (the arena's launch counts in a context of its own)
    finally:
        ix.reserve_redo(0, 0)
    ix.close()


def test_heavy_off(mq, lat, world, baseline, monkeypatch):
    monkeypatch.setenv("MQ_HEAVY_FIRST", "0")
    a = lat.core_answer("default")
    ix = _index(mq, world, a)
    dev = _run(mq, ix, a, "heavy_off", tuples=False)
    assert ix.last_map_order()[1] == 0 and baseline("default")[2][1] > 0
    _bytes_equal(dev, baseline("default")[0], a.pts, "heavy_off against the baseline")
    ix.close()
