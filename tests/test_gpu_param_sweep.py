"""GPU: the parameter sweep of tests/param_sweep.py -- every window length l = 1 .. 64 and every k = 1 .. 32 (test_param_sweep_cases.py proves
the points on the CPU) -- through the fast seeder, the general seeder, seed_read_hybrid, the seeding variants that change the hashes (4) or
the positions (8, 16), the index build and the map phase; every comparison exact: hash, start, end, offset, rev of Index.kminmers_batch
against the oracle, the index's counts and entries, every column of mq_hit.

One test per LEG, not per l: a leg loops over its points, collects every mismatch as (l, hpc, k, read, field) and asserts at the end that
there is none, so that one run shows the whole pattern of a failure (one l only, one residue of l mod 4, every l above 32 ...).  Every leg
asserts last_map_path_counts(), so that the reads demonstrably went through the seeder the leg is named after: a read below l + k - 1
bases is seeded by nobody, one below 16 bases is the general seeder's by design (seed_fast_eligible), everything else ACGT-only is fast."""
import numpy as np
import pytest

import lattice as L
import param_sweep as S

pytestmark = pytest.mark.gpu

FIELDS = ("hash", "start", "end", "offset", "rev")
COLUMNS = ("ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score")
SPEC_IDS = {5: 1, 7: 2}          # MAP_SPECS (mq_host_state.hpp): the pairs compiled for l = 31, hpc, k = 5 / k = 7, SipHash
K_BUILD = (5, 7, 8, 31, 32)      # ref_kminmers_kernel's own copy of the tuple-hash dispatch: the fixed forms and the two k whose length byte wraps


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture(scope="module")
def g(simlib):
    return L.world(simlib)[0]


@pytest.fixture(scope="module")
def fx(g):
    return S.fixed_reads(g)


@pytest.fixture()
def O(oracle):
    yield oracle
    oracle.lib().mqo_set_variant(0)


_WANT = {}


def _want(O, variant, ps, pts, what):
    """the oracle's tuples of a batch, computed once per (variant, parameters, batch) and shared by the legs that need them"""
    key = (variant, tuple(sorted(ps.items())), what)
    if key not in _WANT:
        O.lib().mqo_set_variant(variant)
        po = O.params(**ps)
        _WANT[key] = [L.kminmers_or_none(O, s, po) for _, s in pts]
        O.lib().mqo_set_variant(0)
    return _WANT[key]


def _paths(pts, ps, forced=False):
    seeded = [s for _, s in pts if len(s) >= ps["l"] + ps["k"] - 1]
    general = sum(1 for s in seeded if forced or len(s) < 16 or any(c not in b"ACGT" for c in set(s)))
    return len(seeded) - general, general


def _tuples(mq, O, bad, pts, ps, what, variant=0, forced=False, fast_kh=False, spec=None):
    """one index of these parameters, the batch through kminmers_batch, every difference from the oracle appended to `bad`; returns the
    number of k-min-mers compared.  The environment (MQ_FORCE_GENERAL, MQ_NO_SPEC) is read when the index is made."""
    tag = (ps["l"], ps["use_hpc"], ps["k"])
    want = _want(O, variant | (64 if fast_kh else 0), ps, pts, what)
    ix = mq.Index(mq.Params(seeding_variant=variant, fast_kh=fast_kh, **ps))
    try:
        bases, offs = L.batch(pts)
        got = ix.kminmers_batch(bases, offs)
        paths = _paths(pts, ps, forced)
        if ix.last_map_path_counts() != paths:
            bad.append(tag + ("batch", "paths %r, not %r" % (ix.last_map_path_counts(), paths)))
        if spec is not None and ix.last_map_spec() != spec:
            bad.append(tag + ("batch", "spec %d, not %d" % (ix.last_map_spec(), spec)))
    finally:
        ix.close()
    for i, (name, _) in enumerate(pts):
        if len(got[i]) != len(want[i]):
            bad.append(tag + (name, "count %d, not %d" % (len(got[i]), len(want[i]))))
            continue
        for f in FIELDS:
            if not np.array_equal(got[i][f].astype(np.uint64), want[i][f].astype(np.uint64)):
                bad.append(tag + (name, f))
    return sum(len(w) for w in want)


def _report(bad):
    """the whole pattern of a failure in a few lines: which l, which k, which reads and fields, then the first entries themselves"""
    if not bad:
        return "no mismatch"
    ls, hpcs, ks = (sorted({b[i] for b in bad}) for i in (0, 1, 2))
    what = sorted({" / ".join(str(x) for x in b[3:]) for b in bad})
    return "%d mismatches at l = %s, hpc = %s, k = %s\n  %s\n  first: %s" % (len(bad), ls, hpcs, ks, "\n  ".join(what[:60]), bad[:20])


def _l_points(ls=S.LS, hpcs=(True, False)):
    return [(l, hpc) for l in ls for hpc in hpcs]


def _sweep_l(mq, O, fx, points, variant=0, forced=False):
    bad, n = [], 0
    for l, hpc in points:
        ps = S.l_params(l, hpc, h32=bool(variant & 4))
        n += _tuples(mq, O, bad, S.l_axis_points(fx, l, hpc), ps, "L", variant, forced)
    assert not bad, _report(bad)
    assert n > 500 * len(points)   # (the CPU test: at least 50 minimizers at every point; here: the legs compared something everywhere)
    return n


# ------------------------------------------------------------------ the L axis through both seeders
def test_leg_fast(mq, O, fx):
    pts = _l_points()
    assert len(pts) == 128
    _sweep_l(mq, O, fx, pts)


def test_leg_general(mq, O, fx, monkeypatch):
    monkeypatch.setenv("MQ_FORCE_GENERAL", "1")
    _sweep_l(mq, O, fx, _l_points(), forced=True)


def test_leg_hybrid(mq, O, g):
    """the declined batch at every l: both seeders on one read, joined at l - 1 run heads"""
    pts = S.declined_points(g)
    bad = []
    for l, hpc in _l_points():
        ps = S.l_params(l, hpc)
        assert _paths(pts, ps) == (0, len(pts))
        _tuples(mq, O, bad, pts, ps, "declined")
    assert not bad, _report(bad)


@pytest.mark.parametrize("forced", [False, True], ids=["fast", "general"])
def test_leg_variant4(mq, O, fx, monkeypatch, forced):
    """32-bit hashes and bound: seed_stage_b32 (its frame has period 32: for l > 32 the rotations wrap) and list_hash"""
    if forced:
        monkeypatch.setenv("MQ_FORCE_GENERAL", "1")
    _sweep_l(mq, O, fx, _l_points(), variant=4, forced=forced)


@pytest.mark.parametrize("forced", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("variant", [8, 16])
def test_leg_position_variants(mq, O, fx, monkeypatch, variant, forced):
    """positions read off rawpos(j + 1) - 1 (8) and rawpos(j + l - 1) (16); l = 1 has no second base (mq_index_new refuses it under 8)"""
    if forced:
        monkeypatch.setenv("MQ_FORCE_GENERAL", "1")
    pts = _l_points(S.LS[1:], (True,))
    assert len(pts) == 63
    _sweep_l(mq, O, fx, pts, variant=variant, forced=forced)


# ------------------------------------------------------------------ the index build and the map phase
def _build(mq, O, bad, tag, ref, ps, rng, fast_kh=False):
    """test_index_matches_oracle's assertions for one reference; returns (HIP index, oracle index, oracle params), the HIP index open"""
    O.lib().mqo_set_variant(64 if fast_kh else 0)
    po = O.params(**ps)
    ix, ox = mq.Index(mq.Params(fast_kh=fast_kh, **ps)), O.Index()
    n_gpu, n_cpu = ix.add_ref(0, "ref", ref), ox.add_ref(0, "ref", ref, po)
    if n_gpu != n_cpu:
        bad.append(tag + ("add_ref %d, not %d" % (n_gpu, n_cpu),))
    u = ix.finalize()
    if u != ox.count():
        bad.append(tag + ("finalize %d, not %d" % (u, ox.count()),))
    st = ix.stats()
    if (st["n_keys"], st["n_unique"]) != (ox.keys(), ox.count()):
        bad.append(tag + ("stats %r, not %r" % ((st["n_keys"], st["n_unique"]), (ox.keys(), ox.count())),))
    hs = np.unique(L.kminmers_or_none(O, ref, po)["hash"])
    O.lib().mqo_set_variant(0)
    q = np.concatenate([hs, rng.integers(0, 2**63, size=200, dtype=np.uint64)])
    found, ent, ids = ix.lookup(q)
    n_bad = 0
    for i, h in enumerate(q):
        e = ox.get(int(h))
        same = bool(found[i]) == (e is not None)
        if same and e is not None:
            same = (int(ids[i]), int(ent[i]["start"]), int(ent[i]["end"]), int(ent[i]["offset"]), int(ent[i]["rev"])) == \
                   (int(e["id"]), int(e["start"]), int(e["end"]), int(e["offset"]), int(e["rc"]))
        n_bad += not same
    if n_bad:
        bad.append(tag + ("lookup: %d of %d keys" % (n_bad, q.size),))
    return ix, ox, po


@pytest.mark.parametrize("hpc", [True, False], ids=["hpc", "raw"])
def test_leg_build(mq, O, g, hpc):
    """both references at every l: three segment views through the fast seeder; with the N, the first view declined"""
    ref = S.reference(g)
    rng = np.random.default_rng(1)
    bad = []
    for l in S.LS:
        ps = S.l_params(l, hpc)
        for what, r in (("plain", ref), ("N", S.reference_with_n(ref, l))):
            ix, ox, _ = _build(mq, O, bad, (l, hpc, ps["k"], what), r, ps, rng)
            assert ox.count() > 0 or l <= 3
            ix.close()
    assert not bad, _report(bad)


def _hits_differ(mq, got, want, diag):
    out = []
    if (got["status"] > 2).any():
        out.append("status: records never written")
    if not np.array_equal(got["n_kminmers"].astype(np.uint64), diag["n_kminmers"].astype(np.uint64)):
        out.append("n_kminmers")
    m = want["mapped"] != 0
    if not np.array_equal(got["status"] == 1, m):
        out.append("status")
    else:
        out += [f for f in COLUMNS if not np.array_equal(mq.hit_column(got, f)[m], want[f][m].astype(np.uint64))]
    return out


def test_leg_map(mq, O, g):
    """reads cut from the reference against the index of the build leg, host form and device form, every column of mq_hit"""
    from test_gpu_poison import _launch_poisoned
    ref = S.reference(g)
    reads = S.map_reads(ref)
    bases, offs = L.batch(reads)
    rng = np.random.default_rng(2)
    bad, n_mapped = [], 0
    for l in S.LS:
        ps = S.l_params(l, True)
        tag = (l, True, ps["k"])
        ix, ox, po = _build(mq, O, bad, tag + ("index",), ref, ps, rng)
        want, diag = ox.map_batch_diag(bases, offs, po, threads=4)
        hits = ix.map_batch(bases, offs)
        if ix.last_map_path_counts() != (len(reads), 0):
            bad.append(tag + ("batch", "paths %r" % (ix.last_map_path_counts(),)))
        bad += [tag + ("map_batch", f) for f in _hits_differ(mq, hits, want, diag)]
        dh = _launch_poisoned(mq, ix, bases, offs)
        bad += [tag + ("device form", f) for f in _hits_differ(mq, dh, want, diag)]
        if dh.tobytes() != hits.tobytes():
            bad.append(tag + ("device form", "bytes differ from the host form's"))
        n_mapped += int((want["mapped"] != 0).sum())
        ix.close()
    assert not bad, _report(bad)
    assert n_mapped > 8 * 40   # from l = 12 or so on the error-free reads map: a launch that answered `unmapped` everywhere cannot pass


# ------------------------------------------------------------------ the K axis
def _k_leg(mq, O, g, fx, monkeypatch, fast_kh):
    ref = S.reference(g)
    rng = np.random.default_rng(3)
    bad, n_points = [], 0
    for k in S.KS:
        for l in S.K_AXIS_LS:
            ps = S.k_params(k, l)
            pts = S.k_axis_points(O, g, fx, k, l)
            assert len(pts) == (10 if k >= 4 else 9) and _paths(pts, ps)[0] >= 6   # (the seam's reads below 16 bases are the general seeder's)
            for v in (0, 32):   # a tuple equal to its reverse: rev = 0 under `<`, 1 under `<=` (VAR = true instantiations)
                spec = (0 if fast_kh else SPEC_IDS[k]) if (v == 0 and l == 31 and k in SPEC_IDS) else None
                _tuples(mq, O, bad, pts, ps, "K", v, fast_kh=fast_kh, spec=spec)
                n_points += 1
            if l == 31 and k in SPEC_IDS:   # once more through SpecNone's own fixed forms
                monkeypatch.setenv("MQ_NO_SPEC", "1")
                _tuples(mq, O, bad, pts, ps, "K", 0, fast_kh=fast_kh, spec=0)
                monkeypatch.delenv("MQ_NO_SPEC")
            if k in K_BUILD:
                ix, _, _ = _build(mq, O, bad, (l, True, k, "build"), ref, ps, rng, fast_kh=fast_kh)
                ix.close()
    assert not bad, _report(bad)
    assert n_points == 128


def test_leg_k_sip(mq, O, g, fx, monkeypatch):
    _k_leg(mq, O, g, fx, monkeypatch, False)


def test_leg_k_fast(mq, O, g, fx, monkeypatch):
    _k_leg(mq, O, g, fx, monkeypatch, True)
