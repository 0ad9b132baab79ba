"""CPU: every point of the parameter sweep (tests/param_sweep.py) has the property it is named after -- for all 64 x 2 points of the L axis
and all 32 x 2 points of the K axis, under the frozen seeding and under seeding variant 4 (32-bit hashes and bound).  No GPU: the
constructors and the oracle only.  test_gpu_param_sweep.py runs exactly these inputs through the HIP path."""
import numpy as np
import pytest

import lattice as L
import param_sweep as S


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


L_POINTS = [(l, hpc) for l in S.LS for hpc in (True, False)]
K_POINTS = [(k, l) for k in S.KS for l in S.K_AXIS_LS]


def test_the_axes_are_whole():
    assert S.LS == tuple(range(1, 65)) and S.KS == tuple(range(1, 33))
    assert len(L_POINTS) == 128 and len(K_POINTS) == 64
    assert set(S.K_AXIS_LS) == {14, 31}


def test_the_batch_is_small_and_clean(fx):
    for l, hpc in L_POINTS:
        pts = S.l_axis_points(fx, l, hpc)
        assert len(pts) <= 10 and sum(len(s) for _, s in pts) < 80_000
        assert all(set(s) <= set(b"ACGT") for _, s in pts)
    by = dict(S.l_axis_points(fx, 31, True))
    assert len(by["tile + super-row + 37"]) == L.SD_TILE_RAW + L.SD_SR_RAW + 37 and len(by["two tiles + 1"]) == 2 * L.SD_TILE_RAW + 1
    hp = by["run of %d in 3 kb" % S.HP_RUN]
    assert len(hp) == 3000 and L.run_is_exact(hp, S.HP_AT, S.HP_RUN)
    for l in S.LS:   # under compression the l bases of a window that starts on the run span more than 64 raw ones
        assert S.HP_RUN + l - 1 > 64 and S.HP_AT + S.HP_RUN + l < len(hp)


def _count(O, seq, ps, h32):
    """minimizers the oracle lists (variant 4: mqo_minimizers has no 32-bit form, the k-min-mers of k = 1 are the minimizers)"""
    if h32:
        return len(O.kminmers(seq, O.params(**dict(ps, k=1)))) if len(seq) >= ps["l"] else 0
    return len(O.minimizers(seq, O.params(**ps)))


@pytest.mark.parametrize("h32", [False, True], ids=["h64", "h32"])
def test_l_axis_points(O, fx, h32):
    O.lib().mqo_set_variant(4 if h32 else 0)
    bad = []
    for l, hpc in L_POINTS:
        ps = S.l_params(l, hpc, h32=h32)
        po = O.params(**ps)
        pts = dict(S.l_axis_points(fx, l, hpc))
        k = ps["k"]
        # some minimizers and not every window, in the batch and in each of its long reads
        for name in ("tile + super-row + 37", "two tiles + 1"):
            n, w = _count(O, pts[name], ps, h32), S.windows(pts[name], l, hpc)
            if not 50 <= n < w:
                bad.append((l, hpc, name, "minimizers", n, w))
        n = sum(_count(O, s, ps, h32) for s in pts.values())
        w = sum(S.windows(s, l, hpc) for s in pts.values())
        if not 50 <= n < w:
            bad.append((l, hpc, "batch", "minimizers", n, w))
        # the seam: below l + k - 1 bases nothing, from there on whatever the oracle says
        lens = [len(pts["len=l+k%+d" % d]) for d in (-2, -1, 0)]
        if lens != [l + k - 2, l + k - 1, l + k]:
            bad.append((l, hpc, "seam", "lengths", lens))
        if len(L.kminmers_or_none(O, pts["len=l+k-2"], po)) != 0:
            bad.append((l, hpc, "len=l+k-2", "k-min-mers"))
        for d in (-1, 0):
            s = pts["len=l+k%+d" % d]
            if len(L.kminmers_or_none(O, s, po)) != max(0, _count(O, s, ps, h32) - k + 1):
                bad.append((l, hpc, "len=l+k%+d" % d, "k-min-mers"))
        # lc's parity, in reads of one super-row
        for name, parity in (("lc odd", 1), ("lc even", 0)):
            s = pts[name]
            if not (len(s) < L.SD_SR_RAW and S.lanes_chunk(s, l, hpc) >= 1 and S.lanes_chunk(s, l, hpc) % 2 == parity):
                bad.append((l, hpc, name, "lc", S.lanes_chunk(s, l, hpc)))
            if S.windows(s, l, hpc) != _count(O, s, dict(ps, density=1.0), h32):
                bad.append((l, hpc, name, "windows"))
        # no window's hash shares the bound's high word: every read of the batch stays with the fast seeder
        for name, s in pts.items():
            if S.bound_ties(O, s, ps, h32):
                bad.append((l, hpc, name, "high word of the bound"))
        if not h32:   # the rolling form of the oracle against its naive form
            for name, s in pts.items():
                a, b = O.minimizers(s, po), O.minimizers(s, po, naive=True)
                if a.tobytes() != b.tobytes():
                    bad.append((l, hpc, name, "naive"))
    assert not bad, bad


def test_the_32_bit_hashes_are_the_oracles(O, fx):
    """window_hashes32 (numpy) against the oracle under variant 4: the windows at or below the bound are the k-min-mers of k = 1, in number and place"""
    O.lib().mqo_set_variant(4)
    for l in (1, 2, 3, 14, 31, 32, 33, 47, 64):
        for hpc in (True, False):
            ps = S.l_params(l, hpc, h32=True)
            s = fx["odd"]
            h = S.window_hashes32(s, l, hpc)
            assert h.size == S.windows(s, l, hpc)
            keep = np.flatnonzero(h <= np.uint32(O.lib().mqo_density_bound(ps["density"])))
            km = O.kminmers(s, O.params(**dict(ps, k=1)))
            assert keep.size == len(km) > 0, (l, hpc)
            a = np.frombuffer(s, dtype=np.uint8)
            heads = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1]))) if hpc else np.arange(a.size)
            assert np.array_equal(heads[keep], km["start"].astype(np.int64)), (l, hpc)


def test_declined_batch(g):
    pts = S.declined_points(g)
    assert len(pts) == 2
    for (name, s), at in zip(pts, S.DECLINED_N):
        assert s.count(b"N") == 1 and s[at] == ord("N") and set(s) <= set(b"ACGTN") and 6000 <= len(s) <= 7000
        assert all(c >= L.HYB_MIN_CLEAN + 64 for c in S.clean_sides(s)), (name, S.clean_sides(s))
    assert S.DECLINED_N[0] % L.BLOCK == 0 and S.DECLINED_N[1] % L.BLOCK == L.BLOCK // 2


def test_k_axis_points(O, g, fx):
    bad = []
    n_deep = 0
    for k, l in K_POINTS:
        ps = S.k_params(k, l)
        po = O.params(**ps)
        pts = dict(S.k_axis_points(O, g, fx, k, l))
        n = sum(len(O.minimizers(s, po)) for s in pts.values())
        w = sum(S.windows(s, l, True) for s in pts.values())
        if not 50 <= n < w:
            bad.append((k, l, "batch", "minimizers", n, w))
        if len(L.kminmers_or_none(O, pts["len=l+k-2"], po)) != 0 or len(pts["len=l+k-1"]) != l + k - 1:
            bad.append((k, l, "seam"))
        pal = pts["palindromic"]
        h = O.minimizers(pal, po)["hash"]
        at = S.palindromic_tuples(h, k)
        if not (at.size and len(pal) <= 2 * S.PAL_HALF + 1 and all(np.array_equal(h[i:i + k], h[i:i + k][::-1]) for i in at)):
            bad.append((k, l, "palindromic", "no tuple equals its reverse"))
        # the oracle's orientation of such a tuple: forward under `<`, reversed under `<=`
        km = O.kminmers(pal, po)
        O.lib().mqo_set_variant(32)
        km32 = O.kminmers(pal, po)
        O.lib().mqo_set_variant(0)
        if not ((km["rev"][at] == 0).all() and (km32["rev"][at] == 1).all() and np.array_equal(np.flatnonzero(km["rev"] != km32["rev"]), at)):
            bad.append((k, l, "palindromic", "rev"))
        if k >= 4:
            h = O.minimizers(pts["deep decision"], po)["hash"]
            at = S.deep_tuples(h, k)
            j = k // 2 - 1
            ok = at.size and all(np.array_equal(h[i:i + j], h[i + k - j:i + k][::-1]) and h[i + j] != h[i + k - 1 - j] for i in at)
            if not ok:
                bad.append((k, l, "deep decision", "no tuple decided at the innermost pair"))
            n_deep += 1
        else:
            assert "deep decision" not in pts
        for name, s in pts.items():
            if not set(s) <= set(b"ACGT") or S.bound_ties(O, s, ps):
                bad.append((k, l, name, "high word of the bound"))
    assert not bad, bad
    assert n_deep == 2 * 29


def test_tuple_decisions_by_hand():
    h = np.array([5, 1, 2, 3, 2, 1, 5, 9], dtype=np.uint64)
    assert S.tuple_decisions(h, 7).tolist() == [3, 0] and S.palindromic_tuples(h, 7).tolist() == [0]
    assert S.tuple_decisions(h, 5).tolist() == [0, 2, 0, 0] and S.tuple_decisions(h, 1).tolist() == [0] * 8
    h = np.array([9, 1, 2, 7, 3, 2, 1], dtype=np.uint64)
    assert S.tuple_decisions(h, 6).tolist() == [0, 2] and S.deep_tuples(h, 6).tolist() == [1] and S.deep_tuples(h, 3).size == 0


def test_reference_and_map_reads(O, g):
    ref = S.reference(g)
    assert len(ref) == 2 * L.REF_SEG + L.REF_HALO + 123 and set(ref) <= set(b"ACGT")
    for l in S.LS:
        s = S.reference_with_n(ref, l)
        assert s.count(b"N") == 1 and s.index(b"N") == L.REF_SEG - l and len(s) == len(ref)
    reads = S.map_reads(ref)
    assert len(reads) == S.MAP_READS and all(2000 <= len(s) <= 6000 for _, s in reads)
    assert sum(" rc" in n for n, _ in reads) == 6 and sum(" 1%" in n for n, _ in reads) == 4
    # at the default-like parameters of the axis the error-free reads map, on the strand they were cut from
    po = O.params(**S.l_params(31, True))
    ox = O.Index()
    ox.add_ref(0, "ref", ref, po)
    bases, offs = L.batch(reads)
    want = ox.map_batch(bases, offs, po)
    clean = np.array([" 1%" not in n for n, _ in reads])
    assert (want["mapped"][clean] != 0).all()
    assert np.array_equal(want["rc"][clean] != 0, np.array([" rc" in n for n, _ in reads])[clean])


def test_constructors_name_what_they_give_up_on(O, g):
    with pytest.raises(S.SweepError, match="k = 3"):
        S.deep_read(O, g, 3, 31)
    with pytest.raises(S.SweepError, match="l = 40"):
        S.lc_read(b"ACGT" * 5, 40, False, 1)
