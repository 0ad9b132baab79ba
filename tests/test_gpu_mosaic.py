"""GPU: the chain side of the HIP path on mosaic reads (tests/mosaic.py), product instantiation only: no test hook is set here, the
kernels are the ones a user runs (map_kernel<64, ...>, chain_stage<64>, the default scratch of 2048 Match records and its overflow redo).

Every read set of test_mosaic_cases.py -- the five generated legs, the gap ladders at each g, the n-way ties and near-ties, the reads
whose winner is first seen in a later 64-lane chunk -- is mapped under eight parameter sets and compared with the CPU oracle column by
column (all 64 bits of columns 3 and 4), k-min-mer counts included; then the PAF text, the device-resident form on a poisoned result
buffer, two contexts at once, spans with case folding, the opt-in tuple hash and a seeding variant, and mosaic reads mixed into a
large batch of ordinary reads."""
import numpy as np
import pytest

import mosaic as M

pytestmark = pytest.mark.gpu

PARAM_SETS = {
    "default": dict(),
    "k3": dict(k=3, l=15, density=0.03, c=2, s=5, g=500),
    "k1": dict(k=1, l=15, density=0.05),
    "k12": dict(k=12, l=12, density=0.1, g=0),
    "k32": dict(k=32, l=8, density=0.2),  # mapping at the largest k
    "c0": dict(c=0),                      # the `s != 0 && c != 0` arm of the mapq rule
    "s0": dict(s=0),
    "nohpc": dict(use_hpc=False),
}


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture(scope="module")
def world(oracle, simlib):
    return M.world(oracle, simlib)


def _index_both(mq, oracle, world, ps, **kw):
    g, off, names, _ = world
    P, po = mq.Params(**ps, **kw), oracle.params(**ps)
    ix, ox = mq.Index(P), oracle.Index()
    cnt = ox.build_mt(g, off, names, po, 8)
    for r in range(off.size - 1):
        assert ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])]) == int(cnt[r])
    assert ix.finalize() == ox.count()
    return ix, ox, po


def _same(mq, got, want, diag, tag):
    """status exactly, every numeric PAF column (high words of columns 3 and 4 too) and the k-min-mer count of every read"""
    m = want["mapped"] != 0
    assert np.array_equal(got["status"], m.astype(np.uint32)), (tag, "status", np.flatnonzero(got["status"] != m)[:10].tolist())
    assert np.array_equal(got["n_kminmers"].astype(np.uint64), diag["n_kminmers"].astype(np.uint64)), (tag, "n_kminmers")
    for f in ("ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score"):
        a, b = mq.hit_column(got, f)[m], want[f][m].astype(np.uint64)
        assert np.array_equal(a, b), (tag, f, np.flatnonzero(m)[np.flatnonzero(a != b)[:10]].tolist())


def _set_params(ps, st, name):
    """the parameter set, with the g of a gap ladder's own"""
    ps = dict(ps)
    if name.startswith("gap_"):
        ps["g"] = st["ps"]["g"]
    return ps


@pytest.mark.parametrize("pname", list(PARAM_SETS))
def test_every_mosaic_set_matches_the_oracle(mq, oracle, world, pname):
    ps0 = PARAM_SETS[pname]
    ix, ox, _ = _index_both(mq, oracle, world, ps0)
    tot = dict(reads=0, matches=0, cand=0, over_cap=0, max_m=0, max_c=0, ties=0)
    for name, st in world[3].items():
        ps = _set_params(ps0, st, name)
        po = oracle.params(**ps)
        ix.set_map_params(po.c, po.s, po.g)
        want, diag = ox.map_batch_diag(st["bases"], st["offs"], po, threads=16)
        got = ix.map_batch(st["bases"], st["offs"])
        _same(mq, got, want, diag, (pname, name))
        tot["reads"] += want.size
        tot["matches"] += int(diag["n_matches"].sum())
        tot["cand"] += int(diag["n_candidates"].sum())
        tot["over_cap"] += int((diag["n_matches"] > 2048).sum())
        tot["ties"] += int((diag["tie"] != 0).sum())
        tot["max_m"] = max(tot["max_m"], int(diag["n_matches"].max()))
        tot["max_c"] = max(tot["max_c"], int(diag["n_candidates"].max()))
    print("mosaic parity [%s]: %s" % (pname, tot))
    assert tot["reads"] >= 3000 and tot["matches"] > 0


@pytest.mark.parametrize("leg", ["default", "k1"])
def test_paf_text_identical(mq, oracle, world, leg):
    st = world[3][leg]
    ix, ox, po = _index_both(mq, oracle, world, st["ps"])
    want = ox.map_batch(st["bases"], st["offs"], po, threads=16)
    got = ix.map_batch(st["bases"], st["offs"])
    rn = ["mosaic_%s_%d" % (leg, i) for i in range(want.size)]
    a, b = ix.paf_lines(rn, st["offs"], got), oracle.paf_lines(ox, rn, want)
    assert a == b and len(a) >= want.size // 2


@pytest.mark.parametrize("leg", ["default", "k3", "k1", "k12", "late", "tie_65"])
def test_device_resident_form_on_a_poisoned_buffer(mq, oracle, world, leg):
    """The device-resident entry point into a result buffer filled with 0xFF: every record is written.  A read comes back
    MQ_HIT_OVERFLOW when it has more Match runs than the scratch holds (2048) OR when its minimizer list is denser than its region and
    the pool allow -- the second clause cannot be told from the oracle's counters, so this asserts
        overflow  contains  {n_matches > 2048},   and every record that is not overflow equals the oracle's,
    not equality of the two sets.  On the legs other than k = 1 no read has 2048 runs and the lists are sparse: no overflow at all is
    expected there, and that IS asserted exactly."""
    from test_gpu_poison import _assert_all_written, _launch_poisoned
    st = world[3][leg]
    ix, ox, po = _index_both(mq, oracle, world, st["ps"])
    want, diag = ox.map_batch_diag(st["bases"], st["offs"], po, threads=16)
    got = _launch_poisoned(mq, ix, st["bases"], st["offs"])
    _assert_all_written(got)
    over = got["status"] == mq.MQ_HIT_OVERFLOW
    must = diag["n_matches"] > 2048
    assert (over[must]).all(), np.flatnonzero(must & ~over)[:10].tolist()
    if leg == "k1":
        assert must.sum() >= 20
        print("k=1 leg, device form: %d overflow records, %d reads over 2048 Matches" % (int(over.sum()), int(must.sum())))
    else:
        assert not over.any()
    ok = np.flatnonzero(~over)
    _same(mq, got[ok], want[ok], diag[ok], ("device", leg))


def test_two_contexts_at_once_and_spans_with_case_folding(mq, oracle, world):
    st = world[3]["k3"]
    ix, ox, po = _index_both(mq, oracle, world, st["ps"], fold_case=True)
    bases, offs = st["bases"], st["offs"]
    want, diag = ox.map_batch_diag(bases, offs, po, threads=16)
    c1, c2 = ix.context(), ix.context()
    half = (offs.size - 1) // 2
    b2, o2 = M.select(bases, offs, range(half, offs.size - 1))
    c1.submit(bases, offs)
    c2.submit(b2, o2)
    h1, h2 = c1.wait(), c2.wait()
    _same(mq, h1, want, diag, "ctx1")
    _same(mq, h2, want[half:], diag[half:], "ctx2")
    low = bases.copy()
    low |= 0x20
    starts, lens = offs[:-1].copy(), np.diff(offs.astype(np.int64)).astype(np.uint32)
    c1.submit_spans(low, starts, lens)
    c2.submit(bases, offs)
    h3, h4 = c1.wait(), c2.wait()
    _same(mq, h3, want, diag, "spans, lower case")
    _same(mq, h4, want, diag, "ctx2 again")
    c1.close()
    c2.close()


def test_default_leg_with_fast_tuple_hash_and_a_seeding_variant(mq, oracle, world):
    st = world[3]["default"]
    for variant, fast_kh in ((0, True), (4, False)):
        oracle.lib().mqo_set_variant(variant | (64 if fast_kh else 0))
        try:
            ix, ox, po = _index_both(mq, oracle, world, st["ps"], seeding_variant=variant, fast_kh=fast_kh)
            want, diag = ox.map_batch_diag(st["bases"], st["offs"], po, threads=16)
            _same(mq, ix.map_batch(st["bases"], st["offs"]), want, diag, (variant, fast_kh))
        finally:
            oracle.lib().mqo_set_variant(0)


def test_mosaic_reads_among_ordinary_reads(mq, oracle, simlib, world):
    """2,000 mosaic reads (short ones, so that the batch stays small) scattered over 20,000 ordinary reads: heavy reads share waves with
    ordinary ones, and the launch-order pass may move reads."""
    g, off, names, _ = world
    rng = np.random.default_rng(515)
    mb, mo, _ = M.mosaic_reads(g, off, rng, 2000, 120, (300, 2000), 0.5, M.DEFAULT_DELTAS)
    plain = simlib.make_reads(g, off, 20000, seed=6, len_mean=3000, len_sd=1500, len_min=50, len_max=9000, err=0.01)
    pb, po_ = plain["bases"], plain["offsets"]
    seqs = [mb[int(mo[i]):int(mo[i + 1])] for i in range(2000)] + [pb[int(po_[i]):int(po_[i + 1])] for i in range(20000)]
    order = rng.permutation(len(seqs))
    bases, offs = M.concat([seqs[int(i)] for i in order])
    ix, ox, po = _index_both(mq, oracle, world, dict())
    want, diag = ox.map_batch_diag(bases, offs, po, threads=16)
    got = ix.map_batch(bases, offs)
    _same(mq, got, want, diag, "mixed batch")
    ix.last_map_order()  # (the call works after such a launch; what it moved is the launch-order tests' subject)
    is_mosaic = order < 2000
    assert (diag["n_candidates"][is_mosaic] > 4).sum() >= 500 and (diag["n_candidates"][~is_mosaic] > 4).sum() == 0
