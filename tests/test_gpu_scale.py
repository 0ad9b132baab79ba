"""GPU: the result passes of mq_depth and mq_index_coverage beyond 1,024 tiles and 4,096 reference ids, on the cases of
tests/scale_cases.py (proved to have their properties on the CPU, tests/test_scale_cases.py) against the models of tests/depth_model.py
and tests/coverage_model.py; every comparison is integer equality, field by field (the `_same` of test_gpu_depth.py and of
test_gpu_index_coverage.py).  The one-workgroup scans (depth_scan_kernel, cover_scan_kernel) give each of their 1,024 threads
per = ceil(n_tiles / 1024) consecutive tiles: 1,024, 1,025, 2,049 and 3,079 tiles are per = 1, 2, 3 and 4.  The cases are built for the
library's own tile sizes and every test asserts the tile count it was built for, so a change of a tile constant fails here and does not
drop the suite back to per == 1.

Wall time on an MI355X, first run (a record, not a bound): the slowest test, test_depth_scan_at[1024-one_reference-1], took 0.27 s --
it builds the case, both models and the index, fills four accumulators and takes eight results; the largest case
(test_depth_scan_at[3079-one_tile_each-1]) took 0.22 s, no coverage case more than 0.07 s, the 27 tests of the module 2.8 s together.
Every test passed on that run with the kernels as they were.  Held once against a library whose two scans added `tile_sum[lo]`
instead of `tile_sum[i]` (wrong from the third tile of a thread's range on), every depth case with tiles that sum to non-zero and
every coverage case failed at 2,049 and 3,079 tiles, and none below."""
import numpy as np
import pytest

import coverage_model as CM
import depth_model as DM
import hipmem
import scale_cases as S
from test_gpu_depth import _index
from test_gpu_depth import _same as _same_depth
from test_gpu_index_coverage import _same as _same_coverage
from test_gpu_parity import mq  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
GEOMETRIES = ("one_reference", "one_tile_each", "mixed")
HIT_BYTES = 48


@pytest.fixture(scope="module")
def depth_T(mq):
    t = int(mq.load_library().mqdiag_depth_tile_windows())
    assert t > 0 and t % 64 == 0
    return t


@pytest.fixture(scope="module")
def cover_T(mq):
    t = int(mq.load_library().mqdiag_coverage_tile_bits())
    assert t % (64 * 128) == 0
    return t


@pytest.fixture(scope="module")
def depth_cases(depth_T):
    """(geometry, n, w) -> (refs, hits, {min_mapq: model}): every case and every model computed once"""
    memo = {}

    def get(g, n, w):
        if (g, n, w) not in memo:
            refs = S.DEPTH[g](n, depth_T, w)
            assert S.tiles_of(refs, w, depth_T)[0] == n, (g, n, w, "the case no longer has the tile count it was built for")
            hits = S.depth_hits(refs, depth_T, w, seed=n + w)
            memo[(g, n, w)] = (refs, hits, {q: DM.model(refs, hits, w, q) for q in (0, 60)})
        return memo[(g, n, w)]

    return get


@pytest.fixture(scope="module")
def cover_cases(cover_T):
    """(geometry, n) -> (case, model), computed once"""
    memo = {}

    def get(g, n):
        if (g, n) not in memo:
            c = S.COVERAGE[g](n, cover_T)
            assert S.tiles_of(c.refs, 1, cover_T)[0] == n, (g, n, "the case no longer has the tile count it was built for")
            memo[(g, n)] = (c, CM.model(c.slots, c.refs))
        return memo[(g, n)]

    return get


def _equal(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


@pytest.mark.parametrize("n,geometry,w", [(n, g, 1) for n in S.TILE_COUNTS for g in GEOMETRIES] + [(2049, "mixed", 3)])
def test_depth_scan_at(mq, depth_cases, tmp_path, n, geometry, w):
    """the host route in one call and the device route in three uneven pieces, at min_mapq 0 and 60; a second result() of the same
    accumulator is the first one: the result pass changes no accumulator"""
    assert S.per_of(n) == {1024: 1, 1025: 2, 2049: 3, 3079: 4}[n]
    refs, hits, want = depth_cases(geometry, n, w)
    ix = _index(mq, refs, tmp_path / "s.mqx")
    buf = hipmem.DevBuf.from_numpy(hits)
    cuts = (0, 1, 1 + 64 * 77 + 13, hits.size)
    for q in (0, 60):
        host, dev = mq.api.Depth(ix, window=w, min_mapq=q), mq.api.Depth(ix, window=w, min_mapq=q)
        host.add(hits)
        for a, b in zip(cuts, cuts[1:]):
            dev.add_device(buf.ptr + a * HIT_BYTES, b - a)
        tag = "%s n=%d w=%d q=%d" % (geometry, n, w, q)
        got = host.result()
        _same_depth(got, want[q], "host " + tag)
        _same_depth(dev.result(), want[q], "device " + tag)
        for d in (host, dev):
            again = d.result()
            _same_depth(again, want[q], "a second result, " + tag)
            assert _equal(again, got)
            d.close()
    buf.free()
    ix.close()


def test_depth_many_ids(mq, depth_T, tmp_path):
    """n_ids > 4096: reads are counted per reference with global atomics -- one hit on each of 1,025 references, and 50,000 identical
    ones on the reference with the largest id"""
    refs = S.depth_one_tile_each(1025, depth_T, 1)
    assert S.tiles_of(refs, 1, depth_T)[0] == 1025 and max(i for i, _, _ in refs) + 1 > 4096
    hits = S.many_ids_hits(refs, 1)
    want = DM.model(refs, hits, 1, 60)
    ix = _index(mq, refs, tmp_path / "m.mqx")
    host, dev = mq.api.Depth(ix, window=1, min_mapq=60), mq.api.Depth(ix, window=1, min_mapq=60)
    host.add(hits)
    buf = hipmem.DevBuf.from_numpy(hits)
    dev.add_device(buf.ptr, hits.size)
    for name, d in (("host", host), ("device", dev)):
        got = d.result()
        assert np.array_equal(got[0]["reads"], want[0]["reads"]), (name, got[0]["reads"][-4:], want[0]["reads"][-4:])
        assert int(got[0]["reads"][-1]) == 50001 and got[3]["counted"] == hits.size
        _same_depth(got, want, name + ", many ids")
        d.close()
    buf.free()
    ix.close()


def _coverage_of(mq, path, want, tag, **how):
    ix = mq.Index.load(path, **how)
    try:
        if how:
            assert ix.stats()["table_slots"] == how["table_slots"]
        _same_coverage(ix.coverage(), want, tag)
    finally:
        ix.close()


@pytest.mark.parametrize("n", S.TILE_COUNTS)
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_coverage_scan_at(mq, cover_cases, tmp_path, n, geometry):
    assert S.per_of(n) == {1024: 1, 1025: 2, 2049: 3, 3079: 4}[n]
    c, want = cover_cases(geometry, n)
    path = c.write(tmp_path / "s.mqx")
    _coverage_of(mq, path, want, c.name)
    if n == 2049:  # the mark kernel streams a table of another size
        _coverage_of(mq, path, want, c.name + " (load_sized)", table_slots=4 * max(c.table_slots, 2))


def test_coverage_comb(mq, cover_T, tmp_path):
    """32 runs per word and 4,096 per step of a wave across a tile border, and the same across a step border inside tile 0"""
    c = S.cover_comb(cover_T)
    want = CM.model(c.slots, c.refs)
    assert want[1].size == 4096 + 64 and S.tiles_of(c.refs, 1, cover_T)[0] == 3
    _coverage_of(mq, c.write(tmp_path / "comb.mqx"), want, c.name)
