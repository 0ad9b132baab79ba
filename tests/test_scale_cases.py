"""CPU: every case of tests/scale_cases.py has the property it is named after -- the tile count it was built for, per = 1, 2, 3 and 4
tiles per scan thread, id ranges beyond the workgroup histograms, tiles whose difference array sums below zero, running counts that are
not zero where one thread's range ends, references that begin inside a thread's range, the run of more than 1,024 whole tiles -- and
the two models agree with their second wordings on them.  The tile size is a parameter: the library's own today (256 windows, 65,536
bits), and a smaller one once, so that the builders are shown to follow it.  Nothing here touches the library."""
import numpy as np
import pytest

import coverage_model as CM
import depth_model as DM
import scale_cases as S
from test_coverage_model import _check_against_brute

DEPTH_T, COVER_T = 256, 65536
SMALL_DEPTH_T, SMALL_COVER_T = 64, 128 * 64
GEOMETRIES = ("one_reference", "one_tile_each", "mixed")
_memo = {}


def _depth(g, n, T, w):
    """(refs, hits, the grouped wording at mapq >= 60): built once"""
    key = (g, n, T, w)
    if key not in _memo:
        refs = S.DEPTH[g](n, T, w)
        hits = S.depth_hits(refs, T, w, seed=n + w)
        _memo[key] = (refs, hits, S.grouped_wording(refs, hits, w, 60))
    return _memo[key]


def test_tile_counts_and_per():
    assert [S.per_of(n) for n in S.TILE_COUNTS] == [1, 2, 3, 4] and S.SCAN == 1024
    assert S.boundaries(1025) == list(range(2, 1025, 2)) and S.boundaries(2049)[-1] == 2046 and len(S.boundaries(1024)) == 1023
    for T, CT in ((DEPTH_T, COVER_T), (SMALL_DEPTH_T, SMALL_COVER_T)):
        for n in S.TILE_COUNTS:
            for g in GEOMETRIES:
                for w in (1, 3):
                    refs = S.DEPTH[g](n, T, w)
                    got, tl = S.tiles_of(refs, w, T)
                    assert got == n == tl.shape[0], (g, n, T, w, got)
                    if w > 1 and g == "one_tile_each":
                        assert all(ln % w for _, ln in S.live_refs(refs))
                if T == DEPTH_T or n == 1025:
                    c = S.COVERAGE[g](n, CT)
                    assert S.tiles_of(c.refs, 1, CT)[0] == n, (g, n, CT)
    # tiles_of by hand: 2 and 1 tiles; the reference of length 0 does not exist
    n, tl = S.tiles_of([(7, "b", 10), (3, "a", 1000), (5, "z", 0)], 3, 256)
    assert n == 3 and tl.tolist() == [[0, 0], [0, 1], [1, 0]]
    assert S.tiles_of([], 1, 64)[0] == 0


def test_geometries():
    for T in (DEPTH_T, SMALL_DEPTH_T):
        for n in S.TILE_COUNTS:
            one = S.depth_one_reference(n, T, 1)
            assert len(one) == 1 and S.tiles_of(one, 1, T)[0] == n and (one[0][2] % T) not in (0, 1)  # the last tile is short
            each = S.live_refs(S.depth_one_tile_each(n, T, 1))
            assert len(each) == n > 1000 and each[-1][0] + 1 > 4096 and [i for i, _ in each] == [5 * c + 2 for c in range(n)]
            assert sorted({ln for _, ln in each}) == sorted({min(c, T) for c in (1, 63, 64, 65, T - 1, T)})
            zero = [i for i, _, ln in S.depth_one_tile_each(n, T, 1) if ln == 0]
            assert len(zero) == n // 2 and all(i % 10 == 9 for i in zero)  # 5 c + 4 at the odd c: every second gap
            _, tl = S.tiles_of(S.depth_mixed(n, T, 1), 1, T)
            sizes = np.bincount(tl[:, 0])
            assert sizes[:8].tolist() == [1, 2, 3, 5, 1, 2, 3, 5] and set(sizes[:-1].tolist()) == {1, 2, 3, 5}
    for T in (COVER_T, SMALL_COVER_T):
        each = S.cover_one_tile_each(1025, T)
        assert len(each.refs) == 1025 and max(i for i, _, _ in each.refs) + 1 > 4096
        assert [ln for _, _, ln in each.refs[:6]] == [1, 63, 64, 65, 128, 200]
        mixed = S.cover_mixed(1025, T)
        assert [ln for _, _, ln in mixed.refs[:5]] == [T - 1, T, T + 1, 2 * T + 65, 64]
        assert S.cover_one_reference(1025, T).refs[0][2] == 1025 * T - 100


@pytest.mark.parametrize("T", (DEPTH_T, SMALL_DEPTH_T))
@pytest.mark.parametrize("g", GEOMETRIES)
def test_depth_cases_have_their_properties(T, g):
    for n in S.TILE_COUNTS if T == DEPTH_T else (1025,):
        refs, hits, (wb, ws, diff, first) = _depth(g, n, T, 1)
        per, live = S.per_of(n), S.live_refs(refs)
        assert 19000 < hits.size < 21000
        _, tl = S.tiles_of(refs, 1, T)
        nws = np.array([ln for _, ln in live])
        tile_first = first[tl[:, 0]] + tl[:, 1] * T
        for q in (0, 60):  # the model's tallies (its classify): every counter moves, and about 3 % are turned away whatever the mapq
            cls = DM.classify(refs, hits, q)[0]
            not_mapped, below_mapq, out_of_range = (int((cls == k).sum()) for k in (1, 2, 3))
            assert not_mapped > 50 and out_of_range > 100 and (below_mapq > 1000 if q else below_mapq == 0), (g, n, q)
            assert 0.01 * hits.size < not_mapped + out_of_range < 0.05 * hits.size
        if n < 1025:
            continue
        sums = np.add.reduceat(diff, tile_first)
        # (a reference's difference array sums to 0, so where every reference is one tile no tile can sum below zero: there the +1 / -1
        # pairs stay inside the tiles, and the scan must hand every tile a zero)
        assert ((sums < 0).any() if g != "one_tile_each" else (not sums.any() and (diff < 0).sum() > 100)) and int(diff.sum()) == 0, (g, n)
        running = np.cumsum(diff)
        inside = [b for b in S.boundaries(n) if tl[b, 1] > 0]
        carried = sum(1 for b in inside if running[tile_first[b] - 1] != 0)
        assert 2 * carried >= len(inside) and (g == "one_tile_each") == (not inside), (g, n, carried, len(inside))
        if g != "one_tile_each":
            assert len(inside) > 100
        if g != "one_reference":
            begins = np.flatnonzero(tl[:, 1] == 0)
            assert int((begins % per != 0).sum()) >= 100, (g, n)
        quiet = S.quiet_successors(refs, 1, T)
        assert (len(quiet) >= 8) == (g != "one_reference")
        for k in quiet:
            assert wb[first[k]] == 0 and ws[first[k]] == 0 and wb[first[k] - 1] > 0 and first[k] - 1 == first[k - 1] + nws[k - 1] - 1
            assert not wb[first[k]:first[k] + min(T, nws[k])].any()


def test_depth_deterministic_hits():
    """the hits that carry the count through every thread range, and the ones on the chosen boundaries, are among the records"""
    T, n = DEPTH_T, 2049
    refs, hits, _ = _depth("one_reference", n, T, 1)
    ln = refs[0][2]
    on = hits[(hits["status"] == 1) & (hits["ref_id"] == 1)]
    have = {(int(a), int(b)) for a, b in zip(on["r_start"], on["r_end"])}
    assert (0, ln - 1) in have and (0, 0xFFFFFFFF) in have and (T // 2, (n - 1) * T + 1) in have
    chosen = S.chosen_boundaries(n)
    assert len(chosen) == 3 and chosen[0] == 3 and chosen[-1] == 2046 and all(b % S.per_of(n) == 0 for b in chosen)
    for b in chosen:
        g = b * T
        assert {(g - 1, g), (g - 3, g + 3), (g - 6, g - 1), (g, g + 4)} <= have, b


@pytest.mark.parametrize("w", (1, 3))
@pytest.mark.parametrize("g", GEOMETRIES)
def test_depth_model_against_its_wordings(g, w):
    for T, counts in ((DEPTH_T, S.TILE_COUNTS), (SMALL_DEPTH_T, (1025,))):
        for n in counts:
            refs, hits, (gb, gs, _, _) = _depth(g, n, T, w)
            recs, wb, ws, tot = DM.model(refs, hits, w, 60)
            wb2, ws2 = DM.window_wording(refs, hits, w, 60)
            assert np.array_equal(wb, wb2) and np.array_equal(ws, ws2), (g, n, w)
            assert np.array_equal(wb, gb) and np.array_equal(ws, gs), (g, n, w, "grouped")
            assert tot["offered"] == hits.size == sum(tot[k] for k in DM.TOTALS[1:]) and int(recs["reads"].sum()) == tot["counted"]


def test_depth_many_ids():
    refs = S.depth_one_tile_each(1025, DEPTH_T, 1)
    hits = S.many_ids_hits(refs, 1)
    recs, wb, ws, tot = DM.model(refs, hits, 1, 60)
    assert hits.size == 1025 + 50000 == tot["counted"] and recs["reads"][:-1].tolist() == [1] * 1024 and int(recs["reads"][-1]) == 50001
    assert int(recs["ref_id"][-1]) + 1 > 4096 and np.array_equal(wb, S.grouped_wording(refs, hits, 1, 60)[0])


# ------------------------------------------------------------------ coverage
def _ivs(res):
    return [(int(v["start"]), int(v["end"])) for v in res[1]]


@pytest.mark.parametrize("T", (COVER_T, SMALL_COVER_T))
def test_coverage_against_per_base_array(T):
    """(one_reference: 67 MB of booleans at 1,025 tiles of 65,536 bits -- once)"""
    for c in (S.cover_comb(T), S.cover_one_tile_each(1025, T), S.cover_mixed(1025, T), S.cover_one_reference(1025, T)):
        _check_against_brute(c)


@pytest.mark.parametrize("T", (COVER_T, SMALL_COVER_T))
def test_coverage_cases_have_their_properties(T):
    comb = _ivs(CM.model(S.cover_comb(T).slots, S.cover_comb(T).refs))
    inner = 64 if T >= 4 * S.STEP else 0
    assert len(comb) == 4096 + inner and all(b - a == 1 for a, b in comb) and (T == SMALL_COVER_T or inner == 64)
    assert comb[inner][0] == T - 4096 and comb[-1][0] == T + 4094 and (not inner or (comb[0][0], comb[inner - 1][0]) == (S.STEP - 63, S.STEP + 63))
    for n in S.TILE_COUNTS if T == COVER_T else (1025, 2049):
        # one_reference: the long run is one interval of the model
        c = S.cover_one_reference(n, T)
        recs, ivs, oor = CM.model(c.slots, c.refs)
        t0, whole = S.cover_long_run(n, T)
        assert 19000 < c.slots.size < 21000 and oor == 4 and int((c.slots["count"] == 2).sum()) == 300
        long = [(a, b) for a, b in _ivs((recs, ivs, oor)) if a <= (t0 + 1) * T and b >= (t0 + 1 + whole) * T]
        assert len(long) == 1 and t0 * T < long[0][0] < (t0 + 1) * T and (t0 + 1 + whole) * T < long[0][1] < (t0 + 2 + whole) * T
        assert (whole > S.SCAN) == (n >= 2049) and whole >= min(n // 2, S.SCAN + 1) and int(ivs["end"][-1]) == c.refs[0][2] and ivs.size > 5000
        starts = np.bincount(ivs["start"] // T, minlength=n)
        assert not starts[t0 + 1:t0 + 1 + whole].any() and (starts > 0).sum() > (n - whole) // 2
        assert ((c.slots["end"].astype(np.int64) - c.slots["start"].astype(np.int64)) < T).all()  # no entry longer than a tile
        # one_tile_each
        c = S.cover_one_tile_each(n, T)
        recs, ivs, oor = CM.model(c.slots, c.refs)
        assert recs.size == n and int(recs["ref_id"][-1]) + 1 > 4096 and abs(int((recs["live_kminmers"] == 0).sum()) - n / 3) < 4
        assert set(recs["live_kminmers"].tolist()) == {0, 1, 2, 3}
        for r in recs[recs["live_kminmers"] > 0]:
            mine = ivs[int(r["first_interval"]):int(r["first_interval"]) + int(r["n_intervals"])]
            if int(r["len"]) % 64 == 0:
                assert int(mine[-1]["end"]) == int(r["len"])
            if int(r["len"]) == 1:
                assert int(r["covered_bases"]) == 1
        for ln in S.COVER_LENGTHS:
            assert {0, 1} <= set((recs["live_kminmers"][recs["len"] == ln] > 0).tolist())
        # mixed
        c = S.cover_mixed(n, T)
        recs, ivs, oor = CM.model(c.slots, c.refs)
        assert oor > 50 and (recs["n_intervals"] >= 1).all() and int(recs["ref_id"][-1]) + 1 <= 4096
        for r in recs[:40]:
            mine = _ivs((None, ivs[int(r["first_interval"]):int(r["first_interval"]) + int(r["n_intervals"])]))
            ln = int(r["len"])
            assert mine[0][0] == 0 and mine[-1][1] == ln
            for j in range(1, -(-ln // T)):
                assert any(a < j * T < b for a, b in mine), (ln, j)
        _, tl = S.tiles_of(c.refs, 1, T)
        if n >= 1025:
            assert int((np.flatnonzero(tl[:, 1] == 0) % S.per_of(n) != 0).sum()) >= 100
