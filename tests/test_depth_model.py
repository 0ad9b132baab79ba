"""CPU: the numpy model of the depth accumulator (tests/depth_model.py) held against a second wording of the same rules -- the difference
array over windows -- and against hand-worked answers, on the crafted cases the GPU tests run through the library.  The tile size is the
library's own (mqdiag_depth_tile_windows), so every test here needs the new symbols."""
import numpy as np
import pytest

import depth_model as DM

WINDOWS = (1, 2, 64, 1000, 4096)


@pytest.fixture(scope="module")
def T():
    import mapquik_amd
    t = int(mapquik_amd.load_library().mqdiag_depth_tile_windows())
    assert t > 0 and t % 64 == 0  # whole steps of a wave
    return t


def test_hand_worked():
    refs = [(0, "a", 10), (3, "b", 7)]
    h = DM.hits_of([(1, 0, 60, 2, 8), (1, 0, 60, 9, 40), (1, 0, 0, 0, 0), (1, 3, 60, 6, 6), (0, 0, 60, 0, 9), (2, 3, 60, 0, 1), (1, 1, 60, 0, 0), (1, 3, 60, 7, 9),
                    (1, 0, 60, 5, 4)])
    recs, wb, ws, tot = DM.model(refs, h, 4, 60)
    # a: windows [0,4) [4,8) [8,10): the hit 2..8 puts 2, 4, 1; the hit 9..40 is clipped to 9..9: 0, 0, 1.  b: [0,4) [4,7): the hit 6..6
    assert wb.tolist() == [2, 4, 2, 0, 1] and ws.tolist() == [1, 0, 1, 0, 1]
    assert tot == dict(offered=9, counted=3, not_mapped=2, below_mapq=1, out_of_range=3)
    assert [tuple(int(x) for x in r) for r in recs] == [(0, 0, 10, 3, 0, 2, 8, 0, 4), (3, 0, 7, 2, 3, 1, 1, 1, 1)]
    recs0, wb0, _, tot0 = DM.model(refs, h, 4, 0)
    assert wb0.tolist() == [3, 4, 2, 0, 1] and tot0["counted"] == 4 and tot0["below_mapq"] == 0 and int(recs0["reads"][0]) == 3


@pytest.mark.parametrize("w", WINDOWS + (5000,))
def test_window_wording_and_totals(T, w):
    refs, hits = DM.crafted(T, w) if w != 5000 else ([(0, "a", 1), (2, "b", 5), (3, "c", 100), (7, "d", 999)], DM.crafted(T, 7)[1])
    for q in (0, 1, 60):
        recs, wb, ws, tot = DM.model(refs, hits, w, q)
        wb2, ws2 = DM.window_wording(refs, hits, w, q)
        assert np.array_equal(wb, wb2) and np.array_equal(ws, ws2), (w, q)
        assert tot["offered"] == hits.size == tot["counted"] + tot["not_mapped"] + tot["below_mapq"] + tot["out_of_range"]
        assert int(recs["reads"].sum()) == tot["counted"] == int(ws.sum())
        assert int(recs["n_windows"].sum()) == wb.size and [int(x) for x in recs["ref_id"]] == sorted(i for i, _, n in refs)
        for r in recs:
            mine = wb[int(r["first_window"]):int(r["first_window"] + r["n_windows"])]
            assert int(mine.sum()) == int(r["bases"]) and int((mine == 0).sum()) == int(r["zero_windows"]) and int(mine.max()) == int(r["max_window_bases"])
        if w != 5000:
            assert tot["not_mapped"] == 3 * len(refs) and tot["out_of_range"] > 7 and (q == 0) == (tot["below_mapq"] == 0)
    if w != 5000:
        assert sorted(n for _, _, n in refs) == sorted({n for n in (1, w - 1, w, w + 1, T * w - 1, T * w, T * w + 1, 2 * T * w + 1) if n >= 1})
    else:
        assert (recs["n_windows"] == 1).all()


def test_carry_case(T):
    refs, hits = DM.carry_case(T, 64)
    recs, wb, ws, tot = DM.model(refs, hits, 64, 60)
    assert np.array_equal(wb, DM.window_wording(refs, hits, 64, 60)[0]) and tot["counted"] == 5
    a, b = recs[0], recs[1]
    assert int(a["n_windows"]) == 3 * T and int(b["first_window"]) == 3 * T
    assert (wb[1:2 * T + 1] >= 64).all() and int(wb[3 * T - 1]) == 2 * 64  # full windows through two tile borders; two hits reach a's last window
    assert (wb[3 * T:4 * T] == 0).all() and int(b["zero_windows"]) == int(b["n_windows"]) - 4  # b's first tile: nothing leaked


def test_formatters_agree_with_the_model_writers():
    from mapquik_amd import api

    class Names:
        def ref_info(self, rid):
            return {0: ("chr1", 2500), 7: ("", 3)}[rid]

    refs = [(0, "chr1", 2500), (7, "", 3)]
    recs = np.array([(0, 0, 2500, 3, 0, 4, 3005, 1, 2005), (7, 0, 3, 1, 3, 1, 2, 0, 2)], dtype=api.ref_depth_dtype)
    wb, ws = np.array([2005, 0, 1000, 2], dtype=np.uint64), np.array([3, 0, 1, 1], dtype=np.uint32)
    assert api.format_depth_bed(Names(), recs, wb, ws, 1000) == DM.bed_bytes(refs, recs, wb, ws, 1000)
    assert api.format_depth_tsv(Names(), recs, 1000) == DM.tsv_bytes(refs, recs, 1000)
