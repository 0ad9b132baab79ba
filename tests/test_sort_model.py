"""CPU: the numpy model of the coordinate sorter (tests/sort_model.py) against a second wording -- Python's sorted on (ref_id, r_start,
ordinal) tuples of the hits the rules keep -- and every crafted case against the property it is named after.  The GPU tests run exactly
these cases through the library."""
import numpy as np
import pytest

import sort_model as SM

T = 2048  # any tile size serves here; the GPU tests ask the library for its own


def _second_wording(refs, hits, ordinals, q):
    live = {int(i) for i, _, n in refs if n > 0}
    kept, tot = [], dict(offered=len(hits), kept=0, not_mapped=0, below_mapq=0, out_of_range=0)
    for h, o in zip(hits.tolist(), np.asarray(ordinals).tolist()):
        status, ref_id, mapq, r_start = h[0], h[1], h[3], h[6]
        if status != 1:
            tot["not_mapped"] += 1
        elif mapq < q:
            tot["below_mapq"] += 1
        elif ref_id not in live:
            tot["out_of_range"] += 1
        else:
            tot["kept"] += 1
            kept.append((ref_id, r_start, o))
    kept.sort()
    return kept, tot


def _check(refs, hits, ordinals, q):
    order, recs, tot = SM.model(refs, hits, ordinals, q)
    kept, tot2 = _second_wording(refs, hits, ordinals, q)
    assert tot == tot2 and tot["offered"] == sum(tot[k] for k in SM.TOTALS[1:])
    assert order.tolist() == [k[2] for k in kept]
    assert recs["ref_id"].tolist() == sorted(int(i) for i, _, n in refs if n > 0)
    for r in recs:
        mine = kept[int(r["first"]):int(r["first"]) + int(r["count"])]
        assert all(k[0] == int(r["ref_id"]) for k in mine) and int(r["count"]) == sum(1 for k in kept if k[0] == int(r["ref_id"]))
    assert SM.passes(refs, hits, ordinals, q) == sum(len({(k[0] << 64 | k[1] << 32 | k[2]) >> (8 * d) & 255 for k in kept}) > 1 for d in range(11))
    return order, recs, tot


def test_model_against_sorted_tuples():
    for n in (0, 1, 65, 3000):
        hits, ords = SM.sized(n)
        _check(SM.REFS, hits, ords, 0)
    hits, ords = SM.filter_case(T)
    for q in (0, 1, 60):
        _, _, tot = _check(SM.REFS, hits, ords, q)
        assert all(tot[k] > 0 for k in SM.TOTALS if q or k != "below_mapq") and (q or tot["below_mapq"] == 0)
    assert SM.model(SM.REFS, hits, ords, 1)[2]["below_mapq"] < SM.model(SM.REFS, hits, ords, 60)[2]["below_mapq"]


def test_border_counts_and_runs():
    c = SM.border_counts(T)
    assert c[:5] == [0, 1, 63, 64, 65] and c[5:9] == [T - 1, T, T + 1, 2 * T + 1] and -(-c[9] // T) > SM.SCAN_THREADS and c[9] <= 1 << 20
    assert SM.runs([]) == [] and SM.runs([5, 6, 7, 9, 3, 4]) == [(0, 3), (3, 4), (4, 6)]


@pytest.mark.parametrize("d", range(11))
def test_digit_cases_differ_in_one_digit_only(d):
    refs, hits, ords = SM.digit_case(d)
    dg = SM.digits(hits["ref_id"], hits["r_start"], ords)
    for j in range(11):
        assert np.unique(dg[j]).size == (256 if j == d else 1), (d, j)
    assert SM.passes(refs, hits, ords, 0) == 1 and SM.classify(refs, hits, 0).sum() == 0
    order, recs, tot = _check(refs, hits, ords, 0)
    assert tot["kept"] == 256
    if d < 4:
        assert int(ords.max()) <= (1 << 32) - 2 and (d != 3 or int(ords.max()) == (1 << 32) - 2)
    if d >= 8:
        assert max(i for i, _, _ in refs) == (1 << 24) - 1 and int((recs["count"] == 1).sum()) == 256
    if d < 4:
        assert not np.array_equal(order, ords)  # (shuffled: the sort has something to do)
    else:
        refs, hits, ords = SM.digit_case(d, tagged=True)
        order, _, _ = _check(refs, hits, ords, 0)
        assert SM.passes(refs, hits, ords, 0) == 2 and not np.array_equal(order, ords) and not np.array_equal(order, np.sort(ords))


def test_stability_cases():
    cases, ords = SM.stability_cases(T)
    n = ords.size
    assert n == 3 * T + 17
    for name, hits in cases.items():
        order, _, tot = _check(SM.REFS, hits, ords, 0)
        assert tot["kept"] == n, name
    assert SM.model(SM.REFS, cases["all_keys_equal"], ords, 0)[0].tolist() == list(range(n))
    two = SM.model(SM.REFS, cases["two_keys_lane_by_lane"], ords, 0)[0]
    assert two[:(n + 1) // 2].tolist() == list(range(0, n, 2)) and two[(n + 1) // 2:].tolist() == list(range(1, n, 2))
    assert np.unique(cases["one_bin_but_low_byte"]["r_start"] & 255).size == 1 and np.unique(cases["one_per_bin"]["r_start"][:256]).size == 256
    assert SM.model(SM.REFS, cases["sorted"], ords, 0)[0].tolist() == list(range(n))
    assert SM.model(SM.REFS, cases["reversed"], ords, 0)[0].tolist() == list(range(n))[::-1]


def test_sorted_files_of_a_paf():
    refs = [(0, "one", 5000), (1, "two", 3001), (5, "", 7)]
    rows = [("r0", "two", 40), ("r1", "one", 900), ("r2", "one", 40), ("r3", "two", 40), ("r4", "one", 40)]
    paf = "".join("%s\t100\t0\t100\t+\t%s\t9\t%d\t%d\t1\t1\t%d\n" % (q, r, s, s + 100, 60 if q != "r3" else 0) for q, r, s in rows).encode()
    sp, tsv, recs, tot = SM.sorted_files(refs, paf, 0)
    assert [ln.split(b"\t")[0] for ln in sp.splitlines()] == [b"r2", b"r4", b"r1", b"r0", b"r3"]
    two_at = sum(len(ln) for ln in sp.splitlines(keepends=True)[:3])
    assert sp[two_at:].startswith(b"r0\t") and tsv.decode() == SM.TSV_HEAD + "one\t5000\t3\t0\t0\ntwo\t3001\t2\t3\t%d\n\t7\t0\t5\t%d\n" % (two_at, len(sp))
    sp60, _, _, tot60 = SM.sorted_files(refs, paf, 60)
    assert sp60.count(b"\n") == 4 and tot60["below_mapq"] == 1
    assert SM.log_line(recs, tot, 0) == "Sorted: 5 of 5 hits kept (0 not mapped, 0 below mapq 0, 0 out of range): 5 lines on 2 references"
