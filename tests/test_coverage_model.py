"""CPU: the coverage model (tests/coverage_model.py) against a per-base boolean array on every crafted case, each case's named property,
and the model against the oracle's own map on small contigs.  Nothing here touches the library."""
import numpy as np
import pytest

import coverage_model as CM
import extend_data as X
import merge_data as M
import mqx

TILES = (8192, 65536)


@pytest.fixture(scope="module")
def src(oracle, simlib):
    return mqx.source(oracle, simlib, "small")


def _check_against_brute(c):
    recs, ivs, oor = CM.model(c.slots, c.refs)
    cov, n_live = CM.brute(c.slots, c.refs)
    assert [int(r) for r in recs["ref_id"]] == sorted(cov), c.name
    at = 0
    for r in recs:
        rid = int(r["ref_id"])
        runs = CM.runs_of(cov[rid])
        assert int(r["first_interval"]) == at and int(r["n_intervals"]) == len(runs), c.name
        assert [(int(v["start"]), int(v["end"])) for v in ivs[at:at + len(runs)]] == runs, c.name
        assert int(r["covered_bases"]) == int(cov[rid].sum()) and int(r["live_kminmers"]) == n_live[rid] and int(r["len"]) == cov[rid].size, c.name
        at += len(runs)
    assert at == ivs.size
    live = (c.slots["count"] == 1) & (c.slots["end"] != 0)
    assert oor == int(live.sum()) - sum(n_live.values()), c.name
    return recs, ivs, oor


@pytest.mark.parametrize("T", TILES)
def test_model_against_per_base_array(T, src):
    cases = CM.crafted_cases(T, src)
    assert len({c.name for c in cases}) == len(cases) >= 40
    for c in cases:
        _check_against_brute(c)


@pytest.mark.parametrize("T", TILES)
def test_cases_have_their_properties(T, src):
    by = {c.name: c for c in CM.crafted_cases(T, src)}
    res = {n: CM.model(c.slots, c.refs) for n, c in by.items()}
    iv = lambda n: [(int(v["start"]), int(v["end"])) for v in res[n][1]]  # noqa: E731
    big = 2 * T + 65
    # reference lengths: all nine, each covered at base 0 and at its last base
    recs, ivs, oor = res["reference lengths"]
    assert [int(x) for x in recs["len"]] == list(CM.LENGTHS(T)) and oor == 0
    for r in recs:
        mine = ivs[int(r["first_interval"]):int(r["first_interval"]) + int(r["n_intervals"])]
        assert int(mine[0]["start"]) == 0 and int(mine[-1]["end"]) == int(r["len"])
    assert int(recs["covered_bases"][0]) == 1  # (length 1: covered by a clamped entry only)
    assert iv("start == end") == [(5, 6), (700, 701)] and iv("[1, 1]") == [(1, 2)]
    assert iv("words apart") == [(0, 64), (63, 65), (64, 128)] and [int(x) for x in res["words apart"][0]["n_intervals"]] == [1, 1, 1]
    assert iv("adjacent") == [(0, 128)]
    assert iv("adjacent without overlap") == [(0, 129), (130, 141)]
    assert iv("inside one word") == [(70, 91)] and 70 // 64 == 90 // 64
    assert iv("three words") == [(60, 131)] and 130 // 64 - 60 // 64 == 2
    assert iv("more than a tile") == [(10, T + 101)] and T + 101 - 10 > T
    assert iv("ends on T - 1") == [(T - 50, T)] and iv("starts on T") == [(T, T + 31)]
    assert iv("ends on T - 1, starts on T") == [(T - 50, T + 31)]
    assert iv("crosses T") == [(3, 5), (T - 10, T + 11)]
    a, b = iv("crosses two tile borders")[0]
    assert a // T == 0 and (b - 1) // T == 2 and len(iv("crosses two tile borders")) == 2
    assert iv("whole tiles") == [(0, 2 * T)] and iv("whole reference") == [(0, 2 * T)] and by["whole reference"].refs[0][2] == 2 * T
    # no run across references: 64 and T are covered to their last base, the next reference from its base 0, and they stay apart
    assert iv("no run across references") == [(10, 64), (0, 21), (T - 20, T), (0, 10), (64, 128), (0, 70)]
    assert iv("overlapping and nested") == [(100, 401), (500, 651)] and int(res["overlapping and nested"][0]["live_kminmers"][0]) == 6
    assert iv("dead entries") == [(10, 51)] and int(res["dead entries"][0]["live_kminmers"][0]) == 1 and res["dead entries"][2] == 0
    d = by["dead entries"].slots
    assert sorted(d["count"].tolist()) == [1, 1, 1, 2, 2, 7] and int((d["end"] == 0).sum()) == 2
    assert iv("key 0 live") == [(10, 51), (100, 121)] and iv("key 0 dead") == [(100, 121)] and iv("key 0 alone") == [(10, 51)]
    for n in ("key 0 live", "key 0 dead", "key 0 alone"):
        assert int((by[n].slots["key"] == 0).sum()) == 1 == int(by[n].slots["is_key0"].sum())
    assert iv("out of range") == [(90, 100), (99, 100)] and res["out of range"][2] == 4
    assert [int(x) for x in res["a reference with no live entry"][0]["live_kminmers"]] == [1, 0, 1]
    assert [int(x) for x in res["a reference with no live entry"][0]["n_intervals"]] == [1, 0, 1]
    assert res["no entry at all"][1].size == 0 and res["no entry at all"][0].size == 1
    assert [int(x) for x in res["sparse ids"][0]["ref_id"]] == [5, 1000, mqx.MAX_REF_ID - 1]
    assert iv("sparse ids") == [(0, 11), (290, 300), (0, 64), (3, 10), (T - 1, T + 1)]
    assert [int(x) for x in res["4097 ids"][0]["live_kminmers"]] == [1, 1, 2]
    assert big == CM.LENGTHS(T)[-1]
    # table shapes
    shapes = [c for n, c in by.items() if n.startswith("tiny ")]
    assert sorted({c.table_slots for c in shapes}) == [2, 4, 8] and len(shapes) == 11
    assert by["one_empty"].slots.size == by["one_empty"].table_slots - 1
    mqx.check_table_end(mqx.table_end(src), src)
    for n in ("one_empty", "table_end"):
        assert res[n][1].size > 100 and int(res[n][0]["covered_bases"].sum()) < int(res[n][0]["len"].sum())


def test_model_against_the_oracle(oracle, simlib):
    """every k-min-mer of every contig whose key the oracle's map answers marks its [start, end]: the same coverage as the model's on the
    slot set a build of the same insertions saves"""
    po = oracle.params()
    refs_all = list(range(len(M.LENS)))
    _, _, names = M.contigs(simlib)
    ox = oracle.Index()
    refs = []
    for r in refs_all:
        ox.add_ref(r, names[r], M.contig(simlib, r, upper=True), po)
        refs.append((r, names[r], M.LENS[r]))
    ins = M.insertions(oracle, simlib, refs_all, po)
    cov = {r: np.zeros(M.LENS[r], dtype=bool) for r in refs_all}
    n_live = {r: 0 for r in refs_all}
    dead_keys = 0
    for e in ins:
        if ox.get(int(e["key"])) is not None:
            assert int(e["end"]) < M.LENS[int(e["id"])]
            cov[int(e["id"])][int(e["start"]):int(e["end"]) + 1] = True
            n_live[int(e["id"])] += 1
        else:
            dead_keys += 1
    recs, ivs, oor = CM.model(X.slot_set(ins), refs)
    assert oor == 0 and dead_keys >= 1 and any((~c).any() for c in cov.values())
    assert sum(n_live.values()) == ox.count()
    for r in recs:
        rid, a = int(r["ref_id"]), int(r["first_interval"])
        assert [(int(v["start"]), int(v["end"])) for v in ivs[a:a + int(r["n_intervals"])]] == CM.runs_of(cov[rid])
        assert int(r["covered_bases"]) == int(cov[rid].sum()) and int(r["live_kminmers"]) == n_live[rid]
    # the planted segments lost their cover: S_AB lies in contig 0 at 500 and is live nowhere
    assert not cov[0][1000:500 + M.SEG - 500].any()
