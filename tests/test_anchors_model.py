"""CPU: the expected anchor list (tests/anchors_model.py) before any GPU code is compared with it.  Its two wordings -- chain_model's
runs_of / stays, and the oracle's mqo_chain_matches_explicit / mqo_check_match_compatible -- agree run for run on the mosaic world and on
plain simulated reads; and the list is tied to the pinned PAF columns: its counts sum to the oracle's score, its length and score give the
oracle's mapq, and chain_model.place() applied to the list's ends reproduces every column of the oracle's record.  A read the oracle leaves
unmapped (no candidate, or a tie) has no list.  The GPU counterpart is test_gpu_anchors.py."""
import numpy as np
import pytest

import anchors_model as A
import chain_model
import mosaic as M

COLUMNS = ("rc", "q_len", "q_start", "q_end", "r_len", "r_start", "r_end", "score", "mapq")


@pytest.fixture(scope="module")
def world(oracle, simlib):
    return M.world(oracle, simlib)


@pytest.fixture(scope="module")
def mosaic_index(oracle, world):
    g, off, names, _ = world
    po = oracle.params()
    ox = oracle.Index()
    ox.build_mt(g, off, names, po, 4)
    return ox


def _check(O, ox, po, bases, offs, idx):
    """both wordings and the oracle's record on the reads `idx`; returns (mapped, unmapped, longest list)"""
    want = ox.map_batch(bases, offs, po, threads=4)
    mapped = unmapped = longest = 0
    for i in idx:
        seq = bases[int(offs[i]):int(offs[i + 1])]
        a, b = A.by_model(O, ox, po, seq), A.by_oracle(O, ox, po, seq)
        assert a == b, i
        rec = want[i]
        if not rec["mapped"]:
            assert a is None, i
            unmapped += 1
            continue
        assert a is not None and a.runs, i
        mapped += 1
        longest = max(longest, len(a.runs))
        assert a.ref == int(rec["ref_id"]) and a.rc == bool(rec["rc"]), i
        score = sum(r[4] for r in a.runs)
        assert score == int(rec["score"]), i
        c, s = int(po.c), int(po.s)
        assert int(rec["mapq"]) == (60 if (c != 0 and s != 0 and (len(a.runs) >= c or score >= s)) else 0), i
        placed = chain_model.place(len(seq), int(ox.ref_len(a.ref)), A.ends_candidate(a, po))
        for col in COLUMNS:
            assert placed[col] == int(rec[col]), (i, col)
        if len(a.runs) > 1:  # every kept run has the anchor's strand or equals it field by field; in read order
            assert all(x[0] <= y[0] for x, y in zip(a.runs, a.runs[1:])), i
    return mapped, unmapped, longest


@pytest.mark.parametrize("name", ["default", "mixed", "late", "gap_2000", "gap_0", "gap_50", "tie_2", "tie_5", "tie_65", "near_3", "near_17"])
def test_mosaic_world(oracle, world, mosaic_index, name):
    st = world[3][name]
    po = oracle.params(**st["ps"])  # (c, s, g do not enter the index; the sets used here seed with the defaults)
    n = st["offs"].size - 1
    idx = range(0, n, 4) if name in ("default", "mixed") else range(n) if n <= 60 else range(0, n, max(1, n // 60))
    mapped, unmapped, longest = _check(oracle, mosaic_index, po, st["bases"], st["offs"], idx)
    print(name, "mapped", mapped, "unmapped", unmapped, "longest list", longest)
    if name.startswith("tie_"):
        assert mapped == 0 and unmapped > 0
    else:
        assert mapped > 0
    if name in ("default", "gap_2000"):
        assert longest >= 2


def test_plain_reads(oracle, simlib):
    g, off, names = simlib.make_genome([300000, 200000], seed=77, repeat_frac=0.2)
    reads = simlib.make_reads(g, off, 300, seed=5, len_mean=9000, err=0.02)
    po = oracle.params()
    ox = oracle.Index()
    ox.build_mt(g, off, names, po, 4)
    mapped, unmapped, longest = _check(oracle, ox, po, reads["bases"], reads["offsets"], range(300))
    print("plain: mapped", mapped, "unmapped", unmapped, "longest list", longest)
    assert mapped >= 200 and longest >= 2
