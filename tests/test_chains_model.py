"""CPU: the expected chain list (tests/chains_model.py) before any GPU code is compared with it.  Its two wordings agree on every batch the
GPU tests use; the oracle's own mapping result equals the unique TOP entry column by column, and a read the oracle leaves unmapped has zero
or at least two TOP entries.  And the inputs contain what they are named after: a GPU test over inputs that lack the cases below would
pass vacuously.  The GPU counterpart is test_gpu_chains.py."""
import numpy as np
import pytest

import chains_model as CM
import mosaic as M

COLUMNS = ("ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score")  # of the oracle's record, in the model tuple's order 1 .. 8


@pytest.fixture(scope="module")
def fx(oracle, simlib):
    g, off, names, sets, wrap = CM.batches(oracle, simlib)
    po = oracle.params()
    ox = oracle.Index()
    ox.build_mt(g, off, names, po, 4)
    return dict(ox=ox, po=po, sets=sets, wrap=wrap)


def _check(O, ox, po, bases, offs):
    """both wordings and the oracle's record on every read; returns the model's lists"""
    want = ox.map_batch(bases, offs, po, threads=4)
    exp = CM.batch(O, ox, po, bases, offs)
    assert exp == CM.batch(O, ox, po, bases, offs, word=CM.by_oracle)
    for i, chs in enumerate(exp):
        rec = want[i]
        tops = [c for c in chs if c[0] & CM.TOP]
        assert all(c[8] >= 1 and c[9] >= 1 for c in chs), i
        assert len({c[1] for c in chs}) == len(chs), i  # one chain per reference
        if not rec["mapped"]:
            assert len(tops) != 1, i
            continue
        assert len(tops) == 1, i
        for j, col in enumerate(COLUMNS):
            assert tops[0][1 + j] == int(rec[col]), (i, col)
    return exp


def test_counts(oracle, fx):
    bases, offs = fx["sets"]["counts"]
    exp = _check(oracle, fx["ox"], fx["po"], bases, offs)
    got = [len(c) for c in exp]
    assert tuple(got[:-1]) == CM.COUNTS  # MQ_CHAIN_CHUNK=4 borders, copy-out rounds of 64, two full rounds and one more
    assert got[-1] >= 100  # the default leg's largest count
    diag = fx["ox"].map_batch_diag(bases, offs, fx["po"], threads=4)[1]
    assert [int(x) for x in diag["n_candidates"]] == got
    # every run on a different reference: n_cand == nm, the staging window's tightest case
    assert any(int(diag["n_matches"][i]) == got[i] and got[i] >= 63 for i in range(len(got)))
    # more runs than the MQ_MATCH_CAP the redo tests set, and within it
    assert sum(int(x) > CM.MATCH_CAP for x in diag["n_matches"]) >= 3 and sum(int(x) <= CM.MATCH_CAP for x in diag["n_matches"]) >= 5


def test_the_mosaics_largest_count(oracle, simlib, fx):
    ps, bases, offs = fx["sets"]["most"]
    g, off, names = M.world(oracle, simlib)[:3]
    po = oracle.params(**ps)
    ox = oracle.Index()
    ox.build_mt(g, off, names, po, 4)
    exp = _check(oracle, ox, po, bases, offs)
    diag = ox.map_batch_diag(bases, offs, po, threads=4)[1]
    assert len(exp[0]) >= 180 and int(diag["n_matches"][0]) > 2048  # (and the host-driven redo at the default window)
    # no leg of the mosaic has a read with more candidates
    sets = M.world(oracle, simlib)[3]
    for name in M.LEGS:
        st = sets[name]
        pl, xl = oracle.params(**st["ps"]), oracle.Index()
        xl.build_mt(g, off, names, pl, 4)
        assert int(xl.map_batch_diag(st["bases"], st["offs"], pl, threads=4)[1]["n_candidates"].max()) <= len(exp[0]), name


def test_ties(oracle, fx):
    bases, offs = fx["sets"]["ties"]
    exp = _check(oracle, fx["ox"], fx["po"], bases, offs)
    ways = {CM.n_top(c) for c in exp}
    assert {1, 2, 17, 65} <= ways  # n-way ties (the top score n times) beside near-ties with a unique top
    assert any(CM.n_top(c) == 1 and len(c) == 65 for c in exp)


def test_tie_below_a_larger_winner(oracle, fx):
    bases, offs = fx["sets"]["below"]
    exp = _check(oracle, fx["ox"], fx["po"], bases, offs)
    n = 0
    for c in exp:
        if len(c) == 3 and CM.n_top(c) == 1 and (c[1][0] & CM.TOP) and c[0][8] == c[2][8] < c[1][8]:
            n += 1  # scores a, b, a with b larger: second_count is reached twice, the read is mapped
    assert n >= 3


def test_strands(oracle, fx):
    bases, offs = fx["sets"]["strands"]
    po = oracle.params(g=50)
    exp = _check(oracle, fx["ox"], po, bases, offs)
    kinds = {(c[2], min(c[9], 2)) for chs in exp for c in chs}
    assert kinds == {(0, 1), (0, 2), (1, 1), (1, 2)}  # forward / reverse-strand chains with n_runs == 1 and n_runs > 1


def test_wrapping_coordinates(oracle, fx):
    g, off, names, bases, offs, ps = fx["wrap"]
    po = oracle.params(**ps)
    ox = oracle.Index()
    for r in range(off.size - 1):
        ox.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])], po)
    keep = list(range(0, offs.size - 1, 3))[:40]
    b, o = M.select(bases, offs, keep)
    exp = _check(oracle, ox, po, b, o)
    wrapped = sum(1 for chs in exp for c in chs if c[4] >> 32 or c[5] >> 32)
    assert wrapped >= 3  # find_coords' usize arithmetic wrapped: the high words of columns 3 / 4 are set
    assert any(len(chs) >= 2 for chs in exp)
