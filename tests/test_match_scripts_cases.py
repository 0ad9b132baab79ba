"""CPU proofs for tests/match_scripts.py: conditions on the generated batches, not measurements.

  1  the two references agree on every read: chain_model.runs_of == mqo_chain_matches_explicit run for run, chain_model.map_read == the
     oracle twin's map_batch record for record, anchors_model.by_model == by_oracle; match_scripts.outcome (the model's chain side in one
     pass) equals both, and runs_flipped without a flip is runs_of
  2  every probe is decisive: with the model's decision at element b alone inverted, the expected pair (hit record, anchor list) changes
     for every read of family P
  3  coverage: every (state before, kind) pair, all 57, at lane 0, at lane 63, at a chunk's first element, at a read's last element and
     mid-batch (dense set; the thinned default set: every pair at b = 64 and at b = 384); quirk_ext, quirk_cross_ref, rc_ext and
     check_fail of map_batch_diag each at least 100 over the batch
  4  no read is dropped; family C's run counts are exact

Decisive by the hit record alone (printed by test_every_probe_is_decisive; no floor is asserted): dense 1615 of 1615 probes, default 304 of
304 -- score is the sum of the kept runs' counts and every flip moves an element into or out of the winner's runs.
"""
import ctypes as C

import numpy as np
import pytest

import anchors_model as A
import chain_model
import match_scripts as S

WHICH = ("dense", "default")
PAF = ("rc", "ref_id", "q_len", "q_start", "q_end", "r_len", "r_start", "r_end", "score", "mapq")
_made = {}


def made(O, which):
    """the set's world, the oracle twin of its table, the oracle's answers for both batches"""
    if which not in _made:
        w = S.world(O, which)
        ox = w.table.to_oracle(O)
        ans = {}
        for name, idx in (("main", w.main), ("window", w.window)):
            if idx:
                bases, offs = S.batch_of(w, idx)
                ans[name] = (idx,) + ox.map_batch_diag(bases, offs, w.po, threads=4)
        _made[which] = (w, ox, ans)
    return _made[which]


def _oracle_runs(O, rd):
    """mqo_chain_matches_explicit on the read's k-min-mers and the script's entries (a dead key: no hit; an entry born empty: a hit whose
    end is 0, which the routine itself takes for a miss)"""
    n = rd.K
    ent = np.zeros(n, dtype=O.entry_dtype)
    hit = np.zeros(n, dtype=np.uint8)
    for i, e in enumerate(rd.entries):
        if e is not None:
            ent[i] = (e["id"], e["start"], e["end"], e["offset"], int(e["rc"]), 0)
            hit[i] = 1
        elif rd.kinds.get(i) == "born":
            hit[i] = 1
    ms, refs = np.zeros(n, dtype=O.match_dtype), np.zeros(n, dtype=np.uint64)
    nm = O.lib().mqo_chain_matches_explicit(rd.km.ctypes.data, ent.ctypes.data, hit.ctypes.data, n, ms.ctypes.data, refs.ctypes.data, n)
    return [(int(refs[j]), bool(ms["rc"][j])) + tuple(int(ms[f][j]) for f in ("q_start", "q_end", "r_start", "r_end", "count")) for j in range(nm)]


@pytest.mark.parametrize("which", WHICH)
def test_the_two_references_agree(oracle, which):
    w, ox, ans = made(oracle, which)
    po = w.po
    want = {}
    for idx, recs, diag in ans.values():
        for j, i in enumerate(idx):
            want[i] = (recs[j], diag[j])
    assert sorted(want) == list(range(len(w.reads)))
    for i, rd in enumerate(w.reads):
        runs = chain_model.runs_of(rd.kmers, rd.entries)
        assert S.run_tuples(runs) == _oracle_runs(oracle, rd), rd.name
        assert S.run_tuples(S.runs_flipped(rd.kmers, rd.entries, None)) == S.run_tuples(runs), rd.name
        rec, info = chain_model.map_read(rd.kmers, rd.entries, len(rd.seq), lambda r: S.REF_LEN, int(po.c), int(po.s), int(po.g))
        o, d = want[i]
        assert int(d["n_kminmers"]) == rd.K and int(d["n_matches"]) == len(runs) == info["n_matches"], rd.name
        assert (rec is not None) == bool(o["mapped"]), rd.name
        if rec:
            assert [rec[f] for f in PAF] == [int(o[f]) for f in PAF], rd.name
        m, a = A.by_model(oracle, ox, po, rd.seq), A.by_oracle(oracle, ox, po, rd.seq)
        assert m == a and (m is not None) == (rec is not None), rd.name
        assert S.outcome(runs, len(rd.seq), po) == (rec, m), rd.name


@pytest.mark.parametrize("which", WHICH)
def test_every_probe_is_decisive(oracle, which, capsys):
    w = S.world(oracle, which)
    probes = [rd for rd in w.reads if rd.family == "P"]
    assert len(probes) == len(S.probe_specs(w.cfg)) >= (7 + 9) * 19   # (b = 64 has no room for the two far states)
    by_record, undecided = 0, []
    for rd in probes:
        assert rd.kinds[rd.b] == rd.kind, rd.name   # the probed element is the kind the read is named for
        base = S.outcome(chain_model.runs_of(rd.kmers, rd.entries), len(rd.seq), w.po)
        flip = S.outcome(S.flipped(rd), len(rd.seq), w.po)
        if base == flip:
            undecided.append(rd.name)
        by_record += base[0] != flip[0]
    with capsys.disabled():
        print("\n[match scripts] %s: %d of %d probes decisive by the hit record alone" % (which, by_record, len(probes)))
    assert not undecided, (len(undecided), undecided[:10])


@pytest.mark.parametrize("which", WHICH)
def test_coverage(oracle, which, capsys):
    w, ox, ans = made(oracle, which)
    pr = [rd for rd in w.reads if rd.family in "PR"]
    cov = S.coverage(pr)
    with capsys.disabled():
        print("\n[match scripts] %s: positions of P and R per (state before, kind) and place\n%s" % (which, S.coverage_table(cov)))
    if which == "dense":
        for place in S.PLACES:
            missing = S.ALL_PAIRS - set(cov[place])
            assert not missing, (place, sorted(missing, key=str))
    for b in (64, 384):
        missing = S.ALL_PAIRS - S.coverage_at(pr, b)
        assert not missing, (b, sorted(missing, key=str))
    # the states the probes are named for are the model's: miss -> none, every forward kind -> forward, the reverse ones -> reverse
    for rd in pr:
        if rd.family == "P":
            assert rd.states[rd.b] == (0 if rd.state == "miss" else 2 if rd.state.startswith("rev") else 1), rd.name
    idx, recs, diag = ans["main"]
    for f in ("quirk_ext", "quirk_cross_ref", "rc_ext", "check_fail"):
        assert int(diag[f].sum()) >= 100, (f, int(diag[f].sum()))
    # run lengths from 1 to beyond 100 in the walks, and the records made by hit-breaks alone on either side of both windows
    counts = [r.count for rd in w.reads if rd.family == "R" for r in chain_model.runs_of(rd.kmers, rd.entries)]
    assert min(counts) == 1 and max(counts) >= 100
    exact = sorted(rd.n_runs for rd in w.reads if rd.family == "R" and rd.n_runs)
    assert exact[0] == 49 and 65 in exact


@pytest.mark.parametrize("which", WHICH)
def test_no_read_is_dropped(oracle, which):
    w, ox, ans = made(oracle, which)
    cfg = w.cfg
    fam = {f: [rd for rd in w.reads if rd.family == f] for f in "PRWCN"}
    n_p = len(S.probe_specs(cfg))
    assert len(fam["P"]) == n_p and len(fam["R"]) == cfg["n_walks"] and len(fam["W"]) == len(S.cast_scripts()) and len(fam["C"]) == len(cfg["C"])
    assert len(fam["N"]) == -(-n_p // 10) + -(-cfg["n_walks"] // 10)
    assert sorted(w.main + w.window) == list(range(len(w.reads))) and len(ans["main"][1]) == len(w.main)
    for rd in w.reads:
        assert rd.km.size == rd.K and (rd.seq.count(b"N") == 1) == (rd.family == "N"), rd.name
        if getattr(rd, "n_runs", None):   # hits alone: no miss anywhere, exactly the runs asked for
            assert all(e is not None for e in rd.entries) and len(chain_model.runs_of(rd.kmers, rd.entries)) == rd.n_runs, rd.name
    # the table holds exactly the scripted positions that are no absent key, each under its read's own key
    assert w.table.entries.size == sum(1 for rd in w.reads for k in rd.kinds.values() if k != "absent")
    if cfg["C"]:
        idx, recs, diag = ans["window"]
        assert diag["n_matches"].tolist() == list(cfg["C"]) == [2047, 2048, 2049] and (recs["mapped"] != 0).sum() >= 2
        assert all(w.reads[i].K == S.C_KMM for i in idx)
    # family W: the offsets the names promise, through the casts
    offs = {e["offset"] for rd in fam["W"] for e in rd.entries if e}
    assert {0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE} <= offs
    for rd in fam["W"]:
        lens = sorted(r.count for r in chain_model.runs_of(rd.kmers, rd.entries))
        assert lens == ([7, 9] if "meets" not in rd.name else [2, 3, 3, 4]), (rd.name, lens)
