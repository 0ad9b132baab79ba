"""CPU: the constructions of tests/mosaic.py reach the regimes they are meant for (oracle branch counters), the oracle treats the gap
ladder the way src/chain.rs:132-142 prescribes, and an independent model of the chain side (tests/chain_model.py) agrees with the
oracle on all of it.  The floors below are conditions on the INPUTS (committed seeds and generator arguments), not on the code under
test.  The GPU counterpart is test_gpu_mosaic.py."""
import numpy as np
import pytest

import chain_model
import directed as D
import mosaic as M


@pytest.fixture(scope="module")
def world(oracle, simlib):
    return M.world(oracle, simlib)


class _Indexes:
    """oracle indexes of the mosaic genome, one per seeding parameter set (c, s, g do not enter the index)"""

    def __init__(self, oracle, g, off, names):
        self.O, self.g, self.off, self.names, self.have = oracle, g, off, names, {}

    def get(self, ps):
        po = self.O.params(**ps)
        key = (po.k, po.l, po.density, po.use_hpc)
        if key not in self.have:
            ox = self.O.Index()
            ox.build_mt(self.g, self.off, self.names, po, 4)
            self.have[key] = ox
        return self.have[key], po


@pytest.fixture(scope="module")
def indexes(oracle, world):
    g, off, names, _ = world
    return _Indexes(oracle, g, off, names)


def _diag(indexes, st, ps=None):
    ox, po = indexes.get(st["ps"] if ps is None else ps)
    return ox.map_batch_diag(st["bases"], st["offs"], po, threads=8)


def test_genome_has_many_contigs_and_tiny_ones(world):
    g, off, names, _ = world
    lens = np.diff(off.astype(np.int64))
    assert lens.size >= 300 and (lens == M.TINY_LEN).sum() >= 200 and (lens >= 60_000).sum() >= 40


def test_default_leg_reaches_many_candidates_over_several_chunks(world, indexes):
    out, d = _diag(indexes, world[3]["default"])
    m = out["mapped"] != 0
    got = dict(reads=int(m.size), over64=int((d["n_matches"] > 64).sum()), over8cand=int((d["n_candidates"] > 8).sum()),
               max_cand=int(d["n_candidates"].max()), max_matches=int(d["n_matches"].max()), ties=int((d["tie"] != 0).sum()),
               filtered=int(d["filtered_out"].sum()), clip_start=int((d["clip_start"] > 0).sum()), clip_end=int((d["clip_end"] > 0).sum()),
               fwd=int((m & (out["rc"] == 0)).sum()), rev=int((m & (out["rc"] != 0)).sum()),
               mapq0=int((m & (out["mapq"] == 0)).sum()), mapq60=int((m & (out["mapq"] == 60)).sum()), max_ref=int(out["ref_id"][m].max()))
    print("default leg:", got)
    assert got["reads"] == 400
    assert got["over64"] >= 100 and got["over8cand"] >= 200 and got["max_cand"] >= 30
    assert got["ties"] >= 5 and got["filtered"] >= 1000
    assert got["clip_start"] >= 20 and got["clip_end"] >= 20
    assert got["fwd"] >= 50 and got["rev"] >= 50
    assert got["mapq0"] >= 10 and got["mapq60"] >= 10
    assert got["max_ref"] >= 300  # ref_id is not a small number


def test_k1_leg_overflows_the_default_match_scratch(world, indexes):
    out, d = _diag(indexes, world[3]["k1"])
    got = dict(over2048=int((d["n_matches"] > 2048).sum()), max_matches=int(d["n_matches"].max()), quirk_reads=int((d["quirk_ext"] > 0).sum()))
    print("k=1 leg:", got)
    assert got["over2048"] >= 20  # the default-cap overflow redo is real
    assert got["quirk_reads"] >= 1


@pytest.mark.parametrize("name", ["k3", "k12", "mixed"])
def test_other_legs_reach_several_chunks_too(world, indexes, name):
    out, d = _diag(indexes, world[3][name])
    print(name, "leg: max matches", int(d["n_matches"].max()), "max candidates", int(d["n_candidates"].max()), "ties", int((d["tie"] != 0).sum()))
    assert (d["n_candidates"] > 4).sum() >= 50 and d["filtered_out"].sum() >= 1000
    if name != "mixed":
        assert (d["n_matches"] > 128).sum() >= 20  # three chunks and more


# What src/chain.rs:43-63 and 132-142 prescribe for a run x next to the anchor when the reference advances by `jump` more than the read
# between them (forward strand; the reverse-complemented read is the mirror image, u and v swap and so do r_start's roles):
#   order test first:  the run that comes later in the read must lie strictly further along the reference (r_start) -- a backward jump
#                      that lands in front of the earlier run's START fails it whatever g is;
#   then the gaps:     g_1 - g_2 = -jump exactly, so the run goes iff |jump| > g (|.| in i32, widened: for g >= 2^31 - 1 nothing goes).
# class of jump -> is the non-anchor run filtered out?   (g: the parameter; FAR = M.GAP_FAR)
GAP_TABLE = {
    "zero": lambda g: False,        # (one run anyway)
    "within": lambda g: False,      # 0 < |jump| <= g, either sign, either strand
    "beyond": lambda g: True,       # g < |jump| < segment length, either sign, either strand
    "far_on": lambda g: M.GAP_FAR > g,   # +FAR: only the gap test applies
    "far_back": lambda g: True,     # -FAR: the order test fails for every g, 0x7FFFFFFF and 0xFFFFFFFF included
}


def _gap_class(jump, g):
    if jump == 0:
        return "zero"
    if abs(jump) == M.GAP_FAR:
        return "far_on" if jump > 0 else "far_back"
    return "within" if abs(jump) <= g else "beyond"


HPC_SLACK = 64  # see below: far more than two 31-base windows of random sequence can differ in raw length


@pytest.mark.parametrize("hpc", [True, False])
@pytest.mark.parametrize("g", M.GAP_GS)
def test_gap_ladder_filters_exactly_beyond_g(world, indexes, g, hpc):
    """|gap difference| = |jump| EXACTLY holds without homopolymer compression: both ends of both gaps are raw positions of the same
    windows on the read and on the reference.  Under compression it holds give or take a few bases: a reverse-strand run pairs the read's
    window END with the reference's window START (src/match.rs:31-37) and the raw length of l compressed bases varies, and on either
    strand a junction inside a homopolymer run moves a window's raw start.  So the rungs g - 2 .. g + 2 are held to the table with
    use_hpc=False, and with compression only the reads whose |jump| is further than HPC_SLACK from g (the far jumps; the ordinary jumps
    at the two huge g).  The rungs next to g under compression are compared with the model below and with the GPU."""
    st = world[3]["gap_%d" % g]
    out, d = _diag(indexes, st, dict(g=g, use_hpc=hpc))
    seen = {}
    n_ok = 0
    for i, mt in enumerate(st["meta"]):
        cls = _gap_class(mt["jump"], g)
        if cls == "zero":
            assert d["n_matches"][i] == 1 and d["filtered_out"][i] == 0
            continue
        if d["n_matches"][i] != mt["nseg"]:
            continue  # a jump of a base or two that no minimizer noticed: the run went on across it
        if hpc and abs(abs(mt["jump"]) - g) <= HPC_SLACK:
            continue
        n_ok += 1
        want = (mt["nseg"] - 1) if GAP_TABLE[cls](g) else 0
        assert int(d["filtered_out"][i]) == want, (g, mt, int(d["filtered_out"][i]))
        assert out["mapped"][i] == 1 and int(out["ref_id"][i]) == mt["ctg"] and int(out["rc"][i]) == int(mt["rc"])
        seen[(cls, mt["rc"], mt["jump"] > 0)] = seen.get((cls, mt["rc"], mt["jump"] > 0), 0) + 1
    for cls, rc, pos in {(_gap_class(mt["jump"], g), mt["rc"], mt["jump"] > 0) for mt in st["meta"]}:
        near_g = cls in ("within", "beyond") and g < 4000  # the ladder's rungs are g - 2 .. g + 2
        if cls != "zero" and not (hpc and near_g):
            assert seen.get((cls, rc, pos), 0) >= 3, (g, cls, rc, pos, seen)
    assert n_ok >= (0.1 if hpc else 0.5) * len(st["meta"])


@pytest.mark.parametrize("n", M.TIE_NS)
def test_n_way_ties_are_unmapped_and_near_ties_go_to_the_one_ahead(world, indexes, n):
    st = world[3]["tie_%d" % n]
    out, d = _diag(indexes, st)
    assert out.size >= 3 and (d["tie"] != 0).all() and (d["n_candidates"] >= n).all() and (out["mapped"] == 0).all()
    st = world[3]["near_%d" % n]
    out, d = _diag(indexes, st)
    assert out.size >= 3 and (d["tie"] == 0).all() and (d["n_candidates"] == n).all() and (out["mapped"] == 1).all()
    assert out["ref_id"].tolist() == st["meta"]


def test_late_candidate_wins_from_a_later_chunk(world, indexes):
    st = world[3]["late"]
    out, d = _diag(indexes, st)
    assert (d["n_matches"] >= 71).all() and (d["n_candidates"] == 2).all() and (out["mapped"] == 1).all()
    assert out["ref_id"].tolist() == [m["b"] for m in st["meta"]]  # the reference with ONE Match wins; in the plain form it is the last record
    assert sum(m["mirror"] for m in st["meta"]) >= 4 and sum(not m["mirror"] for m in st["meta"]) >= 4
    assert (d["n_matches"] > 128).sum() >= 3  # ... of the third chunk


# ------------------------------------------------------------------ model == oracle
COLS = ("rc", "ref_id", "q_len", "q_start", "q_end", "r_len", "r_start", "r_end", "score", "mapq")


def _model_eq_oracle(oracle, ox, po, bases, offs, idx):
    out, d = ox.map_batch_diag(bases, offs, po, threads=8)
    n_matches = 0
    for i in idx:
        seq = bases[int(offs[i]):int(offs[i + 1])]
        res, info = chain_model.map_with_oracle(oracle, ox, po, seq)
        assert info["n_matches"] == int(d["n_matches"][i]) and info["n_candidates"] == int(d["n_candidates"][i]), (i, info)
        assert (res is not None) == bool(out["mapped"][i]), i
        if res is not None:
            for c in COLS:
                assert res[c] == int(out[c][i]), (i, c, res[c], int(out[c][i]))  # all 64 bits
        n_matches += info["n_matches"]
    return len(idx), n_matches


def test_model_equals_oracle_on_every_mosaic_set(oracle, world, indexes):
    sets = world[3]
    n_reads = n_matches = 0
    for name, st in sets.items():
        ox, po = indexes.get(st["ps"])
        n = st["offs"].size - 1
        stride = 2 if name in ("default", "k3", "k12") else 3 if name.startswith("gap_") else 1
        a, b = _model_eq_oracle(oracle, ox, po, st["bases"], st["offs"], range(0, n, stride))
        n_reads += a
        n_matches += b
    # the default leg's reads under the other legs' parameters as well (c = 0 / s = 0: the other arm of the mapq rule)
    st = sets["default"]
    for ps in (dict(c=0), dict(s=0), dict(k=3, l=15, density=0.03, c=2, s=5, g=500), dict(k=32, l=8, density=0.2), dict(use_hpc=False)):
        ox, po = indexes.get(ps)
        a, b = _model_eq_oracle(oracle, ox, po, st["bases"], st["offs"], range(1, 400, 8))
        n_reads += a
        n_matches += b
    print("model == oracle on %d reads, %d Matches" % (n_reads, n_matches))
    assert n_reads >= 2000 and n_matches >= 100_000


@pytest.mark.parametrize("case", ["quirk_case", "usize_wrap_case", "tie_case"])
def test_model_equals_oracle_on_the_directed_reads(oracle, simlib, case):
    g, off, names, bases, offs, ps = getattr(D, case)(oracle, simlib)
    po = oracle.params(**ps)
    ox = oracle.Index()
    ox.build_mt(g, off, names, po, 2)
    n = offs.size - 1
    a, b = _model_eq_oracle(oracle, ox, po, bases, offs, range(0, n, 1 if n <= 300 else 5))
    assert a >= 80
