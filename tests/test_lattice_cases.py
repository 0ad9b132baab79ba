"""CPU: every point of the boundary lattice (tests/lattice.py) is constructed and has the property it is named after -- lengths, planted
runs, compressed lengths, minimizer counts (oracle.minimizers), k-min-mer counts (oracle.kminmers), hits and Match runs
(oracle.Index.get, map_batch_diag's n_kminmers / n_matches).  On families A and B the oracle's two minimizer routines (the rolling one
and minimizers(naive=True)) must agree.  Each test prints the number of points it constructed; none is skipped: a constructor that gives
up raises lattice.LatticeError naming the point.  The GPU counterpart is test_gpu_lattice.py."""
import numpy as np
import pytest

import lattice as L


@pytest.fixture(scope="module")
def world(simlib):
    return L.world(simlib)


@pytest.fixture(scope="module")
def ref_index(oracle, world):
    """oracle indexes of the genome, one per parameter set (made on first use)"""
    g, off, names = world
    made = {}

    def get(ps):
        key = tuple(sorted(ps.items()))
        if key not in made:
            po = oracle.params(**ps)
            ox = oracle.Index()
            ox.add_ref(0, names[0], g, po)
            made[key] = (ox, po)
        return made[key]
    return get


def _report(family, n):
    print("lattice family %s: %d points constructed" % (family, n))


def _same_minimizers(oracle, seq, po):
    a, b = oracle.minimizers(seq, po), oracle.minimizers(seq, po, naive=True)
    return a.size == b.size and np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["hash"], b["hash"])


def test_family_a_raw_lengths(oracle, world):
    g = world[0]
    total = 0
    for l in L.A_LS:
        po = oracle.params(**L.a_params(l))
        want = L.length_lattice(l)
        for B in L.A_BASES:   # the rule of the lattice, spelled out
            for d in list(range(-(l + 1), l + 2)) + [15, 16, 17, 63, 64, 65, -15, -16, -17, -63, -64, -65]:
                assert B + d < 0 or B + d in want
        pts = L.raw_length_points(g, l)
        assert [len(s) for _, s in pts] == want and want[0] == 0
        for name, s in pts:
            mz = oracle.minimizers(s, po)
            assert mz.size <= max(0, len(s) - l + 1), name                     # windows = len - l + 1 without compression
            assert _same_minimizers(oracle, s, po), (l, name)
            if len(s) < po.l + po.k - 1:
                assert L.kminmers_or_none(oracle, s, po).size == 0
            else:
                assert L.kminmers_or_none(oracle, s, po).size == max(0, mz.size - po.k + 1), (l, name)
            if len(s) >= L.SD_SR_RAW - 65:
                assert mz.size >= 3, (l, name)                                  # the density gives a read of a tile's length a few
        total += len(pts)
    po = oracle.params(**L.A_DENSE)
    pts = L.raw_length_points(g, po.l)
    for name, s in pts:
        n = max(0, len(s) - po.l + 1)
        assert oracle.minimizers(s, po).size == n and _same_minimizers(oracle, s, po), name   # every window a candidate
        assert L.kminmers_or_none(oracle, s, po).size == max(0, n - po.k + 1)
        assert len(s) < L.SD_SR_RAW or n > L.SD_OWNER_CAP                       # more than one round of stage R per tile
        assert n + po.k <= len(s) * 4 + L.LIST_SLACK                           # and the list fits its region (f = 4 * density + 1 / 512)
    total += len(pts)
    _report("A", total)


def test_family_b_runs_on_the_borders(oracle, world):
    g = world[0]
    total = 0
    for ps in L.B_PARAMS:
        po = oracle.params(**ps)
        pts = L.run_border_points(g, po.l)
        names = [p[0] for p in pts]
        assert len(set(names)) == len(names)
        for r in L.B_RUNS:
            for B in L.B_BASES:
                for d in (-1, 0, 1):
                    assert "run r=%d starts at %d%+d" % (r, B, d) in names
                    assert (B + d - r < 0) != ("run r=%d ends at %d%+d" % (r, B, d) in names)
            assert "run r=%d at the start of the read" % r in names and "run r=%d at the end of the read" % r in names
        for name, s, where in pts:
            assert len(s) >= 3 * L.SD_TILE_RAW
            if where:
                st, r = where
                assert L.run_is_exact(s, st, r), name
                if "starts at" in name:
                    assert st == int(name.split(" at ")[1].replace("+", " +").replace("-", " -").split()[0]) + int(name[-2:])
                if "ends at" in name:
                    assert st + r == int(name.split(" at ")[1].replace("+", " +").replace("-", " -").split()[0]) + int(name[-2:])
                if "the end of the read" in name:
                    assert st + r == len(s)
            elif name.startswith("two whole-tile runs"):
                j = int(name.split(",")[1].split()[0])
                a = np.frombuffer(s, dtype=np.uint8)
                assert (a[L.SD_TILE_RAW:2 * L.SD_TILE_RAW] == a[L.SD_TILE_RAW]).all() and a[L.SD_TILE_RAW - 1] != a[L.SD_TILE_RAW]
                assert (a[3 * L.SD_TILE_RAW:4 * L.SD_TILE_RAW] == a[3 * L.SD_TILE_RAW]).all()
                # run heads of tiles 2 .. 4: the first run's, j between, the second run's -- fewer than l - 1 unless j says otherwise
                assert L.count_heads(s, L.SD_TILE_RAW, 4 * L.SD_TILE_RAW) == j + 2
            else:
                c = int(name.split()[2])
                assert L.compressed_length(s) == c and len(s) > 3 * L.SD_TILE_RAW
                assert oracle.minimizers(s, po).size <= max(0, c - po.l + 1)
            assert _same_minimizers(oracle, s, po), (ps, name)
        for v in ((0,) + L.B_VARIANTS if not ps else (0,)):
            oracle.lib().mqo_set_variant(v)
            try:
                n_kmm = sum(L.kminmers_or_none(oracle, s, po).size for _, s, _ in pts)
            finally:
                oracle.lib().mqo_set_variant(0)
            assert n_kmm > len(pts)
        total += len(pts)
    _report("B", total)


def test_family_c_placements(oracle, world):
    g = world[0]
    reads = L.placement_reads(g)
    assert len(reads[0][1]) < L.BLOCK and len(reads[1][1]) % L.BLOCK == 0 and len(reads[2][1]) == L.SD_TILE_RAW + 1
    assert reads[3][1][-1] == reads[3][1][-7] != reads[3][1][-8]
    pts, where = L.placement_offsets_batch(g, reads)
    bases, offs = L.batch(pts)
    seen = set()
    for i, (w, res) in where.items():
        assert pts[i][1] == reads[w][1] and int(offs[i]) % L.BLOCK == res and 1 <= len(pts[i - 1][1]) <= L.BLOCK
        seen.add((w, res))
    assert seen == {(w, r) for w in range(4) for r in range(L.BLOCK)}
    assert {len(pts[i - 1][1]) for i in where} == set(range(1, L.BLOCK + 1))
    pts2, where2 = L.placement_neighbour_batch(g, reads)
    for i, (w, _) in where2.items():
        assert pts2[i][1] == reads[w][1] and pts2[i - 1][1][-1] == pts2[i][1][0] and pts2[i + 1][1][0] == pts2[i][1][-1]
    pts3, where3 = L.placement_n_batch(g, reads)
    b3, o3 = L.batch(pts3)
    for i, (w, _) in where3.items():
        assert pts3[i][1] == reads[w][1] and b3[int(o3[i + 1])] == ord("N")
    buf, starts, lens = L.fastq_buffer(reads)
    for (name, s), st, ln in zip(reads, starts, lens):
        assert buf[int(st):int(st) + int(ln)].tobytes() == s and buf[int(st) - 1] == ord("\n") and buf[int(st) + int(ln)] == ord("\n")
    for ps in L.C_PARAMS:   # the reads are worth mapping: the long ones have k-min-mers
        po = oracle.params(**ps)
        assert all(L.kminmers_or_none(oracle, s, po).size > 0 for _, s in reads[1:])
    _report("C", len(pts) + len(pts2) + len(pts3) + 2 * len(reads))


def test_family_d_minimizer_counts(oracle, world):
    g = world[0]
    total = 0
    ks = set()
    for ps in L.D_PARAMS:
        po = oracle.params(**ps)
        ks.add(int(po.k))
        want = L.minimizer_counts(po.k)
        for j in L.D_J:
            for e in (-1, 0, 1):
                assert L.LANE_BATCH * j + po.k - 1 + e in want
        assert {po.k, po.k + 1} <= set(want) and (po.k == 1) != (po.k - 1 in want)
        pts = L.minimizer_count_points(oracle, g, ps)
        assert [int(n[2:]) for n, _ in pts] == want
        for (name, s), N in zip(pts, want):
            assert oracle.minimizers(s, po).size == N, (ps, name)
            assert L.kminmers_or_none(oracle, s, po).size == max(0, N - po.k + 1), (ps, name)
            assert g.tobytes().find(s) >= 0
        total += len(pts)
    assert {1, 5, 8, 32} <= ks
    _report("D", total)


def test_family_e_match_run_breaks(oracle, world, ref_index):
    g = world[0]
    total = 0
    for ps in L.E_PARAMS:
        ox, po = ref_index(ps)
        pts = L.match_break_points(oracle, ox, g, ps)
        kinds = {}
        for name, s, (kind, j) in pts:
            strand = name.split()[0].rstrip(":")
            kinds.setdefault((strand, kind), []).append(j)
            m = L.hit_mask(oracle, ox, s, po)
            b = np.frombuffer(s, dtype=np.uint8)
            out, diag = ox.map_batch_diag(b, np.array([0, b.size], dtype=np.uint64), po)
            assert int(diag["n_kminmers"][0]) == m.size
            if kind == "after":
                assert m[:j + 1].all() and not m[j + 1], name
            elif kind == "before":
                assert m[j:].all() and not m[j - 1], name
            else:
                assert int(diag["n_matches"][0]) == j, name
            assert out["mapped"][0] == 1 and int(out["rc"][0]) == (1 if strand == "rc" else 0), name
        for strand in ("fwd", "rc"):
            assert sorted(set(kinds[(strand, "after")])) == sorted(L.E_BREAKS) == sorted(set(kinds[(strand, "before")]))
            assert sorted(kinds[(strand, "runs")]) == sorted(L.E_RUNS)
        total += len(pts)
    _report("E", total)


def test_family_f_general_seeder(oracle, world):
    g = world[0]
    total = 0
    for l in L.A_LS:
        pts = L.raw_length_points(g, l, bases=L.F_BASES)
        assert [len(s) for _, s in pts] == L.length_lattice(l, L.F_BASES)
        total += len(pts)
    pts = L.general_run_points(g)
    assert len(pts) == 2 * len(L.F_RUNS) * len(L.F_RUN_STARTS)
    assert {st % L.GEN_STEP for _, _, (st, r) in pts} == {0, 1, L.GEN_STEP - 1}
    for name, s, (st, r) in pts:
        assert L.run_is_exact(s, st, r), name
        assert (s[st] == ord("N")) == ("of N" in name)
    total += len(pts)
    pts = L.declined_stretch_points(g)
    blocks = set()
    for name, s, (a, c) in pts:
        assert s[a - 1] == ord("N") and s[a + c] == ord("N") and b"N" not in s[a:a + c], name
        blocks.add(L.clean_blocks(a, c))
    # whole 64-byte blocks of the stretch: one block short of the minimum, the minimum itself, one more
    assert {L.HYB_MIN_CLEAN - L.BLOCK, L.HYB_MIN_CLEAN, L.HYB_MIN_CLEAN + L.BLOCK} <= blocks
    total += len(pts)
    pts = L.dense_step_points(g)
    assert [h for _, _, h in pts] == list(L.F_HEADS)
    for name, s, h in pts:
        for step in (2, 3, 4):
            assert L.count_heads(s, step * L.GEN_STEP, (step + 1) * L.GEN_STEP) == h, name
        assert any(c not in b"ACGT" for c in s)
    total += len(pts)
    _report("F", total)


def test_family_g_references(oracle, world):
    g = world[0]
    total = 0
    for ps in L.G_PARAMS:
        po = oracle.params(**ps)
        pts = L.reference_length_points(g, po.l)
        assert [len(s) for _, s in pts] == L.length_lattice(po.l, L.G_BASES)
        total += len(pts)
        pts = L.reference_run_points(g, po.l)
        names = [p[0] for p in pts]
        for r in L.B_RUNS:
            for B in L.G_BASES:
                for d in (-1, 0, 1):
                    assert "ref: run r=%d starts at %d%+d" % (r, B, d) in names
                    assert (B + d - r < 0) != ("ref: run r=%d ends at %d%+d" % (r, B, d) in names)
        n_halo = 0
        for name, s, where in pts:
            if where[0] == "halo":
                n_halo += 1
                assert L.count_heads(s, L.REF_SEG, L.REF_SEG + L.REF_HALO) == where[1], name
            else:
                assert L.run_is_exact(s, *where), name
            assert oracle.kminmers(s, po).size > 0
        assert n_halo == len({1, 2, po.l - 2, po.l - 1, po.l})
        total += len(pts)
    _report("G", total)


# ------------------------------------------------------------------ the core batch of the instantiation matrix, families H and I
def _names(pts, family):
    return [p[0] for p in pts if p[2] == family]


@pytest.mark.parametrize("which", sorted(L.CORE_PARAMS))
def test_core_points_hit_every_size(oracle, world, ref_index, which):
    """every size constant of lattice.py's header appears among core_points exactly and one element to either side: from the points' names
    (which the family proofs above tie to the sequences) and from the oracle's minimizer, k-min-mer and Match-run counts"""
    import time
    g = world[0]
    ps, families = L.CORE_PARAMS[which]
    ox, po = ref_index(ps)
    k, l = int(po.k), int(po.l)
    t0 = time.perf_counter()
    pts = L.core_points(oracle, ox, g, ps, families)
    dt = time.perf_counter() - t0
    assert pts == L.core_points(oracle, ox, g, ps, families)    # deterministic
    names = [p[0] for p in pts]
    assert len(set(names)) == len(names) and len(pts) <= 400
    bases, offs = L.batch(pts)
    _, diag = ox.map_batch_diag(bases, offs, po, threads=4)
    # A: every base exactly, one to either side, and the carry of l - 1 codes (and one more) to either side of it
    lens = {len(p[1]) for p in pts if p[2] == "A"}
    for B in (0, L.BLOCK, L.SD_SR_RAW, L.SD_TILE_RAW, 2 * L.SD_TILE_RAW):
        for d in (-1, 0, 1, -(l - 1), l - 1, l):
            assert B + d < 0 or B + d in lens, (which, B, d)
    for p in pts:
        if p[2] == "A":
            assert p[0] == "A len=%d" % len(p[1])
    # B: runs of every piece / block / super-row / tile size +- 1, starting and ending on the super-row and the tile border +- 1
    nb = set(_names(pts, "B"))
    for c in (L.WORD, L.BLOCK, L.SD_SR_RAW, L.SD_TILE_RAW):
        for r in (c - 1, c, c + 1):
            for B in (L.SD_SR_RAW, L.SD_TILE_RAW):
                for d in (-1, 0, 1):
                    assert "B run r=%d starts at %d%+d" % (r, B, d) in nb, (which, r, B, d)
                    assert (B + d - r < 0) != ("B run r=%d ends at %d%+d" % (r, B, d) in nb)
    for name, s, where in L.run_border_points(g, l, runs=L.CORE_B_RUNS, bases=L.CORE_B_BASES):
        assert where is None or L.run_is_exact(s, *where), name
    # D: the lane-batch and the chunk with its k - 1 shared entries, by the oracle's counts, both strands
    d_idx = [i for i, p in enumerate(pts) if p[2] == "D"]
    n_mz = [oracle.minimizers(pts[i][1], po).size for i in d_idx]
    n_kmm = [int(diag["n_kminmers"][i]) for i in d_idx]
    assert sorted(n_mz) == sorted(L.minimizer_counts(k) * 2)
    assert n_kmm == [max(0, n - k + 1) for n in n_mz]
    for c in (L.LANE_BATCH, L.CHUNK_KMM, 2 * L.CHUNK_KMM, 3 * L.CHUNK_KMM):
        for e in (-1, 0, 1):
            assert n_kmm.count(c + e) == 2, (which, c, e)
    # E: the breaks by name (test_family_e_match_run_breaks proves them for E_PARAMS; the same search here), the runs by n_matches
    if "E" in families:
        ne = _names(pts, "E")
        for strand in ("fwd", "rc"):
            for j in L.E_BREAKS:
                assert any(n.startswith("E %s " % strand) and n.endswith("last hit before the break is %d" % j) for n in ne), (which, strand, j)
                assert any(n.startswith("E %s " % strand) and n.endswith("first hit after the break is %d" % j) for n in ne), (which, strand, j)
        n_breaks = 0
        for name, s, _ in pts:   # the core's own break points, whatever the parameter set: the hit mask around j
            if name.startswith("E ") and " break is " in name:
                j = int(name.split()[-1])
                m = L.hit_mask(oracle, ox, s, po)
                assert (m[:j + 1].all() and not m[j + 1]) if "last hit before" in name else (m[j:].all() and not m[j - 1]), (which, name)
                n_breaks += 1
        assert n_breaks == 2 * 2 * (len(L.E_BREAKS) + sum(1 for j in L.E_BREAKS if j <= L.CHUNK_KMM + 1))
    # the Match-run reads, in every parameter set (E's own, or match_run_points counted up from the undamaged read's runs): by n_matches
    assert "E" in families or "R" in families
    runs = [(p[0], int(diag["n_matches"][i])) for i, p in enumerate(pts) if p[2] == "E" and p[0].endswith("Match runs")]
    assert all(name == "E %s: %d Match runs" % (name.split()[1].rstrip(":"), m) for name, m in runs), runs
    assert sorted(m for _, m in runs) == sorted((L.E_RUNS if "E" in families else L.CORE_RUNS) * 2) and set(L.CORE_RUNS) <= set(L.E_RUNS)
    for c in (L.MAP_LDS_RECS, L.CHAIN_CH):
        for e in (-1, 0, 1):
            assert (diag["n_matches"] == c + e).sum() >= 2, (which, c, e)
    # F: 1-KB steps, the clean stretch in whole blocks, run heads per step around 64 and the ring's 512
    nf = set(_names(pts, "F"))
    for r in L.F_RUNS:
        assert "F general: run of A-like r=%d at %d" % (r, L.CORE_F_START) in nf and "F general: run of N r=%d at %d" % (r, L.CORE_F_START) in nf
    assert {L.GEN_STEP - 1, L.GEN_STEP, L.GEN_STEP + 1, 2 * L.GEN_STEP - 1, 2 * L.GEN_STEP, 2 * L.GEN_STEP + 1} <= set(L.F_RUNS) and L.CORE_F_START % L.GEN_STEP == 0
    dec = L.declined_stretch_points(g, ds=(L.CORE_F_D,))
    assert all("F " + n in nf for n, _, _ in dec) and len(dec) == len(L.F_CLEAN)
    assert {L.clean_blocks(a, c) for _, _, (a, c) in dec} == {L.HYB_MIN_CLEAN - L.BLOCK, L.HYB_MIN_CLEAN, L.HYB_MIN_CLEAN + L.BLOCK}
    for h in L.F_HEADS:
        assert "F dense: %d run heads per 1-KB step" % h in nf
    assert {L.GEN_HASH_HEADS - 1, L.GEN_HASH_HEADS, L.GEN_HASH_HEADS + 1, L.GEN_RING - 1, L.GEN_RING, L.GEN_RING + 1, L.GEN_STEP} <= set(L.F_HEADS)
    print("core batch %s: %d points, %d bases, constructed in %.1f s" % (which, len(pts), bases.size, dt))


@pytest.mark.parametrize("which", ["default", "k3l12"])
def test_family_h_list_capacity(oracle, world, which):
    """family H's reads list exactly the named counts, under the frozen reading and under the variant the matrix also runs H with (16:
    END_COMPRESSED moves `end`, not the selection); regions are adjacent (a neighbour behind every read); the point at the default f16
    does not exist in this genome (a region is 2.6 times the expected list)"""
    g = world[0]
    ps = L.CORE_PARAMS[which][0]
    po = oracle.params(**ps)
    with pytest.raises(L.LatticeError):
        L.list_capacity_points(oracle, g, ps)
    full = L.list_capacity_points(oracle, g, ps, default_too=False)
    # every neighbour's region begins where its read's ends: both start in the same 65,536 bases of the batch (padding reads see to it)
    assert L.regions_adjacent(full) == [True] * (2 * len(L.H_COUNTS))
    assert which != "default" or any(p[2] == "pad" for p in full)       # (the default set's reads of 23 kb would straddle without them)
    _, offs = L.batch(full)
    for i, p in enumerate(full):
        if isinstance(p[2], int):
            assert int(offs[i]) >> 16 == int(offs[i + 1]) >> 16 and full[i + 1][2] is None, p[0]
    pts = [p for p in full if p[2] != "pad"]
    assert [p[2] for p in pts[0::4]] == list(L.H_COUNTS) == [p[2] for p in pts[2::4]]
    assert L.H_COUNTS == (63, 64, 65, 319, 320, 321)
    for i, (name, s, N) in enumerate(pts):
        if N is None:
            assert i % 2 == 1 and s == pts[1][1] and name == "neighbour of " + pts[i - 1][0]
            continue
        assert len(s) < 65536 and L.list_cap(len(s), L.H_F16) == L.LIST_SLACK      # every region is 64 entries at f16 = 1
        assert L.list_cap(len(s), L.default_f16(po.density)) > N                   # ... and holds the list at the default
        assert (b"N" in s) == name.endswith("with an N") and s.count(b"N") <= 1
        for v in (0, 16):
            oracle.lib().mqo_set_variant(v)
            try:
                assert oracle.minimizers(s, po).size == N and L.kminmers_or_none(oracle, s, po).size == N - po.k + 1, (which, name, v)
            finally:
                oracle.lib().mqo_set_variant(0)
    assert min(p[2] for p in pts if p[2]) <= L.LIST_SLACK < max(p[2] for p in pts if p[2])
    _report("H " + which, len(pts))


def test_family_i_lower_case_on_the_borders(oracle, world):
    g = world[0]
    pts = L.fold_border_points(g)
    seen = set()
    for name, s, (where, up) in pts:
        a, u = np.frombuffer(s, dtype=np.uint8), np.frombuffer(up, dtype=np.uint8)
        assert len(s) == 3 * L.SD_TILE_RAW and s.upper() == up and set(up) <= set(b"ACGTN")
        assert np.flatnonzero(a != u).tolist() == sorted(where), name            # the lower-case bytes sit where they are named
        assert L.compressed_length(s.upper()) == L.compressed_length(up)          # folding gives the read back: the case changes no run
        if name.startswith("lower-case byte"):
            assert where == [int(name.split()[-1])]
            seen.add(where[0])
        elif name.startswith("mixed-case run"):
            st, r = L.SD_TILE_RAW - L.I_RUN // 2, L.I_RUN
            assert L.run_is_exact(up, st, r) and where == list(range(st, st + r, 2))
            assert L.compressed_length(s) == L.compressed_length(up) + r - 1     # unfolded, every byte of the run is a run of its own
        elif name.startswith("lower-case n run"):
            st = int(name.split()[-1])
            assert up[st:st + L.I_N_RUN] == b"N" * L.I_N_RUN and s[st:st + L.I_N_RUN] == b"n" * L.I_N_RUN and st - L.GEN_STEP in (-1, 0, 1)
        else:
            st = where[0]
            assert len(where) == L.HYB_MIN_CLEAN == L.clean_blocks(st, len(where)) and up[st - 1] == up[st + len(where)] == ord("N")
            assert b"N" not in up[st:st + len(where)] and s[st:st + len(where)].islower()
    assert seen == set(L.I_BYTES) | {0, 3 * L.SD_TILE_RAW - 1}
    assert {L.WORD, L.BLOCK, L.SD_SR_RAW, L.SD_TILE_RAW} <= seen and all({c - 1, c + 1} <= seen for c in (L.WORD, L.BLOCK, L.SD_SR_RAW, L.SD_TILE_RAW))
    _report("I", len(pts))
