"""CPU: every case of tests/offset_cases.py has the property it is named after -- the shapes of the batch, which read lies across 2^32 at
the two straddling shifts and which reads lie wholly behind it, the residues mod 64 of the first offset, the periodic-window rule of
order_reads_kernel on the tandem reads (flagged wherever the batch lies) and on every other read (never flagged), the offsets of the
batch with a read past the length limit, and the staged records' places and joined bytes.  The GPU counterpart is test_gpu_offsets.py."""
import numpy as np
import pytest

import offset_cases as K

P32 = K.P32


@pytest.fixture(scope="module")
def b(simlib, oracle):
    return K.batch(simlib, oracle)


def _len(b, name):
    r = b["idx"][name]
    return int(b["offs"][r + 1] - b["offs"][r])


def test_the_batch_is_deterministic_and_has_its_shapes(b, simlib, oracle):
    again = K.batch(simlib, oracle)
    assert again["bases"].tobytes() == b["bases"].tobytes() and np.array_equal(again["offs"], b["offs"]) and again["names"] == b["names"]
    l, k = b["l"], b["k"]
    assert (l, k) == (31, 5)
    n = len(b["names"])
    assert n == K.N_SIM + 8 + len(K.TANDEM_PERIODS) and b["offs"].size == n + 1 and int(b["offs"][-1]) == b["bases"].size
    assert b["names"][:3] == ["sim0", "sim1", "sim2"] and b["names"][-1] == "sim%d" % (K.N_SIM - 1)
    assert b["names"][K.LONG_AT] == "short_l+k-2" and b["names"][K.LONG_AT - 1] == "sim%d" % (K.LONG_AT - 1)
    assert [_len(b, "short_l+k%+d" % d) for d in (-2, -1)] + [_len(b, "short_l+k")] == [l + k - 2, l + k - 1, l + k]
    assert _len(b, "empty") == 0
    assert (_len(b, "len12287"), _len(b, "len12289")) == (12288 - 1, 12288 + 1)
    r = b["idx"]["with_N"]
    s = b["bases"][int(b["offs"][r]):int(b["offs"][r + 1])]
    assert (s == ord("N")).sum() == 1 and s[s.size // 2] == ord("N") and set(s.tobytes()) == set(b"ACGTN")
    r = b["idx"]["homopolymer"]
    assert set(b["bases"][int(b["offs"][r]):int(b["offs"][r + 1])].tobytes()) == {ord("A")}
    for p in K.TANDEM_PERIODS:
        r = b["idx"]["tandem%d" % p]
        s = b["bases"][int(b["offs"][r]):int(b["offs"][r + 1])]
        assert 2000 <= s.size <= 6000 and np.array_equal(s[p:], s[:-p]) and len(set(s[:p].tobytes())) >= 2  # period p (or a divisor of it)
    sim = np.array([_len(b, "sim%d" % i) for i in range(K.N_SIM)])
    assert 2500 < sim.mean() < 3500 and sim.min() >= 512  # (every simulated read is long enough for the ordering pass to look at)
    assert set(b["bases"].tobytes()) == set(b"ACGTN") and 600_000 < b["bases"].size < 800_000


def test_the_oracle_s_records_of_the_batch(b):
    """what the GPU tests compare with is a batch that maps: nearly every simulated read, the read with an N and the two long cuts"""
    want, diag, idx = b["want"], b["diag"], b["idx"]
    sim = np.array([idx["sim%d" % i] for i in range(K.N_SIM)])
    assert (want["mapped"][sim] != 0).sum() >= 0.9 * K.N_SIM
    for name in ("with_N", "len12287", "len12289", K.STRADDLE_SIM):
        assert want["mapped"][idx[name]] != 0, name
    for name in ("short_l+k-2", "empty", "homopolymer"):
        assert want["mapped"][idx[name]] == 0 and diag["n_kminmers"][idx[name]] == 0, name
    for p in K.TANDEM_PERIODS:  # (the arrays are not in the genome)
        assert want["mapped"][idx["tandem%d" % p]] == 0


def test_shift_residues_and_what_lies_where(b):
    offs = b["offs"]
    n = offs.size - 1
    assert K.SHIFT_NAMES == ("1", "63", "64", "4096+17", "straddle_sim", "straddle_tandem", "2^32", "2^32+1", "2^33+5")
    S = {name: K.shift_of(b, name) for name in K.SHIFT_NAMES}
    assert [S[x] for x in ("1", "63", "64", "4096+17", "2^32", "2^32+1", "2^33+5")] == [1, 63, 64, 4113, 2 ** 32, 2 ** 32 + 1, 2 ** 33 + 5]
    # the first offset's residues mod 64: 0 (twice), 1 (twice), 5, 17, 63 and the two of the straddling shifts
    assert {name: s % 64 for name, s in S.items()} == {"1": 1, "63": 63, "64": 0, "4096+17": 17, "straddle_sim": 37, "straddle_tandem": 21, "2^32": 0,
                                                        "2^32+1": 1, "2^33+5": 5}
    for name in ("1", "63", "64", "4096+17"):
        assert K.straddling(offs, S[name]) == [] and K.wholly_behind(offs, S[name]) == []
    for name in ("2^32", "2^32+1", "2^33+5"):
        assert K.straddling(offs, S[name]) == [] and K.wholly_behind(offs, S[name]) == list(range(n))
    for name, who in (("straddle_sim", K.STRADDLE_SIM), ("straddle_tandem", "tandem7")):
        r = b["idx"][who]
        assert S[name] < P32 and int(offs[0]) + S[name] < P32
        assert K.straddling(offs, S[name]) == [r] and K.wholly_behind(offs, S[name]) == list(range(r + 1, n))
        assert int(offs[r]) + S[name] < P32 < int(offs[r + 1]) + S[name]
        assert min(P32 - (int(offs[r]) + S[name]), int(offs[r + 1]) + S[name] - P32) >= 900  # well inside: a seeder's tile on either side
    # the simulated straddler lies in front of the named shapes, the tandem one among them: at either shift some reads are on each side
    assert b["idx"][K.STRADDLE_SIM] < K.LONG_AT < b["idx"]["tandem7"]
    st = K.tandem_behind_shift(b)
    first = b["idx"]["tandem%d" % K.TANDEM_PERIODS[0]]
    assert int(offs[first]) + st == P32 and K.straddling(offs, st) == [] and K.wholly_behind(offs, st) == list(range(first, n))
    assert all(b["idx"]["tandem%d" % p] >= first for p in K.TANDEM_PERIODS)


def test_straddle_shift_on_other_offsets():
    offs = np.array([0, 7, 7, 5000, 5300, 9000], dtype=np.uint64)
    for r in (2, 3, 4):
        for res in (None, 0, 3, 63):
            s = K.straddle_shift(offs, r, res)
            assert K.straddling(offs, s) == [r] and K.wholly_behind(offs, s) == list(range(r + 1, 5))
            assert res is None or s % 64 == res
    with pytest.raises(AssertionError):
        K.straddle_shift(offs, 0)  # too short to lie across anything with room on both sides


def test_the_periodic_window_rule(b):
    """window_periodic's rule on order_reads_kernel's three windows.  The tandem reads and the homopolymer read satisfy it at every residue
    mod 64 of the first offset (so wherever the batch is put); no other read does at any place the GPU tests put the batch."""
    bases, offs, idx = b["bases"], b["offs"], b["idx"]
    periodic_reads = sorted([idx["tandem%d" % p] for p in K.TANDEM_PERIODS] + [idx["homopolymer"]])
    for r in periodic_reads:
        o0, ln = int(offs[r]), int(offs[r + 1] - offs[r])
        assert ln >= 512
        for res in range(64):
            ws = [w - res for w in K.windows(o0 + res, ln)]
            assert all(o0 <= w and w + 48 <= o0 + ln for w in ws)  # the windows lie inside the read
            assert all(K.periodic(bases[w:w + 48]) for w in ws), (b["names"][r], res)
    want = np.zeros(offs.size - 1, dtype=bool)
    want[periodic_reads] = True
    places = [0] + [K.shift_of(b, name) for name in K.SHIFT_NAMES] + [K.tandem_behind_shift(b)]
    for s in places:
        assert np.array_equal(K.flagged(bases, offs, s), want), s
    assert want.sum() == 7 >= len(K.TANDEM_PERIODS)
    # the rule itself on hand-made windows: 27 of 32 is the bound, lag 16 the largest lag
    rng = np.random.default_rng(3)
    w = K.ACGT[rng.integers(0, 4, 48)]
    assert not K.periodic(w)
    t = np.tile(K.ACGT[rng.integers(0, 4, 16)], 3)
    assert K.periodic(t)
    for n_bad, ok in ((5, True), (6, False)):
        v = np.tile(np.frombuffer(b"ACGTTGCAAGCTCATG", dtype=np.uint8), 3).copy()  # period 16 and no shorter lag comes near
        for i in range(n_bad):
            v[32 + 3 * i] = ord("A") if v[32 + 3 * i] != ord("A") else ord("C")     # positions 32..47: in the lagged copy only, one mismatch each
        assert K.periodic(v) == ok, n_bad


def test_the_batch_with_a_read_past_the_limit(b):
    n = b["offs"].size - 1
    lens = np.diff(b["offs"].astype(np.int64))
    for L in K.LONG_READS:
        o, pieces = K.with_long_read(b, L)
        assert L >> 32 != 0 and o.dtype == np.uint64 and o.size == n + 2
        ln = [int(o[i + 1]) - int(o[i]) for i in range(n + 1)]
        assert ln[K.LONG_AT] == L and [i for i, x in enumerate(ln) if x >> 32] == [K.LONG_AT]
        assert ln[:K.LONG_AT] + ln[K.LONG_AT + 1:] == lens.tolist()
        assert int(o[-1]) - int(o[0]) == b["bases"].size + L
        # the pieces place every ordinary read, and nothing inside the long read
        assert sum(p.size for _, p in pieces) == b["bases"].size
        for r in range(n + 1):
            if r == K.LONG_AT:
                continue
            src = r if r < K.LONG_AT else r - 1
            at, piece = pieces[0] if r < K.LONG_AT else pieces[1]
            got = piece[int(o[r]) - at:int(o[r + 1]) - at]
            assert got.tobytes() == b["bases"][int(b["offs"][src]):int(b["offs"][src + 1])].tobytes()
        assert pieces[0][0] + pieces[0][1].size == int(o[K.LONG_AT]) and pieces[1][0] == int(o[K.LONG_AT + 1])
    assert 0 < K.LONG_AT < n and b["idx"]["tandem2"] > K.LONG_AT  # reads on both sides; the tandem reads behind it


def test_the_staged_records(b):
    recs = K.staged_records(b["g"])
    assert [r[0] for r in recs] == ["one_line", "wrap60", "wrap80_crlf_nofinal"]
    assert K.STAGE_BYTES == 2 ** 32 + 3 * 2 ** 20
    ends = []
    for name, at, region, seq, lines in recs:
        assert 40_000 <= len(seq) <= 120_000 and set(seq) <= set(b"ACGT")
        assert K.join_lines(region) == seq, name
        assert at + len(region) <= K.STAGE_BYTES
        ends.append((at, at + len(region)))
    assert all(ends[i][1] <= ends[i + 1][0] for i in range(2))
    (a0, a1), (b0, _), (c0, _) = ends
    assert a0 == P32 - 50_000 and a0 < P32 < a1 and not recs[0][4] and b"\n" not in recs[0][2]
    assert b0 == P32 + 2 ** 20 + 1 and c0 == P32 + 2 * 2 ** 20 + 15
    w60 = recs[1][2].split(b"\n")
    assert w60[-1] == b"" and all(len(x) == 60 for x in w60[:-2]) and 0 < len(w60[-2]) < 60 and b"\r" not in recs[1][2]
    w80 = recs[2][2].split(b"\r\n")
    assert all(len(x) == 80 for x in w80[:-1]) and 0 < len(w80[-1]) < 80 and not recs[2][2].endswith(b"\n")
    # the join rule on its edges: a '\r' in front of a '\n' or at the very end goes, any other stays
    assert K.join_lines(b"AC\r\nGT\r") == b"ACGT" and K.join_lines(b"A\rC\n\nG\r\r\nT") == b"A\rCG\rT" and K.join_lines(b"") == b""
