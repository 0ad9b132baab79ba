"""GPU: the one-line record scanners (mq_ctx_submit_fasta / mq_ctx_submit_fastx(MQ_FASTX_FASTQ) -> mq_ctx_wait_fasta,
mapquik_amd/csrc/mq_fastx.hpp) on the case table of tests/fastx_records_cases.py against the line model of
tests/fastx_records_model.py: the IRREGULAR decision, the line-end list, the record count -- and the hits, byte for byte, against
map_batch on the model's sequences.  One event on every border of the kernels' units (a), irregular twins on a tile border and the
context's state behind each (b), the line-end list exactly full and one entry over (c), pieces of 1,024 / 1,025 / 2,049 tiles (d),
the contract's decision table on every small piece (e); a and c once more into a poisoned hit buffer.

Two worlds: the fold_case world of tests/test_gpu_fasta_scan.py (a, b, d), and a LENGTH PROBE (c, e): an index with k = l = 1,
density 1 and no homopolymer compression lists one k-min-mer per byte of a read (tests/test_fastx_records_model.py::
test_the_length_probe), so hits["n_kminmers"][r] is the length of the span the scanner handed over and the cut of a '\\r' shows on reads
of one or two bytes.

Cost of a piece (submit + wait: copy, four kernels, one synchronisation, the map launch of a regular piece; plus this module's Python):
each test prints "fastx_records timing <family>: <pieces> pieces <seconds> s".  The first run on an MI355X: 37 us a piece over the
5,461 small FASTA pieces (most of them irregular: no map launch), 235 us a piece over family a (a dozen reads each, map_batch for the
expected hits included), 29 ms for the piece of 2,049 tiles with its map_batch; no test of this module took more than 0.3 s."""
import time

import numpy as np
import pytest

import fastx_records_cases as K
import fastx_records_model as M
from fastx_records_model import FASTA, FASTQ

pytestmark = pytest.mark.gpu

PER_PIECE_US = 37  # submit + wait of a small piece, measured on the first run (a record, not a bound: see the module's docstring)


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture(scope="module")
def world(mq, simlib):
    """the fold_case world of tests/test_gpu_fasta_scan.py: same genome seed, same reads"""
    g, off, names = simlib.make_genome([700000, 400000], seed=91, repeat_frac=0.1, tandem_frac=0.02)
    ix = mq.Index(mq.Params(fold_case=True))
    for r in range(2):
        ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])])
    ix.finalize()
    reads = K.world_reads(simlib)
    return dict(ix=ix, reads=reads, few=K.few(reads))


@pytest.fixture(scope="module")
def probe(mq):
    """the length probe: n_kminmers of a read = its length"""
    ix = mq.Index(mq.Params(k=1, l=1, density=1.0, use_hpc=False))
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(5).integers(0, 4, 400)]
    ix.add_ref(0, "probe", ref)
    ix.finalize()
    return ix


def _map(ix, seqs):
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return ix.map_batch(bases, offs)


def _check(ix, ctx, case, want=None, length_probe=False):
    """one piece through the context against the model and map_batch (want: map_batch's hits of the model's sequences, when the caller
    has them already); returns the hits"""
    name, piece, begin, fmt, _ = case
    ends, spans, irregular = M.records(piece, begin, fmt)
    ctx.submit_fasta(np.frombuffer(piece, dtype=np.uint8), begin=begin, fastq=fmt == FASTQ)
    hits, lines, flags = ctx.wait_fasta()
    assert (flags & 1) == int(irregular), name
    if irregular:
        assert hits.size == 0 and lines.size == 0, name
        return hits
    assert lines.tolist() == ends, name
    assert hits.size == len(spans), name
    if not spans:
        return hits
    if want is None:
        want = _map(ix, M.sequences(piece, spans))
    assert np.array_equal(hits.view(np.uint8), want.view(np.uint8)), name
    if length_probe:
        assert hits["n_kminmers"].tolist() == [n for _, n in spans], name
    return hits


def _timing(family, n, t0):
    print("fastx_records timing %s: %d pieces %.3f s" % (family, n, time.perf_counter() - t0))


def _poisoned(poison, monkeypatch):
    if poison:
        monkeypatch.setenv("MQ_FX_POISON_HITS", "1")  # the hit buffer is filled with 0xFF before the map kernels of every piece


@pytest.mark.parametrize("poison", [False, True])
def test_one_event_on_every_border(mq, world, monkeypatch, poison):
    from test_gpu_poison import _assert_all_written
    ix = world["ix"]
    cases = K.boundary_cases(world["few"])
    assert len(cases) == K.N_BOUNDARY
    _poisoned(poison, monkeypatch)
    ctx = ix.context()
    mapped, t0 = 0, time.perf_counter()
    for case in cases:
        assert case[4](case[1]), case[0]
        hits = _check(ix, ctx, case)
        assert hits.size >= 1, case[0]
        _assert_all_written(hits)
        mapped += int((hits["status"] == 1).sum())
    _timing("a" + ("_poisoned" if poison else ""), len(cases), t0)
    ctx.close()
    assert mapped > 100  # (the floor of families a and d together; d asserts its own as well)


def test_irregular_twins_and_the_context_s_state(mq, world):
    ix, few = world["ix"], world["few"]
    ok = {fmt: ("ok_" + fmt, K.body(few, fmt), 0, fmt, None) for fmt in (FASTA, FASTQ)}
    want = _map(ix, [s for _, s in few])
    cases = K.irregular_twins(few)
    assert len(cases) == K.N_TWINS
    ctx = ix.context()
    t0 = time.perf_counter()
    for k, case in enumerate(cases):
        assert case[4](case[1]), case[0]
        hits = _check(ix, ctx, case)
        assert hits.size == 0 and M.records(case[1], case[2], case[3])[2], case[0]
        # the next regular piece on the same context: its full result (the twin's own format, then the other one)
        for fmt in ((case[3],) if k % 2 else (case[3], FASTQ if case[3] == FASTA else FASTA)):
            assert _check(ix, ctx, ok[fmt], want).size == len(few), case[0]
    _timing("b", len(cases), t0)
    ctx.close()
    assert (want["status"] == 1).sum() >= 8


@pytest.mark.parametrize("poison", [False, True])
def test_line_end_list_exactly_full(mq, probe, monkeypatch, poison):
    """lines == capacity: every record reported (the unterminated piece writes its virtual line end into the list's last entry);
    lines == capacity + 1: irregular, nothing reported (the unterminated piece must not write that entry)"""
    from test_gpu_poison import _assert_all_written
    _poisoned(poison, monkeypatch)
    ctx = probe.context()
    t0 = time.perf_counter()
    cases = K.capacity_cases()
    for case in cases + cases[::-1]:  # (and in the other order: a full list behind an overfull one, on the same context)
        assert case[4](case[1]), case[0]
        hits = _check(probe, ctx, case, length_probe=True)
        _assert_all_written(hits)
        assert hits.size == (K.SHORTEST[case[3]][1] if case[0].startswith("c_full_") else 0), case[0]
    _timing("c" + ("_poisoned" if poison else ""), 2 * len(cases), t0)
    ctx.close()


@pytest.mark.parametrize("n_tiles,fmt", K.TILE_RUNS)
def test_tile_runs(mq, world, n_tiles, fmt):
    """more tiles than the scan has threads: a thread owns 2 (1,025 tiles) or 3 (2,049) tiles and the last threads own none; a record
    border on the border of two threads' runs, a line end in the last tile"""
    ix = world["ix"]
    piece, border, sb = K.tile_run_piece(n_tiles, fmt, world["reads"])
    assert (len(piece) + K.TILE - 1) // K.TILE == n_tiles and piece[border - 1] == K.NL and piece[border] == K.FIRST[fmt]
    ctx = ix.context()
    t0 = time.perf_counter()
    hits = _check(ix, ctx, ("d_%d_%s" % (n_tiles, fmt), piece, 0, fmt, None))
    _timing("d_%d_%s" % (n_tiles, fmt), 1, t0)
    ctx.close()
    assert hits.size > 900 and (hits["status"] == 1).sum() > 100


@pytest.mark.parametrize("family", ["fasta", "prefixed", "fastq", "sampled"])
def test_small_pieces(mq, probe, family):
    """the decision table: every small piece, each compared with the model; the expected hits of all regular pieces of the family come
    from ONE map_batch call"""
    cases = {"fasta": K.small_fasta, "prefixed": K.small_fasta_prefixed, "fastq": K.small_fastq, "sampled": K.sampled_fastq}[family]()
    assert len(cases) == K.N_SMALL[family]
    model = [M.records(p, b, f) for _, p, b, f, _ in cases]
    seqs, first = [], []
    for (_, piece, _, _, _), (_, spans, _) in zip(cases, model):
        first.append(len(seqs))
        seqs += M.sequences(piece, spans)
    want_all = _map(probe, seqs)
    assert want_all["n_kminmers"].tolist() == [len(s) for s in seqs]
    ctx = probe.context()
    n_regular, t0 = 0, time.perf_counter()
    for case, (_, spans, irregular), at in zip(cases, model, first):
        hits = _check(probe, ctx, case, want_all[at:at + len(spans)], length_probe=True)
        n_regular += 0 if irregular else 1
    _timing("e_" + family, len(cases), t0)
    ctx.close()
    assert n_regular >= 20 and len(seqs) >= 20
