"""No GPU: the case table of the one-line record scanners (tests/fastx_records_cases.py) against itself -- every case has the property it
is named after, every family has its count, the model (tests/fastx_records_model.py) calls regular what must be regular -- and the
model against the host parser the product falls back to (parse_chunk, and the driver's line-end scan, through feeder_dump, one chunk per
file): a piece the device may call regular yields the same reads as the host parser.  Also the length probe the GPU side relies on: with
k = l = 1, density 1 and no homopolymer compression the oracle lists one k-min-mer per byte of a read."""
import os
import subprocess

import numpy as np
import pytest

import fasta_lines_model as ML
import fastx_records_cases as K
import fastx_records_model as M
from fastx_records_model import FASTA, FASTQ


@pytest.fixture(scope="module")
def reads(simlib):
    return K.world_reads(simlib)


@pytest.fixture(scope="module")
def few(reads):
    return K.few(reads)


@pytest.fixture(scope="module")
def tool():
    from mapquik_amd import build as B
    return B.build_feeder_dump()


def _check_family(cases, n, regular):
    assert len(cases) == len({c[0] for c in cases}) == n
    for name, piece, begin, fmt, prop in cases:
        assert prop(piece), name
        ends, spans, irregular = M.records(piece, begin, fmt)
        assert irregular == (not regular(name)), name
        assert len(ends) == M.LINES_PER_RECORD[fmt] * len(spans) and (not irregular or not ends), name


def test_every_boundary_case_has_its_property(few):
    cases = K.boundary_cases(few)
    assert K.N_BOUNDARY == 276
    _check_family(cases, K.N_BOUNDARY, lambda name: True)
    for name, piece, begin, fmt, _ in cases:  # the reads come through whole, behind (or in front of) whatever the constructor placed
        seqs = M.sequences(piece, M.records(piece, begin, fmt)[1])
        want = [s for _, s in few]
        if "_end_" not in name:
            assert seqs[-12:] == want, name
        elif fmt == FASTA:  # the last read ends where the piece ends, less the bytes that end its line
            start, n = M.records(piece, begin, fmt)[1][-1]
            assert start + n + len(K.END_FORMS[name.split("_")[2]]) == len(piece) and n > 0, name
    # the '\r' of every CR case is cut, wherever the line ends
    for name, piece, begin, fmt, _ in cases:
        if "_cr" in name:
            assert not any(s.endswith(b"\r") for s in M.sequences(piece, M.records(piece, begin, fmt)[1])), name


def test_every_irregular_twin_has_its_property(few):
    cases = K.irregular_twins(few)
    assert K.N_TWINS == 27
    _check_family(cases, K.N_TWINS, lambda name: False)
    # each twin is one offence away from regular: the block in front of it alone is regular
    for name, piece, begin, fmt, _ in cases:
        cut = piece.rfind(b"\n" + bytes([K.FIRST[fmt]]), 0, K.TILE - 60) + 1
        assert cut > 0 and not M.records(piece[:cut], 0, fmt)[2], name


def test_capacity_cases_fill_the_list_exactly():
    cases = K.capacity_cases()
    _check_family(cases, K.N_CAPACITY, lambda name: name.startswith("c_full_"))
    by = {c[0]: c[1] for c in cases}
    # the numbers of the FASTA cases: 2,521 records, 10 more bases: 15,136 bytes, 5,042 line ends in a list of 5,042; 9: a list of 5,041
    assert K.capacity_pad(FASTA, True) == 10
    full, over = by["c_full_fasta_nl"], by["c_over_fasta_nl"]
    assert (len(full), M.line_cap(len(full)), len(M.line_ends(full))) == (15136, 5042, 5042)
    assert (len(over), M.line_cap(len(over)), len(M.line_ends(over))) == (15135, 5041, 5042)
    assert len(M.records(full, 0, FASTA)[1]) == 2521
    # without the last '\n' the virtual line end is the list's last entry (index capacity - 1), or the one that does not fit
    for fmt, lpr in ((FASTA, 2), (FASTQ, 4)):
        n = K.SHORTEST[fmt][1]
        full, over = by["c_full_%s_no_nl" % fmt], by["c_over_%s_no_nl" % fmt]
        assert full.count(b"\n") == M.line_cap(len(full)) - 1 and M.records(full, 0, fmt)[0][-1] == len(full)
        assert over.count(b"\n") == M.line_cap(len(over)) and len(M.line_ends(over)) == lpr * n
        assert len(M.records(by["c_full_%s_nl" % fmt], 0, fmt)[1]) == n
    assert K.SHORTEST[FASTQ][1] == 1192 and len(by["c_full_fastq_nl"]) == 9 * 1192 + 2 * K.capacity_pad(FASTQ, True) == 10752


def test_tile_run_cases(reads):
    n = 0
    for name, piece, begin, fmt, prop in K.tile_run_cases(reads):
        n += 1
        assert prop(piece), name
        ends, spans, irregular = M.records(piece, begin, fmt)
        assert not irregular and len(spans) > 900 and len(piece) <= 34 * (1 << 20), name
        assert ends == (np.flatnonzero(np.frombuffer(piece, dtype=np.uint8) == 10)).tolist(), name
    assert n == len(K.TILE_RUNS) == 4


def test_small_pieces_and_the_decision_table():
    fa, pre, fq, smp = K.small_fasta(), K.small_fasta_prefixed(), K.small_fastq(), K.sampled_fastq()
    assert (len(fa), len(pre), len(fq), len(smp)) == (5461, 341, 4802, 2000) == tuple(K.N_SMALL[k] for k in ("fasta", "prefixed", "fastq", "sampled"))
    assert len({c[1] for c in fa}) == 5461 and [c[:4] for c in smp] == [c[:4] for c in K.sampled_fastq()]
    n_regular = {}
    for fam, cases in (("fasta", fa), ("prefixed", pre), ("fastq", fq), ("sampled", smp)):
        for name, piece, begin, fmt, prop in cases:
            assert prop(piece), name
        n_regular[fam] = sum(not M.records(p, b, f)[2] for _, p, b, f, _ in cases)
    # the junk in front of `begin` changes no decision
    assert [M.records(p, b, f)[2] for _, p, b, f, _ in pre] == [M.records(p, 0, f)[2] for _, p, _, f, _ in fa if len(p) <= 4]
    assert n_regular["fasta"] > 300 and n_regular["fastq"] > 20 and 300 < n_regular["sampled"] < 1500, n_regular
    # the contract's corners, spelled out
    R = M.records
    assert R(b"", 0, FASTA) == ([], [], False) and R(b"xx\n", 3, FASTQ) == ([], [], False)
    assert R(b">\n", 0, FASTA)[2] and R(b">\n\n", 0, FASTA) == ([1, 2], [(2, 0)], False)
    assert R(b">\nA", 0, FASTA) == ([1, 3], [(2, 1)], False) and R(b">\nA\r", 0, FASTA) == ([1, 4], [(2, 1)], False)
    assert R(b">\n\r\n", 0, FASTA) == ([1, 3], [(2, 0)], False) and R(b">\n\r\r\n", 0, FASTA)[1] == [(2, 1)]
    assert R(b"\n>\nA\n", 0, FASTA)[2] and R(b">\n>\n", 0, FASTA)[2] and R(b"A\nA\n", 0, FASTA)[2] and R(b"\r\nA\n", 0, FASTA)[2]
    assert R(b"@\n\n+\n\n", 0, FASTQ) == ([1, 2, 4, 5], [(2, 0)], False) and R(b"@\n\n+\n", 0, FASTQ)[2]
    assert R(b"@\nA\r\n+\nA", 0, FASTQ) == ([1, 4, 6, 8], [(2, 1)], False) and R(b"@\nA\n+\nA\r", 0, FASTQ)[1] == [(2, 1)]
    assert R(b"@\n@\n+\n+\n", 0, FASTQ)[1] == [(2, 1)] and R(b"@\nAA\n+\nA\n", 0, FASTQ)[2] and R(b"@\nA\n\nA\n", 0, FASTQ)[2]


def _dump(tool, path, fmt, env=None):
    """([(length, sequence)], stderr) of feeder_dump over the file as ONE chunk, one thread"""
    r = subprocess.run([tool, str(path), fmt, str(1 << 30), "1"], capture_output=True, timeout=300, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, (str(path), r.stderr[-2000:])
    out = []
    for ln in r.stdout.split(b"\n")[:-1]:
        _, n, s = ln.rsplit(b"\t", 2)
        out.append((int(n), s))
    return out, r.stderr.decode()


def _host_equals_model(tool, tmp_path, name, piece, fmt):
    """the host parser's reads of a piece the model calls regular: FASTA through parse_chunk and through the driver's own line-end scan
    (which must call the piece regular too); FASTQ through parse_chunk and through the lean reader the driver uses by default"""
    ends, spans, irregular = M.records(piece, 0, fmt)
    assert not irregular, name
    want = [(n, piece[s:s + n]) for s, n in spans]
    p = tmp_path / ("%s.%s" % (name, "fa" if fmt == FASTA else "fq"))
    p.write_bytes(piece)
    if fmt == FASTA:
        assert _dump(tool, p, fmt)[0] == want, (name, "parse_chunk")
        got, err = _dump(tool, p, fmt, {"FEEDER_DUMP_UNPARSED": "1"})
        assert got == want, (name, "line-end scan")
        assert "unparsed chunks %d irregular 0 " % (1 if piece else 0) in err, (name, err)
    else:
        assert _dump(tool, p, fmt, {"MQ_FEEDER_NO_LEAN_FASTQ": "1"})[0] == want, (name, "parse_chunk")
        assert _dump(tool, p, fmt)[0] == want, (name, "lean reader")


def test_model_equals_the_host_parser_on_the_lattice(tool, tmp_path, few):
    n = 0
    for name, piece, begin, fmt, _ in K.boundary_cases(few) + [c for c in K.capacity_cases() if c[0].startswith("c_full_")]:
        if begin:
            continue
        _host_equals_model(tool, tmp_path, name, piece, fmt)
        n += 1
    assert n == K.N_BOUNDARY - 2 * len(K.UNITS) * len(K.DELTAS) + 4


def test_host_parser_on_the_irregular_twins(tool, tmp_path, few):
    """What the driver does with a piece the device hands back: FASTA -- its own line-end scan calls the piece irregular as the model
    does, and parse_chunk gives the reads of the several-lines rule (tests/fasta_lines_model.py) where that rule has an answer; FASTQ --
    the pieces are malformed files: parse_chunk must end by itself, with reads or with its error."""
    n = 0
    for name, piece, begin, fmt, _ in K.irregular_twins(few):
        p = tmp_path / (name + (".fa" if fmt == FASTA else ".fq"))
        p.write_bytes(piece)
        n += 1
        if fmt == FASTQ:
            r = subprocess.run([tool, str(p), fmt, str(1 << 30), "1"], capture_output=True, timeout=300, env=dict(os.environ, MQ_FEEDER_NO_LEAN_FASTQ="1"))
            assert r.returncode in (0, 1) and (r.returncode == 0 or b"malformed" in r.stderr), (name, r.returncode, r.stderr[-500:])
            continue
        got, err = _dump(tool, p, fmt, {"FEEDER_DUMP_UNPARSED": "1"})
        assert "unparsed chunks 1 irregular 1 " in err, (name, err)
        assert got == _dump(tool, p, fmt)[0], name
        recs = ML.records(piece)
        if recs is not None:
            assert got == [(len(s), s) for _, _, s in recs], name
        else:
            # a header with no sequence byte: an empty read there, and every other read as if that header line were not in the file
            assert "hdr_no_seq" in name or "last_cut_short" in name, name
            lone = b">lonely header\n" if "hdr_no_seq" in name else b">the last header\n"
            rest = piece.replace(lone, b"")
            ends, spans, irregular = M.records(rest, 0, fmt)
            assert not irregular and len(got) == len(spans) + piece.count(lone) and piece.count(lone) == (2 if "hdr_no_seq" in name else 1), name
            assert [x for x in got if x[0]] == [(k, rest[a:a + k]) for a, k in spans], name
    assert n == K.N_TWINS


def test_model_equals_the_host_parser_on_small_pieces(tool, tmp_path):
    """300 of the enumerated and sampled pieces (begin = 0) that the model calls regular, drawn with a fixed seed"""
    pool = [c for c in K.small_fasta() + K.small_fastq() + K.sampled_fastq() if not M.records(c[1], 0, c[3])[2]]
    rng = np.random.default_rng(77)
    pick = sorted(rng.choice(len(pool), 300, replace=False).tolist())
    assert {pool[k][3] for k in pick} == {FASTA, FASTQ}
    for k in pick:
        name, piece, _, fmt, _ = pool[k]
        _host_equals_model(tool, tmp_path, name, piece, fmt)


def test_the_length_probe(oracle):
    """k = l = 1, density 1, no homopolymer compression: one k-min-mer per byte, whatever the byte -- hits["n_kminmers"] of a read mapped
    against such an index is the length of the span the scanner handed over"""
    po = oracle.params(k=1, l=1, density=1.0, use_hpc=False)
    for s in (b"A", b"ACGT", b"AC\rGT", b"A\r", b"NNN", b">", b"@A", b"+", b"AAAA", b"ACGTN" * 20):
        assert len(oracle.kminmers(s, po)) == len(s), s
    assert len(oracle.kminmers(b"", po)) == 0
