"""No GPU: the line model of MQ_FASTX_FASTA_LINES (tests/fasta_lines_model.py) against the host parser -- parse_chunk through
feeder_dump, one chunk per file: ids and sequences of every regular case -- and the case table of tests/fasta_lines_cases.py against
itself: every boundary case has the property it is named after, the irregular set is exactly the three conditions, and the piece of
2,400 tiny records stays within the span arrays while 40,000 do not."""
import subprocess

import numpy as np
import pytest

import fasta_lines_cases as K
import fasta_lines_model as M


def _reads(n=6, seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        s = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, 150 + 977 * i)].tobytes()
        out.append((b"read%d" % i, s))
    return out


def _whole_file_cases():
    rd = _reads()
    out = {}
    for w in (1, 15, 16, 17, 60, 70, 80, 1023, 1024, 1025):
        out["w%d" % w] = K.fasta(rd, w)
    out["crlf"] = K.fasta(rd, 60, b"\r\n")
    out["crlf_no_final_newline"] = K.fasta(rd, 60, b"\r\n", final_newline=False)
    out["final_cr_without_nl"] = K.fasta(rd, 60, b"\r\n")[:-1]
    out["no_final_newline"] = K.fasta(rd, 70, final_newline=False)
    out["mixed_wrap"] = b"".join(K.fasta([r], 10 ** 6 if i % 2 else 70) for i, r in enumerate(rd))
    out["empty_lines"] = b"".join(b">" + i + b"\n" + K.wrap(s[:100], 60) + b"\n\n" + K.wrap(s[100:], 60) + b"\n" for i, s in rd)
    out["lone_cr_inside_a_line"] = b">a x\nAC\rGT\nTT\n>b\nGG\r\n\r\nCC\n"
    return out


@pytest.fixture(scope="module")
def tool():
    from mapquik_amd import build as B
    return B.build_feeder_dump()


def _parse_chunk(tool, data, tmp_path, name):
    """[(id, sequence)] as parse_chunk gives them: feeder_dump's lines, split at the last two TABs"""
    p = tmp_path / (name + ".fa")
    p.write_bytes(data)
    r = subprocess.run([tool, str(p), "fasta", str(1 << 30), "2"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = []
    for ln in r.stdout.split(b"\n")[:-1]:
        i, n, s = ln.rsplit(b"\t", 2)
        assert int(n) == len(s)
        out.append((i, s))
    return out


def test_model_equals_the_host_parser_on_every_regular_case(tool, tmp_path):
    cases = dict(_whole_file_cases())
    for name, piece, _ in K.boundary_cases(_reads()):
        cases[name] = piece
    cases["just_under_the_span_cap"] = K.JUST_UNDER_THE_SPAN_CAP
    n_regular = 0
    for name, data in cases.items():
        recs = M.records(data)
        if recs is None:
            assert name in K.IRREGULAR_BOUNDARY, name
            continue
        n_regular += 1
        got = _parse_chunk(tool, data, tmp_path, name)
        assert [(M.fasta_id(data[hb:he]), s) for hb, he, s in recs] == got, name
    assert n_regular == len(cases) - len(K.IRREGULAR_BOUNDARY) >= 40


def test_begin_shifts_the_spans_and_nothing_else():
    for name, data in _whole_file_cases().items():
        want = M.records(data)
        got = M.records(b"x" * 36 + b"\n" + data, 37)
        assert got == [(hb + 37, he + 37, s) for hb, he, s in want], name
    assert M.records(b"", 0) == [] and M.records(b"xx\n", 3) == []


def test_every_boundary_case_has_its_property():
    rd = _reads()
    cases = K.boundary_cases(rd)
    assert len({n for n, _, _ in cases}) == len(cases) >= 9 + 18 + 2
    for name, piece, prop in cases:
        assert prop(piece), name
        recs = M.records(piece)
        assert (recs is None) == (name in K.IRREGULAR_BOUNDARY), name
        if recs is not None:  # the reads come through whole, behind whatever the constructor put in front
            assert [s for _, _, s in recs][-len(rd):] == [s for _, s in rd], name
            assert [M.fasta_id(piece[hb:he]) for hb, he, _ in recs][-len(rd):] == [i for i, _ in rd], name
    # a '>' away from a line start opens no record
    for name, piece, _ in cases:
        if name.startswith("gt_in_"):
            assert len(M.records(piece)) == len(rd) + (2 if "sequence" in name else 1), name


def test_the_irregular_set_is_exactly_the_three_conditions():
    for name, piece in K.IRREGULAR_PIECES.items():
        assert M.records(piece) is None, name
    # each piece meets its own condition and no other
    p = K.IRREGULAR_PIECES["no_leading_gt"]
    assert p[0] != 0x3E and M.records(p[p.index(b">"):]) is not None
    p = K.IRREGULAR_PIECES["record_without_sequence"]
    assert p[0] == 0x3E and len(M.header_starts(p)) <= M.span_cap(len(p)) and M.records(p[3:]) is not None
    p = K.IRREGULAR_PIECES["more_records_than_spans"]
    assert p[0] == 0x3E and len(M.header_starts(p)) == 40000 > M.span_cap(len(p))
    # and the other way round: a piece with none of the three is regular, whatever else it holds
    for odd in (b">a\n\n\nAC\n", b">a\r\nA\r", b">\nA", b">a>b\nA>C\n", b">a\nA\n\n>b\n\nC"):
        assert M.records(odd) is not None, odd
    assert M.records(b">a\n\r\n") is None and M.records(b">a") is None and M.records(b">a\n>b\nAC\n>c\n") is None


def test_span_cap_of_the_tiny_record_pieces():
    """2,400 records of 6 bytes fit the span arrays of their piece ((14,400 / 16 + 4,096) / 2 = 2,498); 40,000 do not (9,548)."""
    small, big = K.JUST_UNDER_THE_SPAN_CAP, K.IRREGULAR_PIECES["more_records_than_spans"]
    assert M.span_cap(len(small)) == 2498 and M.span_cap(len(big)) == 9548
    recs = M.records(small)
    assert recs is not None and len(recs) == 2400 <= M.span_cap(len(small))
    assert all(s == b"AC" for _, _, s in recs) and recs[1][:2] == (6, 8)
    assert M.records(big) is None
