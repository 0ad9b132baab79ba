"""Case table for MQ_FASTX_FASTA_LINES (line-wrapped FASTA reads joined on the device): a wrapper, and a small constructor that places
ONE event at a chosen absolute position of a piece.  The kernels' units are tiles of 16,384 bytes, iterations of 1,024 and lane pieces
of 16 (fasta_lines_model.TILE / ITER / LANE).  Every case is (name, piece bytes, property): the property is a predicate on the bytes
that says the case is what its name says -- tests/test_fasta_lines_model.py checks it on the CPU, tests/test_gpu_fasta_lines.py runs
the same table on the device.  `reads` everywhere: [(id bytes, sequence bytes)], sequences non-empty and free of line ends."""
import numpy as np

from fasta_lines_model import ITER, LANE, TILE


def wrap(seq, width, nl=b"\n"):
    """seq in lines of `width` bytes, every line closed by nl (numpy: a read of megabytes at width 1 stays quick)"""
    a = np.frombuffer(seq, dtype=np.uint8)
    full = a.size // width
    e = np.frombuffer(nl, dtype=np.uint8)
    rows = np.empty((full, width + e.size), dtype=np.uint8)
    rows[:, :width] = a[:full * width].reshape(full, width)
    rows[:, width:] = e
    rest = a[full * width:].tobytes()
    return rows.tobytes() + (rest + nl if rest else b"")


def fasta(reads, width=80, nl=b"\n", final_newline=True, desc=b" d"):
    txt = b"".join(b">" + i + desc + nl + wrap(s, width, nl) for i, s in reads)
    return txt if final_newline else txt[:-len(nl)]


def filler(nbytes):
    """one whole record (id 'f', bases 'A' in 60-column lines) of exactly nbytes >= 5 bytes: what stands in front of a placed event"""
    assert nbytes >= 5
    if nbytes < 80:
        return b">f" + b"x" * (nbytes - 5) + b"\nA\n"
    n_lines = (nbytes - 10) // 61
    rest = nbytes - 61 * n_lines
    return b">f" + b"x" * (rest - 3) + b"\n" + (b"A" * 60 + b"\n") * n_lines


def _hdr(i):
    return b">" + i + b" d"


def header_start_at(pos, reads):
    """a header start at pos; its '\\n' is the byte in front"""
    return filler(pos) + fasta(reads, 70)


def cr_then_nl_at(pos, reads):
    """CR-LF lines; a sequence line's '\\r' at pos - 1 and its '\\n' at pos"""
    (i, s), rest = reads[0], reads[1:]
    assert len(s) > 60
    return filler(pos - 1 - 60 - len(_hdr(i)) - 2) + _hdr(i) + b"\r\n" + wrap(s, 60, b"\r\n") + fasta(rest, 60, b"\r\n")


def header_crosses(pos, reads):
    """a header line that begins 5 bytes in front of pos and ends behind it"""
    return filler(pos - 5) + fasta(reads, 70, desc=b" a header line that is long enough to cross")


def long_header_at(pos, reads):
    """a header line of more than three tiles (two whole tiles without an event, wherever it starts) beginning at pos"""
    (i, s), rest = reads[0], reads[1:]
    return filler(pos) + b">" + i + b" " + b"h" * (3 * TILE + 100) + b"\n" + wrap(s, 80) + fasta(rest, 80)


def seq_line_ends_at(pos, reads):
    """a sequence line whose '\\n' is at pos - 1: the next line starts at pos"""
    (i, s), rest = reads[0], reads[1:]
    assert len(s) > 120
    return filler(pos - 1 - 60 - len(_hdr(i)) - 1) + _hdr(i) + b"\n" + wrap(s, 60) + fasta(rest, 60)


def gt_in_sequence_at(pos, reads):
    """a '>' at pos in the middle of a sequence line (of a small record of its own: the reads keep their bytes)"""
    return filler(pos - 3 - 9) + b">g\nACGTACGTA>CGTACGT\nAC\n" + fasta(reads, 80)


def gt_in_header_at(pos, reads):
    """a '>' at pos in the middle of a header line, behind the id"""
    (i, s), rest = reads[0], reads[1:]
    return filler(pos - len(_hdr(i)) - 1) + _hdr(i) + b" >x>\n" + wrap(s, 80) + fasta(rest, 80)


def _is_line_start(d, p):
    return p == 0 or d[p - 1] == 0x0A


def boundary_cases(reads):
    """[(name, piece, property(piece) -> bool)]; every placed case at its unit border and one byte to either side"""
    out = []
    units = {"tile": 2 * TILE, "iteration": TILE + 3 * ITER, "lane": TILE + ITER + 5 * LANE}
    for unit, at in units.items():
        for pos in (at - 1, at, at + 1):
            out.append(("header_start_%s_%d" % (unit, pos), header_start_at(pos, reads),
                        lambda d, p=pos: d[p] == 0x3E and d[p - 1] == 0x0A))
    at = 2 * TILE
    for pos in (at - 1, at, at + 1):
        out.append(("cr_last_nl_first_%d" % pos, cr_then_nl_at(pos, reads), lambda d, p=pos: d[p - 1] == 0x0D and d[p] == 0x0A and not _is_line_start(d, p - 1)))
        out.append(("header_crosses_%d" % pos, header_crosses(pos, reads),
                    lambda d, p=pos: d[p - 5] == 0x3E and _is_line_start(d, p - 5) and d.find(b"\n", p - 5) > p))
        out.append(("long_header_%d" % pos, long_header_at(pos, reads),
                    lambda d, p=pos: d[p] == 0x3E and _is_line_start(d, p) and d.find(b"\n", p) - p > 3 * TILE))
        out.append(("seq_line_ends_%d" % pos, seq_line_ends_at(pos, reads),
                    lambda d, p=pos: d[p - 1] == 0x0A and d[p] not in (0x3E, 0x0A) and d[p - 2] not in (0x0A, 0x0D) and d.rfind(b"\n", 0, p - 1) + 1 < p - 1
                    and d[d.rfind(b"\n", 0, p - 1) + 1] != 0x3E))
        out.append(("gt_in_sequence_%d" % pos, gt_in_sequence_at(pos, reads),
                    lambda d, p=pos: d[p] == 0x3E and d[p - 1] == 0x41 and d[d.rfind(b"\n", 0, p) + 1] != 0x3E))
        out.append(("gt_in_header_%d" % pos, gt_in_header_at(pos, reads),
                    lambda d, p=pos: d[p] == 0x3E and not _is_line_start(d, p) and d[d.rfind(b"\n", 0, p) + 1] == 0x3E))
    body = fasta(reads, 80)
    out.append(("ends_inside_a_header_line", body + b">the last header has no line end", lambda d: d[d.rfind(b"\n") + 1] == 0x3E and not d.endswith(b"\n")))
    out.append(("last_line_without_newline", body[:-1], lambda d: not d.endswith(b"\n") and d[d.rfind(b"\n") + 1] != 0x3E))
    return out


IRREGULAR_BOUNDARY = {"ends_inside_a_header_line"}  # that record has no sequence

# pieces that come back MQ_FASTA_IRREGULAR, by the condition each one meets
IRREGULAR_PIECES = {
    "no_leading_gt": b"ACGT\n>a\nACGT\n",
    "record_without_sequence": b">a\n>b\nACGT\n",
    "more_records_than_spans": b">a\nAC\n" * 40000,
}
JUST_UNDER_THE_SPAN_CAP = b">a\nAC\n" * 2400
