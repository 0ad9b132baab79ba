"""A plain-Python restatement of the record rule of MQ_FASTX_FASTA_LINES (include/mapquik_hip.h; the FASTA rule of parse_chunk,
mapquik_amd/csrc/host/fastx_records.hpp), written from the rule's text and not from the kernels of mq_fastx_lines.hpp:

  * a header start is a '>' at position `begin`, or directly behind a '\\n';
  * a header line runs from a header start to the next '\\n', or to the end of the piece;
  * record r is header line r plus everything up to the next header start;
  * a byte belongs to the sequence of record r when it lies behind r's header line, is not '\\n', and is not a '\\r' whose next byte
    is '\\n' or which is the piece's last byte; empty lines contribute nothing;
  * a '>' that is not at a line start is an ordinary byte, in a header and in a sequence line.

Irregular (None): a non-empty piece that does not start with '>', more records than the span arrays hold, a record without a sequence
byte.  An empty piece is regular and has no records."""

TILE, ITER, LANE = 16384, 1024, 16  # the kernels' units: a wave's tile, one iteration of 64 lanes, a lane's piece


def span_cap(nbytes):
    """records the span arrays of a piece of nbytes bytes hold: half of the line capacity min(nbytes / 16 + 4096, 2^28)"""
    return min(nbytes // 16 + 4096, 1 << 28) // 2


def header_starts(data, begin=0):
    """positions of every '>' at `begin` or directly behind a '\\n' (bytes.find, so that a piece of many megabytes stays quick)"""
    hs = [begin] if begin < len(data) and data[begin] == 0x3E else []
    p = data.find(b"\n>", begin)
    while p >= 0:
        hs.append(p + 1)
        p = data.find(b"\n>", p + 1)
    return hs


def records(data, begin=0):
    """None (irregular) or [(hdr_begin, hdr_end, sequence bytes)] of data[begin:]; header r is data[hdr_begin:hdr_end]."""
    data = bytes(data)
    end = len(data)
    if begin >= end:
        return []
    if data[begin] != 0x3E:
        return None
    hs = header_starts(data, begin)
    if len(hs) > span_cap(end):
        return None
    out = []
    for r, hb in enumerate(hs):
        nxt = hs[r + 1] if r + 1 < len(hs) else end
        he = data.find(b"\n", hb, nxt)
        if he < 0:
            he = nxt  # (only the last header line can lack its '\n': a header start lies behind one)
        # everything behind the header line, split at every '\n'; a '\r' goes when a '\n' follows it or when it is the piece's last byte (a
        # region that ends in front of a header start ends with '\n', so its last part is empty unless the piece ends here)
        seq = b"".join(ln[:-1] if ln.endswith(b"\r") else ln for ln in data[he + 1:nxt].split(b"\n"))
        if not seq:
            return None
        out.append((hb, he, seq))
    return out


def fasta_id(header_line):
    """seq_io's id() of a header line ('>' first, no '\\n'): the bytes behind '>' up to the first space; one trailing '\\r' is not part of it"""
    if len(header_line) > 1 and header_line.endswith(b"\r"):
        header_line = header_line[:-1]
    return header_line[1:].split(b" ")[0]
