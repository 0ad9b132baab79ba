"""A plain-Python restatement of what mq_ctx_submit_fasta / mq_ctx_submit_fastx(MQ_FASTX_FASTQ) / mq_ctx_wait_fasta promise for a piece
buf[begin, len(buf)) (include/mapquik_hip.h), written from the header's text and not from the kernels of mq_fastx.hpp:

  * a line end is every '\\n' at a position in [begin, len(buf)), ascending, and len(buf) itself when the piece is not empty and its
    last byte is not '\\n' (a last line without '\\n' ends where the piece ends);
  * the line-end list holds line_cap(len(buf)) = min(len(buf) / 16 + 4096, 2^28) entries -- len(buf) is the piece's END OFFSET, whatever
    lies in front of `begin` counts; more line ends than that: irregular;
  * a line count that is no multiple of the lines of a record (FASTA 2, FASTQ 4): irregular;
  * FASTA record r = lines 2r (header) and 2r + 1 (sequence): irregular when the header line is empty or does not start with '>', or
    when the sequence line is not empty and starts with '>'; the read is the sequence line without ONE trailing '\\r';
  * FASTQ record r = lines 4r .. 4r + 3: irregular when the header line is empty or does not start with '@', when the third line is
    empty or does not start with '+', or when the sequence and the quality line differ in length once ONE trailing '\\r' is cut from
    each; the read is the sequence line without that '\\r'; an empty sequence with an empty quality line is a record;
  * a '\\r' is cut wherever the line ends: in front of a '\\n', or as the last byte of a last line without '\\n';
  * an empty piece (len(buf) == begin) is regular and has no records;
  * an irregular piece reports nothing: no line ends, no records.

records() returns (line_ends, spans, irregular) with spans = [(start, length)] of every read."""
import numpy as np

FASTA, FASTQ = "fasta", "fastq"
LINES_PER_RECORD = {FASTA: 2, FASTQ: 4}
NL, CR = 0x0A, 0x0D


def line_cap(nbytes):
    """entries of the line-end list of a piece that ends at offset nbytes"""
    return min(nbytes // 16 + 4096, 1 << 28)


def line_ends(buf, begin=0):
    """every '\\n' in buf[begin:], and len(buf) for a last line without one (numpy for the pieces of many megabytes only)"""
    n = len(buf)
    if n - begin > (1 << 20):
        out = (np.flatnonzero(np.frombuffer(buf, dtype=np.uint8)[begin:] == NL) + begin).tolist()
    else:
        out = []
        p = buf.find(b"\n", begin)
        while p >= 0:
            out.append(p)
            p = buf.find(b"\n", p + 1)
    if n > begin and buf[n - 1] != NL:
        out.append(n)
    return out


def _starts_with(buf, line, byte):
    """the line (start, end) is not empty and its first byte is `byte`"""
    return line[0] < line[1] and buf[line[0]] == byte


def _without_cr(buf, line):
    """the line (start, end) as (start, length), one trailing '\\r' not counted"""
    start, end = line
    return start, end - start - (1 if end > start and buf[end - 1] == CR else 0)


def records(buf, begin=0, fmt=FASTA):
    buf = bytes(buf)
    assert 0 <= begin <= len(buf)
    lpr = LINES_PER_RECORD[fmt]
    irregular = ([], [], True)
    ends = line_ends(buf, begin)
    if len(ends) > line_cap(len(buf)) or len(ends) % lpr:
        return irregular
    # line i = buf[start, end): it starts at `begin`, or behind the line end in front of it
    lines = list(zip([begin] + [e + 1 for e in ends[:-1]], ends))
    spans = []
    for r in range(0, len(lines), lpr):
        if fmt == FASTA:
            header, seq = lines[r:r + 2]
            if not _starts_with(buf, header, 0x3E) or _starts_with(buf, seq, 0x3E):
                return irregular
        else:
            header, seq, plus, qual = lines[r:r + 4]
            if not _starts_with(buf, header, 0x40) or not _starts_with(buf, plus, 0x2B):
                return irregular
            if _without_cr(buf, seq)[1] != _without_cr(buf, qual)[1]:
                return irregular
        spans.append(_without_cr(buf, seq))
    return ends, spans, False


def sequences(buf, spans):
    return [bytes(buf[s:s + n]) for s, n in spans]
