"""Case table for the one-line record scanners (mq_ctx_submit_fasta / mq_ctx_submit_fastx(MQ_FASTX_FASTQ), mapquik_amd/csrc/mq_fastx.hpp):
small constructors that place ONE event at a chosen absolute position of a piece.  The kernels are built from a lane's load of 16 bytes,
a wave's pass of 1,024, a tile of 16,384 and -- beyond 1,024 tiles -- a scan thread's run of several tiles; the list of line ends holds
len / 16 + 4096 entries.  Every case is (name, piece, begin, fmt, prop): prop(piece) is a predicate on the bytes that says the event
sits where the name says.  tests/test_fastx_records_model.py checks every prop on the CPU and the model (tests/fastx_records_model.py)
against the host parser; tests/test_gpu_fastx_records.py runs the same table on the device.

  a  boundary_cases    one event at U + d, U in UNITS, d in DELTAS, both formats: all regular
  b  irregular_twins   the irregularities the header names, the offending line start / line end at 16,384 + d
  c  capacity_cases    pieces of the shortest records with exactly as many line ends as the list holds, and one (line) too many
  d  tile_run_cases    1,024 / 1,025 / 2,049 tiles: a record border on the border of two scan threads' runs
  e  small pieces      every FASTA piece of up to 6 bytes over {'>', 'A', CR, LF}; every 4-line FASTQ piece over a 7-line vocabulary;
                       2,000 sampled 2- and 3-record FASTQ pieces; the FASTA pieces of up to 4 bytes behind 37 bytes of junk

`reads` everywhere: [(id bytes, sequence bytes)], sequences free of line ends."""
import itertools

import numpy as np

import fastx_records_model as M
from fastx_records_model import FASTA, FASTQ

LANE, PASS, TILE = 16, 1024, 16384
UNITS = (LANE, PASS, TILE, 2 * TILE)
DELTAS = (-1, 0, 1)
NL, CR, GT, AT, PLUS = 0x0A, 0x0D, 0x3E, 0x40, 0x2B
FIRST = {FASTA: GT, FASTQ: AT}
LPR = M.LINES_PER_RECORD
MIN_FILLER = {FASTA: 5, FASTQ: 9}
JUNK = b"\n>@+\r"


def world_reads(simlib):
    """the 700 reads of the fold_case world of tests/test_gpu_fasta_scan.py (same genome seed, same reads) as [(id, sequence)]"""
    g, off, names = simlib.make_genome([700000, 400000], seed=91, repeat_frac=0.1, tandem_frac=0.02)
    rd = simlib.make_reads(g, off, 700, seed=12, len_mean=9000, len_sd=5000, len_min=1)
    rn = simlib.read_names(rd, names)
    o = rd["offsets"]
    return [(rn[i].encode(), rd["bases"][int(o[i]):int(o[i + 1])].tobytes()) for i in range(len(rn))]


def few(reads):
    """a dozen of the reads of 300 .. 6,000 bases (the `few` of tests/test_gpu_fasta_lines.py): what stands behind a placed event"""
    pick = [r for r in reads if 300 <= len(r[1]) <= 6000][:12]
    assert len(pick) == 12
    return pick


# ---------------------------------------------------------------- records and blocks of an exact size
def record(i, s, fmt, nl=b"\n"):
    if fmt == FASTA:
        return b">" + i + b" d" + nl + s + nl
    return b"@" + i + b" d" + nl + s + nl + b"+" + nl + b"I" * len(s) + nl


def body(reads, fmt, nl=b"\n"):
    return b"".join(record(i, s, fmt, nl) for i, s in reads)


def bases(n, src):
    """n bases: src over and over"""
    return (src * (n // len(src) + 1))[:n]


def fq(m, src, h=0, seq_end=b"\n", end=b"\n", short=0, third=b"+"):
    """one FASTQ record "@e" + h bytes, m bases, `third`, m - short qualities: 6 + h + 2 m - short bytes in front of `end`"""
    return b"@e" + b"x" * h + b"\n" + bases(m, src) + seq_end + third + b"\n" + b"I" * (m - short) + end


def filler(n, fmt, src):
    """one whole record of exactly n bytes, its sequence padded"""
    assert n >= MIN_FILLER[fmt]
    if fmt == FASTA:
        return b">f\n" + bases(n - 4, src) + b"\n"
    h = (n - 7) % 2
    return fq((n - 7 - h) // 2, src, h)


def block(n, reads, fmt):
    """exactly n bytes of whole records: the reads in turn for as long as they fit, then one filler record"""
    if n == 0:
        return b""
    parts, room = [], n
    for i, s in itertools.cycle(reads):
        rec = record(i, s, fmt)
        if room - len(rec) < MIN_FILLER[fmt]:
            break
        parts.append(rec)
        room -= len(rec)
    parts.append(filler(room, fmt, reads[0][1]))
    return b"".join(parts)


def _split(pos, lo, fmt, reads):
    """(block in front, offset of the event inside its own record): the offset is at least lo; a position too small for a block has none"""
    rem = lo + 30
    if pos - rem < MIN_FILLER[fmt]:
        assert pos >= lo
        return b"", pos
    return block(pos - rem, reads, fmt), rem


def _line_no(d, p, begin=0):
    """index of the line that position p lies in (a '\\n' lies in the line it ends)"""
    return d.count(b"\n", begin, p)


def _line_start(d, p, begin=0):
    return max(begin, d.rfind(b"\n", begin, p) + 1)


# ---------------------------------------------------------------- a: one event on every border
def _hdr_nl_at(pos, fmt, rd):
    pre, rem = _split(pos, 2, fmt, rd)
    src = rd[0][1]
    hdr = bytes([FIRST[fmt]]) + bases(rem - 1, b"e" + b"x" * 63)
    rec = hdr + b"\n" + bases(50, src) + b"\n" + (b"+\n" + b"I" * 50 + b"\n" if fmt == FASTQ else b"")
    return pre + rec + body(rd, fmt)


def _seq_nl_at(pos, fmt, rd, cr=False):
    """the sequence line's '\\n' at pos; cr: its '\\r' at pos and the '\\n' behind it"""
    pre, rem = _split(pos, 4, fmt, rd)
    src, e = rd[0][1], b"\r\n" if cr else b"\n"
    rec = b">e\n" + bases(rem - 3, src) + e if fmt == FASTA else fq(rem - 3, src, seq_end=e)
    return pre + rec + body(rd, fmt)


def _qual_nl_at(pos, rd, cr=False):
    pre, rem = _split(pos, 8, FASTQ, rd)
    h = (rem - 6) % 2
    return pre + fq((rem - 6 - h) // 2, rd[0][1], h, end=b"\r\n" if cr else b"\n") + body(rd, FASTQ)


def _plus_at(pos, rd):
    pre, rem = _split(pos, 5, FASTQ, rd)
    return pre + fq(rem - 4, rd[0][1]) + body(rd, FASTQ)


def _hdr_first_at(pos, fmt, rd):
    return block(pos, rd, fmt) + body(rd, fmt)


def _begin_at(pos, fmt, rd):
    """junk in front of `begin` = pos: line ends, record openers, separators and CRs that must not be seen; the byte in front is '\\n'"""
    return bases(pos - 1, JUNK) + b"\n" + body(rd, fmt)


END_FORMS = {"nl": b"\n", "none": b"", "cr": b"\r", "crnl": b"\r\n"}


def _end_at(pos, fmt, rd, form):
    """a piece of exactly pos bytes whose last line ends in `form`"""
    e = END_FORMS[form]
    pre, rem = _split(pos, 10, fmt, rd)
    src = rd[0][1]
    if fmt == FASTA:
        return pre + b">e\n" + bases(rem - 3 - len(e), src) + e
    h = (rem - 6 - len(e)) % 2
    return pre + fq((rem - 6 - len(e) - h) // 2, src, h, end=e)


def boundary_cases(reads):
    """family a; reads: few(world_reads)"""
    rd, out = reads, []
    for fmt in (FASTA, FASTQ):
        lpr, c0 = LPR[fmt], FIRST[fmt]
        for unit in UNITS:
            for dlt in DELTAS:
                p = unit + dlt
                tag = "%s_%d%+d" % (fmt, unit, dlt)

                def add(ev, piece, prop, begin=0):
                    out.append(("a_%s_%s" % (ev, tag), piece, begin, fmt, prop))
                add("hdr_nl", _hdr_nl_at(p, fmt, rd), lambda d, p=p, lpr=lpr, c0=c0: d[p] == NL and _line_no(d, p) % lpr == 0 and d[_line_start(d, p)] == c0)
                add("seq_nl", _seq_nl_at(p, fmt, rd), lambda d, p=p, lpr=lpr: d[p] == NL and d[p - 1] != CR and _line_no(d, p) % lpr == 1)
                add("seq_cr", _seq_nl_at(p, fmt, rd, cr=True), lambda d, p=p, lpr=lpr: d[p] == CR and d[p + 1] == NL and _line_no(d, p) % lpr == 1)
                add("hdr_first", _hdr_first_at(p, fmt, rd), lambda d, p=p, lpr=lpr, c0=c0: d[p] == c0 and d[p - 1] == NL and _line_no(d, p) % lpr == 0)
                add("seq_first", _hdr_nl_at(p - 1, fmt, rd), lambda d, p=p, lpr=lpr: d[p - 1] == NL and d[p] in b"ACGT" and _line_no(d, p) % lpr == 1)
                if fmt == FASTQ:
                    add("plus", _plus_at(p, rd), lambda d, p=p: d[p] == PLUS and d[p - 1] == NL and _line_no(d, p) % 4 == 2)
                    add("qual_nl", _qual_nl_at(p, rd), lambda d, p=p: d[p] == NL and d[p - 1] != CR and _line_no(d, p) % 4 == 3)
                    add("qual_cr", _qual_nl_at(p, rd, cr=True), lambda d, p=p: d[p] == CR and d[p + 1] == NL and _line_no(d, p) % 4 == 3)
                add("begin", _begin_at(p, fmt, rd), lambda d, p=p, c0=c0: d[p] == c0 and d[p - 1] == NL and set(d[:p]) == set(JUNK), begin=p)
                add("end_nl", _end_at(p, fmt, rd, "nl"), lambda d, p=p: len(d) == p and d[-1] == NL and d[-2] != CR)
                add("end_none", _end_at(p, fmt, rd, "none"), lambda d, p=p: len(d) == p and d[-1] not in (NL, CR))
                add("end_cr", _end_at(p, fmt, rd, "cr"), lambda d, p=p: len(d) == p and d[-1] == CR and d[-2] not in (NL, CR))
                add("end_crnl", _end_at(p, fmt, rd, "crnl"), lambda d, p=p: len(d) == p and d[-2:] == b"\r\n")
    return out


N_BOUNDARY = (10 + 13) * len(UNITS) * len(DELTAS)


# ---------------------------------------------------------------- b: irregular twins on a tile border
def _spread(rd, fmt, extra, times):
    """the reads with `extra` put in front of `times` of them, evenly: an offence repeated so that the LINE COUNT stays a multiple of the
    record's lines -- the scan's count then says nothing and the record that holds the offence has to notice it"""
    step = len(rd) // (times + 1)
    return b"".join((extra if k and k % step == 0 and k // step <= times else b"") + record(i, s, fmt) for k, (i, s) in enumerate(rd))


def irregular_twins(reads):
    """family b; reads: few(world_reads)"""
    rd, src, out = reads, reads[0][1], []
    for dlt in DELTAS:
        p = TILE + dlt
        for fmt in (FASTA, FASTQ):
            lpr, c0 = LPR[fmt], FIRST[fmt]

            def add(ev, piece, prop):
                out.append(("b_%s_%s_%d%+d" % (ev, fmt, TILE, dlt), piece, 0, fmt, prop))
            # a sequence over two lines; the second one starts at p, where a header ('+' line) must start
            if fmt == FASTA:
                two = b">e\n" + bases(40, src) + b"\n" + bases(40, src) + b"\n"
            else:
                two = b"@e\n" + bases(40, src) + b"\n" + bases(40, src) + b"\n+\n" + b"I" * 80 + b"\n"
            add("seq_two_lines", block(p - 44, rd, fmt) + two + _spread(rd, fmt, two, lpr - 1),
                lambda d, p=p, lpr=lpr: d[p - 1] == NL and d[p] in b"ACGT" and _line_no(d, p) % lpr == (0 if lpr == 2 else 2) and _line_no(d, len(d)) % lpr == 0)
            # a blank line between records: its '\n' at p
            add("blank_line", block(p, rd, fmt) + b"\n" + _spread(rd, fmt, b"\n", lpr - 1),
                lambda d, p=p, lpr=lpr: d[p - 1] == NL and d[p] == NL and _line_no(d, p) % lpr == 0 and _line_no(d, len(d)) % lpr == 0)
            # the last record cut short: its first byte at p (FASTA: a header and nothing else; FASTQ: no quality line)
            cut = b">the last header\n" if fmt == FASTA else b"@e\n" + bases(40, src) + b"\n+\n"
            add("last_cut_short", block(p, rd, fmt) + cut,
                lambda d, p=p, c0=c0, n=lpr - 1: d[p] == c0 and d[p - 1] == NL and d.count(b"\n", p) == n and d[-1] == NL)
            if fmt == FASTA:
                # a header without a sequence line: its '>' at p, the next header right behind it
                lone = b">lonely header\n"
                add("hdr_no_seq", block(p, rd, fmt) + lone + _spread(rd, fmt, lone, 1),
                    lambda d, p=p: d[p] == GT and d[p - 1] == NL and d[d.find(b"\n", p) + 1] == GT and _line_no(d, p) % 2 == 0 and _line_no(d, len(d)) % 2 == 0)
            else:
                # one quality short: the quality line's '\n' at p
                pre, rem = _split(p, 9, fmt, rd)
                h = (rem - 5) % 2
                add("one_qual_short", pre + fq((rem - 5 - h) // 2, src, h, short=1) + body(rd, fmt),
                    lambda d, p=p: d[p] == NL and _line_no(d, p) % 4 == 3 and
                    (p - _line_start(d, p)) + 1 == len(d[:_line_start(d, p) - 1].split(b"\n")[-2]))
                # a third line that is not '+': its first byte at p
                pre, rem = _split(p, 5, fmt, rd)
                add("third_not_plus", pre + fq(rem - 4, src, third=b"-") + body(rd, fmt),
                    lambda d, p=p: d[p] == 0x2D and d[p - 1] == NL and _line_no(d, p) % 4 == 2)
    return out


N_TWINS = (4 + 5) * len(DELTAS)


# ---------------------------------------------------------------- c: the line-end list exactly full
SHORTEST = {FASTA: (b">a\nAC\n", 2521), FASTQ: (b"@a\nA\n+\nI\n", 1192)}  # the shortest regular record, and how many of them fill the list


def short_records(fmt, n, p, terminated=True):
    """n records of the shortest regular shape, the last sequence (and its quality) p bases longer"""
    unit = SHORTEST[fmt][0]
    last = b">a\nAC" + b"A" * p + b"\n" if fmt == FASTA else b"@a\nA" + b"C" * p + b"\n+\nI" + b"I" * p + b"\n"
    d = unit * (n - 1) + last
    return d if terminated else d[:-1]


def capacity_pad(fmt, terminated):
    """the smallest p at which the SHORTEST[fmt] records' line ends all fit the list: one base less and they are one too many"""
    n = SHORTEST[fmt][1]
    for p in range(1, 64):
        d = short_records(fmt, n, p, terminated)
        if LPR[fmt] * n <= M.line_cap(len(d)):
            return p
    raise AssertionError("no pad below 64 fills the list")


def capacity_cases():
    """family c: (name, piece, 0, fmt, prop) -- 'full': line ends == capacity (regular); 'over': one line end more (irregular)"""
    out = []
    for fmt in (FASTA, FASTQ):
        n = SHORTEST[fmt][1]
        for terminated in (True, False):
            p = capacity_pad(fmt, terminated)
            tag = "%s_%s" % (fmt, "nl" if terminated else "no_nl")
            out.append(("c_full_" + tag, short_records(fmt, n, p, terminated), 0, fmt,
                        lambda d, n=n, lpr=LPR[fmt], t=terminated: d.count(b"\n") + (0 if t else 1) == lpr * n == M.line_cap(len(d)) and d.endswith(b"\n") == t))
            out.append(("c_over_" + tag, short_records(fmt, n, p - 1, terminated), 0, fmt,
                        lambda d, n=n, lpr=LPR[fmt], t=terminated: d.count(b"\n") + (0 if t else 1) == lpr * n == M.line_cap(len(d)) + 1 and d.endswith(b"\n") == t))
    return out


N_CAPACITY = 8


# ---------------------------------------------------------------- d: more tiles than scan threads
TILE_RUNS = ((1024, FASTA), (1025, FASTA), (1025, FASTQ), (2049, FASTA))
RUN_THREAD = 511  # the border between the runs of scan threads 510 and 511


def tile_run_piece(n_tiles, fmt, reads):
    """a piece of n_tiles tiles (the last one holds 777 bytes).  With per = ceil(n_tiles / 1024) tiles to a scan thread, a record's last
    '\\n' is the last byte of thread 510's run and the next record's first byte the first of thread 511's; FASTQ: a sequence line's '\\n'
    is the last byte of thread 299's run as well.  Returns (piece, border, sequence border or None)."""
    per = (n_tiles + 1023) // 1024
    border, total = RUN_THREAD * per * TILE, (n_tiles - 1) * TILE + 777
    parts, at, seq_border = [], 0, None
    if fmt == FASTQ:
        seq_border = 300 * per * TILE
        head = block(seq_border - 44, reads, fmt) + fq(40, reads[0][1])  # "@e\n" + 40 bases: the sequence line's '\n' at offset 43
        parts.append(head)
        at = len(head)
    parts.append(block(border - at, reads, fmt))
    parts.append(block(total - border, reads, fmt))
    return b"".join(parts), border, seq_border


def tile_run_cases(reads):
    """family d, one case at a time (the pieces are 17 to 34 MB); reads: world_reads"""
    for n_tiles, fmt in TILE_RUNS:
        piece, border, sb = tile_run_piece(n_tiles, fmt, reads)
        per = (n_tiles + 1023) // 1024

        def prop(d, n_tiles=n_tiles, fmt=fmt, border=border, sb=sb, per=per):
            ok = (len(d) + TILE - 1) // TILE == n_tiles and border % (per * TILE) == 0 and border // (per * TILE) < (n_tiles + per - 1) // per
            ok = ok and d[border - 1] == NL and d[border] == FIRST[fmt] and _line_no(d, border) % LPR[fmt] == 0
            ok = ok and d[-1] == NL and len(d) - 1 >= (n_tiles - 1) * TILE  # a line end in the last tile
            if sb is not None:
                ok = ok and sb % (per * TILE) == 0 and d[sb - 1] == NL and d[sb] == PLUS and _line_no(d, sb) % 4 == 2
            return ok
        yield ("d_%d_tiles_%s" % (n_tiles, fmt), piece, 0, fmt, prop)


# ---------------------------------------------------------------- e: small pieces, exhaustively
FASTA_BYTES = b">A\r\n"
FASTQ_LINES = (b"", b"@", b"@A", b"+", b"A", b"AA", b"A\r")
PREFIX = bases(36, JUNK) + b"\n"  # 37 bytes of junk that end a line


def small_fasta():
    """every byte string over FASTA_BYTES of length 0 .. 6: 5,461 pieces"""
    out = []
    for n in range(7):
        for t in itertools.product(FASTA_BYTES, repeat=n):
            out.append(("e_fasta_%d" % len(out), bytes(t), 0, FASTA, lambda d, n=n: len(d) == n and set(d) <= set(FASTA_BYTES)))
    return out


def small_fasta_prefixed():
    """the pieces of small_fasta() of up to 4 bytes behind PREFIX, begin = 37: 341 pieces"""
    return [("e_prefixed_" + name[2:], PREFIX + d, len(PREFIX), FASTA, lambda b, d=d: b[:37] == PREFIX and b[36] == NL and b[37:] == d)
            for name, d, _, _, _ in small_fasta() if len(d) <= 4]


def _from_lines(lines, terminated):
    return b"\n".join(lines) + (b"\n" if terminated else b"")


def _is_lines(d, n_lines):
    ls = d.split(b"\n")  # (an unterminated empty last line leaves no byte: the split then shows one part less)
    return len(ls) in (n_lines, n_lines + 1) and all(x in FASTQ_LINES for x in ls)


def small_fastq():
    """every sequence of 4 lines of FASTQ_LINES, the last one terminated or not: 4,802 pieces"""
    out = []
    for t in itertools.product(FASTQ_LINES, repeat=4):
        for terminated in (True, False):
            out.append(("e_fastq_%d" % len(out), _from_lines(t, terminated), 0, FASTQ, lambda d: _is_lines(d, 4)))
    return out


def sampled_fastq(n=2000, seed=20251):
    """n pieces of 2 or 3 records (4 lines each) of FASTQ_LINES.  Uniform draws would leave one piece in thousands regular, so every line is
    drawn from the whole vocabulary with probability 1/4 and otherwise from the lines that keep its record regular ('@' lines, '+', a
    quality as long as the sequence): about a quarter of the pieces are regular, the others break one rule somewhere."""
    rng = np.random.default_rng(seed)
    cut = {x: len(x[:-1] if x.endswith(b"\r") else x) for x in FASTQ_LINES}
    out = []
    for k in range(n):
        lines = []
        for _ in range(int(rng.integers(2, 4))):
            rec = []
            for j in range(4):
                legal = [(b"@", b"@A"), FASTQ_LINES, (b"+",), FASTQ_LINES][j]
                if j == 3:
                    legal = [x for x in FASTQ_LINES if cut[x] == cut[rec[1]]]
                pool = FASTQ_LINES if rng.random() < 0.25 else legal
                rec.append(pool[int(rng.integers(0, len(pool)))])
            lines += rec
        n_lines = len(lines)
        out.append(("e_sampled_%d" % k, _from_lines(lines, bool(rng.integers(0, 2))), 0, FASTQ, lambda d, n_lines=n_lines: _is_lines(d, n_lines)))
    return out


N_SMALL = {"fasta": 5461, "prefixed": 341, "fastq": 4802, "sampled": 2000}
