"""GPU: the lines of a line-wrapped FASTA record joined in device memory (mq_join.hpp behind mq_index_staged_sequence and
mq_index_add_ref_staged_lines).  The rule is RefLoader::prepare's (host/ref_loader.hpp) and seq_io's (src/closures.rs:46-94 reads the
reference through it): the region behind the header line is split at every '\\n', one trailing '\\r' is cut from each piece, the pieces
are concatenated -- `model` below.  Bytes: every directed shape and 400 random regions against the model.  Index: a five-record file
image staged in odd pieces, records added back to back, against mq_index_add_ref on the model-joined sequences and the oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TILE = 16384  # FX_TILE


def model(region):
    return b"".join(ln[:-1] if ln.endswith(b"\r") else ln for ln in region.split(b"\n"))


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


_ALPHA = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)


def _bases(rng, n):
    return _ALPHA[rng.integers(0, _ALPHA.size, n)].tobytes()


def _wrap(seq, w, nl, final=True):
    out = nl.join(seq[i:i + w] for i in range(0, len(seq), w))
    return out + nl if final and seq else out


class Image:
    """Regions laid into one staging-buffer image: each at an offset of the residue mod 16 it asks for, any bytes between them."""

    def __init__(self, rng):
        self.rng, self.parts, self.size, self.regions, self.cuts = rng, [], 0, [], set()
        self._fill(int(rng.integers(0, 40)))

    def _fill(self, n):
        if n:
            self.parts.append(np.frombuffer(b"\n\r>ACGT ", dtype=np.uint8)[self.rng.integers(0, 8, n)].tobytes())
            self.size += n

    def add(self, name, region, mod16=None, cut_at=None):
        """cut_at: an offset inside the region where a piece of the upload must end"""
        self._fill(int(self.rng.integers(1, 40)))
        if mod16 is not None:
            self._fill((mod16 - self.size) % 16)
        if cut_at is not None:
            self.cuts.add(self.size + cut_at)
        self.regions.append((name, self.size, region))
        self.parts.append(region)
        self.size += len(region)

    def bytes(self):
        return b"".join(self.parts)


def _stage(mq, ix, blob, cuts, rng, last_first=True):
    """the image in odd-sized pieces (and the cuts asked for), issued last-first"""
    buf = np.frombuffer(blob, dtype=np.uint8)
    ix.stage_begin(buf.size)
    pts = {0, buf.size} | {c for c in cuts if 0 < c < buf.size}
    p = 0
    while p < buf.size:
        p += int(rng.integers(1, 3_000_001)) | 1
        if p < buf.size:
            pts.add(p)
    pts = sorted(pts)
    pieces = [(pts[i], buf[pts[i]:pts[i + 1]]) for i in range(len(pts) - 1)]
    return [ix.stage_piece(at, piece) for at, piece in (reversed(pieces) if last_first else pieces)]


def _directed(rng):
    """(name, region, at % 16 or None, cut offset or None)"""
    for style, nl in (("lf", b"\n"), ("crlf", b"\r\n")):
        for w in (1, 15, 16, 17, 59, 60, 61, 80, 1023, 1024, 1025, 16383, 16384, 16385):
            for m in range(16):
                n = {1: 1500, 15: 3000}.get(w, max(2500, 2 * w + 9) if m else max(40000, 3 * w + 11))
                yield "wrap%d-%s-at%d" % (w, style, m), _wrap(_bases(rng, n), w, nl), m, None
        for m in (0, 1, 7, 15):
            # a '\r' as the last byte of a tile, its '\n' the first of the next (tiles start at `at` rounded down to 16); once the upload is cut between them
            for t in (1, 2):
                k = t * TILE - m - 1  # offset in the region of the tile's last byte
                for cut in (None, k + 1):
                    yield "cr-ends-tile%d-%s-at%d-%s" % (t, style, m, cut), _bases(rng, k) + b"\r\n" + _wrap(_bases(rng, 500), 70, nl), m, cut
                # ... and a '\r' there that is NOT followed by '\n': kept
                yield "lone-cr-ends-tile%d-%s-at%d" % (t, style, m), _bases(rng, k) + b"\rA" + nl + _bases(rng, 50) + nl, m, None
            yield "no-final-newline-%s-at%d" % (style, m), _wrap(_bases(rng, 20011), 80, nl, final=False), m, None
            yield "ends-in-bare-cr-%s-at%d" % (style, m), _wrap(_bases(rng, 4000), 60, nl) + _bases(rng, 31) + b"\r", m, None
            yield "ends-in-bare-cr-at-tile-end-%s-at%d" % (style, m), _wrap(_bases(rng, 60), 60, nl) + _bases(rng, TILE - m - 1 - 60 - len(nl)) + b"\r", m, None
            yield "only-a-cr-%s-at%d" % (style, m), b"\r", m, None
            yield "blank-lines-%s-at%d" % (style, m), (nl + _bases(rng, 60) + nl + nl + nl + _bases(rng, 7) + nl + _bases(rng, 80) + nl + _bases(rng, 1) + nl
                                                      + _wrap(_bases(rng, 18000), 33, nl) + nl + nl), m, None
            yield "mixed-widths-%s-at%d" % (style, m), b"".join(_bases(rng, int(x)) + nl for x in rng.integers(0, 300, 400)), m, None
            yield "lone-cr-and-gt-inside-%s-at%d" % (style, m), (b"AC\rGT>AC" + nl + b">\r\rA" + nl + b"\r" + b"A" + nl + b"AC GT\tN" + nl + b"\r\r" + nl + _bases(rng, 17000).replace(b"a", b"\r")
                                                                + nl + b">tail"), m, None
            yield "empty-%s-at%d" % (style, m), b"", m, None
            for k in (1, 2, 15, 16, 17, 1024, TILE, TILE + 1, 40001):
                yield "newlines-only-%d-%s-at%d" % (k, style, m), (nl * k)[:k], m, None


def _random_regions(rng, n):
    """0 to 200,000 bytes; line lengths geometric around a mean of 2 to 30,000 (empty lines among them); a '\\r' in front of half the line
    ends, in front of another '\\r' now and then, and anywhere in a line"""
    for i in range(n):
        size = int(rng.integers(0, 200_001)) if i % 8 else int(rng.integers(0, 40))
        a = _ALPHA[rng.integers(0, _ALPHA.size, size)]
        ends = rng.random(size) < 1.0 / float(rng.choice([2, 20, 70, 1000, 30000]))
        a[ends] = 10
        for _ in range(2):
            before = np.flatnonzero(ends)
            before = before[before > 0] - 1
            a[before[rng.random(before.size) < 0.5]] = 13
            ends = a == 13
        a[rng.random(size) < 0.002] = 13
        region = a.tobytes()
        yield "random%d" % i, region, None, (int(rng.integers(0, len(region))) if len(region) and i % 5 == 0 else None)


def test_joined_bytes_equal_the_model(mq):
    rng = np.random.default_rng(20240611)
    im = Image(rng)
    for name, region, m, cut in list(_directed(rng)) + list(_random_regions(rng, 400)):
        im.add(name, region, m, cut)
    assert len(im.regions) > 900 and sum(1 for n, _, _ in im.regions if n.startswith("random")) == 400
    assert {at % 16 for n, at, _ in im.regions if n.startswith("random")} == set(range(16))
    blob = im.bytes()
    ix = mq.Index(mq.Params())
    tickets = _stage(mq, ix, blob, im.cuts, rng)
    bad = []
    for name, at, region in im.regions:
        assert blob[at:at + len(region)] == region
        got = ix.staged_sequence(at, len(region)).tobytes()
        want = model(region)
        if got != want:
            d = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
            bad.append((name, at, len(region), len(got), len(want), d))
    assert not bad, bad[:20]
    # bytes == 0 at the buffer's two ends; a region that is the whole image; behind a ticket of its own
    assert ix.staged_sequence(0, 0).size == 0 and ix.staged_sequence(len(blob), 0).size == 0
    assert ix.staged_sequence(0, len(blob)).tobytes() == model(blob)
    name, at, region = im.regions[5]
    assert ix.staged_sequence(at, len(region), after_ticket=tickets[-1]).tobytes() == model(region)
    ix.close()


def test_errors(mq):
    L = mq.load_library()
    region = b"ACGT\nAC\r\nGT\n"
    ix = mq.Index(mq.Params())
    with pytest.raises(mq.MapquikError, match="before mq_index_stage_begin"):
        ix.staged_sequence(0, 4)
    with pytest.raises(mq.MapquikError, match="before mq_index_stage_begin"):
        ix.add_ref_staged_lines(0, "x", 0, 4)
    assert L.mq_index_staged_sequence(ix.handle, 0, 4, 0xFFFFFFFFFFFFFFFF, None, 0) == -5  # MQ_ESTATE
    assert L.mq_index_add_ref_staged_lines(ix.handle, 0, b"x", 0, 4, 0xFFFFFFFFFFFFFFFF, None) == -5
    ix.stage_begin(100)
    t = ix.stage_piece(10, np.frombuffer(region, dtype=np.uint8))
    for at, n in ((50, 51), (101, 0), (0, 101), (2 ** 63, 2 ** 63)):  # a region outside the buffer
        with pytest.raises(mq.MapquikError, match="outside the staging buffer"):
            ix.staged_sequence(at, n)
        with pytest.raises(mq.MapquikError, match="outside the staging buffer"):
            ix.add_ref_staged_lines(0, "x", at, n)
    with pytest.raises(mq.MapquikError, match="unknown ticket"):
        ix.staged_sequence(10, len(region), after_ticket=t + 1)
    with pytest.raises(mq.MapquikError, match="unknown ticket"):
        ix.add_ref_staged_lines(0, "x", 10, len(region), after_ticket=5)
    assert L.mq_index_add_ref_staged_lines(ix.handle, 0, b"x", 10, len(region), 5, None) == -1  # MQ_EINVAL
    assert ix.stats()["n_refs"] == 0  # nothing was registered by any of these
    # cap smaller than the result: MQ_EINVAL, and nothing is written
    want = model(region)
    out = np.full(64, 0xEE, dtype=np.uint8)
    for cap in (0, 1, len(want) - 1):
        assert L.mq_index_staged_sequence(ix.handle, 10, len(region), 0xFFFFFFFFFFFFFFFF, out.ctypes.data_as(C.c_void_p), cap) == -1
        assert (out == 0xEE).all()
    assert L.mq_index_staged_sequence(ix.handle, 10, len(region), 0xFFFFFFFFFFFFFFFF, None, 0) == len(want)  # (no buffer: the length alone)
    assert L.mq_index_staged_sequence(ix.handle, 10, len(region), 0xFFFFFFFFFFFFFFFF, out.ctypes.data_as(C.c_void_p), len(want)) == len(want)
    assert out[:len(want)].tobytes() == want and (out[len(want):] == 0xEE).all()
    # a duplicate ref_id; a record that joins to nothing is a reference of length 0; seq_len may be NULL
    assert ix.add_ref_staged_lines(3, "a", 10, len(region)) == (0, len(want))
    with pytest.raises(mq.MapquikError, match="duplicate ref_id"):
        ix.add_ref_staged_lines(3, "b", 10, len(region))
    assert ix.add_ref_staged_lines(4, "nothing", 14, 1) == (0, 0) and ix.add_ref_staged_lines(5, "empty", 100, 0) == (0, 0)
    assert L.mq_index_add_ref_staged_lines(ix.handle, 6, b"c", 10, 5, 0xFFFFFFFFFFFFFFFF, None) == 0
    assert [ix.ref_info(r) for r in (3, 4, 5, 6)] == [("a", len(want)), ("nothing", 0), ("empty", 0), ("c", 4)]
    ix.finalize()
    with pytest.raises(mq.MapquikError):  # the staging buffer went with finalize
        ix.staged_sequence(10, 4)
    with pytest.raises(mq.MapquikError):
        ix.add_ref_staged_lines(7, "late", 10, 4)
    ix.close()


@pytest.fixture(scope="module")
def genome(simlib):
    # (the contigs of tests/test_gpu_reference_stream.py: records around the streamer's 16-MB blocks, two too short to be seeded or nearly)
    g, off, names = simlib.make_genome([20_000_000, 17_000_000, 3_000_000, 40, 1200], seed=41, repeat_frac=0.05, threads=4)
    seqs = [g[int(off[r]):int(off[r + 1])].tobytes() for r in range(len(names))]
    reads = simlib.make_reads(g, off, 1500, seed=6, threads=4)
    return dict(g=g, off=off, names=names, seqs=seqs, reads=reads)


def _file_image(seqs, names, rng):
    """Five records: wrapped at 80; at 60 with CR-LF; the others mixed.  Returns (image, [(offset, length) of every record's region])."""
    def mixed(s, nl_choices):
        out, p = [], 0
        while p < len(s):
            w = int(rng.choice([1, 13, 60, 61, 70, 80, 200, 5000]))
            out.append(s[p:p + w] + nl_choices[int(rng.integers(0, len(nl_choices)))])
            p += w
            if rng.random() < 0.02:
                out.append(nl_choices[0])  # a blank line
        return b"".join(out)
    bodies = [_wrap(seqs[0], 80, b"\n"), _wrap(seqs[1], 60, b"\r\n"), mixed(seqs[2], [b"\n", b"\r\n"]), mixed(seqs[3], [b"\n"])[:-1] + b"\r\n\n", mixed(seqs[4], [b"\r\n", b"\n"])[:-1]]
    parts, regions, size = [], [], 0
    for r, body in enumerate(bodies):
        hdr = b">" + names[r].encode() + b" contig %d" % r + (b"\r\n" if r == 1 else b"\n")
        parts += [hdr, body]
        regions.append((size + len(hdr), len(body)))
        size += len(hdr) + len(body)
    return b"".join(parts), regions


def _build_both(mq, P, seqs, names, rng):
    """(index built by add_ref on the sequences, its counts), (index built by add_ref_staged_lines on the file image, its counts and lengths)"""
    a = mq.Index(P)
    want = [a.add_ref(r, names[r], np.frombuffer(seqs[r], dtype=np.uint8)) for r in range(len(names))]
    blob, regions = _file_image(seqs, names, rng)
    for (at, n), s in zip(regions, seqs):
        assert model(blob[at:at + n]) == s
    b = mq.Index(P)
    _stage(mq, b, blob, (), rng)
    got = [b.add_ref_staged_lines(r, names[r], at, n) for r, (at, n) in enumerate(regions)]  # back to back: bld.seq is reused record after record
    return a, want, b, got


def _same_index(a, b, names, seqs, reads):
    for r in range(len(names)):
        assert a.ref_info(r) == b.ref_info(r) == (names[r], len(seqs[r]))
    assert a.finalize() == b.finalize()
    sa, sb = a.stats(), b.stats()
    assert sa == sb and sa["n_refs"] == len(names)
    ha, hb = a.map_batch(reads["bases"], reads["offsets"]), b.map_batch(reads["bases"], reads["offsets"])
    assert ha.size == reads["offsets"].size - 1 and np.array_equal(ha.view(np.uint8), hb.view(np.uint8))
    return ha


def test_index_of_joined_records_equals_add_ref_and_the_oracle(mq, oracle, simlib, genome):
    w = genome
    rng = np.random.default_rng(7)
    P, po = mq.Params(), oracle.params()
    a, want, b, got = _build_both(mq, P, w["seqs"], w["names"], rng)
    ox = oracle.Index()
    ocounts = [ox.add_ref(r, w["names"][r], w["g"][int(w["off"][r]):int(w["off"][r + 1])], po) for r in range(len(w["names"]))]
    assert [c for c, _ in got] == want == ocounts and want[0] > 100000 and want[3] == 0
    assert [n for _, n in got] == [len(s) for s in w["seqs"]]
    hits = _same_index(a, b, w["names"], w["seqs"], w["reads"])
    assert b.stats()["n_unique"] == ox.count()
    owant = ox.map_batch(w["reads"]["bases"], w["reads"]["offsets"], po, threads=4)
    rn = simlib.read_names(w["reads"], w["names"])
    lines = b.paf_lines(rn, w["reads"]["offsets"], hits)
    assert lines == oracle.paf_lines(ox, rn, owant) and len(lines) > 1000
    a.close()
    b.close()


@pytest.mark.parametrize("how", ["fold_case", "variant16", "ref_cap8"])
def test_index_of_joined_records_other_paths(mq, genome, monkeypatch, how):
    """MQ_FLAG_FOLD_CASE on half-lower-case records (the joined bytes reach the seeders as they are); seeding variant 16 (the build keeps a
    third list); MQ_REF_CAP=8 (every segment takes the redo path)."""
    w = genome
    rng = np.random.default_rng(8)
    seqs = [s[:len(s) // 2].lower() + s[len(s) // 2:] for s in w["seqs"]] if how == "fold_case" else w["seqs"]
    if how == "ref_cap8":
        monkeypatch.setenv("MQ_REF_CAP", "8")
    P = mq.Params(fold_case=how == "fold_case", seeding_variant=16 if how == "variant16" else 0)
    a, want, b, got = _build_both(mq, P, seqs, w["names"], rng)
    assert [c for c, _ in got] == want and want[0] > 100000
    assert [n for _, n in got] == [len(s) for s in seqs]
    _same_index(a, b, w["names"], seqs, w["reads"])
    a.close()
    b.close()


def test_one_region_of_more_than_1024_tiles(mq):
    """17 MB wrapped at 80 columns, CR-LF in its second half: join_scan_kernel's threads take more than one tile each"""
    rng = np.random.default_rng(1024)
    region = _wrap(_bases(rng, 9_000_000), 80, b"\n") + _wrap(_bases(rng, 8_000_000), 80, b"\r\n", final=False)
    assert len(region) > 1024 * TILE + 200_000
    blob = b">big\n" + region + b">next\n"
    ix = mq.Index(mq.Params())
    _stage(mq, ix, blob, (), rng)
    assert ix.staged_sequence(5, len(region)).tobytes() == model(region)
    ix.close()
