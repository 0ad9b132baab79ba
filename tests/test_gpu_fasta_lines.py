"""GPU: line-wrapped FASTA reads found and joined on the device (mq_ctx_submit_fastx with MQ_FASTX_FASTA_LINES / mq_ctx_wait_fasta_lines,
mapquik_amd/csrc/mq_fastx_lines.hpp) against the line model of tests/fasta_lines_model.py -- header spans and joined lengths -- and
against map_batch on the model's sequences -- the hits, byte for byte: what closures.rs:100-123 hands to find_matches (id, sequence)
must not depend on who joined the lines.  Whole files at many wrap widths, one event placed on every border of the kernels' units
(tests/fasta_lines_cases.py), the irregular pieces and the context's state, a poisoned hit buffer, the overflow redo, and the native
driver with --reads-join device against the oracle's PAF."""
import os
import subprocess

import numpy as np
import pytest

import fasta_lines_cases as K
import fasta_lines_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture(scope="module")
def world(mq, oracle, simlib):
    g, off, names = simlib.make_genome([700000, 400000], seed=91, repeat_frac=0.1, tandem_frac=0.02)
    P, po = mq.Params(fold_case=True), oracle.params()
    ix, ox = mq.Index(P), oracle.Index()
    for r in range(2):
        s = g[int(off[r]):int(off[r + 1])]
        assert ix.add_ref(r, names[r], s) == ox.add_ref(r, names[r], s, po)
    assert ix.finalize() == ox.count()
    reads = simlib.make_reads(g, off, 700, seed=12, len_mean=9000, len_sd=5000, len_min=1)
    rn = simlib.read_names(reads, names)
    o = reads["offsets"]
    seqs = [reads["bases"][int(o[i]):int(o[i + 1])].tobytes() for i in range(len(rn))]
    return dict(ix=ix, ox=ox, po=po, reads=reads, names=rn, seqs=seqs, genome=(g, off, names))


def _map(ix, seqs):
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return ix.map_batch(bases, offs)


def _check(ix, ctx, piece, begin=0, recs=None, want=None):
    """one LINES piece through the context against the model (recs: the model's records of the piece at begin 0) and map_batch"""
    if recs is None:
        recs = M.records(piece)
    if want is None:
        want = _map(ix, [s for _, _, s in recs])
    buf = np.frombuffer((b"x" * (begin - 1) + b"\n" if begin else b"") + piece, dtype=np.uint8)
    ctx.submit_fasta(buf, begin=begin, lines=True)
    hits, hb, he, sl, flags = ctx.wait_fasta_lines()
    assert flags == 0 and hits.size == len(recs)
    assert hb.tolist() == [a + begin for a, _, _ in recs]
    assert he.tolist() == [b + begin for _, b, _ in recs]
    assert sl.tolist() == [len(s) for _, _, s in recs]
    assert np.array_equal(hits.view(np.uint8), want.view(np.uint8))
    return hits


def _whole_files(world):
    rd = list(zip([n.encode() for n in world["names"]], world["seqs"]))
    low = [(i, s.lower() if k % 3 == 0 else s) for k, (i, s) in enumerate(rd)]
    cases = [("w%d" % w, K.fasta(rd, w)) for w in (1, 15, 16, 17, 60, 70, 80, 1023, 1024, 1025)]
    cases.append(("mixed_wrap", b"".join(K.fasta([r], 10 ** 9 if k % 2 else 70) for k, r in enumerate(rd))))
    cases.append(("crlf", K.fasta(rd, 60, b"\r\n")))
    cases.append(("crlf_no_final_newline", K.fasta(rd, 80, b"\r\n", final_newline=False)))
    cases.append(("no_final_newline", K.fasta(rd, 70, final_newline=False)))
    cases.append(("final_cr_without_nl", K.fasta(rd, 60, b"\r\n")[:-1]))
    cases.append(("every_third_lower_case", K.fasta(low, 70)))
    cases.append(("empty_lines", b"".join(b">" + i + b" e\n" + K.wrap(s[:100], 60) + b"\n\n" + (K.wrap(s[100:], 60) if len(s) > 100 else b"") + b"\n" for i, s in rd)))
    return cases


def test_parity_with_the_model_and_map_batch(mq, world):
    ix = world["ix"]
    ctx = ix.context()
    upper = _map(ix, world["seqs"])
    assert (upper["status"] == 1).sum() > 500
    for name, piece in _whole_files(world):
        recs = M.records(piece)
        assert recs is not None and len(recs) == 700, name
        want = upper if [s for _, _, s in recs] == world["seqs"] else _map(ix, [s for _, _, s in recs])
        for begin in (0, 37):
            hits = _check(ix, ctx, piece, begin, recs, want)
            assert (hits["status"] == 1).sum() > 500, name
    ctx.close()


@pytest.fixture(scope="module")
def few(world):
    """a dozen of the world's reads of 300 .. 6,000 bases: what the boundary constructor puts behind its event"""
    pick = [k for k, s in enumerate(world["seqs"]) if 300 <= len(s) <= 6000][:12]
    assert len(pick) == 12
    return [(world["names"][k].encode(), world["seqs"][k]) for k in pick]


def test_one_event_on_every_border(mq, world, few):
    ix = world["ix"]
    ctx = ix.context()
    mapped = 0
    for name, piece, prop in K.boundary_cases(few):
        assert prop(piece), name
        if name in K.IRREGULAR_BOUNDARY:
            ctx.submit_fasta(np.frombuffer(piece, dtype=np.uint8), lines=True)
            hits, hb, he, sl, flags = ctx.wait_fasta_lines()
            assert flags & 1 and hits.size == hb.size == he.size == sl.size == 0, name
            continue
        hits = _check(ix, ctx, piece)
        mapped += int((hits["status"] == 1).sum())
    assert mapped > 100
    ctx.close()


def test_more_than_1024_tiles(mq, world):
    """17 MB of 80-column lines: fl_scan_kernel's threads take several tiles each"""
    rd = list(zip([n.encode() for n in world["names"]], world["seqs"]))
    piece = K.fasta(rd, 80)
    piece = piece * (17_000_000 // len(piece) + 1)
    assert len(piece) > 1024 * M.TILE + 200_000
    recs = M.records(piece)
    ix = world["ix"]
    ctx = ix.context()
    hits = _check(ix, ctx, piece, 0, recs)
    assert hits.size == len(recs) >= 1400 and (hits["status"] == 1).sum() > 1000
    ctx.close()


def test_irregular_pieces_and_the_context_s_state(mq, world, few):
    ix = world["ix"]
    L = ix._L
    ctx = ix.context()
    ok = K.fasta(few, 70)
    for name, piece in K.IRREGULAR_PIECES.items():
        ctx.submit_fasta(np.frombuffer(piece, dtype=np.uint8), lines=True)
        hits, hb, he, sl, flags = ctx.wait_fasta_lines()
        assert flags & 1 and hits.size == hb.size == he.size == sl.size == 0, name
        _check(ix, ctx, ok)  # the next regular piece on the same context: its full result
    # an empty piece is regular and has no records; the piece just under the span cap reports every record
    ctx.submit_fasta(np.zeros(0, dtype=np.uint8), lines=True)
    hits, hb, he, sl, flags = ctx.wait_fasta_lines()
    assert flags == 0 and hits.size == 0
    hits = _check(ix, ctx, K.JUST_UNDER_THE_SPAN_CAP)
    assert hits.size == 2400 and not (hits["status"] != 0).any()
    # the wrong wait answers MQ_ESTATE (-5) and leaves the piece pending: the right one then succeeds
    import ctypes as C
    n, nl, fl = C.c_uint32(), C.c_uint32(), C.c_uint32()
    a, b, c3, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    buf = np.frombuffer(ok, dtype=np.uint8)
    ctx.submit_fasta(buf, lines=True)
    assert L.mq_ctx_wait_fasta(ctx._h, C.byref(n), C.byref(a), C.byref(nl), C.byref(d), C.byref(fl)) == -5
    hits, hb, he, sl, flags = ctx.wait_fasta_lines()
    assert flags == 0 and hits.size == len(few)
    single = np.frombuffer(K.fasta(few, 10 ** 9), dtype=np.uint8)
    ctx.submit_fasta(single)
    assert L.mq_ctx_wait_fasta_lines(ctx._h, C.byref(n), C.byref(a), C.byref(b), C.byref(c3), C.byref(d), C.byref(fl)) == -5
    hits, lines, flags = ctx.wait_fasta()
    assert flags == 0 and hits.size == len(few) and lines.size == 2 * len(few)
    fq = np.frombuffer(b"".join(b"@" + i + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in few), dtype=np.uint8)
    ctx.submit_fasta(fq, fastq=True)
    assert L.mq_ctx_wait_fasta_lines(ctx._h, C.byref(n), C.byref(a), C.byref(b), C.byref(c3), C.byref(d), C.byref(fl)) == -5
    hits, lines, flags = ctx.wait_fasta()
    assert flags == 0 and hits.size == len(few)
    assert L.mq_ctx_wait_fasta_lines(ctx._h, C.byref(n), C.byref(a), C.byref(b), C.byref(c3), C.byref(d), C.byref(fl)) == -5  # after none
    # the old format is untouched: a wrapped piece is still irregular there; any other format value is refused
    ctx.submit_fasta(buf, lines=False)
    hits, lines, flags = ctx.wait_fasta()
    assert flags & 1 and hits.size == 0
    assert L.mq_ctx_submit_fastx(ctx._h, buf.ctypes.data_as(C.c_void_p), 0, buf.size, 3) == -1
    with pytest.raises(ValueError):
        ctx.submit_fasta(buf, fastq=True, lines=True)
    _check(ix, ctx, ok)
    ctx.close()


def test_every_record_is_written_into_a_poisoned_hit_buffer(mq, world, monkeypatch):
    """MQ_FX_POISON_HITS (read by mq_ctx_wait_fasta_lines): the context's device hit buffer is filled with 0xFF before the map kernels
    of this one piece are launched; a record no wave writes would keep status 0xFFFFFFFF"""
    from test_gpu_poison import _assert_all_written
    ix = world["ix"]
    rd = list(zip([n.encode() for n in world["names"]], world["seqs"]))
    piece = K.fasta(rd, 80)
    ctx = ix.context()
    monkeypatch.setenv("MQ_FX_POISON_HITS", "1")
    hits = _check(ix, ctx, piece)
    monkeypatch.delenv("MQ_FX_POISON_HITS")
    _assert_all_written(hits)
    assert hits.size == 700
    ctx.close()


def test_overflow_reads_are_redone(mq, oracle, simlib):
    """a read with more Match runs than the default scratch holds (the k = 1 leg of tests/mosaic.py): status 2 on the plain device form,
    map_batch's hit through wait_fasta_lines"""
    import mosaic
    from hipmem import DevBuf, device_sync
    g, off, names = mosaic.mosaic_genome(simlib)
    ps, bases, offs, _ = mosaic.leg("k1", g, off)
    ix = mq.Index(mq.Params(**ps))
    for r in range(off.size - 1):
        ix.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])])
    ix.finalize()
    n = offs.size - 1
    db, do, out = DevBuf.from_numpy(bases), DevBuf.from_numpy(offs), DevBuf(n * mq.hit_dtype.itemsize)
    ix.reserve(n, int(offs[-1]))
    ix.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), out.ptr)
    device_sync()
    dev = out.to_numpy(mq.hit_dtype, n)
    for x in (db, do, out):
        x.free()
    over = np.flatnonzero(dev["status"] == mq.MQ_HIT_OVERFLOW)
    assert over.size >= 1  # the read does overflow on the plain device form
    pick = [int(over[0])] + [k for k in range(n) if k not in over][:5] + [int(k) for k in over[1:3]]
    o = offs.astype(np.int64)
    rd = [(b"m%d" % k, bases[o[k]:o[k + 1]].tobytes()) for k in pick]
    want = _map(ix, [s for _, s in rd])
    assert not (want["status"] == mq.MQ_HIT_OVERFLOW).any()
    ctx = ix.context()
    hits = _check(ix, ctx, K.fasta(rd, 70), 0, None, want)
    assert not (hits["status"] == mq.MQ_HIT_OVERFLOW).any()
    ctx.close()


def test_native_driver_with_reads_join_device(mq, oracle, world, tmp_path):
    """the 70-column file of test_gpu_fasta_scan.py's driver test, three chunk sizes: the oracle's PAF and unmapped list; no chunk comes
    back irregular with --reads-join device, every wrapped one does with --reads-join host"""
    from mapquik_amd import build
    exe = build.build_cli()
    ox, po, rd, rn = world["ox"], world["po"], world["reads"], world["names"]
    g, off, names = world["genome"]
    ref = tmp_path / "ref.fa"
    with open(ref, "wb") as w:
        for r in range(2):
            w.write(b">" + names[r].encode() + b"\n" + g[int(off[r]):int(off[r + 1])].tobytes() + b"\n")
    want = ox.map_batch(rd["bases"], rd["offsets"], po, threads=4)
    want_txt = "".join(x + "\n" for x in oracle.paf_lines(ox, rn, want))
    assert len(want_txt) > 10000
    multi = tmp_path / "reads_multi.fa"
    multi.write_bytes(K.fasta(list(zip([n.encode() for n in rn], world["seqs"])), 70))
    k = 0
    for chunk in ("20000", "300000", "33554432"):
        for where in ("device", "host"):
            k += 1
            prefix = str(tmp_path / ("o%d" % k))
            r = subprocess.run([exe, str(multi), "--reference", str(ref), "-p", prefix, "--batch-bases", chunk, "--threads", "3", "--unmapped", "--reads-join", where],
                               capture_output=True, text=True, env=dict(os.environ, MQ_DRIVER_TIMING="1"))
            assert r.returncode == 0, r.stderr
            assert open(prefix + ".paf").read() == want_txt, (chunk, where)
            assert open(prefix + ".unmapped.out").read().split() == [n for n, w_ in zip(rn, want) if not w_["mapped"]]
            ln = [x for x in r.stderr.splitlines() if x.startswith("unparsed chunks ")][0].split()
            unparsed, irregular = int(ln[2]), int(ln[4])
            assert unparsed > 0 and (irregular == 0 if where == "device" else irregular > 0), (chunk, where, unparsed, irregular)
