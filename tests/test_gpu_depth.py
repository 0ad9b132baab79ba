"""GPU: the depth accumulator (mq_depth) against the numpy model of tests/depth_model.py (held against a second wording on the CPU,
tests/test_depth_model.py): crafted hit arrays on every window, tile and reference border by the host route and the device route, the
scan's carry, exactness under contention and beyond 32 bits, order and batch independence, lifetime and state, and end to end behind
map_batch / map_batch_device and through both drivers' --depth.  Every test here needs the new symbols."""
import glob
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import depth_model as DM
import extend_data as X
import hipmem
import mqx
from test_gpu_parity import mq  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
MQ_EINVAL, MQ_ESTATE = -1, -5
WINDOWS = (1, 2, 64, 1000, 4096)


@pytest.fixture(scope="module")
def T(mq):
    t = int(mq.load_library().mqdiag_depth_tile_windows())
    assert t > 0 and t % 64 == 0
    return t


def _index(mq, refs, path):
    """a finalized index with exactly these (id, name, length) references: a file with one live slot, loaded"""
    slot = np.zeros(1, dtype=mqx.slot_dtype)
    slot["key"], slot["end"], slot["count"], slot["id_rc"] = 77, 1, 1, refs[0][0] << 1
    mqx.write(str(path), mqx.params(), 4, refs, slot)
    return mq.Index.load(str(path))


def _same(got, want, tag=""):
    (gr, gb, gs, gt), (wr, wb, ws, wt) = got, want
    assert gt == wt, (tag, gt, wt)
    assert gr.dtype.itemsize == 64 and gb.dtype == np.uint64 and gs.dtype == np.uint32
    for f in DM.ref_depth_dtype.names:
        assert np.array_equal(gr[f].astype(np.uint64), wr[f].astype(np.uint64)), (tag, f, gr[f][:8], wr[f][:8])
    for name, g, w in (("window_bases", gb, wb), ("window_starts", gs, ws)):
        assert g.size == w.size, (tag, name, g.size, w.size)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (tag, name, bad[:4], g[bad[:4]], w[bad[:4]])


def _by_device(mq, d, hits, stream=0):
    buf = hipmem.DevBuf.from_numpy(hits) if hits.size else hipmem.DevBuf(16)
    d.add_device(buf.ptr, hits.size, stream)
    return buf  # (the caller keeps it alive until the result has waited for the device)


@pytest.fixture(scope="module")
def crafted(T):
    """(refs, hits, {min_mapq: model}) per window: every model computed once"""
    out = {}
    for w in WINDOWS + (5000,):
        refs, hits = DM.crafted(T, w) if w != 5000 else ([(0, "a", 1), (2, "b", 5), (3, "c", 100), (7, "d", 999)], DM.crafted(T, 7)[1])
        out[w] = (refs, hits, {q: DM.model(refs, hits, w, q) for q in (0, 1, 60)})
    return out


@pytest.mark.parametrize("w", WINDOWS + (5000,))
def test_crafted_hits_both_routes(mq, crafted, tmp_path, w):
    refs, hits, want = crafted[w]
    ix = _index(mq, refs, tmp_path / "c.mqx")
    for q in (0, 1, 60):
        host, dev = mq.api.Depth(ix, window=w, min_mapq=q), mq.api.Depth(ix, window=w, min_mapq=q)
        host.add(hits)
        keep = _by_device(mq, dev, hits)
        _same(host.result(), want[q], "host w=%d q=%d" % (w, q))
        _same(dev.result(), want[q], "device w=%d q=%d" % (w, q))
        keep.free()
        host.close()
        dev.close()
    ix.close()


def test_scan_carry(mq, T, tmp_path):
    for w in (1, 64):
        refs, hits = DM.carry_case(T, w)
        ix = _index(mq, refs, tmp_path / ("k%d.mqx" % w))
        d = mq.api.Depth(ix, window=w, min_mapq=60)
        d.add(hits)
        got = d.result()
        _same(got, DM.model(refs, hits, w, 60), "carry w=%d" % w)
        assert (got[1][3 * T:4 * T] == 0).all() and int(got[1][2 * T]) >= w
        d.close()
        ix.close()


def test_contention_and_width(mq, tmp_path):
    refs = [(3, "big", 3 << 20)]
    ix = _index(mq, refs, tmp_path / "b.mqx")
    d = mq.api.Depth(ix, window=1000, min_mapq=0)
    same = DM.hits_of([(1, 3, 60, 5010, 5500)] * 100000)
    d.add(same)
    _, wb, ws, tot = d.result()
    assert int(wb[5]) == 100000 * 491 and int(ws[5]) == 100000 and int(wb.sum()) == int(wb[5]) and tot["counted"] == 100000
    d.close()
    d = mq.api.Depth(ix, window=1 << 20, min_mapq=0)
    wide = DM.hits_of([(1, 3, 0, 1 << 20, (2 << 20) - 1)] * 5000)
    keep = _by_device(mq, d, wide)
    recs, wb, ws, tot = d.result()
    assert wb.tolist() == [0, 5000 << 20, 0] and 5000 << 20 > 1 << 32 and ws.tolist() == [0, 5000, 0]
    assert int(recs["bases"][0]) == int(recs["max_window_bases"][0]) == 5000 << 20 and int(recs["zero_windows"][0]) == 2
    keep.free()
    d.close()
    ix.close()


def test_order_batches_threads_midway_clear(mq, crafted, tmp_path):
    w = 64
    refs, hits, want = crafted[w]
    ix = _index(mq, refs, tmp_path / "o.mqx")
    rng = np.random.default_rng(5)
    shuffled = hits[rng.permutation(hits.size)]
    d = mq.api.Depth(ix, window=w, min_mapq=60)
    d.add(hits[:0])  # n = 0 is legal
    keep = [_by_device(mq, d, hits[:0])]
    assert d.result()[3] == dict(offered=0, counted=0, not_mapped=0, below_mapq=0, out_of_range=0) and int(d.result()[1].sum()) == 0
    d.add(shuffled)
    _same(d.result(), want[60], "shuffled, one batch")
    for size in (63, 64, 65, 257, 1):
        d.clear()
        assert int(d.result()[1].sum()) == 0 and d.result()[3]["offered"] == 0
        part = shuffled if size > 1 else shuffled[:300]
        for j, at in enumerate(range(0, part.size, size)):
            if j & 1:
                keep.append(_by_device(mq, d, part[at:at + size]))
            else:
                d.add(part[at:at + size])
        _same(d.result(), want[60] if size > 1 else DM.model(refs, part, w, 60), "batches of %d" % size)
    # a result taken mid-way is the model of the prefix and disturbs nothing
    d.clear()
    half = hits.size // 2
    d.add(hits[:half])
    _same(d.result(), DM.model(refs, hits[:half], w, 60), "mid-way")
    keep.append(_by_device(mq, d, hits[half:]))
    _same(d.result(), want[60], "behind a mid-way result")
    # two host threads at once
    d.clear()
    errs = []

    def feed(part):
        try:
            for at in range(0, part.size, 97):
                d.add(part[at:at + 97])
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=feed, args=(p,)) for p in (shuffled[:half], shuffled[half:])]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs
    _same(d.result(), want[60], "two threads")
    for k in keep:
        k.free()
    d.close()
    ix.close()


def test_lifetime_and_state(mq, simlib):
    L = mq.load_library()
    import ctypes as C
    _, _, names = X.contigs(simlib)
    ix = mq.Index(mq.Params())
    for r in range(X.SPLIT):
        ix.add_ref(r, names[r], X.contig(simlib, r))
    h = C.c_void_p()
    assert L.mq_depth_new(ix.handle, 1000, 60, C.byref(h)) == MQ_ESTATE and b"not finalized" in L.mq_last_error() and not h.value
    ix.finalize()
    for bad in (0, (1 << 24) + 1):
        assert L.mq_depth_new(ix.handle, bad, 60, C.byref(h)) == MQ_EINVAL and not h.value
    big = mq.api.Depth(ix, window=1 << 24, min_mapq=0)
    assert big.result()[0]["n_windows"].tolist() == [1] * X.SPLIT
    big.close()
    d = mq.api.Depth(ix, window=1000, min_mapq=0)
    refs = [(r, names[r], X.LENS[r]) for r in range(X.SPLIT)]
    hits = DM.hits_of([(1, r, 60, 100, X.LENS[r] - 7) for r in range(X.SPLIT)] + [(1, X.SPLIT, 60, 0, 10), (1, 9, 60, 0, 10)])
    d.add(hits)
    want = DM.model(refs, hits, 1000, 0)
    _same(d.result(), want, "before")
    other = mq.Index(mq.Params())
    other.add_ref(0, names[X.SPLIT + 1], X.contig(simlib, X.SPLIT + 1))
    other.finalize()
    ix.reopen()
    ix.add_ref(X.SPLIT, names[X.SPLIT], X.contig(simlib, X.SPLIT))
    ix.finalize()
    ix.merge(other, id_base=9)
    d.add(hits)  # ids 3 and 9 exist in the index now; the accumulator keeps its snapshot
    got = d.result()
    _same(got, DM.model(refs, np.concatenate([hits, hits]), 1000, 0), "behind reopen and merge")
    assert got[3]["out_of_range"] == 4 and got[0]["ref_id"].tolist() == list(range(X.SPLIT))
    fresh = mq.api.Depth(ix, window=1000, min_mapq=0)
    assert fresh.result()[0]["ref_id"].tolist() == list(range(X.SPLIT + 1)) + [9]
    fresh.close()
    d.close()
    other.close()
    ix.close()


# ------------------------------------------------------------------ end to end
N_READS = 40  # of extend_data's reads: the oracle maps them onto all six contigs and leaves windows of 1,000 bases without a read


@pytest.fixture(scope="module")
def world(mq, simlib):
    _, _, names = X.contigs(simlib)
    ix = mq.Index(mq.Params())
    for r in range(len(X.LENS)):
        ix.add_ref(r, names[r], X.contig(simlib, r))
    ix.finalize()
    r = X.reads(simlib)
    bases, offs = r["bases"][:int(r["offsets"][N_READS])], r["offsets"][:N_READS + 1].astype(np.uint64)
    yield ix, [(i, names[i], X.LENS[i]) for i in range(len(X.LENS))], bases, offs
    ix.close()


def test_the_chosen_reads_make_the_comparison_real(oracle, simlib):
    """on the CPU, with the oracle: hits on at least three references and an empty window somewhere"""
    _, _, names = X.contigs(simlib)
    po, ox = oracle.params(), oracle.Index()
    for r in range(len(X.LENS)):
        ox.add_ref(r, names[r], X.contig(simlib, r), po)
    r = X.reads(simlib)
    want = ox.map_batch(r["bases"][:int(r["offsets"][N_READS])], r["offsets"][:N_READS + 1], po, threads=2)
    m = want["mapped"] != 0
    rows = [(1, int(a), int(q), int(s), int(e)) for a, q, s, e in zip(want["ref_id"][m], want["mapq"][m], want["r_start"][m], want["r_end"][m])]
    recs, _, _, tot = DM.model([(i, names[i], X.LENS[i]) for i in range(len(X.LENS))], DM.hits_of(rows), 1000, 60)
    assert int((recs["reads"] > 0).sum()) >= 3 and int(recs["zero_windows"].sum()) > 0 and tot["counted"] > 10


def test_behind_map_batch_and_map_batch_device(mq, world):
    ix, refs, bases, offs = world
    hits = ix.map_batch(bases, offs)
    want = DM.model(refs, hits, 1000, 60)
    assert int((want[0]["reads"] > 0).sum()) >= 3 and int(want[0]["zero_windows"].sum()) > 0 and want[3]["counted"] > 10
    one = mq.api.Depth(ix)  # window 1000, mapq >= 60
    one.add(hits)
    _same(one.result(), want, "map_batch, then add")
    ctx = ix.context()
    ctx.reserve_redo(16, 40000)
    two = mq.api.Depth(ix)
    stream = hipmem.new_stream()
    db, do, dout = hipmem.DevBuf.from_numpy(np.concatenate([bases, np.zeros(64, np.uint8)])), hipmem.DevBuf.from_numpy(offs), hipmem.DevBuf(N_READS * 48)
    ctx.map_batch_device(db.ptr, do.ptr, N_READS, int(offs[-1] - offs[0]), dout.ptr, stream)
    two.add_device(dout.ptr, N_READS, stream)  # no host synchronisation in between
    got = two.result()
    assert np.array_equal(dout.to_numpy(mq.hit_dtype, N_READS).view(np.uint8), hits.view(np.uint8))
    _same(got, want, "map_batch_device, then add_device on its stream")
    _same(got, one.result(), "the two routes")
    for x in (one, two, ctx):
        x.close()
    assert hipmem.hip().hipStreamDestroy(stream) == 0
    for b in (db, do, dout):
        b.free()


def test_drivers(mq, simlib, world, tmp_path):
    """--depth of both drivers: the two files are the formatters' bytes for the model of the PAF the same run wrote, the same from either
    driver; the PAF is the one without the flag; the native driver also over two (fake) GPUs and with a second pass, whose hits count too"""
    from mapquik_amd import build
    _, refs, bases, offs = world
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    native, python = [build.build_cli()], [sys.executable, "-m", "mapquik_amd"]
    t = lambda n: str(tmp_path / n)  # noqa: E731
    with open(t("reads.fa"), "wb") as f:
        for i in range(N_READS):
            f.write(b">r%d\n" % i + bases[int(offs[i]):int(offs[i + 1])].tobytes() + b"\n")
    with open(t("ref.fa"), "wb") as f:
        for i, name, _ in refs:
            f.write(b">" + name.encode() + b"\n" + X.contig(simlib, i).tobytes() + b"\n")
    common = [t("reads.fa"), "--reference", t("ref.fa")]

    def run(cmd, p, extra, **more):
        res = subprocess.run(cmd + common + ["-p", t(p)] + extra, capture_output=True, text=True, timeout=300, env=dict(env, **more))
        assert res.returncode == 0, (p, res.stderr[-2000:])
        return res.stdout

    def expect(pafs, w, q):
        h = np.concatenate([DM.hits_of_paf(open(p).read(), refs) for p in pafs])
        recs, wb, ws, tot = DM.model(refs, h, w, q)
        return DM.bed_bytes(refs, recs, wb, ws, w), DM.tsv_bytes(refs, recs, w), recs, tot

    run(native, "n0", [])
    run(python, "p0", [])
    outs = {"n1": run(native, "n1", ["--depth"]), "p1": run(python, "p1", ["--depth"]),
            "n2": run(native, "n2", ["--depth", "--gpus", "2", "--batch-bases", "60000", "--depth-window", "64", "--depth-min-mapq", "0"], MQ_FAKE_MULTI="1")}
    paf0 = open(t("n0.paf"), "rb").read()
    assert paf0.count(b"\n") > 10 and open(t("p0.paf"), "rb").read() == paf0 and not os.path.exists(t("n0.depth.bed"))
    for p, w, q in (("n1", 1000, 60), ("p1", 1000, 60), ("n2", 64, 0)):
        assert open(t(p + ".paf"), "rb").read() == paf0, (p, "the PAF changes with --depth")
        bed, tsv, recs, tot = expect([t(p + ".paf")], w, q)
        assert open(t(p + ".depth.bed"), "rb").read() == bed and open(t(p + ".depth.tsv"), "rb").read() == tsv, p
        line = [ln for ln in outs[p].splitlines() if ln.startswith("Depth: ")]
        assert len(line) == 1 and line[0].startswith("Depth: %d of %d hits counted" % (tot["counted"], N_READS)) and line[0].endswith(
            ": %d bases in %d windows of %d" % (int(recs["bases"].sum()), int(recs["n_windows"].sum()), w)), (p, line)
    assert open(t("n1.depth.bed"), "rb").read() == open(t("p1.depth.bed"), "rb").read() and open(t("n1.depth.tsv"), "rb").read() == open(t("p1.depth.tsv"), "rb").read()
    # a first pass that leaves reads behind (k = 15: the oracle maps 34 of the 40, ten of them with mapq 0), a second pass at the defaults
    run(native, "s0", ["-k", "15", "--second-pass", "5,31,0.01"])
    run(native, "s1", ["-k", "15", "--second-pass", "5,31,0.01", "--depth", "--depth-min-mapq", "0"])
    first, second = [t("s1.paf")], glob.glob(t("s1-*.paf"))
    assert len(second) == 1 and open(second[0]).read().count("\n") > 0
    assert open(t("s1.paf"), "rb").read() == open(t("s0.paf"), "rb").read()
    bed, tsv, recs, tot = expect(first + second, 1000, 0)
    assert open(t("s1.depth.bed"), "rb").read() == bed and open(t("s1.depth.tsv"), "rb").read() == tsv
    assert tot["counted"] == open(t("s1.paf")).read().count("\n") + open(second[0]).read().count("\n") and not glob.glob(t("s1-*.depth.bed"))
