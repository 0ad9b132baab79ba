"""GPU: the coordinate sorter (mq_sorter) against the numpy model of tests/sort_model.py (held against a second wording on the CPU,
tests/test_sort_model.py): kept counts on every wave, tile and scan border by the host route and the device route, each of the key's 11
digits as the only one that differs, stability under pressure, filtering, independence of order / batches / threads / streams, capacity,
state and lifetime, and end to end behind map_batch / map_batch_device and through both drivers' --sort.  Every test here needs the new
symbols."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import extend_data as X
import hipmem
import mqx
import sort_model as SM
from test_gpu_parity import mq  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
MQ_EINVAL, MQ_ESTATE, MQ_EOVERFLOW = -1, -5, -6
EMPTY = dict(offered=0, kept=0, not_mapped=0, below_mapq=0, out_of_range=0)


@pytest.fixture(scope="module")
def T(mq):
    t = int(mq.load_library().mqdiag_sort_tile_records())
    assert t > 0 and t % 256 == 0
    return t


def _index(mq, refs, path):
    """a finalized index with exactly these (id, name, length) references: a file with one live slot, loaded"""
    slot = np.zeros(1, dtype=mqx.slot_dtype)
    slot["key"], slot["end"], slot["count"], slot["id_rc"] = 77, 1, 1, refs[0][0] << 1
    mqx.write(str(path), mqx.params(), 4, refs, slot)
    return mq.Index.load(str(path))


@pytest.fixture(scope="module")
def ix(mq, tmp_path_factory):
    i = _index(mq, SM.REFS, tmp_path_factory.mktemp("sort") / "r.mqx")
    yield i
    i.close()


def _same(got, want, tag=""):
    (go, gr, gt), (wo, wr, wt) = got, want
    assert gt == wt, (tag, gt, wt)
    assert go.dtype == np.uint32 and gr.dtype.itemsize == 24 and go.size == wo.size, (tag, go.size, wo.size)
    bad = np.flatnonzero(go != wo)
    assert bad.size == 0, (tag, "order", bad.size, bad[:4], go[bad[:4]], wo[bad[:4]])
    for f in SM.sort_ref_dtype.names:
        assert np.array_equal(gr[f].astype(np.uint64), wr[f].astype(np.uint64)), (tag, f, gr[f][:8], wr[f][:8])


def _feed(s, hits, ords, dev=None, stream=0):
    """every stretch of consecutive ordinals in one add call: by the host route, or from the device copy `dev` of hits"""
    for a, b in SM.runs(ords):
        if dev is None:
            s.add(hits[a:b], int(ords[a]))
        else:
            s.add_device(dev.ptr + 48 * a, b - a, int(ords[a]), stream)


def _dev(hits):
    return hipmem.DevBuf.from_numpy(hits) if hits.size else hipmem.DevBuf(16)


@pytest.fixture(scope="module")
def sized(T):
    """n -> (hits, ordinals, model): every model computed once"""
    out = {}
    for n in SM.border_counts(T):
        hits, ords = SM.sized(n)
        out[n] = (hits, ords, SM.model(SM.REFS, hits, ords, 0), SM.passes(SM.REFS, hits, ords, 0))
    return out


@pytest.mark.parametrize("route", ["host", "device"])
def test_sizes_at_every_border(mq, ix, T, sized, route):
    for n, (hits, ords, want, npass) in sized.items():
        s = mq.api.Sorter(ix, capacity=n if route == "device" else 0, min_mapq=0)
        keep = _dev(hits) if route == "device" else None
        _feed(s, hits, ords, keep)
        _same(s.result(), want, "%s n=%d" % (route, n))
        assert s.passes() == npass, (route, n, s.passes(), npass)
        s.close()
        if keep:
            keep.free()


@pytest.fixture(scope="module")
def sparse(mq, tmp_path_factory):
    i = _index(mq, SM.DIGIT_REFS, tmp_path_factory.mktemp("sortd") / "d.mqx")
    yield i
    i.close()


@pytest.mark.parametrize("d", range(SM.DIGITS))
def test_each_digit_alone(mq, ix, sparse, d):
    for tagged in (False, True) if d >= 4 else (False,):
        refs, hits, ords = SM.digit_case(d, tagged)
        s = mq.api.Sorter(ix if refs is SM.REFS else sparse, min_mapq=0)
        _feed(s, hits, ords)
        got = s.result()
        _same(got, SM.model(refs, hits, ords, 0), "digit %d tagged %d" % (d, tagged))
        assert s.passes() == (2 if tagged else 1) == SM.passes(refs, hits, ords, 0)
        if d >= 8:
            mine = got[1][np.isin(got[1]["ref_id"], SM.DIGIT_IDS[d])]
            assert mine["count"].tolist() == [1] * 256 and mine["first"].tolist() == list(range(256))
        s.close()


def test_stability_under_pressure(mq, ix, T):
    cases, ords = SM.stability_cases(T)
    for name, hits in cases.items():
        want, npass = SM.model(SM.REFS, hits, ords, 0), SM.passes(SM.REFS, hits, ords, 0)
        host, dev = mq.api.Sorter(ix), mq.api.Sorter(ix, capacity=hits.size)
        keep = _dev(hits)
        _feed(host, hits, ords)
        _feed(dev, hits, ords, keep)
        for s, tag in ((host, "host"), (dev, "device")):
            _same(s.result(), want, "%s %s" % (name, tag))
            assert s.passes() == npass, (name, tag, s.passes(), npass)
            s.close()
        keep.free()


def test_filtering(mq, ix, T):
    hits, ords = SM.filter_case(T)
    keep = _dev(hits)
    for q in (0, 1, 60):
        want = SM.model(SM.REFS, hits, ords, q)
        assert want[2]["offered"] == sum(want[2][k] for k in SM.TOTALS[1:]) and want[2]["out_of_range"] > 0 and want[2]["not_mapped"] > 0
        host, dev = mq.api.Sorter(ix, min_mapq=q), mq.api.Sorter(ix, capacity=hits.size, min_mapq=q)
        _feed(host, hits, ords)
        _feed(dev, hits, ords, keep)
        _same(host.result(), want, "host q=%d" % q)
        _same(dev.result(), want, "device q=%d" % q)
        assert host.passes() == SM.passes(SM.REFS, hits, ords, q)
        host.close()
        dev.close()
    keep.free()


def test_order_batches_threads_streams_midway_clear(mq, ix, T):
    hits, ords = SM.filter_case(T)
    want = SM.model(SM.REFS, hits, ords, 1)
    rng = np.random.default_rng(3)
    s = mq.api.Sorter(ix, capacity=hits.size, min_mapq=1)
    s.add(hits[:0], 9)  # n = 0 is legal
    assert s.result()[2] == EMPTY and s.result()[0].size == 0 and s.passes() == 0
    streams = [hipmem.new_stream(), hipmem.new_stream()]
    keep = _dev(hits)
    for size in (1, 63, 64, 65, 257, T + 1):
        s.clear()
        assert s.result()[2] == EMPTY
        part = slice(0, hits.size) if size > 1 else slice(100, 400)
        cuts = list(range(part.start, part.stop, size))
        for j in rng.permutation(len(cuts)).tolist():  # the batches in another order, alternately by the host and on two streams
            a, b = cuts[j], min(cuts[j] + size, part.stop)
            if j % 3 == 0:
                s.add(hits[a:b], int(ords[a]))
            else:
                s.add_device(keep.ptr + 48 * a, b - a, int(ords[a]), streams[j % 3 - 1])
        _same(s.result(), want if size > 1 else SM.model(SM.REFS, hits[part], ords[part], 1), "batches of %d" % size)
    # a result taken mid-way is the model of the prefix; more adds follow and the next result covers everything
    s.clear()
    half = hits.size // 2
    s.add(hits[:half], int(ords[0]))
    _same(s.result(), SM.model(SM.REFS, hits[:half], ords[:half], 1), "mid-way")
    s.add_device(keep.ptr + 48 * half, hits.size - half, int(ords[half]), streams[0])
    _same(s.result(), want, "behind a mid-way result")
    _same(s.result(), want, "a second result of the same content")
    # two host threads at once
    s.clear()
    errs = []

    def feed(a, b):
        try:
            for at in range(a, b, 97):
                s.add(hits[at:min(at + 97, b)], int(ords[at]))
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=feed, args=r) for r in ((0, half), (half, hits.size))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs
    _same(s.result(), want, "two threads")
    # a clear, then a different set
    s.clear()
    other, oords = SM.sized(T + 1)
    s.add(other, 0)
    _same(s.result(), SM.model(SM.REFS, other, oords, 1), "another set behind a clear")
    s.close()
    keep.free()
    for st in streams:
        assert hipmem.hip().hipStreamDestroy(st) == 0


def test_capacity(mq, ix, T):
    L = mq.load_library()
    n = T + 65
    hits, ords = SM.sized(n)
    want = SM.model(SM.REFS, hits, ords, 0)
    keep = _dev(hits)
    s = mq.api.Sorter(ix, capacity=n)
    s.add_device(keep.ptr, n, 0)  # exactly the capacity
    _same(s.result(), want, "at capacity")
    assert L.mq_sort_add_device(s._h, C.c_void_p(keep.ptr), 1, n, None) == MQ_EOVERFLOW and b"capacity" in L.mq_last_error()
    _same(s.result(), want, "nothing changed")
    s.reserve(2 * n + 1)  # keeps the contents, the sorted ones included
    s.reserve(5)          # never shrinks
    s.add_device(keep.ptr, n, n)
    s.add_device(keep.ptr, 1, 2 * n)
    assert L.mq_sort_add_device(s._h, C.c_void_p(keep.ptr), 1, 2 * n + 1, None) == MQ_EOVERFLOW
    three = np.concatenate([hits, hits, hits[:1]])
    _same(s.result(), SM.model(SM.REFS, three, np.arange(three.size), 0), "behind a reserve")
    s.close()
    grow = mq.api.Sorter(ix, capacity=0)  # the host route grows from nothing
    for a in range(0, n, 100):
        grow.add(hits[a:a + 100], a)
    _same(grow.result(), want, "grown from capacity 0")
    # the limits: ordinals and offered stay below 2^32 - 1
    grow.clear()
    assert L.mq_sort_add(grow._h, hits.ctypes.data_as(C.c_void_p), 2, 0xFFFFFFFE) == MQ_EINVAL
    assert L.mq_sort_add(grow._h, hits.ctypes.data_as(C.c_void_p), 1, 0xFFFFFFFF) == MQ_EINVAL
    assert L.mq_sort_add_device(grow._h, C.c_void_p(keep.ptr), 3, 0xFFFFFFFD, None) == MQ_EINVAL
    assert L.mq_sort_add_device(grow._h, C.c_void_p(keep.ptr + 8), 1, 0, None) == MQ_EINVAL and b"16-byte" in L.mq_last_error()
    grow.add(hits[:2], 0xFFFFFFFD)  # ... and 2^32 - 2 is an ordinal
    assert grow.result()[2]["kept"] == 2 and sorted(grow.result()[0].tolist()) == [0xFFFFFFFD, 0xFFFFFFFE]
    h = C.c_void_p()
    assert L.mq_sort_new(ix.handle, (1 << 32) - 1, 0, C.byref(h)) == MQ_EINVAL and not h.value
    assert L.mq_sort_reserve(grow._h, (1 << 32) - 1) == MQ_EINVAL
    grow.close()
    keep.free()


def test_state_and_lifetime(mq, ix, simlib, T):
    L = mq.load_library()
    _, _, names = X.contigs(simlib)
    raw = mq.Index(mq.Params())
    raw.add_ref(0, names[0], X.contig(simlib, 0))
    h = C.c_void_p()
    assert L.mq_sort_new(raw.handle, 0, 0, C.byref(h)) == MQ_ESTATE and b"not finalized" in L.mq_last_error() and not h.value
    raw.close()
    hits, ords = SM.sized(T + 1)
    s = mq.api.Sorter(ix)
    s.add(hits, 0)
    assert L.mq_sort_result(s._h, None, None, None, None, None) == 0  # any output may be NULL
    nk = C.c_uint64()
    assert L.mq_sort_result(s._h, None, C.byref(nk), None, None, None) == 0 and nk.value == T + 1
    assert L.mq_sort_add(s._h, None, 1, 0) == MQ_EINVAL and L.mq_sort_add(s._h, None, 0, 0) == 0
    s.close()
    # a free with adds queued on a caller's stream waits for them
    stream = hipmem.new_stream()
    keep = _dev(hits)
    s = mq.api.Sorter(ix, capacity=8 * (T + 1))
    for j in range(8):
        s.add_device(keep.ptr, T + 1, j * (T + 1), stream)
    s.close()
    assert hipmem.hip().hipStreamSynchronize(stream) == 0 and hipmem.hip().hipStreamDestroy(stream) == 0
    keep.free()


# ------------------------------------------------------------------ end to end
N_READS = 40  # of extend_data's reads, as tests/test_gpu_depth.py: the oracle maps them onto all six contigs


@pytest.fixture(scope="module")
def world(mq, simlib):
    _, _, names = X.contigs(simlib)
    wix = mq.Index(mq.Params())
    for r in range(len(X.LENS)):
        wix.add_ref(r, names[r], X.contig(simlib, r))
    wix.finalize()
    r = X.reads(simlib)
    bases, offs = r["bases"][:int(r["offsets"][N_READS])], r["offsets"][:N_READS + 1].astype(np.uint64)
    yield wix, [(i, names[i], X.LENS[i]) for i in range(len(X.LENS))], bases, offs
    wix.close()


def test_behind_map_batch_and_map_batch_device(mq, world):
    wix, refs, bases, offs = world
    hits = wix.map_batch(bases, offs)
    want = SM.model(refs, hits, np.arange(N_READS) + 1000, 0)
    assert int((want[1]["count"] > 0).sum()) >= 3 and want[2]["kept"] > 10 and not np.array_equal(want[0], np.sort(want[0]))
    one = mq.api.Sorter(wix)
    one.add(hits, 1000)
    _same(one.result(), want, "map_batch, then add")
    ctx = wix.context()
    ctx.reserve_redo(16, 40000)
    two = mq.api.Sorter(wix, capacity=N_READS)
    stream = hipmem.new_stream()
    db, do, dout = hipmem.DevBuf.from_numpy(np.concatenate([bases, np.zeros(64, np.uint8)])), hipmem.DevBuf.from_numpy(offs), hipmem.DevBuf(N_READS * 48)
    ctx.map_batch_device(db.ptr, do.ptr, N_READS, int(offs[-1] - offs[0]), dout.ptr, stream)
    two.add_device(dout.ptr, N_READS, 1000, stream)  # no host synchronisation in between
    got = two.result()
    assert np.array_equal(dout.to_numpy(mq.hit_dtype, N_READS).view(np.uint8), hits.view(np.uint8))
    _same(got, want, "map_batch_device, then add_device on its stream")
    for x in (one, two, ctx):
        x.close()
    assert hipmem.hip().hipStreamDestroy(stream) == 0
    for b in (db, do, dout):
        b.free()


def test_drivers(mq, simlib, world, tmp_path):
    """--sort of both drivers: the two files are the model's for the PAF the same run wrote, the same bytes from either driver; the PAF is
    the one without the flag; both also in small chunks (the native driver over two fake GPUs) with a mapq threshold nothing passes"""
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

    run(native, "n0", [])
    outs = {"n1": run(native, "n1", ["--sort"]), "p1": run(python, "p1", ["--sort"]),
            "n2": run(native, "n2", ["--sort", "--sort-min-mapq", "61", "--gpus", "2", "--batch-bases", "60000"], MQ_FAKE_MULTI="1"),
            "p2": run(python, "p2", ["--sort", "--sort-min-mapq", "61", "--batch-bases", "60000"])}
    paf0 = open(t("n0.paf"), "rb").read()
    assert paf0.count(b"\n") > 10 and not os.path.exists(t("n0.sorted.paf"))
    for p, q in (("n1", 0), ("p1", 0), ("n2", 61), ("p2", 61)):
        assert open(t(p + ".paf"), "rb").read() == paf0, (p, "the PAF changes with --sort")
        sp, tsv, recs, tot = SM.sorted_files(refs, paf0, q)
        assert open(t(p + ".sorted.paf"), "rb").read() == sp and open(t(p + ".sorted.tsv"), "rb").read() == tsv, p
        tot = dict(tot, offered=N_READS, not_mapped=N_READS - paf0.count(b"\n"))
        assert SM.log_line(recs, tot, q) in outs[p].splitlines(), (p, outs[p])
    # (the sort and the threshold both do something: no mapq passes 60, so the second pair of runs keeps nothing and writes an empty file)
    assert SM.sorted_files(refs, paf0, 0)[0] != paf0 and SM.sorted_files(refs, paf0, 61)[3]["below_mapq"] == paf0.count(b"\n")
