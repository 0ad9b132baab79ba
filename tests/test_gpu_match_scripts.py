"""GPU: crafted index payloads through every Match-run transition (tests/match_scripts.py; test_match_scripts_cases.py proves on the CPU
that the two references agree on every read, that every probe is decisive and what the batches cover).  One crafted table per parameter
set goes to the library through a file (mqx.Table.to_file, mq.Index.load) and to the oracle through Index.add / set_ref.  Every row asserts
that its configuration took effect (spec id, seeding paths), and that the records of the device form and of the host form, both written
into 0xFF-filled buffers, equal the oracle's column for column, n_kminmers included.  Every mismatch of a row is reported, as
(family, border, state, kind, field, got, want).

  row            configuration                                            set
  product pair   SpecFixed<5,31,hpc> (spec id 1)                          default
  nospec         MQ_NO_SPEC=1 / the parameters no spec fits               default / dense
  chunk4         MQ_CHAIN_CHUNK=4                                         dense
  instrumented   probe_stats                                              dense
  split          MQ_PIPELINE=split                                        dense
  variant        seeding variant 32 (the <.., VAR> pair; no tuple of      default
                 these reads is a palindrome, so keys and strands stay)
  fast_kh        MQ_FLAG_FAST_KH, keys from the oracle's bit 64           default
  anchors        a reserving context, spans and pool against the model    dense
  window         2047 / 2048 / 2049 runs back to back (family C)          dense

Timings on an MI355X (pytest --durations=0; none is asserted): the module 11.6 s for 10 tests.  The first dense row pays for the dense
set's construction and the oracle's answer, 6.5 s (1,800 reads of 832 k-min-mers finished key by key, see match_scripts.read_with_kminmers);
product pair, variant and fast_kh about 1 s each (the default set's three constructions), anchors 1.0 s (the model's lists), window 0.2 s,
every other row 0.02 s.  The answers are computed once per module.
No kernel fault was found, and no sensitivity build was made for this module.
"""
import numpy as np
import pytest

import anchors_model as A
import match_scripts as S
import mqx
from test_gpu_lattice import COLUMNS, _expect_paths
from test_gpu_lattice_matrix import _host_poisoned
from test_gpu_poison import _assert_all_written, _launch_poisoned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


class _Answer:
    pass


_answers = {}


def answer(O, which, variant=0, batch="main"):
    """a set's batch, the oracle twin of its table and the oracle's records, once per module"""
    key = (which, variant, batch)
    if key not in _answers:
        w = S.world(O, which, variant)
        a = _Answer()
        a.w, a.po = w, w.po
        a.idx = w.main if batch == "main" else w.window
        a.reads = [w.reads[i] for i in a.idx]
        a.bases, a.offs = S.batch_of(w, a.idx)
        a.pts = S.points_of(w, a.idx)
        O.lib().mqo_set_variant(variant)
        try:
            a.ox = w.table.to_oracle(O)
            a.want, a.diag = a.ox.map_batch_diag(a.bases, a.offs, a.po, threads=8)
        finally:
            O.lib().mqo_set_variant(0)
        a.paths = _expect_paths(a.pts, a.po)
        n_dirty = sum(1 for rd in a.reads if rd.with_n)
        assert a.paths == (len(a.reads) - n_dirty, n_dirty) and (batch != "main" or n_dirty >= 10)
        assert int((a.want["mapped"] != 0).sum()) >= len(a.reads) // 2
        _answers[key] = a
    return _answers[key]


def _load(mq, a, tmp_path, flags=0):
    """the set's table through a file; flags: the parameter word's (a seeding variant, MQ_FLAG_FAST_KH).  Environment hooks are read here."""
    t = a.w.table
    if flags:
        t = mqx.Table(dict(t.params, flags=flags), t.table_slots, t.refs, t.entries, t.name)
    p = str(tmp_path / "scripts.mqx")
    hdr = t.to_file(p)
    ix = mq.Index.load(p)
    st = ix.stats()
    assert {k: st[k] for k in mqx.HEADER_NAMES} == hdr
    return ix


def _compare(mq, got, a, what):
    """every record against the oracle's; all mismatches, named by what the read probes"""
    w, d = a.want, a.diag
    bad = []
    m = w["mapped"] != 0
    cols = [("status", got["status"].astype(np.uint64), np.where(m, 1, 0).astype(np.uint64), np.ones(m.size, bool)),
            ("n_kminmers", got["n_kminmers"].astype(np.uint64), d["n_kminmers"].astype(np.uint64), np.ones(m.size, bool))]
    cols += [(f, mq.hit_column(got, f), w[f].astype(np.uint64), m) for f in COLUMNS]
    for f, g, x, where in cols:
        for i in np.flatnonzero(where & (g != x)):
            bad.append(a.reads[i].label() + (f, int(g[i]), int(x[i])))
    assert not bad, "%s: %d fields differ from the oracle's: %s" % (what, len(bad), bad[:40])


def _run(mq, ix, a, what, spec, host=True):
    dev = _launch_poisoned(mq, ix, a.bases, a.offs)
    _assert_all_written(dev)
    assert ix.last_map_path_counts() == a.paths, (what, "device form", ix.last_map_path_counts(), a.paths)
    assert ix.last_map_spec() == spec, (what, "device form", ix.last_map_spec(), spec)
    _compare(mq, dev, a, (what, "device form"))
    if host:
        hh = _host_poisoned(mq, ix, a)
        _assert_all_written(hh)
        assert ix.last_map_path_counts() == a.paths and ix.last_map_spec() == spec, (what, "host form")
        _compare(mq, hh, a, (what, "host form"))
        assert hh.tobytes() == dev.tobytes(), (what, "host form against device form")
    return dev


def test_product_pair(mq, oracle, tmp_path):
    a = answer(oracle, "default")
    ix = _load(mq, a, tmp_path)
    _run(mq, ix, a, "product pair", spec=1)
    ix.close()


@pytest.mark.parametrize("which", ["default", "dense"])
def test_nospec(mq, oracle, tmp_path, monkeypatch, which):
    if which == "default":
        monkeypatch.setenv("MQ_NO_SPEC", "1")
    a = answer(oracle, which)
    ix = _load(mq, a, tmp_path)
    _run(mq, ix, a, ("nospec", which), spec=0)
    ix.close()


def test_chunk4(mq, oracle, tmp_path, monkeypatch):
    monkeypatch.setenv("MQ_CHAIN_CHUNK", "4")
    a = answer(oracle, "dense")
    ix = _load(mq, a, tmp_path)
    _run(mq, ix, a, "chunk4", spec=0)
    ix.close()


def test_instrumented(mq, oracle, tmp_path):
    from hipmem import DevBuf, device_sync, memset
    a = answer(oracle, "dense")
    ix = _load(mq, a, tmp_path)
    n = a.offs.size - 1
    db, do, out = DevBuf.from_numpy(a.bases), DevBuf.from_numpy(a.offs), DevBuf(n * mq.hit_dtype.itemsize)
    memset(out, 0xFF)
    ix.reserve(n, int(a.offs[-1]))
    lookups, _ = ix.probe_stats(db.ptr, do.ptr, n, int(a.offs[-1]), out.ptr)
    device_sync()
    hits = out.to_numpy(mq.hit_dtype, n)
    cyc, _ = ix.last_read_cycles(n)
    for b in (db, do, out):
        b.free()
    assert lookups == int(a.diag["n_kminmers"].sum()) and (cyc != 0).all()   # every read went through the instrumented pair
    assert ix.last_map_path_counts() == a.paths
    _assert_all_written(hits)
    _compare(mq, hits, a, "instrumented")
    ix.close()


def test_split(mq, oracle, tmp_path, monkeypatch):
    monkeypatch.setenv("MQ_PIPELINE", "split")
    a = answer(oracle, "dense")
    ix = _load(mq, a, tmp_path)
    _run(mq, ix, a, "split", spec=0)
    ix.close()


def _same_reads(a, b):
    assert [rd.seq for rd in a.w.reads] == [rd.seq for rd in b.w.reads]


def test_variant(mq, oracle, tmp_path):
    """seeding variant 32 (a palindromic tuple counts as reversed): none of these reads' tuples is one, so the oracle switched to the
    variant gives the same keys and strands -- asserted -- and the library runs the <.., VAR> pair on them"""
    a, base = answer(oracle, "default", 32), answer(oracle, "default")
    _same_reads(a, base)
    for x, y in zip(a.w.reads, base.w.reads):
        assert x.km.tobytes() == y.km.tobytes(), x.name
    assert a.want.tobytes() == base.want.tobytes()
    P = mq.Params(seeding_variant=32)
    assert P.seeding_variant == 32
    ix = _load(mq, a, tmp_path, flags=int(P.flags))
    assert ix.get_params().seeding_variant == 32
    _run(mq, ix, a, "variant 32", spec=0)
    ix.close()


def test_fast_kh(mq, oracle, tmp_path):
    """MQ_FLAG_FAST_KH: the table's keys are the oracle's under bit 64 -- every one differs from SipHash's, every other field equal"""
    a, base = answer(oracle, "default", 64), answer(oracle, "default")
    for x, y in zip(a.w.reads, base.w.reads):
        assert not (x.km["hash"] == y.km["hash"]).any() and all(np.array_equal(x.km[f], y.km[f]) for f in ("start", "end", "offset", "rev")), x.name
    P = mq.Params(fast_kh=True)
    ix = _load(mq, a, tmp_path, flags=int(P.flags))
    assert ix.get_params().fast_kh
    _run(mq, ix, a, "fast_kh", spec=0)
    ix.close()


def test_anchors(mq, oracle, tmp_path):
    """a reserving context: spans and pool equal the model's run for run for every mapped read, {0, 0} otherwise; hits the oracle's"""
    from test_gpu_anchors import _check, _reserving
    a = answer(oracle, "dense")
    exp = A.batch(oracle, a.ox, a.po, a.bases, a.offs)
    assert [e is not None for e in exp] == (a.want["mapped"] != 0).tolist()
    need = sum(len(e.runs) for e in exp if e)
    ix = _load(mq, a, tmp_path)
    c = _reserving(ix, len(exp), need)
    hits = c.map_batch(a.bases, a.offs)
    assert c.last_map_spec() == 0
    _compare(mq, hits, a, "anchors, host form")
    spans, anchors, info = got = c.anchors()
    bad = []
    for r, e in enumerate(exp):   # every read first, named: (family, border, state, kind, "anchors", got, want)
        f, n = int(spans["first"][r]), int(spans["count"][r])
        have = [tuple(int(v) for v in x) for x in anchors[f:f + n].tolist()] if n and f != 0xFFFFFFFF else []
        want = A.as32(e.runs) if e else []
        if have != want or (e is None and (f, n) != (0, 0)):
            bad.append(a.reads[r].label() + ("anchors", have[:6], want[:6]))
    assert not bad, "anchors: %d reads differ from the model's: %s" % (len(bad), bad[:20])
    assert _check(got, exp, need) == 0
    c.close()
    ix.close()


def test_window(mq, oracle, tmp_path):
    """family C, 2047 / 2048 / 2049 runs back to back: the host form redoes the third read and equals the oracle; the device form without a
    redo arena reports MQ_HIT_OVERFLOW for that read alone; with an arena it equals the oracle"""
    a = answer(oracle, "dense", batch="window")
    assert a.diag["n_matches"].tolist() == [2047, 2048, 2049]
    ix = _load(mq, a, tmp_path)
    hh = _host_poisoned(mq, ix, a)
    _compare(mq, hh, a, "window, host form")
    raw = _launch_poisoned(mq, ix, a.bases, a.offs)
    assert raw["status"].tolist()[2] == 2 and (raw["status"][:2] < 2).all(), raw["status"].tolist()
    assert raw[:2].tobytes() == hh[:2].tobytes()
    ix.reserve_redo(3, max(len(rd.seq) for rd in a.reads))
    try:
        dev = _launch_poisoned(mq, ix, a.bases, a.offs)
        assert ix.redo_counts() == (1, 0)
        _compare(mq, dev, a, "window, device form with an arena")
        assert dev.tobytes() == hh.tobytes()
    finally:
        ix.reserve_redo(0, 0)
    ix.close()
