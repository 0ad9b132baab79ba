"""GPU: mq_index_coverage -- which bases of which reference the live k-min-mers of a finalized index span -- against the numpy model of
tests/coverage_model.py (held against a per-base array and the oracle on the CPU, tests/test_coverage_model.py): crafted index files on
every edge of the bitmap's words and tiles through every way a file becomes a table, built indexes through save, resize, extension and
merge, the result's lifetime, and both drivers' --coverage.  Every test here needs the new symbols."""
import os
import subprocess
import sys

import numpy as np
import pytest

import coverage_model as CM
import extend_data as X
import mqx
from test_gpu_parity import mq  # noqa: F401  (the module fixture)

pytestmark = pytest.mark.gpu
MQ_ESTATE = -5


def _same(got, want, tag=""):
    (gr, gi, go), (wr, wi, wo) = got, want
    assert go == wo, (tag, go, wo)
    assert gr.dtype.itemsize == 48 and gi.dtype.itemsize == 8
    for f in CM.ref_coverage_dtype.names:
        assert np.array_equal(gr[f].astype(np.uint64), wr[f].astype(np.uint64)), (tag, f, gr[f][:8], wr[f][:8])
    assert gi.size == wi.size, (tag, gi.size, wi.size)
    for f in ("start", "end"):
        bad = np.flatnonzero(gi[f] != wi[f])
        assert bad.size == 0, (tag, f, bad[:4], gi[bad[:4]], wi[bad[:4]])


@pytest.fixture(scope="module")
def T(mq):
    t = int(mq.load_library().mqdiag_coverage_tile_bits())
    assert t % (64 * 128) == 0
    return t


@pytest.fixture(scope="module")
def cases(T, oracle, simlib):
    cs = CM.crafted_cases(T, mqx.source(oracle, simlib, "small"))
    return [(c, CM.model(c.slots, c.refs)) for c in cs]


def test_crafted_files(mq, cases, tmp_path):
    """Index.load -> coverage() is the model's, records, intervals and out_of_range; the same through load_sized at another table size and
    through clone_sized"""
    for j, (c, want) in enumerate(cases):
        path = c.write(tmp_path / ("c%d.mqx" % j))
        ix = mq.Index.load(path)
        _same(ix.coverage(), want, c.name)
        other = 4 * max(c.table_slots, 2)
        sized = mq.Index.load(path, table_slots=other)
        assert sized.stats()["table_slots"] == other
        _same(sized.coverage(), want, c.name + " (load_sized)")
        cl = ix.clone(0, table_slots=2 * mqx.pow2_above(max(c.slots.size, 1)))
        _same(cl.coverage(), want, c.name + " (clone_sized)")
        for x in (cl, sized, ix):
            x.close()


def _built(mq, simlib, refs):
    _, _, names = X.contigs(simlib)
    ix = mq.Index(mq.Params())
    for r in refs:
        ix.add_ref(r, names[r], X.contig(simlib, r))
    ix.finalize()
    return ix


def _model_of_file(ix, path):
    ix.save(str(path))
    _, _, refs, slots = mqx.read(str(path))
    return CM.model(slots, refs), refs, slots


def test_built_index_save_resize_extend(mq, simlib, tmp_path):
    first, second = list(range(X.SPLIT)), list(range(X.SPLIT, len(X.LENS)))
    ix = _built(mq, simlib, first)
    want, refs, _ = _model_of_file(ix, tmp_path / "a.mqx")
    got = ix.coverage()
    _same(got, want, "built")
    assert got[1].size > 3 and 0 < int(got[0]["covered_bases"].sum()) < sum(X.LENS[r] for r in first) and got[2] == 0
    _same(ix.coverage(), want, "a second call")
    ix.resize(table_slots=2 * ix.stats()["table_slots"])
    _same(ix.coverage(), want, "resized")
    # the second part repeats segments of the first (extend_data.PLANTS): bases of an old reference lose their cover
    _, _, names = X.contigs(simlib)
    ix.reopen()
    for r in second:
        ix.add_ref(r, names[r], X.contig(simlib, r))
    ix.finalize()
    want2, _, _ = _model_of_file(ix, tmp_path / "ab.mqx")
    got2 = ix.coverage()
    _same(got2, want2, "extended")
    old, new = got[0], got2[0][:len(first)]
    assert np.array_equal(old["ref_id"], new["ref_id"]) and (new["covered_bases"] <= old["covered_bases"]).all()
    assert (new["covered_bases"] < old["covered_bases"]).any() and (new["live_kminmers"] < old["live_kminmers"]).any()
    ix.close()


def test_merge_and_merge_file(mq, simlib, tmp_path):
    first, second = list(range(X.SPLIT)), list(range(X.SPLIT, len(X.LENS)))
    b = _built(mq, simlib, second)
    b.save(str(tmp_path / "b.mqx"))
    for route in ("merge", "merge_file"):
        a = _built(mq, simlib, first)
        if route == "merge":
            a.merge(b, id_base=0)
        else:
            a.merge_file(str(tmp_path / "b.mqx"), id_base=0)
        want, refs, _ = _model_of_file(a, tmp_path / (route + ".mqx"))
        assert [r[0] for r in refs] == first + second
        _same(a.coverage(), want, route)
        a.close()
    b.close()


def test_lifetime_and_state(mq, simlib):
    L = mq.load_library()
    _, _, names = X.contigs(simlib)
    ix = mq.Index(mq.Params())
    for r in range(X.SPLIT):
        ix.add_ref(r, names[r], X.contig(simlib, r))

    def raw(h):
        return L.mq_index_coverage(h, None, None, None, None, None)

    assert raw(ix.handle) == MQ_ESTATE and b"not finalized" in L.mq_last_error()
    ix.finalize()
    r = X.reads(simlib)
    n = 64
    bases, offs = r["bases"][:int(r["offsets"][n])], r["offsets"][:n + 1]
    ctx = ix.context()
    before = ctx.map_batch(bases, offs).copy()
    ctx.submit(bases, offs)
    assert raw(ix.handle) == MQ_ESTATE and b"submitted batch" in L.mq_last_error()
    assert L.mqdiag_coverage_held(ix.handle) == 0
    ctx.wait()
    one = ix.coverage()
    assert L.mqdiag_coverage_held(ix.handle) > 0
    _same(ix.coverage(), one, "two calls in a row")
    assert np.array_equal(ctx.map_batch(bases, offs).view(np.uint8), before.view(np.uint8)), "contexts map the same hits behind a coverage() call"
    assert (before["status"] == 1).sum() > n // 4  # (the index holds 129 of the 236 kb the reads come from: 35 of 64 expected)
    ix.coverage_release()
    assert L.mqdiag_coverage_held(ix.handle) == 0
    other = mq.Index(mq.Params())
    other.add_ref(0, names[X.SPLIT], X.contig(simlib, X.SPLIT))
    other.finalize()
    for change in (lambda: ix.resize(table_slots=2 * ix.stats()["table_slots"]), lambda: ix.merge(other, id_base=7), lambda: (ix.reopen(), ix.finalize())):
        ix.coverage()
        assert L.mqdiag_coverage_held(ix.handle) > 0
        change()
        assert L.mqdiag_coverage_held(ix.handle) == 0
    assert [int(x) for x in ix.coverage()[0]["ref_id"]] == [0, 1, 2, 7]
    ctx.close()
    other.close()
    ix.close()


def _fasta(simlib, path, refs):
    _, _, names = X.contigs(simlib)
    with open(path, "wb") as f:
        for r in refs:
            f.write(b">" + names[r].encode() + b"\n" + X.contig(simlib, r).tobytes() + b"\n")
    return str(path)


def test_drivers(mq, simlib, cases, tmp_path):
    """--coverage of both drivers on a crafted index and on a built one: the two files are the model's bytes from either driver, and the
    PAF is the same bytes as without the flag"""
    from mapquik_amd import build
    env = dict(os.environ, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    drivers = {"native": [build.build_cli()], "python": [sys.executable, "-m", "mapquik_amd"]}
    r = X.reads(simlib)
    rd = tmp_path / "reads.fa"
    with open(rd, "wb") as f:
        for i in range(40):
            f.write(b">r%d\n" % i + r["bases"][int(r["offsets"][i]):int(r["offsets"][i + 1])].tobytes() + b"\n")
    t = lambda n: str(tmp_path / n)  # noqa: E731
    fa = _fasta(simlib, tmp_path / "ref.fa", [0, 1, 2, 3])
    crafted = next(c for c, _ in cases if c.name == "no run across references")
    crafted.write(t("crafted.mqx"))
    seeding = {"built": [], "crafted": ["-k", "3", "-l", "12", "-d", "0.05"]}
    source = {"built": ["--reference", fa, "--save-index", t("built.mqx")], "crafted": ["--index", t("crafted.mqx")]}
    out = {}
    for kind in ("built", "crafted"):
        for d, cmd in drivers.items():
            for flag in ([], ["--coverage"]):
                p = "%s_%s_%d" % (kind, d, len(flag))
                res = subprocess.run(cmd + [str(rd)] + seeding[kind] + source[kind] + ["-p", t(p)] + flag, capture_output=True, text=True, timeout=300, env=env)
                assert res.returncode == 0, (kind, d, flag, res.stderr[-2000:])
                out[(kind, d, len(flag))] = (open(t(p + ".paf"), "rb").read(), res.stdout)
                assert os.path.exists(t(p + ".coverage.bed")) == bool(flag) == os.path.exists(t(p + ".coverage.tsv"))
        _, _, refs, slots = mqx.read(t(kind + ".mqx"))
        recs, ivs, oor = CM.model(slots, refs)
        line = "Coverage: %d of %d bases in %d intervals (%d entries out of range)" % (int(recs["covered_bases"].sum()), int(recs["len"].sum()), ivs.size, oor)
        for d in drivers:
            assert out[(kind, d, 1)][0] == out[(kind, d, 0)][0], (kind, d, "the PAF changes with --coverage")
            assert line in out[(kind, d, 1)][1] and "Coverage:" not in out[(kind, d, 0)][1], (kind, d, out[(kind, d, 1)][1])
            p = "%s_%s_1" % (kind, d)
            assert open(t(p + ".coverage.bed"), "rb").read() == CM.bed_bytes(refs, recs, ivs), (kind, d)
            assert open(t(p + ".coverage.tsv"), "rb").read() == CM.tsv_bytes(refs, recs), (kind, d)
        if kind == "built":
            assert len(out[(kind, "native", 0)][0]) > 1000 and ivs.size > 3
