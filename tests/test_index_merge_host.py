"""Index merge, the parts that need no GPU: the two prototypes in the header, in INTEGRATION.md and in api.EXPORTS under an unchanged
MQ_ABI_VERSION; the dict model of tests/merge_data.py (the GPU test's expectation for crafted files) held against the probe-order model of
tests/mqx.py and against the oracle's Index.add on the contigs the GPU test uses; the native driver's --merge-index -- parsing, order,
id_base of each call, error exits -- in the stand-alone `mapquik_asan` / `mapquik_tsan` of `make asan tsan` over the host-only stub
tests/cpp/stub_mapquik_hip_merge.cc (nothing is loaded into Python); the Python driver's usage error.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import extend_data as X
import merge_data as M
import mqx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
NEW = ("mq_index_merge", "mq_index_merge_file")
USAGE = "--merge-index merges into the index given with --index or built from --reference"
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1", MQ_STUB_MERGE_LOG="1")


def test_prototypes_in_header_and_integration_md():
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define MQ_ABI_VERSION 4\b", hdr)
    assert re.search(r"int mq_index_merge\(mq_index \*dst, const mq_index \*src, uint32_t id_base\);", hdr)
    assert re.search(r"int mq_index_merge_file\(mq_index \*dst, const char \*path, uint32_t id_base\);", hdr)
    assert "the same key in two slots of the file" in hdr  # the one corruption a merge cannot see
    assert re.search(r"pub fn mq_index_merge\(dst: \*mut MqIndex, src: \*const MqIndex, id_base: u32\) -> c_int;", integ)
    assert re.search(r"pub fn mq_index_merge_file\(dst: \*mut MqIndex, path: \*const c_char, id_base: u32\) -> c_int;", integ)
    from mapquik_amd import api
    assert api.MQ_ABI_VERSION == 4 and all(n in api.EXPORTS for n in NEW)
    assert callable(api.Index.merge) and callable(api.Index.merge_file)


def test_library_exports_the_entry_points():
    import mapquik_amd
    out = subprocess.run(["nm", "-D", "--defined-only", mapquik_amd.build.LIB], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) <= exported
    L = mapquik_amd.load_library()
    assert L.mq_abi_version() == 4 and all(hasattr(L, n) for n in NEW)


# ------------------------------------------------------------------ the model
def _table_of(model, table_slots):
    """the model's keys placed by mqx's probe order; every key is found by its walk, an absent key is not"""
    keys = [k for k in model.d]
    at = M.place(keys, table_slots)
    assert all(M.walk_finds(at, k, table_slots) for k in keys)
    return at


def test_model_on_crafted_cases():
    """Every crafted pair of the GPU test through the dict model: the counts a merge must report (claimed, born dead, turned dead) add up
    to the merged header, the merged key set fits the destination's table with an empty slot left (exactly one in the first case),
    every key is found along its probe walk in a table built in EITHER order (destination first, as a merge does; all at once, as a
    build does), and the source key of `behind the wrap` lies in bucket 0 or later although its home is the last bucket."""
    names = []
    for name, dst, src, id_base, declared in M.crafted_cases():
        names.append(name)
        hd, hs = dst.header(), src.header()
        model = M.Model(dst.slots())
        before = (model.n_keys(), model.n_unique())
        assert before == (hd["n_keys"], hd["n_unique"]), name
        claimed, born_dead, turned_dead = model.merge(src.slots(), id_base)
        assert model.n_keys() == before[0] + claimed and model.n_unique() == before[1] + claimed - born_dead - turned_dead, name
        assert model.n_kminmers == hd["n_kminmers"] + hs["n_kminmers"]
        # against mqx.header_counts on the concatenated slot arrays (the same rule, written there for a file)
        both = np.concatenate([dst.slots(), src.slots()])
        assert (model.n_kminmers, model.n_keys(), model.n_unique()) == mqx.header_counts(both), name
        ts = dst.table_slots
        assert model.n_keys() < ts, name
        dkeys, skeys = [int(k) for k in dst.entries["key"]], [int(k) for k in src.entries["key"] if int(k) not in set(int(x) for x in dst.entries["key"])]
        merged_order = M.place(dkeys + skeys, ts)
        _table_of(model, ts)
        assert all(M.walk_finds(merged_order, k, ts) for k in model.d), name
        absent = [int(k) for k in np.random.default_rng(5).integers(1, 2**64, size=300, dtype=np.uint64) if int(k) not in model.d]
        assert not any(M.walk_finds(merged_order, k, ts) for k in absent), name
        moved = {(int(s["id_rc"]) >> 1) + id_base for s in src.slots()}
        assert max(moved) < mqx.MAX_REF_ID and not moved & {r[0] for r in dst.refs}, name
        if name == "one empty slot":
            assert model.n_keys() == ts - 1 and declared is not None and 8 * sum(declared) <= ts
        if name == "behind the wrap":
            where = {k: s for s, k in merged_order.items()}
            for k in skeys:
                assert (k & (ts - 1)) >> 1 == ts // 2 - 1 and where[k] < ts - 2, (name, hex(k), where[k])
        if name == "sparse ids":
            assert max(moved) == mqx.MAX_REF_ID - 1
    assert {"key 0 in the source only", "key 0 live in both", "key 0 dead in the source", "count 7", "end 0", "2-slot source", "4-slot source"} <= set(names)
    # the three kinds of key-0 case do what their names say
    for name, dst, src, id_base, _ in M.crafted_cases():
        if name.startswith("key 0"):
            m = M.Model(dst.slots())
            was = m.live(0)
            m.merge(src.slots(), id_base)
            assert (was, m.live(0)) == {"key 0 in the source only": (False, True), "key 0 live in both": (True, False), "key 0 dead in the source": (True, False)}[name]


def test_model_against_the_oracle(oracle, simlib):
    """merge(A, B) and the two orders of merging A, B, C by the model = the oracle's map of everything: the same keys, the same live set
    with the same payloads.  Each of the three classes of key occurs (live in both, dead in A, dead in B), and a key once in each of
    A, B, C."""
    po = oracle.params(k=3, l=9, density=0.15)
    parts = {n: X.slot_set(M.insertions(oracle, simlib, ids, po)) for n, ids in (("A", M.A_IDS), ("B", M.B_IDS), ("C", M.C_IDS))}
    twice_a, twice_b, once_each, once = X.kinds(parts["A"], parts["B"])
    print("keys dead in A, dead in B, live in both, once in all:", (twice_a, twice_b, once_each, once))
    assert twice_a > 0 and twice_b > 0 and once_each > 0 and once > 0
    assert set(parts["A"]["key"].tolist()) & set(parts["B"]["key"].tolist()) & set(parts["C"]["key"].tolist())
    _, _, names = M.contigs(simlib)
    ox = oracle.Index()
    for r in range(len(M.LENS)):
        ox.add_ref(r, names[r], M.contig(simlib, r, upper=True), po)
    whole = M.sorted_slots(X.slot_set(M.insertions(oracle, simlib, range(len(M.LENS)), po)))
    left = M.Model(parts["A"])
    left.merge(parts["B"], 0)
    left.merge(parts["C"], 0)
    bc = M.Model(parts["B"])
    bc.merge(parts["C"], 0)
    right = M.Model(parts["A"])
    right.merge(bc.slots(), 0)
    for m in (left, right):
        assert M.sorted_slots(m.slots()).tobytes() == whole.tobytes()
        assert m.n_unique() == ox.count() and m.n_keys() == ox.keys()
    for k in list(left.d)[::5]:
        e = ox.get(k)
        assert (e is not None) == left.live(k)
        if e is not None:
            assert [int(e["start"]), int(e["end"]), int(e["offset"]), (int(e["id"]) << 1) | int(e["rc"])] == left.d[k][:4]
    # ids moved: B built under ids 0, 1 and merged behind A's three
    b01 = X.slot_set(M.insertions(oracle, simlib, M.B_IDS, po, ids=[0, 1]))
    ab = M.Model(parts["A"])
    ab.merge(b01, 3)
    want = M.Model(parts["A"])
    want.merge(parts["B"], 0)
    assert M.sorted_slots(ab.slots()).tobytes() == M.sorted_slots(want.slots()).tobytes()


# ------------------------------------------------------------------ the native driver over the stub
@pytest.fixture(scope="module")
def exes():
    r = subprocess.run(["make", "-C", ROOT, "asan", "tsan"], capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        pytest.fail("make asan tsan failed:\n" + r.stderr[-2000:])
    return dict(asan=os.path.join(LIB, "mapquik_asan"), tsan=os.path.join(LIB, "mapquik_tsan"))


def _run(exe, args):
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=_ENV)


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_driver_flag_over_the_stub(exes, tmp_path, san):
    """--reference + two --merge-index: the stub is called once per file, in command-line order, after the reference was indexed, each
    with the id behind every id the index has by then; the log names each file; the run maps.  A file that is no index ends the run
    with the library's text (exit 101) and no PAF.  --merge-index without --index / --reference is a usage error (exit 2), with
    --index it gets as far as the stub's refusal to load; --index --save-index alone stays the usage error it was."""
    exe = exes[san]
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rd, fa = tmp_path / "reads.fa", tmp_path / "ref.fa"
    rd.write_bytes(b"".join(b">r%d\n" % i + acgt[rng.integers(0, 4, 400)].tobytes() + b"\n" for i in range(50)))
    fa.write_bytes(b">one\n" + acgt[rng.integers(0, 4, 5000)].tobytes() + b"\n>two\n" + acgt[rng.integers(0, 4, 3000)].tobytes() + b"\n")
    b, c, junk = tmp_path / "b.mqx", tmp_path / "c.mqx", tmp_path / "junk.mqx"
    for f in (b, c):
        f.write_bytes(b"MQHIPIX2" + b"\0" * 88)
    junk.write_bytes(b"not an index")
    p = str(tmp_path / "x")
    r = _run(exe, [str(rd), "--reference", str(fa), "--merge-index", str(c), "--merge-index", str(b), "-p", p])
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    calls = [ln for ln in r.stderr.splitlines() if ln.startswith("stub: mq_index_merge_file")]
    assert calls == ["stub: mq_index_merge_file c.mqx id_base 2", "stub: mq_index_merge_file b.mqx id_base 3"], r.stderr[-2000:]
    out = r.stdout
    assert "Merged index %s: 1 references" % c in out and "Merged index %s: 1 references" % b in out
    assert out.index("Indexed reference two") < out.index(str(c)) < out.index(str(b)) < out.index("unique k-min-mers in")
    assert (tmp_path / "x.paf").read_bytes().count(b"\n") == 50
    r = _run(exe, [str(rd), "--reference", str(fa), "--merge-index", str(b), "--merge-index", str(junk), "-p", str(tmp_path / "y")])
    assert r.returncode == 101 and "ReadOnlyIndex::merge_file: stub (mq_index_merge_file): not an index: %s" % junk in r.stderr, (r.returncode, r.stderr[-2000:])
    r = _run(exe, [str(rd), "--merge-index", str(b), "-p", p])
    assert r.returncode == 2 and USAGE in r.stderr, (r.returncode, r.stderr)
    r = _run(exe, [str(rd), "--merge-index"])
    assert r.returncode == 2 and "needs a value" in r.stderr
    r = _run(exe, [str(rd), "--index", str(b), "--merge-index", str(c), "--save-index", str(tmp_path / "bc.mqx"), "-p", p])
    assert r.returncode == 101 and "ReadOnlyIndex::load: stub" in r.stderr, (r.returncode, r.stderr)  # past the usage checks: --save-index is legal beside --merge-index
    r = _run(exe, [str(rd), "--index", str(b), "--save-index", str(tmp_path / "bc.mqx"), "-p", p])
    assert r.returncode == 2, (r.returncode, r.stderr)
    r = _run(exe, ["--help"])
    assert r.returncode == 0 and "--merge-index" in r.stdout


def test_python_driver_usage_error(capsys):
    from mapquik_amd import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["reads.fa", "-p", "x", "--merge-index", "b.mqx"])
    err = capsys.readouterr().err
    assert ei.value.code == 2 and USAGE in err and "unrecognized arguments" not in err, err
    opt = cli.build_parser().parse_args(["reads.fa", "--index", "a.mqx", "--merge-index", "b.mqx", "--merge-index", "c.mqx"])
    assert opt.merge_index == ["b.mqx", "c.mqx"]  # repeatable, in command-line order
