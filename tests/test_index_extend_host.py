"""Reopen / resize / sized load and clone, the parts that need no GPU: the four prototypes in the header and in INTEGRATION.md under
an unchanged MQ_ABI_VERSION; the native driver's new flags in the stand-alone `mapquik_asan` of `make asan` (ASan + UBSan over the
host-only stub tests/cpp/stub_mapquik_hip_extend.cc; nothing is loaded into Python); and the pure-Python model of "extend" (the union of
two slot sets with counts capped at 2, tests/extend_data.py) held against the oracle's Index.add on the contigs the GPU test uses --
the GPU test's expectation, made without the library.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import extend_data as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
NEW = ("mq_index_reopen", "mq_index_resize", "mq_index_load_sized", "mq_index_clone_sized")
USAGE = "--add-reference adds to the index given with --index"
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")


def test_prototypes_in_header_and_integration_md():
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define MQ_ABI_VERSION 4\b", hdr)
    protos = {
        "mq_index_reopen": r"int\s+mq_index_reopen\(mq_index \*idx\);",
        "mq_index_resize": r"int\s+mq_index_resize\(mq_index \*idx, uint64_t table_slots, uint32_t slots_per_kminmer\);",
        "mq_index_load_sized": r"mq_index \*mq_index_load_sized\(const char \*path, int device, uint64_t table_slots, uint32_t slots_per_kminmer\);",
        "mq_index_clone_sized": r"mq_index \*mq_index_clone_sized\(const mq_index \*src, int device, uint64_t table_slots, uint32_t slots_per_kminmer\);",
    }
    for name in NEW:
        assert re.search(protos[name], hdr), name
        assert re.search(r"pub fn %s\(" % name, integ), name
    from mapquik_amd import api
    assert api.MQ_ABI_VERSION == 4 and all(n in api.EXPORTS for n in NEW)


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-C", ROOT, "asan"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("make asan failed:\n" + r.stderr[-2000:])
    return os.path.join(LIB, "mapquik_asan")


def _run(exe, args):
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=_ENV)


def test_driver_flags_over_the_stub(exe, tmp_path):
    """The new flags parse; the runs end where the stub refuses to load an index file (exit 101, the stub's text) -- with --table-factor
    through mq_index_load_sized, without it through mq_index_load.  --add-reference without --index, or beside --reference, is a usage
    error (exit 2) before anything runs."""
    rd, fa, ixf = tmp_path / "reads.fa", tmp_path / "b.fa", tmp_path / "a.mqx"
    rd.write_text(">r\nACGTACGTACGT\n")
    fa.write_text(">b\nACGTTGCAACGTTGCA\n")
    ixf.write_bytes(b"")
    p = str(tmp_path / "x")
    r = _run(exe, [str(rd), "--index", str(ixf), "--add-reference", str(fa), "--save-index", str(tmp_path / "ab.mqx"), "-p", p])
    assert r.returncode == 101 and "ReadOnlyIndex::load: stub" in r.stderr and "load_sized" not in r.stderr, (r.returncode, r.stderr)
    r = _run(exe, [str(rd), "--index", str(ixf), "--table-factor", "2", "-p", p])
    assert r.returncode == 101 and "stub (mq_index_load_sized)" in r.stderr, (r.returncode, r.stderr)
    r = _run(exe, [str(rd), "--index", str(ixf), "-p", p])
    assert r.returncode == 101 and "ReadOnlyIndex::load: stub" in r.stderr and "load_sized" not in r.stderr, (r.returncode, r.stderr)
    r = _run(exe, [str(rd), "--add-reference", str(fa), "-p", p])
    assert r.returncode == 2 and USAGE in r.stderr, (r.returncode, r.stderr)
    r = _run(exe, [str(rd), "--reference", str(fa), "--add-reference", str(fa), "-p", p])
    assert r.returncode == 2 and USAGE in r.stderr, (r.returncode, r.stderr)
    r = _run(exe, [str(rd), "--index", str(ixf), "--save-index", str(tmp_path / "c.mqx"), "-p", p])
    assert r.returncode == 2, (r.returncode, r.stderr)  # as before: nothing to save without --add-reference
    r = _run(exe, ["--help"])
    assert r.returncode == 0 and "--add-reference" in r.stdout


@pytest.mark.parametrize("args", [["--add-reference", "b.fa"], ["--reference", "a.fa", "--add-reference", "b.fa"]])
def test_python_driver_usage_error(capsys, args):
    """exit 2 with the driver's own text: the flag is known to the parser, and refused without --index or beside --reference"""
    from mapquik_amd import cli
    with pytest.raises(SystemExit) as ei:
        cli.main(["reads.fa", "-p", "x"] + args)
    err = capsys.readouterr().err
    assert ei.value.code == 2 and USAGE in err and "unrecognized arguments" not in err, err


def test_extend_model_against_the_oracle(oracle, simlib):
    """At every split point the model of "A, then B added" is the oracle's map of everything: the same keys, the same live set with the
    same payloads.  At the split 3 | 3 each of the four kinds of key occurs."""
    n = len(X.LENS)
    whole = X.slot_set(X.insertions(oracle, simlib, range(n)))
    ox = oracle.Index()
    po = oracle.params()
    for r in range(n):
        ox.add_ref(r, "c%d" % r, X.contig(simlib, r), po)
    live = (whole["count"] == 1) & (whole["end"] != 0)
    assert int(live.sum()) == ox.count() and whole.size == ox.keys()
    for i in np.flatnonzero(live)[::7]:
        e = ox.get(int(whole["key"][i]))
        assert e is not None, i
        assert (int(e["id"]) << 1 | int(e["rc"]), int(e["start"]), int(e["end"]), int(e["offset"])) == tuple(int(whole[f][i]) for f in ("id_rc", "start", "end", "offset"))
    for i in np.flatnonzero(~live)[::3]:
        assert ox.get(int(whole["key"][i])) is None
    for split in range(n + 1):
        a = X.slot_set(X.insertions(oracle, simlib, range(split)))
        b = X.slot_set(X.insertions(oracle, simlib, range(split, n)))
        m = X.extend_model(a, b)
        assert X.sorted_slots(m).tobytes() == X.sorted_slots(whole).tobytes(), split
        if split == X.SPLIT:
            k = X.kinds(a, b)
            print("keys twice in A, twice in B, once in each, once in all:", k)
            assert all(x > 0 for x in k), k
