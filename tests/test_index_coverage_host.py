"""CPU: the boundary of the index coverage -- prototypes in the header, in INTEGRATION.md, in api.EXPORTS and in the library's dynamic
symbols; the record sizes; the native driver's --coverage over the host-only stub in the stand-alone sanitizer builds (nothing is loaded
into Python); the Python driver's parser and the two formatters on canned arrays.  Every test here needs the new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
NEW = ("mq_index_coverage", "mq_index_coverage_release")
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1", MQ_STUB_MERGE_LOG="1", MQ_STUB_COVERAGE_LOG="1")
TSV_HEAD = "#ref\tlen\tlive_kminmers\tcovered\tfraction\tintervals\n"


def test_prototypes_in_header_integration_md_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "mapquik_hip_diag.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define MQ_ABI_VERSION 4\b", hdr)
    assert re.search(r"int mq_index_coverage\(mq_index \*idx, const mq_ref_coverage \*\*refs, uint64_t \*n_refs,\s*const mq_cov_interval \*\*intervals, "
                     r"uint64_t \*n_intervals, uint64_t \*out_of_range\);", hdr)
    assert re.search(r"int mq_index_coverage_release\(mq_index \*idx\);", hdr)
    assert re.search(r"uint32_t ref_id, reserved;\s*uint64_t len, live_kminmers, covered_bases, n_intervals, first_interval;", hdr)
    assert re.search(r"typedef struct mq_cov_interval \{ uint32_t start, end; \} mq_cov_interval;", hdr)
    assert re.search(r"uint64_t mqdiag_coverage_tile_bits\(void\);", diag)
    assert re.search(r"pub fn mq_index_coverage\(i: \*mut MqIndex, refs: \*mut \*const MqRefCoverage, n_refs: \*mut u64, intervals: \*mut \*const MqCovInterval, "
                     r"n_intervals: \*mut u64, out_of_range: \*mut u64\) -> c_int;", integ)
    assert re.search(r"pub fn mq_index_coverage_release\(i: \*mut MqIndex\) -> c_int;", integ)
    from mapquik_amd import api
    assert api.MQ_ABI_VERSION == 4 and all(n in api.EXPORTS for n in NEW)
    assert api.ref_coverage_dtype.itemsize == 48 and api.cov_interval_dtype.itemsize == 8
    assert callable(api.Index.coverage) and callable(api.Index.coverage_release)


def test_library_exports_the_entry_points():
    import mapquik_amd
    out = subprocess.run(["nm", "-D", "--defined-only", mapquik_amd.build.LIB], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) | {"mqdiag_coverage_tile_bits"} <= exported
    L = mapquik_amd.load_library()
    assert L.mq_abi_version() == 4 and all(hasattr(L, n) for n in NEW)
    t = int(L.mqdiag_coverage_tile_bits())
    assert t > 0 and t % (64 * 128) == 0  # whole steps of a wave: 64 lanes, two words each


# ------------------------------------------------------------------ the native driver over the stub
@pytest.fixture(scope="module")
def exes():
    r = subprocess.run(["make", "-C", ROOT, "asan", "tsan"], capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        pytest.fail("make asan tsan failed:\n" + r.stderr[-2000:])
    return dict(asan=os.path.join(LIB, "mapquik_asan"), tsan=os.path.join(LIB, "mapquik_tsan"))


def _run(exe, args, **env):
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=dict(_ENV, **env))


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_driver_flag_over_the_stub(exes, tmp_path, san):
    """--reference + two --merge-index + --coverage: the stub is called once, behind the last merge (it sees all four references) and before
    mapping; both files hold the stub's canned coverage in the stated formats; the PAF is the one without the flag; the stub's failure
    ends the run with exit 101 and no PAF; --help names the flag."""
    exe = exes[san]
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rd, fa = tmp_path / "reads.fa", tmp_path / "ref.fa"
    rd.write_bytes(b"".join(b">r%d\n" % i + acgt[rng.integers(0, 4, 400)].tobytes() + b"\n" for i in range(50)))
    fa.write_bytes(b">one\n" + acgt[rng.integers(0, 4, 5000)].tobytes() + b"\n>two\n" + acgt[rng.integers(0, 4, 3001)].tobytes() + b"\n")
    b, c = tmp_path / "b.mqx", tmp_path / "c.mqx"
    for f in (b, c):
        f.write_bytes(b"MQHIPIX2" + b"\0" * 88)
    base = [str(rd), "--reference", str(fa), "--merge-index", str(c), "--merge-index", str(b)]
    r0 = _run(exe, base + ["-p", str(tmp_path / "w")])
    assert r0.returncode == 0 and "stub: mq_index_coverage" not in r0.stderr and "Coverage:" not in r0.stdout
    assert not (tmp_path / "w.coverage.bed").exists()
    r = _run(exe, base + ["--coverage", "-p", str(tmp_path / "x")])
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    calls = [ln for ln in r.stderr.splitlines() if ln.startswith("stub: ")]
    assert calls == ["stub: mq_index_merge_file c.mqx id_base 2", "stub: mq_index_merge_file b.mqx id_base 3", "stub: mq_index_coverage 4 references"], r.stderr[-2000:]
    out = r.stdout
    assert "Coverage: 7501 of 10001 bases in 8 intervals (0 entries out of range)\n" in out
    assert out.index("Merged index %s" % b) < out.index("Coverage:") < out.index("unique k-min-mers in") < out.index("Mapped query sequences")
    assert (tmp_path / "x.coverage.bed").read_text() == "one\t0\t1250\none\t2500\t5000\ntwo\t0\t750\ntwo\t1500\t3001\nc.mqx\t0\t250\nc.mqx\t500\t1000\nb.mqx\t0\t250\nb.mqx\t500\t1000\n"
    assert (tmp_path / "x.coverage.tsv").read_text() == TSV_HEAD + ("one\t5000\t10\t3750\t0.750000\t2\ntwo\t3001\t10\t2251\t0.750083\t2\n"
                                                                   "c.mqx\t1000\t10\t750\t0.750000\t2\nb.mqx\t1000\t10\t750\t0.750000\t2\n")
    assert (tmp_path / "x.paf").read_bytes() == (tmp_path / "w.paf").read_bytes() and (tmp_path / "x.paf").read_bytes().count(b"\n") == 50
    r = _run(exe, base + ["--coverage", "-p", str(tmp_path / "y")], MQ_STUB_COVERAGE_FAIL="1")
    assert r.returncode == 101 and "ReadOnlyIndex::coverage: stub (mq_index_coverage): no device memory" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not (tmp_path / "y.paf").exists() and not (tmp_path / "y.coverage.bed").exists()
    r = _run(exe, ["--help"])
    assert r.returncode == 0 and "--coverage" in r.stdout


# ------------------------------------------------------------------ the Python driver
class _Names:
    def ref_info(self, rid):
        return {0: ("chr1", 1000), 7: ("", 3), 9: ("decoy", 64)}[rid]


def test_python_driver_parser_and_formatters():
    from mapquik_amd import api, cli
    opt = cli.build_parser().parse_args(["reads.fa", "--index", "a.mqx", "--merge-index", "b.mqx", "--coverage"])
    assert opt.coverage is True and cli.build_parser().parse_args(["reads.fa"]).coverage is False
    assert "--coverage" in cli.build_parser().format_help()
    refs = np.array([(0, 0, 1000, 12, 333, 2, 0), (7, 0, 3, 0, 0, 0, 2), (9, 0, 64, 1, 64, 1, 2)], dtype=api.ref_coverage_dtype)
    ivs = np.array([(0, 300), (967, 1000), (0, 64)], dtype=api.cov_interval_dtype)
    assert api.format_coverage_bed(_Names(), refs, ivs) == b"chr1\t0\t300\nchr1\t967\t1000\ndecoy\t0\t64\n"
    assert api.format_coverage_tsv(_Names(), refs) == TSV_HEAD.encode() + b"chr1\t1000\t12\t333\t0.333000\t2\n\t3\t0\t0\t0.000000\t0\ndecoy\t64\t1\t64\t1.000000\t1\n"
    assert api.format_coverage_bed(_Names(), refs[:0], ivs[:0]) == b"" and api.format_coverage_tsv(_Names(), refs[:0]) == TSV_HEAD.encode()
    # the same bytes as the model's writer (the GPU test holds the drivers' files against it)
    import coverage_model as CM
    names = [(0, "chr1", 1000), (7, "", 3), (9, "decoy", 64)]
    assert CM.bed_bytes(names, refs, ivs) == api.format_coverage_bed(_Names(), refs, ivs) and CM.tsv_bytes(names, refs) == api.format_coverage_tsv(_Names(), refs)
