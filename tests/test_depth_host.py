"""CPU: the boundary of the depth accumulator -- prototypes in the header, in INTEGRATION.md, in api.EXPORTS and in the library's dynamic
symbols; the record sizes; the native driver's --depth over the host-only stub in the stand-alone sanitizer builds (nothing is loaded
into Python); the Python driver's parser and the two formatters on canned arrays.  Every test here needs the new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import depth_model as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
NEW = ("mq_depth_new", "mq_depth_free", "mq_depth_clear", "mq_depth_add", "mq_depth_add_device", "mq_depth_result")
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1", MQ_STUB_DEPTH_LOG="1")


def test_prototypes_in_header_integration_md_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "mapquik_hip_diag.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define MQ_ABI_VERSION 4\b", hdr)
    for proto in (r"int mq_depth_new\(mq_index \*idx, uint32_t window, uint32_t min_mapq, mq_depth \*\*out\);", r"void mq_depth_free\(mq_depth \*d\);",
                  r"int mq_depth_clear\(mq_depth \*d\);", r"int mq_depth_add\(mq_depth \*d, const mq_hit \*hits, uint32_t n\);",
                  r"int mq_depth_add_device\(mq_depth \*d, const mq_hit \*d_hits, uint32_t n, void \*stream\);",
                  r"int mq_depth_result\(mq_depth \*d, const mq_ref_depth \*\*refs, uint64_t \*n_refs, const uint64_t \*\*window_bases,\s*const uint32_t \*\*window_starts, "
                  r"uint64_t \*n_windows, mq_depth_totals \*totals\);"):
        assert re.search(proto, hdr), proto
    assert re.search(r"uint32_t ref_id, reserved;\s*uint64_t len, n_windows, first_window, reads, bases, zero_windows, max_window_bases;", hdr)
    assert re.search(r"uint64_t offered, counted, not_mapped, below_mapq, out_of_range;", hdr)
    assert re.search(r"uint64_t mqdiag_depth_tile_windows\(void\);", diag)
    for proto in (r"pub fn mq_depth_new\(i: \*mut MqIndex, window: u32, min_mapq: u32, out: \*mut \*mut MqDepth\) -> c_int;", r"pub fn mq_depth_free\(d: \*mut MqDepth\);",
                  r"pub fn mq_depth_clear\(d: \*mut MqDepth\) -> c_int;", r"pub fn mq_depth_add\(d: \*mut MqDepth, hits: \*const MqHit, n: u32\) -> c_int;",
                  r"pub fn mq_depth_add_device\(d: \*mut MqDepth, d_hits: \*const MqHit, n: u32, stream: \*mut c_void\) -> c_int;",
                  r"pub fn mq_depth_result\(d: \*mut MqDepth, refs: \*mut \*const MqRefDepth, n_refs: \*mut u64, window_bases: \*mut \*const u64, "
                  r"window_starts: \*mut \*const u32, n_windows: \*mut u64, totals: \*mut MqDepthTotals\) -> c_int;",
                  r"pub struct MqRefDepth \{", r"pub struct MqDepthTotals \{", r"pub struct MqDepth \{ _private"):
        assert re.search(proto, integ), proto
    from mapquik_amd import api
    assert api.MQ_ABI_VERSION == 4 and all(n in api.EXPORTS for n in NEW)
    assert api.ref_depth_dtype.itemsize == 64 and api.depth_totals_dtype.itemsize == 40
    assert api.ref_depth_dtype.names == DM.ref_depth_dtype.names and api.depth_totals_dtype.names == DM.TOTALS
    assert all(callable(getattr(api.Depth, m)) for m in ("add", "add_device", "result", "clear", "close"))


def test_library_exports_the_entry_points():
    import mapquik_amd
    out = subprocess.run(["nm", "-D", "--defined-only", mapquik_amd.build.LIB], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) | {"mqdiag_depth_tile_windows", "mqdiag_depth_result_ms"} <= exported
    L = mapquik_amd.load_library()
    assert L.mq_abi_version() == 4 and all(hasattr(L, n) for n in NEW)
    t = int(L.mqdiag_depth_tile_windows())
    assert t > 0 and t % 64 == 0  # whole steps of a wave: a window per lane


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
    """--depth over the stub, whose accumulator is the rules spelled out on the host: one accumulator, made behind the index phase; one
    mq_depth_add per chunk with that chunk's hits (several chunks, two fake GPUs); one result; both files are the formatters' bytes for
    the model of the PAF the same run wrote; the PAF is the one without the flag; a failing add ends the run with exit 101 and no PAF;
    --help names the flags."""
    exe = exes[san]
    rng = np.random.default_rng(4)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rd, fa = tmp_path / "reads.fa", tmp_path / "ref.fa"
    lens = [int(x) for x in rng.integers(30, 900, 120)]  # (the stub leaves a read below 50 bases unmapped)
    rd.write_bytes(b"".join(b">r%d\n" % i + acgt[rng.integers(0, 4, n)].tobytes() + b"\n" for i, n in enumerate(lens)))
    fa.write_bytes(b">one\n" + acgt[rng.integers(0, 4, 5000)].tobytes() + b"\n>two\n" + acgt[rng.integers(0, 4, 3001)].tobytes() + b"\n")
    refs = [(0, "one", 5000), (1, "two", 3001)]
    base = [str(rd), "--reference", str(fa), "--batch-bases", "8000", "--gpus", "2"]
    r0 = _run(exe, base + ["-p", str(tmp_path / "w")], MQ_FAKE_MULTI="1")
    assert r0.returncode == 0 and "stub: mq_depth" not in r0.stderr and "Depth:" not in r0.stdout, r0.stderr[-2000:]
    assert not (tmp_path / "w.depth.bed").exists()
    for flags, w, q in ((["--depth"], 1000, 60), (["--depth", "--depth-window", "333", "--depth-min-mapq", "0"], 333, 0)):
        p = "x%d" % w
        r = _run(exe, base + flags + ["-p", str(tmp_path / p)], MQ_FAKE_MULTI="1")
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        calls = [ln for ln in r.stderr.splitlines() if ln.startswith("stub: mq_depth")]
        assert calls[0] == "stub: mq_depth_new window %d min_mapq %d, 2 references" % (w, q) and calls[-1] == "stub: mq_depth_result 120 offered", calls
        adds = [tuple(int(x) for x in re.findall(r"\d+", ln)) for ln in calls[1:-1]]
        assert all(ln.startswith("stub: mq_depth_add ") for ln in calls[1:-1]) and len(adds) >= 4, calls
        paf = (tmp_path / (p + ".paf")).read_text()
        assert sum(a for a, _ in adds) == 120 and sum(m for _, m in adds) == paf.count("\n") == sum(1 for n in lens if n >= 50)
        assert paf == (tmp_path / "w.paf").read_text()
        recs, wb, ws, tot = DM.model(refs, DM.hits_of_paf(paf, refs), w, q)
        tot = dict(tot, offered=120, not_mapped=120 - paf.count("\n"))
        assert DM.log_line(recs, tot, w, q) + "\n" in r.stdout, r.stdout
        assert r.stdout.index("unique k-min-mers in") < r.stdout.index("Depth:") < r.stdout.index("Mapped query sequences")
        assert (tmp_path / (p + ".depth.bed")).read_bytes() == DM.bed_bytes(refs, recs, wb, ws, w)
        assert (tmp_path / (p + ".depth.tsv")).read_bytes() == DM.tsv_bytes(refs, recs, w)
        assert int(recs["reads"][0]) == paf.count("\n") and int(recs["reads"][1]) == 0  # (the stub maps to the first reference)
    r = _run(exe, base + ["--depth", "-p", str(tmp_path / "y")], MQ_FAKE_MULTI="1", MQ_STUB_DEPTH_FAIL="1")
    assert r.returncode == 101 and "mq_depth_add: stub (mq_depth_add): no device memory" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not (tmp_path / "y.paf").exists() and not (tmp_path / "y.depth.bed").exists()
    r = _run(exe, [str(rd), "--reference", str(fa), "--depth", "--depth-window", "0", "-p", str(tmp_path / "z")])
    assert r.returncode == 2 and "--depth-window" in r.stderr
    r = _run(exe, ["--help"])
    assert r.returncode == 0 and all(f in r.stdout for f in ("--depth ", "--depth-window", "--depth-min-mapq"))


# ------------------------------------------------------------------ the Python driver
class _Names:
    def ref_info(self, rid):
        return {0: ("chr1", 2500), 7: ("", 3), 9: ("decoy", 1000)}[rid]


def test_python_driver_parser_and_formatters():
    from mapquik_amd import api, cli
    ap = cli.build_parser()
    opt = ap.parse_args(["reads.fa", "--index", "a.mqx", "--depth", "--depth-window", "64", "--depth-min-mapq", "0"])
    assert opt.depth is True and opt.depth_window == 64 and opt.depth_min_mapq == 0
    dflt = ap.parse_args(["reads.fa"])
    assert dflt.depth is False and dflt.depth_window == 1000 and dflt.depth_min_mapq == 60
    assert all(f in ap.format_help() for f in ("--depth", "--depth-window", "--depth-min-mapq"))
    recs = np.array([(0, 0, 2500, 3, 0, 4, 2145, 0, 2005), (7, 0, 3, 1, 3, 0, 0, 1, 0), (9, 0, 1000, 1, 4, 2, 5, 0, 5)], dtype=api.ref_depth_dtype)
    wb, ws = np.array([2005, 125, 15, 0, 5], dtype=np.uint64), np.array([3, 0, 1, 0, 2], dtype=np.uint32)
    # means: 2.005 is below 2.005 in binary -> "2.00"; 0.125 is a tie in binary -> to even, "0.12"; 15 / 500 = 0.03; 0.005 lies above -> "0.01"
    bed = b"chr1\t0\t1000\t2005\t3\t2.00\nchr1\t1000\t2000\t125\t0\t0.12\nchr1\t2000\t2500\t15\t1\t0.03\n\t0\t3\t0\t0\t0.00\ndecoy\t0\t1000\t5\t2\t0.01\n"
    assert api.format_depth_bed(_Names(), recs, wb, ws, 1000) == bed
    tsv = DM.TSV_HEAD.encode() + b"chr1\t2500\t4\t2145\t0.86\t0\t2.00\n\t3\t0\t0\t0.00\t1\t0.00\ndecoy\t1000\t2\t5\t0.01\t0\t0.01\n"
    assert api.format_depth_tsv(_Names(), recs, 1000) == tsv
    assert api.format_depth_bed(_Names(), recs[:0], wb[:0], ws[:0], 1000) == b"" and api.format_depth_tsv(_Names(), recs[:0], 1000) == DM.TSV_HEAD.encode()
    names = [(0, "chr1", 2500), (7, "", 3), (9, "decoy", 1000)]
    assert DM.bed_bytes(names, recs, wb, ws, 1000) == bed and DM.tsv_bytes(names, recs, 1000) == tsv
    tot = dict(offered=9, counted=6, not_mapped=1, below_mapq=1, out_of_range=1)
    assert cli.depth_log_line(tot, recs, 1000, 60) == DM.log_line(recs, tot, 1000, 60) == "Depth: 6 of 9 hits counted (1 not mapped, 1 below mapq 60, 1 out of range): 2150 bases in 5 windows of 1000"
