"""CPU: the boundary of the coordinate sorter -- prototypes in the header, in INTEGRATION.md, in api.EXPORTS and in the library's dynamic
symbols; the record sizes; the native driver's --sort over the host-only stub in the stand-alone sanitizer builds (nothing is loaded
into Python); the Python driver's parser and formatter on canned arrays.  Every test here needs the new symbols."""
import os
import re
import subprocess

import numpy as np
import pytest

import sort_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
NEW = ("mq_sort_new", "mq_sort_free", "mq_sort_clear", "mq_sort_reserve", "mq_sort_add", "mq_sort_add_device", "mq_sort_result")
DIAG = ("mqdiag_sort_tile_records", "mqdiag_sort_passes", "mqdiag_sort_result_ms")
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1", MQ_STUB_SORT_LOG="1")


def test_prototypes_in_header_integration_md_and_exports():
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "mapquik_hip_diag.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define MQ_ABI_VERSION 4\b", hdr)
    for proto in (r"int mq_sort_new\(mq_index \*idx, uint64_t capacity, uint32_t min_mapq, mq_sorter \*\*out\);", r"void mq_sort_free\(mq_sorter \*s\);",
                  r"int mq_sort_clear\(mq_sorter \*s\);", r"int mq_sort_reserve\(mq_sorter \*s, uint64_t capacity\);",
                  r"int mq_sort_add\(mq_sorter \*s, const mq_hit \*hits, uint32_t n, uint32_t first_ordinal\);",
                  r"int mq_sort_add_device\(mq_sorter \*s, const mq_hit \*d_hits, uint32_t n, uint32_t first_ordinal, void \*stream\);",
                  r"int mq_sort_result\(mq_sorter \*s, const uint32_t \*\*order, uint64_t \*n_kept, const mq_sort_ref \*\*refs, uint64_t \*n_refs,\s*mq_sort_totals \*totals\);"):
        assert re.search(proto, hdr), proto
    assert re.search(r"uint32_t ref_id, reserved;\s*uint64_t first, count;", hdr)
    assert re.search(r"uint64_t offered, kept, not_mapped, below_mapq, out_of_range;", hdr)
    for proto in (r"uint64_t mqdiag_sort_tile_records\(void\);", r"int mqdiag_sort_passes\(mq_sorter \*s, uint32_t \*passes\);", r"int mqdiag_sort_result_ms\(mq_sorter \*s, float \*ms\);"):
        assert re.search(proto, diag), proto
    for proto in (r"pub fn mq_sort_new\(i: \*mut MqIndex, capacity: u64, min_mapq: u32, out: \*mut \*mut MqSorter\) -> c_int;", r"pub fn mq_sort_free\(s: \*mut MqSorter\);",
                  r"pub fn mq_sort_clear\(s: \*mut MqSorter\) -> c_int;", r"pub fn mq_sort_reserve\(s: \*mut MqSorter, capacity: u64\) -> c_int;",
                  r"pub fn mq_sort_add\(s: \*mut MqSorter, hits: \*const MqHit, n: u32, first_ordinal: u32\) -> c_int;",
                  r"pub fn mq_sort_add_device\(s: \*mut MqSorter, d_hits: \*const MqHit, n: u32, first_ordinal: u32, stream: \*mut c_void\) -> c_int;",
                  r"pub fn mq_sort_result\(s: \*mut MqSorter, order: \*mut \*const u32, n_kept: \*mut u64, refs: \*mut \*const MqSortRef, n_refs: \*mut u64, "
                  r"totals: \*mut MqSortTotals\) -> c_int;",
                  r"pub struct MqSortRef \{ pub ref_id: u32, pub reserved: u32, pub first: u64, pub count: u64 \}",
                  r"pub struct MqSortTotals \{ pub offered: u64, pub kept: u64, pub not_mapped: u64, pub below_mapq: u64, pub out_of_range: u64 \}", r"pub struct MqSorter \{ _private"):
        assert re.search(proto, integ), proto
    from mapquik_amd import api
    assert api.MQ_ABI_VERSION == 4 and all(n in api.EXPORTS for n in NEW)
    assert api.sort_ref_dtype.itemsize == 24 and api.sort_totals_dtype.itemsize == 40
    assert api.sort_ref_dtype.names == SM.sort_ref_dtype.names and api.sort_totals_dtype.names == SM.TOTALS
    assert all(callable(getattr(api.Sorter, m)) for m in ("add", "add_device", "reserve", "result", "clear", "close"))


def test_library_exports_the_entry_points():
    import mapquik_amd
    out = subprocess.run(["nm", "-D", "--defined-only", mapquik_amd.build.LIB], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) | set(DIAG) <= exported
    L = mapquik_amd.load_library()
    assert L.mq_abi_version() == 4 and all(hasattr(L, n) for n in NEW)
    t = int(L.mqdiag_sort_tile_records())
    assert t > 0 and t % 256 == 0  # whole rounds of the 256-thread workgroup that ranks a tile


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
    """--sort over the stub, whose sorter is the rules spelled out on the host: one sorter per pass, made behind the index phase; one
    mq_sort_add per chunk (several chunks, two fake GPUs) whose first ordinals are the chunks' first read numbers in input order; one
    result; sorted.paf is the model's permutation of the lines of the PAF the same run wrote and the tsv's offsets point at each
    reference's first line; the PAF is the one without the flag; a failing add ends the run with exit 101 and no PAF; --help names the
    flags."""
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
    assert r0.returncode == 0 and "stub: mq_sort" not in r0.stderr and "Sorted:" not in r0.stdout, r0.stderr[-2000:]
    assert not (tmp_path / "w.sorted.paf").exists()
    mapped = sum(1 for n in lens if n >= 50)
    for flags, q in ((["--sort"], 0), (["--sort", "--sort-min-mapq", "61"], 61)):
        p = "x%d" % q
        r = _run(exe, base + flags + ["-p", str(tmp_path / p)], MQ_FAKE_MULTI="1")
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        calls = [ln for ln in r.stderr.splitlines() if ln.startswith("stub: mq_sort")]
        assert calls[0] == "stub: mq_sort_new capacity 0 min_mapq %d, 2 references" % q and calls[-1] == "stub: mq_sort_result 120 offered", calls
        adds = [tuple(int(x) for x in re.findall(r"\d+", ln)) for ln in calls[1:-1]]
        assert all(ln.startswith("stub: mq_sort_add ") for ln in calls[1:-1]) and len(adds) >= 4, calls
        # the chunks arrive in input order and each begins where the one before it ended
        assert [a[1] for a in adds] == np.concatenate([[0], np.cumsum([a[0] for a in adds])[:-1]]).tolist() and sum(a[0] for a in adds) == 120
        paf = (tmp_path / (p + ".paf")).read_bytes()
        assert paf == (tmp_path / "w.paf").read_bytes() and paf.count(b"\n") == mapped and sum(a[2] for a in adds) == (mapped if q == 0 else 0)
        sp, tsv, recs, tot = SM.sorted_files(refs, paf, q)
        tot = dict(tot, offered=120, not_mapped=120 - mapped)
        assert SM.log_line(recs, tot, q) + "\n" in r.stdout, r.stdout
        assert r.stdout.index("unique k-min-mers in") < r.stdout.index("Sorted:") < r.stdout.index("Mapped query sequences")
        got = (tmp_path / (p + ".sorted.paf")).read_bytes()
        assert got == sp and (tmp_path / (p + ".sorted.tsv")).read_bytes() == tsv
        if q == 0:
            starts = [int(ln.split(b"\t")[7]) for ln in got.splitlines()]
            assert starts == sorted(starts) and len(set(starts)) > 10 and got != paf and sorted(got.splitlines()) == sorted(paf.splitlines())
            rows = [ln.split("\t") for ln in tsv.decode().splitlines()[1:]]
            assert [r_[0] for r_ in rows] == ["one", "two"] and rows[0][2:] == [str(mapped), "0", "0"] and rows[1][2:] == ["0", str(mapped), str(len(got))]
        else:
            assert got == b""
    r = _run(exe, base + ["--sort", "-p", str(tmp_path / "y")], MQ_FAKE_MULTI="1", MQ_STUB_SORT_FAIL="1")
    assert r.returncode == 101 and "mq_sort_add: stub (mq_sort_add): no device memory" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not (tmp_path / "y.paf").exists() and not (tmp_path / "y.sorted.paf").exists()
    r = _run(exe, [str(rd), "--reference", str(fa), "--sort", "--sort-min-mapq", "-1", "-p", str(tmp_path / "z")])
    assert r.returncode == 2 and "--sort-min-mapq" in r.stderr
    r = _run(exe, ["--help"])
    assert r.returncode == 0 and all(f in r.stdout for f in ("--sort ", "--sort-min-mapq"))


def test_driver_second_pass_and_failing_result_over_the_stub(exes, tmp_path):
    """--second-pass: one sorter per pass, each pass's PAF sorted under that pass's own prefix.  A failing mq_sort_result ends the run
    with exit 101 and leaves neither the PAF nor a sorted file behind, as a failing add does."""
    import glob
    exe = exes["asan"]
    rng = np.random.default_rng(6)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rd, fa = tmp_path / "reads.fa", tmp_path / "ref.fa"
    lens = [int(x) for x in rng.integers(30, 400, 60)]  # (the stub leaves a read below 50 bases unmapped, in either pass)
    rd.write_bytes(b"".join(b">r%d\n" % i + acgt[rng.integers(0, 4, n)].tobytes() + b"\n" for i, n in enumerate(lens)))
    fa.write_bytes(b">one\n" + acgt[rng.integers(0, 4, 5000)].tobytes() + b"\n")
    refs = [(0, "one", 5000)]
    short = sum(1 for n in lens if n < 50)
    assert 0 < short < 60
    r = _run(exe, [str(rd), "--reference", str(fa), "--sort", "--second-pass", "7,31,0.02", "-p", str(tmp_path / "s")])
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    calls = [ln.split()[1] for ln in r.stderr.splitlines() if ln.startswith("stub: mq_sort")]
    new, res = [i for i, c in enumerate(calls) if c == "mq_sort_new"], [i for i, c in enumerate(calls) if c == "mq_sort_result"]
    assert len(new) == len(res) == 2 and new[0] < res[0] < new[1] < res[1], calls
    offered = [int(re.findall(r"\d+", ln)[0]) for ln in r.stderr.splitlines() if ln.startswith("stub: mq_sort_result")]
    assert offered == [60, short]  # the second pass sorts its own reads: the ones the first left unmapped
    second = glob.glob(str(tmp_path / "s-*.sorted.paf"))
    assert len(second) == 1
    for prefix in (str(tmp_path / "s"), second[0][:-len(".sorted.paf")]):
        paf = open(prefix + ".paf", "rb").read()
        sp, tsv, _, _ = SM.sorted_files(refs, paf, 0)
        assert open(prefix + ".sorted.paf", "rb").read() == sp and open(prefix + ".sorted.tsv", "rb").read() == tsv, prefix
    assert open(str(tmp_path / "s.paf"), "rb").read().count(b"\n") == 60 - short and r.stdout.count("Sorted: ") == 2
    r = _run(exe, [str(rd), "--reference", str(fa), "--sort", "-p", str(tmp_path / "f")], MQ_STUB_SORT_FAIL="result")
    assert r.returncode == 101 and "mq_sort_result: stub (mq_sort_result): no device memory" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not glob.glob(str(tmp_path / "f.*paf")) and not (tmp_path / "f.sorted.tsv").exists()


# ------------------------------------------------------------------ the Python driver
class _Names:
    def ref_info(self, rid):
        return {0: ("chr1", 2500), 7: ("", 3), 9: ("decoy", 1000)}[rid]


def test_python_driver_parser_and_formatter():
    from mapquik_amd import api, cli
    ap = cli.build_parser()
    opt = ap.parse_args(["reads.fa", "--index", "a.mqx", "--sort", "--sort-min-mapq", "30"])
    assert opt.sort is True and opt.sort_min_mapq == 30
    dflt = ap.parse_args(["reads.fa"])
    assert dflt.sort is False and dflt.sort_min_mapq == 0
    assert all(f in ap.format_help() for f in ("--sort", "--sort-min-mapq"))
    recs = np.array([(0, 0, 0, 2), (7, 0, 2, 0), (9, 0, 2, 1)], dtype=api.sort_ref_dtype)
    tsv = SM.TSV_HEAD.encode() + b"chr1\t2500\t2\t0\t0\n\t3\t0\t2\t150\ndecoy\t1000\t1\t2\t150\n"
    assert api.format_sorted_tsv(_Names(), recs, [0, 70, 150, 233]) == tsv
    assert api.format_sorted_tsv(_Names(), recs[:0], [0]) == SM.TSV_HEAD.encode()
    tot = dict(offered=9, kept=3, not_mapped=4, below_mapq=1, out_of_range=1)
    assert cli.sort_log_line(tot, recs, 30) == SM.log_line(recs, tot, 30) == "Sorted: 3 of 9 hits kept (4 not mapped, 1 below mapq 30, 1 out of range): 3 lines on 2 references"
