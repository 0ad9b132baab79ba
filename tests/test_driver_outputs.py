"""The native driver's output contract where no other host test asserts it exactly (no GPU): the stand-alone `mapquik_asan` of
`make asan` (ASan + UBSan; nothing is loaded into Python) over the host-only stub of the C ABI (tests/cpp/stub_mapquik_hip*.cc), on
inputs of test_sanitizers.py's size.  Pinned here: the sequence of stdout lines with the reference's wording (src/closures.rs:58,
main.rs:270-271; durations masked), `.unmapped.out` and the `--second-pass` FASTA in input order and equal between `--gpus 1` and `2`,
the files that a failure leaves behind, and an error exit after the first stream slots exist that frees them (LeakSanitizer).
The stub cannot save or load an index file (both calls fail with the message "stub"): an `--index` run is pinned up to that error."""
import os
import re
import subprocess

import pytest

from test_sanitizers import _inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
_SAN_WORDS = ("AddressSanitizer", "ThreadSanitizer", "LeakSanitizer", "runtime error:")
_DURATION = re.compile(r"\d+(\.\d+)?(ns|µs|ms|s)(?=\.?$)")
_RSS = re.compile(r"^Maximum RSS: [0-9.e-]+GB$")


@pytest.fixture(scope="module")
def exe():
    r = subprocess.run(["make", "-C", ROOT, "asan"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("make asan failed:\n" + r.stderr[-2000:])
    return os.path.join(LIB, "mapquik_asan")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return _inputs(tmp_path_factory.mktemp("driver_outputs"))


def _run(exe, p, reads, prefix, extra=(), env=None, ref="ref1.fa"):
    args = [exe, p[reads]] + (["--reference", p[ref]] if ref else []) + ["-p", prefix, "--batch-bases", "20000", "--threads", "4"] + list(extra)
    r = subprocess.run(args, capture_output=True, text=True, timeout=300, env=dict(_ENV, **(env or {})))
    assert not [w for w in _SAN_WORDS if w in r.stderr], r.stderr[-3000:]
    return r


def _masked(stdout):
    return [_RSS.sub("Maximum RSS: <R>GB", _DURATION.sub("<T>", ln)) for ln in stdout.splitlines()]


def _left_behind(prefix):
    d, base = os.path.split(prefix)
    return sorted((f[len(base):], os.path.getsize(os.path.join(d, f))) for f in os.listdir(d) if f.startswith(base))


_WARNINGS = ["Warning: Using default k value (5).", "Warning: Using default l value (31).", "Warning: Using default buffer size (1X).",
             "Warning: Using default queue length (200).", "Warning: Using default density value (1%).",
             "Warning: Using default minimum chain length (4).", "Warning: Using default minimum number of matching seeds (11).",
             "Warning: Using default maximum seed gap difference (2000).", "Using HPC ntHash, with SIMD"]


def _stub_kminmers(path):
    """what the stub's mq_index_add_ref counts for the records of a single-line FASTA: (name, len // 100) and the index's total"""
    lines = open(path, "rb").read().split(b"\n")
    recs = [(lines[i][1:].split()[0].decode(), lines[i + 1]) for i in range(0, len(lines) - 1, 2)]
    return [(n, len(s) // 100) for n, s in recs], sum(len(s) // 100 + (sum(s[::4096]) & 1) for n, s in recs)


def _one_pass_tail(p, ref="ref1.fa"):
    per_ref, total = _stub_kminmers(p[ref])
    return (["Indexed reference %s: %d k-min-mers." % nr for nr in per_ref] +
            ["Indexed %d unique k-min-mers in <T>." % total, "Mapped query sequences in <T>."])


_TOTALS = ["Total execution time: <T>", "Maximum RSS: <R>GB"]


def test_stdout_of_a_fasta_run(exe, files, tmp_path):
    p, recs = files
    r = _run(exe, p, "reads.fa", str(tmp_path / "o"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert _masked(r.stdout) == (["Input file: " + p["reads.fa"], "Format: FASTA", "Reference file: " + p["ref1.fa"], "Format: FASTA"] + _WARNINGS +
                                 _one_pass_tail(p) + _TOTALS)
    assert _left_behind(str(tmp_path / "o"))[0][0] == ".paf" and len(_left_behind(str(tmp_path / "o"))) == 1


def test_stdout_of_an_index_run_up_to_the_stub_s_refusal(exe, files, tmp_path):
    p, recs = files
    prefix = str(tmp_path / "o")
    r = _run(exe, p, "reads.fa", prefix, ["--index", str(tmp_path / "no.mqx")], ref=None)
    assert r.returncode == 101 and r.stderr.splitlines()[-1] == "mapquik: ReadOnlyIndex::load: stub", (r.returncode, r.stderr[-2000:])
    assert _masked(r.stdout) == ["Input file: " + p["reads.fa"], "Format: FASTA"] + _WARNINGS  # (no "Reference file" lines: none was named)
    assert _left_behind(prefix) == [(".paf", 0)]


@pytest.fixture(scope="module")
def second_pass_runs(exe, files, tmp_path_factory):
    """one --second-pass run per GPU count: (process, prefix)"""
    p, recs = files
    out = {}
    for gpus in (1, 2):
        prefix = str(tmp_path_factory.mktemp("second_%d" % gpus) / "o")
        out[gpus] = (_run(exe, p, "reads.fa", prefix, ["--gpus", str(gpus), "--second-pass", "3,15,0.05"], {"MQ_STUB_DEVICES": str(gpus)}), prefix)
    return out


@pytest.mark.parametrize("gpus", [1, 2])
def test_second_pass_stdout_and_unmapped_reads_in_input_order(second_pass_runs, files, gpus):
    p, recs = files
    r, prefix = second_pass_runs[gpus]
    assert r.returncode == 0, r.stderr[-2000:]
    second = prefix + "-3-15-0.05"
    assert _masked(r.stdout) == (["Input file: " + p["reads.fa"], "Format: FASTA", "Reference file: " + p["ref1.fa"], "Format: FASTA"] + _WARNINGS +
                                 _one_pass_tail(p) + ["Second pass: %s.fa with k=3 l=15 density=0.05" % second] + _one_pass_tail(p) + _TOTALS)
    short = [(a, b) for a, b in recs if len(b) < 50]  # the stub leaves these unmapped, in both passes
    assert len(short) > 100
    names = "".join(a + "\n" for a, b in short)
    assert open(prefix + ".unmapped.out").read() == names and open(second + ".unmapped.out").read() == names
    assert open(second + ".fa").read() == "".join(">%s\n%s\n" % ab for ab in short)
    assert [ln.split("\t")[0] for ln in open(prefix + ".paf")] == [a for a, b in recs if len(b) >= 50]
    assert os.path.getsize(second + ".paf") == 0
    assert [s for s, n in _left_behind(prefix)] == ["-3-15-0.05.fa", "-3-15-0.05.paf", "-3-15-0.05.unmapped.out", ".paf", ".unmapped.out"]


def test_one_and_two_gpus_write_the_same_files(second_pass_runs):
    (r1, a), (r2, b) = second_pass_runs[1], second_pass_runs[2]
    for suffix in (".paf", ".unmapped.out", "-3-15-0.05.fa", "-3-15-0.05.paf", "-3-15-0.05.unmapped.out"):
        assert open(a + suffix, "rb").read() == open(b + suffix, "rb").read(), suffix


def test_files_left_behind_a_missing_reference(exe, files, tmp_path):
    p, recs = files
    prefix = str(tmp_path / "o")
    missing = dict(p, **{"ref1.fa": str(tmp_path / "nowhere.fa")})
    r = _run(exe, missing, "reads.fa", prefix, ["--unmapped"])
    assert r.returncode == 101 and r.stderr.splitlines()[-1] == "mapquik: Error opening compressed file: " + missing["ref1.fa"], r.stderr[-2000:]
    assert _left_behind(prefix) == [(".paf", 0), (".unmapped.out", 0)]  # the PAF is created first (src/closures.rs:32)


def _junk_reference(p, tmp_path):
    junk = tmp_path / "junk.fa"
    junk.write_bytes(b"this is not FASTA\n>a\nACGT\n")
    return dict(p, **{"ref1.fa": str(junk)})


def test_files_left_behind_a_malformed_reference_record(exe, files, tmp_path):
    p, recs = files
    prefix = str(tmp_path / "o")
    r = _run(exe, _junk_reference(p, tmp_path), "reads.fa", prefix, ["--second-pass", "3,15,0.05"], {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=0"})
    assert r.returncode == 101 and r.stderr.splitlines()[-1] == "mapquik: malformed FASTA record", r.stderr[-2000:]
    assert _left_behind(prefix) == [("-3-15-0.05.fa", 0), (".paf", 0), (".unmapped.out", 0)]


@pytest.mark.parametrize("fail_at", [0, 20])
def test_a_failure_in_the_map_phase_leaves_no_paf(exe, files, tmp_path, fail_at):
    p, recs = files
    prefix = str(tmp_path / "o")
    r = _run(exe, p, "reads.fa", prefix, ["--unmapped"], {"MQ_DRIVER_FAIL_AT": str(fail_at)})
    assert r.returncode == 101 and r.stderr.splitlines()[-1] == "mapquik: injected failure (MQ_DRIVER_FAIL_AT)", (r.returncode, r.stderr[-2000:])
    assert [s for s, n in _left_behind(prefix)] == [".unmapped.out"]
    assert _masked(r.stdout)[-1].startswith("Indexed ") and _masked(r.stdout)[-1].endswith(" unique k-min-mers in <T>.")


@pytest.mark.parametrize("case", ["save_index", "malformed_reference"])
def test_an_error_after_the_first_stream_slots_exist_frees_them(exe, files, tmp_path, case):
    """The first GPU's stream slots are made by a thread of their own beside the reference phase; an error between there and the map
    phase (the index cannot be saved; a reference record is malformed) must free them before their index, and leak nothing:
    exit 101 with detect_leaks=1 and no report."""
    p, recs = files
    prefix = str(tmp_path / "o")
    if case == "save_index":
        r = _run(exe, p, "reads.fa", prefix, ["--save-index", str(tmp_path / "no_such_directory" / "i.mqx")])
        assert r.stderr.splitlines()[-1] == "mapquik: ReadOnlyIndex::save: stub"
    else:
        r = _run(exe, _junk_reference(p, tmp_path), "reads.fa", prefix)
        assert r.stderr.splitlines()[-1] == "mapquik: malformed FASTA record"
    assert r.returncode == 101, (r.returncode, r.stderr[-2000:])
    assert _left_behind(prefix) == [(".paf", 0)]
