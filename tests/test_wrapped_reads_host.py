"""Host side of `--reads-join device` (no GPU): the native driver under AddressSanitizer + UBSan and ThreadSanitizer (stand-alone
binaries of `make asan tsan`; nothing is loaded into Python), linked against the host-only stub of the C ABI
(tests/cpp/stub_mapquik_hip_reads_lines.cc restates MQ_FASTX_FASTA_LINES and mq_ctx_wait_fasta_lines on the host).  A line-wrapped reads
FASTA must give the same .paf and .unmapped.out whether its chunks come back irregular and are compacted by a host thread
(`--reads-join host`, the default) or are submitted as MQ_FASTX_FASTA_LINES and only their header lines are read on the host
(`device`); the same under --second-pass, whose FASTA of unmapped reads is joined on the host from the regions of such a chunk."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-C", ROOT, "asan", "tsan"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("make asan tsan failed:\n" + r.stderr[-2000:])
    return {k: os.path.join(LIB, "mapquik_" + k) for k in ("asan", "tsan")}


_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1",
            UBSAN_OPTIONS="print_stacktrace=1", MQ_DRIVER_TIMING="1")


def _bases(rng, n):
    return np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, n)].tobytes()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """a reference, and 400 reads of 1 .. 6,000 bases (the stub leaves those under 50 unmapped) wrapped at 60 (LF) and 70 columns
    (CR-LF, no final newline), with a '>' inside some lines and an empty line here and there"""
    d = tmp_path_factory.mktemp("wrapped_reads")
    rng = np.random.default_rng(11)
    ref = d / "ref.fa"
    ref.write_bytes(b">chr1\n" + _bases(rng, 200_000) + b"\n")
    reads = [(b"r%d" % i, _bases(rng, int(rng.integers(1, 60)) if i % 7 == 0 else int(rng.integers(60, 6000)))) for i in range(400)]
    out = {"ref": str(ref)}
    for name, w, nl, final in (("w60", 60, b"\n", True), ("w70_crlf", 70, b"\r\n", False)):
        parts = []
        for k, (i, s) in enumerate(reads):
            if k % 5 == 0 and len(s) > 30:
                s = s[:17] + b">" + s[18:]  # a '>' in the middle of a line opens no record
            body = b"".join(s[j:j + w] + nl for j in range(0, len(s), w))
            if k % 11 == 0:
                body += nl  # an empty line between records
            parts.append(b">" + i + b" np:i:%d >x" % k + nl + body)
        txt = b"".join(parts)
        if not final:
            txt = txt[:-len(nl)] if not txt.endswith(nl + nl) else txt[:-2 * len(nl)]
        p = d / (name + ".fa")
        p.write_bytes(txt)
        out[name] = str(p)
    return out


def _run(exe, reads, ref, prefix, extra):
    r = subprocess.run([exe, reads, "--reference", ref, "-p", prefix, "--threads", "3", "--unmapped"] + extra, capture_output=True, text=True,
                       timeout=900, env=_ENV)
    bad = [w for w in ("AddressSanitizer", "ThreadSanitizer", "LeakSanitizer", "runtime error:") if w in r.stderr]
    assert not bad and r.returncode == 0, (r.returncode, r.stderr[-3000:])
    return r


def _counts(stderr):
    ln = [x for x in stderr.splitlines() if x.startswith("unparsed chunks ")][0].split()
    return int(ln[2]), int(ln[4])


@pytest.mark.parametrize("san", ["asan", "tsan"])
@pytest.mark.parametrize("name", ["w60", "w70_crlf"])
def test_host_and_device_join_write_the_same_files(built, files, tmp_path, san, name):
    for chunk in ("20000", "300000", "33554432"):
        outs = {}
        for where in ("host", "device"):
            prefix = str(tmp_path / ("%s_%s" % (where, chunk)))
            r = _run(built[san], files[name], files["ref"], prefix, ["--batch-bases", chunk, "--reads-join", where])
            outs[where] = (open(prefix + ".paf").read(), open(prefix + ".unmapped.out").read())
            unparsed, irregular = _counts(r.stderr)
            # (host: a chunk that happens to hold short, one-line reads only is regular there too)
            assert unparsed > 0 and (irregular > unparsed // 2 if where == "host" else irregular == 0), (where, chunk, unparsed, irregular)
        assert outs["host"] == outs["device"], (name, chunk)
        assert outs["host"][0].count("\n") > 300 and outs["host"][1].count("\n") > 40


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_second_pass_joins_unmapped_reads_on_the_host(built, files, tmp_path, san):
    outs = {}
    for where in ("host", "device"):
        prefix = str(tmp_path / where)
        _run(built[san], files["w70_crlf"], files["ref"], prefix, ["--batch-bases", "300000", "--reads-join", where, "--second-pass", "3,15,0.05"])
        second = prefix + "-3-15-0.05"
        outs[where] = [open(p).read() for p in (prefix + ".paf", prefix + ".unmapped.out", second + ".fa", second + ".paf", second + ".unmapped.out")]
    assert outs["host"] == outs["device"]
    assert outs["host"][2].count(">") > 40 and "\r" not in outs["host"][2]


def test_default_is_host_and_other_words_are_refused(built, files, tmp_path):
    prefix = str(tmp_path / "d")
    r = _run(built["asan"], files["w60"], files["ref"], prefix, ["--batch-bases", "300000"])
    unparsed, irregular = _counts(r.stderr)
    assert unparsed > 0 and irregular > unparsed // 2  # without the option a wrapped chunk comes back irregular, as it always did
    for word in ("sideways", "", "Device"):
        r = subprocess.run([built["asan"], files["w60"], "--reference", files["ref"], "-p", prefix, "--reads-join", word], capture_output=True, text=True, timeout=300, env=_ENV)
        assert r.returncode == 2 and "--reads-join wants device or host" in r.stderr, (word, r.returncode, r.stderr[-500:])
    r = subprocess.run([built["asan"], "--help"], capture_output=True, text=True, timeout=60)
    assert "--reads-join <device|host>" in r.stdout


def test_the_seam_names_the_function():
    import re
    import mapquik_amd
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\bmq_ctx_wait_fasta_lines\s*\(", hdr) and "#define MQ_FASTX_FASTA_LINES 2u" in hdr and "#define MQ_ABI_VERSION 4" in hdr
    assert "pub fn mq_ctx_wait_fasta_lines(" in integ and "mq_ctx_wait_fasta_lines" in mapquik_amd.api.EXPORTS
    assert callable(mapquik_amd.api.Context.wait_fasta_lines)
    with pytest.raises(ValueError):
        mapquik_amd.api.Context.submit_fasta(object(), b">a\nA\n", fastq=True, lines=True)
