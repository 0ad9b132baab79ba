"""`--anchors` of the native driver without a GPU: the stand-alone `mapquik_asan` / `mapquik_tsan` of `make asan tsan` (ASan + UBSan, TSan;
nothing is loaded into Python) over the host-only stub tests/cpp/stub_mapquik_hip_anchors.cc, whose canned anchors are a function of the
canned hits.  The stream slots reserve, a chunk's anchors are taken when its slot is waited for, a formatter builds their text beside the
PAF text and the ordered writer writes it: `<prefix>.anchors` is what the stub's rule gives for the PAF's own columns, reads in input order,
over many chunks and every way a chunk reaches a slot; the `.paf` is byte-identical with and without the flag; a pool that is too small
ends the run with exit code 101 and a message that names what was needed.  The five prototypes are in the header, in INTEGRATION.md and
in api.EXPORTS."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
NEW = ("mq_ctx_reserve_anchors", "mq_ctx_anchors", "mq_ctx_anchors_device", "mq_map_reserve_anchors", "mq_map_anchors")
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")


def test_prototypes_in_header_and_integration_md():
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define MQ_ABI_VERSION 4\b", hdr)
    assert re.search(r"int mq_ctx_reserve_anchors\(mq_ctx \*ctx, uint32_t max_reads, uint64_t max_anchors\);", hdr)
    assert re.search(r"typedef struct mq_anchor \{\s*uint32_t q_start, q_end, r_start, r_end, count;\s*\} mq_anchor;", hdr)
    assert re.search(r"#define MQ_ANCHORS_DROPPED 0xFFFFFFFFu", hdr)
    from mapquik_amd import api
    for name in NEW:
        assert re.search(r"int %s\(" % name, hdr) and re.search(r"pub fn %s\(" % name, integ) and name in api.EXPORTS, name
    assert api.MQ_ABI_VERSION == 4 and api.anchor_dtype.itemsize == 20 and api.anchor_span_dtype.itemsize == 8


@pytest.fixture(scope="module")
def exes():
    r = subprocess.run(["make", "-C", ROOT, "asan", "tsan"], capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        pytest.fail("make asan tsan failed:\n" + r.stderr[-2000:])
    return dict(asan=os.path.join(LIB, "mapquik_asan"), tsan=os.path.join(LIB, "mapquik_tsan"))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a reference and 600 reads of 1 .. 3,000 bases (those below 50 get no canned hit), as one-line FASTA, wrapped FASTA, FASTQ and gzip"""
    wd = tmp_path_factory.mktemp("anchors_host")
    rng = np.random.default_rng(20)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = acgt[rng.integers(0, 4, 50000)].tobytes()
    (wd / "ref.fa").write_bytes(b">chrStub some description\n" + ref + b"\n")
    seqs = [acgt[rng.integers(0, 4, int(n))].tobytes() for n in np.concatenate([rng.integers(1, 3001, 590), np.arange(45, 55)])]
    (wd / "reads.fa").write_bytes(b"".join(b">read%d extra\n" % i + s + b"\n" for i, s in enumerate(seqs)))
    (wd / "wrapped.fa").write_bytes(b"".join(b">read%d\n" % i + b"".join(s[j:j + 60] + b"\n" for j in range(0, len(s), 60)) for i, s in enumerate(seqs)))
    fq = b"".join(b"@read%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n" for i, s in enumerate(seqs))
    (wd / "reads.fq").write_bytes(fq)
    with gzip.open(wd / "reads.fq.gz", "wb") as f:
        f.write(fq)
    return wd


def _run(exe, args, env=None):
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=600, env=dict(_ENV, **(env or {})))


def _expected_anchors(paf_text):
    """the stub's rule (tests/cpp/stub_mapquik_hip_anchors.cc) applied to the PAF's own columns"""
    out = []
    for ln in paf_text.splitlines():
        c = ln.split("\t")
        q_start, r_start, score = int(c[2]), int(c[7]), int(c[9])
        cnt = 1 + score % 3
        for j in range(cnt):
            out.append("\t".join([c[0], str(q_start + 10 * j), str(q_start + 10 * j + 6), c[4], c[5], str(r_start + 10 * j), str(r_start + 10 * j + 6),
                                  str(score // cnt + (score % cnt if j == 0 else 0))]))
    return "".join(x + "\n" for x in out)


CASES = [("reads.fa", []), ("reads.fq", []), ("reads.fq.gz", []), ("wrapped.fa", []), ("wrapped.fa", ["--reads-join", "device"])]


@pytest.mark.parametrize("san", ["asan", "tsan"])
@pytest.mark.parametrize("reads,extra", CASES)
def test_anchors_file_over_the_stub(exes, inputs, tmp_path, san, reads, extra):
    exe = exes[san]
    base = [str(inputs / reads), "--reference", str(inputs / "ref.fa"), "--batch-bases", "65536", "--unmapped"] + extra
    r0 = _run(exe, base + ["-p", str(tmp_path / "plain")])
    assert r0.returncode == 0, r0.stderr[-3000:]
    r1 = _run(exe, base + ["--anchors", "-p", str(tmp_path / "anch")])
    assert r1.returncode == 0, r1.stderr[-3000:]
    paf0, paf1 = (tmp_path / "plain.paf").read_bytes(), (tmp_path / "anch.paf").read_bytes()
    assert paf0 == paf1 and paf1.count(b"\n") >= 500
    assert (tmp_path / "plain.unmapped.out").read_bytes() == (tmp_path / "anch.unmapped.out").read_bytes()
    assert not (tmp_path / "plain.anchors").exists()
    got = (tmp_path / "anch.anchors").read_text()
    assert got == _expected_anchors(paf1.decode())
    assert [ln.split("\t")[0] for ln in paf1.decode().splitlines()] == sorted({ln.split("\t")[0] for ln in got.splitlines()}, key=lambda s: int(s[4:]))  # input order, every mapped read


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_a_pool_that_is_too_small_ends_the_run(exes, inputs, tmp_path, san):
    """MQ_STUB_ANCHORS_CAP=7: whatever the slots reserve, the stub's pool holds seven anchors -- every chunk drops reads"""
    r = _run(exes[san], [str(inputs / "reads.fa"), "--reference", str(inputs / "ref.fa"), "--batch-bases", "65536", "--anchors", "-p", str(tmp_path / "small")],
             env=dict(MQ_STUB_ANCHORS_CAP="7"))
    assert r.returncode == 101, (r.returncode, r.stderr[-2000:])
    m = re.search(r"--anchors: the anchor pool of a stream slot was too small for (\d+) reads of a chunk: (\d+) entries needed, 7 reserved", r.stderr)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) > 7, r.stderr[-2000:]
    assert not (tmp_path / "small.paf").exists()  # no partial PAF behind a failure


def test_help_names_the_flag(exes):
    r = _run(exes["asan"], ["--help"])
    assert r.returncode == 0 and "--anchors" in r.stdout
