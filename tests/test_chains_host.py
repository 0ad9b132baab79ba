"""The chains output without a GPU: the six prototypes and the two records in the header, in INTEGRATION.md, in api.EXPORTS and among the
library's exported symbols; the record layouts of the Python binding; the ABI version, which additions do not move.  And `--chains` of
the native driver without a GPU: the stand-alone `mapquik_asan` / `mapquik_tsan` of `make asan tsan` (ASan + UBSan, TSan; nothing is
loaded into Python) over the host-only stub tests/cpp/stub_mapquik_hip_chains.cc, whose canned chains are a function of the canned hits:
the stream slots reserve, a chunk's chains are taken when its slot is waited for, a formatter builds their text and the ordered writer
writes it; the `.paf` is byte-identical with and without the flag; a pool that is too small ends the run with exit code 101 and a message
that names what was needed; `--chains` and `--anchors` go together.  `mq_format_paf_chain` itself is called by a stand-alone program of
its own (tests/cpp/chains_format_test.cc, built beside the sanitizer drivers) and compared with a Python formatter."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mapquik_amd", "lib")
_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1", TSAN_OPTIONS="halt_on_error=1")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mq_ctx_reserve_chains", "mq_ctx_chains", "mq_ctx_chains_device", "mq_map_reserve_chains", "mq_map_chains", "mq_format_paf_chain")


def test_prototypes_in_header_and_integration_md():
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"#define MQ_ABI_VERSION 4\b", hdr)
    assert re.search(r"int mq_ctx_reserve_chains\(mq_ctx \*ctx, uint32_t max_reads, uint64_t max_chains\);", hdr)
    assert re.search(r"int mq_format_paf_chain\(const mq_index \*idx, const char \*q_id, uint64_t q_len, const mq_chain \*chain, char \*buf, size_t cap\);", hdr)
    assert re.search(r"#define MQ_CHAINS_DROPPED 0xFFFFFFFFu", hdr) and re.search(r"#define MQ_CHAIN_TOP 1u", hdr)
    assert "one of its legal orders" in hdr  # the order of a read's chains, and why it is a legal one
    m = re.search(r"typedef struct mq_chain \{(.*?)\} mq_chain;", hdr, re.S)
    fields = re.findall(r"\b(flags|ref_id|rc|mapq|q_start|q_end|r_start|r_end|score|n_runs|q_start_hi|q_end_hi)\b(?=[,;])", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    from mapquik_amd import api
    assert tuple(fields) == api.chain_dtype.names  # field for field the layout of mq_hit
    assert [n for n in api.chain_dtype.names if n not in ("flags", "n_runs")] == [n for n in api.hit_dtype.names if n not in ("status", "n_kminmers")]
    assert api.chain_dtype.names.index("n_runs") == api.hit_dtype.names.index("n_kminmers") == 9
    for name in NEW:
        assert re.search(r"int %s\(" % name, hdr) and re.search(r"pub fn %s\(" % name, integ) and name in api.EXPORTS, name
    assert "pub struct MqChain " in integ and "pub struct MqChainSpan " in integ
    assert api.MQ_ABI_VERSION == 4 and api.chain_dtype.itemsize == 48 and api.chain_span_dtype.itemsize == 8
    assert api.MQ_CHAIN_TOP == 1 and api.MQ_CHAINS_DROPPED == 0xFFFFFFFF


def test_library_exports_the_entry_points():
    import mapquik_amd
    out = subprocess.run(["nm", "-D", "--defined-only", mapquik_amd.build.LIB], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(NEW) <= exported
    L = mapquik_amd.load_library()
    assert L.mq_abi_version() == 4 and all(hasattr(L, n) for n in NEW)
    import mapquik_amd as mq
    assert mq.chain_dtype.itemsize == 48 and mq.MQ_CHAIN_TOP == mq.MQ_HIT_MAPPED


@pytest.fixture(scope="module")
def exes():
    r = subprocess.run(["make", "-C", ROOT, "asan", "tsan"], capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        pytest.fail("make asan tsan failed:\n" + r.stderr[-2000:])
    return dict(asan=os.path.join(LIB, "mapquik_asan"), tsan=os.path.join(LIB, "mapquik_tsan"),
                fmt_asan=os.path.join(LIB, "chains_format_asan"), fmt_tsan=os.path.join(LIB, "chains_format_tsan"))


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """a reference and 600 reads of 1 .. 3,000 bases (those below 50 get no canned hit), as one-line FASTA, wrapped FASTA, FASTQ and gzip"""
    wd = tmp_path_factory.mktemp("chains_host")
    rng = np.random.default_rng(21)
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


def _expected_chains(paf_text):
    """the stub's rule (tests/cpp/stub_mapquik_hip_chains.cc) applied to the PAF's own columns"""
    out = []
    for ln in paf_text.splitlines():
        c = ln.split("\t")
        score = int(c[9])
        out.append(ln + "\ttp:A:P\tcn:i:%d" % (1 + score % 2))
        for j in range(1, 1 + score % 3):
            d = list(c)
            d[4] = "+" if c[4] == "-" else "-"
            d[7], d[9], d[11] = str(int(c[7]) + j), str(score // (j + 1)), "0"
            out.append("\t".join(d) + "\ttp:A:S\tcn:i:1")
    return "".join(x + "\n" for x in out)


CASES = [("reads.fa", []), ("reads.fq", []), ("reads.fq.gz", []), ("wrapped.fa", []), ("wrapped.fa", ["--reads-join", "device"])]


@pytest.mark.parametrize("san", ["asan", "tsan"])
@pytest.mark.parametrize("reads,extra", CASES)
def test_chains_file_over_the_stub(exes, inputs, tmp_path, san, reads, extra):
    exe = exes[san]
    base = [str(inputs / reads), "--reference", str(inputs / "ref.fa"), "--batch-bases", "65536", "--unmapped"] + extra
    r0 = _run(exe, base + ["-p", str(tmp_path / "plain")])
    assert r0.returncode == 0, r0.stderr[-3000:]
    r1 = _run(exe, base + ["--chains", "-p", str(tmp_path / "chn")])
    assert r1.returncode == 0, r1.stderr[-3000:]
    r2 = _run(exe, base + ["--chains", "--anchors", "-p", str(tmp_path / "both")])
    assert r2.returncode == 0, r2.stderr[-3000:]
    paf0 = (tmp_path / "plain.paf").read_bytes()
    assert paf0 == (tmp_path / "chn.paf").read_bytes() == (tmp_path / "both.paf").read_bytes() and paf0.count(b"\n") >= 500
    assert (tmp_path / "plain.unmapped.out").read_bytes() == (tmp_path / "chn.unmapped.out").read_bytes()
    assert not (tmp_path / "plain.chains").exists() and not (tmp_path / "chn.anchors").exists()
    got = (tmp_path / "chn.chains").read_text()
    assert got == _expected_chains(paf0.decode()) == (tmp_path / "both.chains").read_text()
    assert (tmp_path / "both.anchors").stat().st_size > 0
    assert [ln.split("\t")[0] for ln in paf0.decode().splitlines()] == [ln.split("\t")[0] for ln in got.splitlines() if "tp:A:P" in ln]  # input order


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_a_pool_that_is_too_small_ends_the_run(exes, inputs, tmp_path, san):
    """MQ_STUB_CHAINS_CAP=7: whatever the slots reserve, the stub's pool holds seven chains -- every chunk drops reads"""
    r = _run(exes[san], [str(inputs / "reads.fa"), "--reference", str(inputs / "ref.fa"), "--batch-bases", "65536", "--chains", "-p", str(tmp_path / "small")],
             env=dict(MQ_STUB_CHAINS_CAP="7"))
    assert r.returncode == 101, (r.returncode, r.stderr[-2000:])
    m = re.search(r"--chains: the chain pool of a stream slot was too small for (\d+) reads of a chunk: (\d+) entries needed, 7 reserved", r.stderr)
    assert m and int(m.group(1)) >= 1 and int(m.group(2)) > 7, r.stderr[-2000:]
    assert not (tmp_path / "small.paf").exists()  # no partial PAF behind a failure


def test_help_names_the_flag(exes):
    r = _run(exes["asan"], ["--help"])
    assert r.returncode == 0 and "--chains" in r.stdout


def _paf_chain(q_id, q_len, ch, refs):
    """the twelve columns of mq_format_paf_chain, worded in Python; ch: the twelve words of an mq_chain"""
    flags, ref, rc, mapq, q_start, q_end, r_start, r_end, score, n_runs, qs_hi, qe_hi = ch
    name, r_len = refs[ref]
    return "\t".join(str(x) for x in (q_id, q_len, (qs_hi << 32) | q_start, (qe_hi << 32) | q_end, "-" if rc else "+", name, r_len, r_start, r_end, score, r_len, mapq))


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_format_paf_chain_against_a_python_formatter(exes, san):
    """the program's chains (tests/cpp/chains_format_test.cc), TOP and not, both strands, wrapped 64-bit columns: the same bytes from the
    formula above; flags and n_runs do not enter the line; a small buffer reports the full length (the program's exit code); an unknown
    reference and a null argument are refused"""
    refs = {0: ("chrA some text", 5000), 7: ("chrB", 777)}
    cases = [("read1", 4500, (1, 0, 0, 60, 12, 4321, 100, 4409, 37, 3, 0, 0)),
             ("r/2 x", 701, (0, 7, 1, 0, 0, 700, 5, 705, 2, 1, 0, 0)),
             ("wrap", 5000000000, (1, 7, 1, 60, 0xFFFFEF8F, 9, 0, 776, 11, 2, 0xFFFFFFFF, 1)),
             ("z", 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0))]
    r = _run(exes["fmt_" + san], [])
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    want = [_paf_chain(q, n, ch, refs) for q, n, ch in cases] + ["unknown_ref 1", "null_args 1"]
    assert r.stdout.splitlines() == want
    assert want[2].split("\t")[2] == str(0xFFFFFFFFFFFFEF8F) and want[0].split("\t")[4] == "+" and want[1].split("\t")[4] == "-"
