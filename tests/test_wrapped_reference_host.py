"""Host side of `--ref-join device` (no GPU): the native driver's reference streamer in its second mode -- a record is its header line
plus every line up to the next line that starts with '>' -- under AddressSanitizer + UBSan and ThreadSanitizer, linked against the
host-only stub of the C ABI (tests/cpp/stub_mapquik_hip_lines.cc restates the join of mq_index_add_ref_staged_lines on the host and,
with MQ_STUB_DUMP_REFS=<dir>, writes every joined sequence to <dir>/<ref_id>.seq).  What the streamer hands over must join to what
RefLoader::prepare (host/ref_loader.hpp) and seq_io (src/closures.rs:46-94) make of the same record; the ids are seq_io's id()."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")
BLOCK = 16 << 20  # RefStreamer::BLOCK


def model(region):
    return b"".join(ln[:-1] if ln.endswith(b"\r") else ln for ln in region.split(b"\n"))


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-C", ROOT, "asan", "tsan"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("make asan tsan failed:\n" + r.stderr[-2000:])
    return {k: os.path.join(LIB, "mapquik_" + k) for k in ("asan", "tsan")}


_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1",
            UBSAN_OPTIONS="print_stacktrace=1")


def _bases(rng, n):
    return np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.integers(0, 9, n)].tobytes()


def _wrap(seq, w, nl):
    return b"".join(seq[i:i + w] + nl for i in range(0, len(seq), w))


def _reads(tmp_path):
    p = tmp_path / "reads.fa"
    rng = np.random.default_rng(5)
    p.write_bytes(b"".join(b">r%d\n" % i + _bases(rng, 50 + 37 * i) + b"\n" for i in range(40)))
    return str(p)


def _run_and_compare(exe, reads, tmp_path, tag, records, extra=()):
    """records: [(header line without '>' and line end, line end of the header, region bytes)]: the file is their concatenation."""
    ref = tmp_path / ("ref_%s.fa" % tag)
    with open(ref, "wb") as f:
        for hdr, nl, region in records:
            f.write(b">" + hdr + nl + region)
    dump = tmp_path / ("dump_%s" % tag)
    dump.mkdir()
    r = subprocess.run([exe, reads, "--reference", str(ref), "-p", str(tmp_path / ("out_" + tag)), "--threads", "4", "--ref-join", "device"] + list(extra),
                       capture_output=True, text=True, timeout=900, env=dict(_ENV, MQ_STUB_DUMP_REFS=str(dump), MQ_DRIVER_TIMING="1"))
    bad = [w for w in ("AddressSanitizer", "ThreadSanitizer", "LeakSanitizer", "runtime error:") if w in r.stderr]
    assert not bad and r.returncode == 0, (r.returncode, r.stderr[-3000:])
    assert "reference streamed: every record handed to ref_extract (lines joined on the device)" in r.stderr, r.stderr[-1500:]
    assert "host loader" not in r.stderr and "reference buffer page-locked" not in r.stderr
    ids = [m.group(1) for m in re.finditer(r"^Indexed reference (.*): \d+ k-min-mers\.$", r.stdout, flags=re.M)]
    assert ids == [hdr.split(b" ")[0].decode() for hdr, _, _ in records]  # seq_io's id(): the header up to its first space
    assert sorted(os.listdir(dump)) == sorted("%d.seq" % i for i in range(len(records)))
    for i, (_, _, region) in enumerate(records):
        got = (dump / ("%d.seq" % i)).read_bytes()
        assert got == model(region), (tag, i, len(got), len(model(region)))


@pytest.mark.parametrize("san", ["asan", "tsan"])
def test_wrapped_at_80_columns(built, tmp_path, san):
    """An 80-column file of two blocks and a half: long and tiny records, a record without a sequence, blank lines between records and
    in front of the first, a '>' inside a line, no final newline; with and without --low-memory."""
    rng = np.random.default_rng(1)
    a, b, c = _bases(rng, 20_000_003), _bases(rng, 17_000_000), _bases(rng, 1200)
    records = [(b"chr1 first contig", b"\n", _wrap(a, 80, b"\n")),
               (b"chr2", b"\n", _wrap(b, 80, b"\n") + b"\n\n"),
               (b"empty nothing follows", b"\n", b""),
               (b"tiny\tx y", b"\n", b"ACGTAC>GT\nAC\rGT\n\nTTGA\n"),
               (b"last one", b"\n", _wrap(c, 80, b"\n")[:-1])]
    reads = _reads(tmp_path)
    # blank lines in front of the first record are skipped, as seq_io does
    lead = tmp_path / "ref_blank_lead.fa"
    lead.write_bytes(b"\n\r\n>x 1\nACGT\nAC\n>y\nGG\nTT")
    dump = tmp_path / "dump_blank_lead"
    dump.mkdir()
    r = subprocess.run([built[san], reads, "--reference", str(lead), "-p", str(tmp_path / "bl"), "--ref-join", "device"], capture_output=True, text=True, timeout=300,
                       env=dict(_ENV, MQ_STUB_DUMP_REFS=str(dump), MQ_DRIVER_TIMING="1"))
    assert r.returncode == 0 and "lines joined on the device" in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    assert (dump / "0.seq").read_bytes() == b"ACGTAC" and (dump / "1.seq").read_bytes() == b"GGTT"
    for extra in ([], ["--low-memory"]):
        sub = tmp_path / ("w80" + "".join(extra))
        sub.mkdir()
        _run_and_compare(built[san], reads, sub, "w80", records, extra)


@pytest.mark.parametrize("san", ["asan", "tsan"])
@pytest.mark.parametrize("where", ["inside", "first_byte", "cr_last_byte", "nl_last_byte"])
def test_crlf_header_across_a_block_border(built, tmp_path, san, where):
    """CR-LF line ends, and the second record's header line at the border of the streamer's first and second 16-MB block: the header
    straddles it; its '>' is the second block's first byte; its '\\r' is the first block's last byte and its '\\n' the second's first;
    its '\\n' is the first block's last byte (the sequence opens the second block)."""
    rng = np.random.default_rng(2)
    nl = b"\r\n"
    h1, h2 = b"chrA the first one", b"chrB a header line that lies on the border of two blocks"
    start2 = {"inside": BLOCK - 10,                       # the header line straddles the border
              "first_byte": BLOCK,
              "cr_last_byte": BLOCK - 1 - (1 + len(h2)),  # '>' + h2 + '\r' end at BLOCK - 1, the '\n' is at BLOCK
              "nl_last_byte": BLOCK - 1 - (2 + len(h2))}[where]  # ... the '\n' at BLOCK - 1
    body = start2 - (1 + len(h1) + 2)  # bytes of record 1's region: lines of 60 + CR-LF, the last line whatever is left
    full, rem = divmod(body, 62)
    if 0 < rem < 3:  # the last line needs a base in front of its CR-LF: take it from the line before
        full, rem = full - 1, rem + 62
    n1 = full * 60 + (rem - 2 if rem else 0)
    a = _bases(rng, n1)
    region1 = _wrap(a[:full * 60], 60, nl) + (a[full * 60:] + nl if rem else b"")
    assert len(region1) == body
    b = _bases(rng, 700_001)
    records = [(h1, nl, region1), (h2, nl, _wrap(b, 60, nl)), (b"chrC", nl, _wrap(_bases(rng, 90), 60, nl)[:-1])]  # (the file ends in a bare '\r')
    _run_and_compare(built[san], _reads(tmp_path), tmp_path, where, records)


def test_junk_in_front_of_the_first_record_is_the_loader_s_error(built, tmp_path):
    junk = tmp_path / "junk.fa"
    junk.write_bytes(b"this is not FASTA\n>a\nACGT\n")
    # (an error exit of the driver leaves its stream slots to the operating system, with the flag and without: no leak check here)
    env = dict(_ENV, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0")
    r = subprocess.run([built["asan"], _reads(tmp_path), "--reference", str(junk), "-p", str(tmp_path / "j"), "--ref-join", "device"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 101 and "malformed FASTA record" in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    r = subprocess.run([built["asan"], _reads(tmp_path), "--reference", str(junk), "-p", str(tmp_path / "j"), "--ref-join", "sideways"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 2 and "--ref-join wants device or host" in r.stderr


def test_the_seam_names_both_functions():
    import mapquik_amd
    hdr = open(os.path.join(ROOT, "include", "mapquik_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    diag = open(os.path.join(ROOT, "include", "mapquik_hip_diag.h")).read()
    for name in ("mq_index_add_ref_staged_lines", "mq_index_staged_sequence"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert "pub fn %s(" % name in integ, name
        assert name in mapquik_amd.api.EXPORTS, name
        assert name not in diag
    assert "#define MQ_ABI_VERSION 4" in hdr
    assert callable(mapquik_amd.Index.add_ref_staged_lines) and callable(mapquik_amd.Index.staged_sequence)
