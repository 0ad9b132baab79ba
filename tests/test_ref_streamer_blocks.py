"""The reference streamer's block borders, all of them (no GPU): RefStreamer (host/ref_loader.hpp) takes its block size as an argument,
so a file of a few dozen bytes is streamed at EVERY block size from 1 to its size + 1 -- every byte of it is once a block's first and
once its last, every "\\r\\n" and every header line once lies across a border -- by the stand-alone feeder_dump under AddressSanitizer +
UBSan and under ThreadSanitizer (make asan tsan), 3 reader threads.  At every block size the records must be those of one block that
holds the whole file, and those must be what a model of the two record trackers' rules says (LineRecords: `refstream`, RegionRecords:
`refstream-lines`; the rules are quoted in their class comments)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "mapquik_amd", "lib")


@pytest.fixture(scope="module")
def built():
    r = subprocess.run(["make", "-C", ROOT, "asan", "tsan"], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        pytest.fail("make asan tsan failed:\n" + r.stderr[-2000:])
    return {k: os.path.join(LIB, "feeder_dump_" + k) for k in ("asan", "tsan")}


_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1",
            UBSAN_OPTIONS="print_stacktrace=1")

_THREE = [(b"chrA", b"ACGTACGTACGTACGTAC"), (b"b", b"GGCA"), (b"chrC", b"TTGACCAGTTGA")]


def _single(nl):
    return b"".join(b">" + h + nl + s + nl for h, s in _THREE)


def _wrapped(nl, w=7):
    return b"".join(b">" + h + nl + b"".join(s[i:i + w] + nl for i in range(0, len(s), w)) for h, s in _THREE)


INPUTS = {
    "lf": _single(b"\n"),
    "crlf": _single(b"\r\n"),
    "no_final_newline": _single(b"\n")[:-1],
    "ends_in_bare_cr": _single(b"\r\n")[:-1],
    "blank_lines": b"\n\r\n" + b">a\nACGT\n" + b"\r\n\n" + b">b\r\nGG\r\n" + b"\n\r\n",
    "empty_sequence_line": b">a\nACGT\n>e\n\n>c\nGG\n",
    "header_is_the_last_line": b">a\nACGT\n>b\n",
    "ends_inside_a_header_line": b">a\nACGT\n>bcd ef",
    "ends_inside_a_crlf_header_line": b">a\r\nACGT\r\n>bcd\r",
    "gt_inside_a_sequence_line": b">a\nAC>GT\n>b\nG>\n",
    "spaces_and_a_tab_in_the_header": b">id\twith tab  and spaces \nACGT\n> x\nGG\n",
    "junk_in_front": b"junk\n>a\nACGT\n",
    "cr_gt": b"\r>a\nAC\n",
    "empty": b"",
    "blank_only": b"\n\r\n\n",
    "wrapped_lf": _wrapped(b"\n"),
    "wrapped_crlf": _wrapped(b"\r\n"),
}
IRREGULAR = {"refstream": {"wrapped_lf", "wrapped_crlf", "header_is_the_last_line", "ends_inside_a_header_line",
                           "ends_inside_a_crlf_header_line", "junk_in_front", "cr_gt", "empty", "blank_only"},
             "refstream-lines": {"junk_in_front", "cr_gt", "empty", "blank_only"}}


def _id(header_line):
    """seq_io's id(): behind the '>' up to the first space (a TAB is part of it)"""
    return header_line[1:].split(b" ")[0]


def model_lines(data):
    """LineRecords: header line, sequence line, header line, ...; (id, offset of the sequence line, its length), or None: irregular.
    A line's '\\r' is cut in front of its '\\n' only: a last line without '\\n' keeps it (the streamer counts it into the sequence)."""
    recs, pos, hdr = [], 0, None
    parts = data.split(b"\n")
    for i, ln in enumerate(parts):
        last = i == len(parts) - 1
        if last and not ln:
            break  # nothing behind the last '\n'
        start, pos = pos, pos + len(ln) + 1
        body = ln[:-1] if not last and ln.endswith(b"\r") else ln
        if hdr is None:
            if not body:
                continue  # a blank line where a header may start: skipped
            if ln[:1] != b">":
                return None  # text before the first '>', a sequence that goes on over several lines
            hdr = body
        elif ln[:1] == b">":
            return None  # a header without its sequence line
        else:
            recs.append((_id(hdr), start, len(body)))
            hdr = None
    return recs if recs and hdr is None else None  # (a header as the last line; an empty or all-blank file)


def model_regions(data):
    """RegionRecords: a record is its header line and everything behind that line's '\\n' up to the next line that starts with '>';
    (id, offset of the region, its length), or None: irregular."""
    recs, pos = [], 0
    parts = data.split(b"\n")
    for i, ln in enumerate(parts):
        start, pos = pos, min(pos + len(ln) + 1, len(data))
        if ln[:1] == b">":
            if recs:
                recs[-1][2] = start - recs[-1][1]
            recs.append([_id(ln[:-1] if len(ln) > 1 and ln.endswith(b"\r") else ln), pos, len(data) - pos])
        elif not recs and ln.strip(b"\r"):
            return None  # text before the first '>' other than blank lines ("\r>a" is such text)
    return [tuple(r) for r in recs] or None  # (an empty or all-blank file)


MODELS = {"refstream": model_lines, "refstream-lines": model_regions}


def _parse(stdout):
    """{block size: None (irregular) or [(id, at, len)]} from the output of block size 0"""
    res, b = {}, None
    for ln in stdout.split(b"\n")[:-1]:
        if ln.startswith(b"block "):
            b = int(ln[6:])
            assert b not in res
            res[b] = []
        elif ln == b"irregular":
            assert res[b] == []
            res[b] = None
        else:
            f = ln.rsplit(b"\t", 2)
            res[b].append((f[0], int(f[1]), int(f[2])))
    return res


def test_the_models_know_the_expected_outcomes():
    for mode, model in MODELS.items():
        assert {name for name, data in INPUTS.items() if model(data) is None} == IRREGULAR[mode], mode
    assert model_lines(INPUTS["lf"]) == [(b"chrA", 6, 18), (b"b", 28, 4), (b"chrC", 39, 12)]
    assert model_lines(INPUTS["crlf"]) == [(b"chrA", 7, 18), (b"b", 31, 4), (b"chrC", 44, 12)]
    assert model_lines(INPUTS["spaces_and_a_tab_in_the_header"]) == [(b"id\twith", 26, 4), (b"", 35, 2)]
    w = INPUTS["wrapped_lf"]
    assert model_regions(w) == [(b"chrA", 6, w.index(b">b") - 6), (b"b", w.index(b">b") + 3, 5), (b"chrC", w.index(b">chrC") + 6, 14)]
    assert model_regions(INPUTS["ends_inside_a_crlf_header_line"]) == [(b"a", 4, 6), (b"bcd", 15, 0)]


@pytest.mark.parametrize("san", ["asan", "tsan"])
@pytest.mark.parametrize("mode", ["refstream", "refstream-lines"])
def test_every_block_size_gives_the_records_of_one_block(built, tmp_path, san, mode):
    for name, data in INPUTS.items():
        path = tmp_path / (name + ".fa")
        path.write_bytes(data)
        r = subprocess.run([built[san], str(path), mode, "0", "3"], capture_output=True, timeout=300, env=_ENV)
        bad = [w for w in (b"AddressSanitizer", b"ThreadSanitizer", b"LeakSanitizer", b"runtime error:") if w in r.stderr]
        assert not bad and r.returncode == 0, (name, r.returncode, r.stderr[-3000:])
        got = _parse(r.stdout)
        assert sorted(got) == list(range(1, len(data) + 2)), name
        whole = got[len(data) + 1]
        differ = {b: v for b, v in got.items() if v != whole}
        assert not differ, (name, mode, whole, sorted(differ.items())[:3])
        assert whole == MODELS[mode](data), (name, mode)
