"""GPU: the native driver with `--ref-join device` -- a line-wrapped reference FASTA streamed to the device like a single-line one, the
lines of every record joined there (mq_index_add_ref_staged_lines), never in host memory -- against the oracle and against the same
file run without the flag (host loader / chunked reader).  Reference behaviour: src/closures.rs:24-94 (the index phase reads the
file through seq_io, which joins the lines, and prints one line per record)."""
import itertools
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(oracle, simlib, tmp_path_factory):
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    from mapquik_amd import build
    exe = build.build_cli()
    wd = tmp_path_factory.mktemp("wrappedref")
    # records around the streamer's 16-MB blocks, and two that are (nearly) too short to be seeded
    g, off, names = simlib.make_genome([20_000_000, 17_000_000, 3_000_000, 40, 1200], seed=41, repeat_frac=0.05, threads=4)
    po = oracle.params()
    ox = oracle.Index()
    counts = [ox.add_ref(r, names[r], g[int(off[r]):int(off[r + 1])], po) for r in range(len(names))]
    reads = simlib.make_reads(g, off, 1500, seed=6, threads=4)
    rn = simlib.read_names(reads, names)
    want = ox.map_batch(reads["bases"], reads["offsets"], po, threads=4)
    want_txt = "".join(x + "\n" for x in oracle.paf_lines(ox, rn, want))
    rd = wd / "reads.fa"
    o = reads["offsets"]
    with open(rd, "wb") as f:
        for i, n in enumerate(rn):
            f.write(b">" + n.encode() + b"\n" + reads["bases"][int(o[i]):int(o[i + 1])].tobytes() + b"\n")
    return dict(exe=exe, wd=wd, g=g, off=off, names=names, counts=counts, unique=ox.count(), reads=str(rd), want_txt=want_txt)


def _write_ref(path, w, nl=b"\n", wrap=0, final=True, blank_between=False, wrap_from=0):
    g, off, names = w["g"], w["off"], w["names"]
    with open(path, "wb") as f:
        for r in range(len(names)):
            s = g[int(off[r]):int(off[r + 1])].tobytes()
            last = r + 1 == len(names)
            f.write(b">" + names[r].encode() + b" contig %d of the test genome" % r + nl)
            if wrap and r >= wrap_from:
                body = nl.join(s[i:i + wrap] for i in range(0, len(s), wrap))
            else:
                body = s
            f.write(body + (nl if final or not last else b""))
            if blank_between:
                f.write(nl + nl)


_runs = itertools.count()


def _run(w, ref, extra=(), env=None):
    prefix = str(w["wd"] / ("o%d" % next(_runs)))  # (a prefix of its own per run: no PAF of an earlier run is ever read)
    r = subprocess.run([w["exe"], w["reads"], "--reference", str(ref), "-p", prefix, "--threads", "3"] + list(extra), capture_output=True, text=True,
                       timeout=900, env=dict(os.environ, MQ_DRIVER_TIMING="1", **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return r, open(prefix + ".paf").read()


SHAPES = {"wrap80": dict(wrap=80), "wrap60_crlf": dict(wrap=60, nl=b"\r\n"), "wrapped_from_third": dict(wrap=70, wrap_from=2),
          "blank_between": dict(wrap=80, blank_between=True), "nofinal": dict(wrap=80, final=False), "plain": dict()}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_wrapped_reference_streamed_and_joined_on_the_device(world, shape):
    w = world
    ref = w["wd"] / ("ref_%s.fa" % shape)
    _write_ref(ref, w, **SHAPES[shape])
    want_lines = ["Indexed reference %s: %d k-min-mers." % (n, c) for n, c in zip(w["names"], w["counts"])]
    r0, paf0 = _run(w, ref)  # without the flag: the host loader joins the lines (a single-line file is streamed as it always was)
    assert "lines joined on the device" not in r0.stderr
    assert ("reference streamed" in r0.stderr) == (shape == "plain")
    for extra in ([], ["--low-memory"]):
        r, paf = _run(w, ref, extra=["--ref-join", "device"] + extra)
        assert "reference streamed: every record handed to ref_extract (lines joined on the device)" in r.stderr, r.stderr[-1500:]
        assert "host loader" not in r.stderr and "reference buffer page-locked" not in r.stderr
        assert [ln for ln in r.stdout.splitlines() if ln.startswith("Indexed reference ")] == want_lines
        assert "Indexed %d unique k-min-mers in " % w["unique"] in r.stdout
        assert paf == w["want_txt"] and len(paf) > 50000
        assert paf == paf0


def test_junk_and_save_index(world):
    w = world
    junk = w["wd"] / "ref_junk.fa"
    junk.write_bytes(b"this is not FASTA\n>a\nACGT\n")
    rr = subprocess.run([w["exe"], w["reads"], "--reference", str(junk), "-p", str(w["wd"] / "junk"), "--threads", "2", "--ref-join", "device"], capture_output=True,
                        text=True, timeout=600)
    assert rr.returncode == 101 and "malformed FASTA record" in rr.stderr
    # --save-index of an index built from joined records; --index maps against it
    ref = w["wd"] / "ref_save.fa"
    _write_ref(ref, w, wrap=60)
    ixf = str(w["wd"] / "wrapped.mqx")
    r, paf = _run(w, ref, extra=["--ref-join", "device", "--save-index", ixf])
    assert "lines joined on the device" in r.stderr and paf == w["want_txt"] and "Saved index to %s in " % ixf in r.stdout
    prefix = str(w["wd"] / "from_index")
    r2 = subprocess.run([w["exe"], w["reads"], "--index", ixf, "-p", prefix, "--threads", "3"], capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-2000:]
    assert open(prefix + ".paf").read() == w["want_txt"]
    assert "Loaded index %s: %d references, %d k-min-mers." % (ixf, len(w["names"]), sum(w["counts"])) in r2.stdout
