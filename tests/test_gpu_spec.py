"""GPU: the map kernel pair compiled for its parameters (SpecFixed, mq_device.hpp; MAP_SPECS, mq_host_state.hpp) against the pair that
reads them at run time (SpecNone, forced by MQ_NO_SPEC=1).  Both must write BYTE-identical mq_hit records.

One batch per parameter set, mapped in two fresh child processes (this file run as a script: one with MQ_NO_SPEC=1, one without), each
through both entry forms -- mq_map_batch_device on device-resident reads and the host-buffer mq_ctx_submit / mq_ctx_wait -- into
0xFF-filled result buffers.  The parent compares the four buffers byte by byte, checks every status, and compares status, the eight
numeric PAF columns and the k-min-mer count with the CPU oracle's.  Which pair ran comes from mqdiag_last_map_spec (0: SpecNone), which
seeding path from mq_last_map_path_counts.

Reads: a few hundred simulated reads plus the shapes at which a constant k, l, use_hpc or fold could go wrong (lattice.py's constructors):
l+k-2, l+k-1, l+k bases; compressed length l-1, l, l+1; one and two tiles of 12,288 raw bases +-1 (the carry of l-1 codes); minimizer lists
of k-1, k, 64*6+k-1 and 64*6+k entries (the map phase's chunk with its k-1 shared entries); a read with an N (map_declined_kernel); a
homopolymer-only read; and, with case folding, lower-case reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COLUMNS = ("ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score")
# (name, oracle / index parameters, fold_case, fast_kh, the spec id the launch must report without MQ_NO_SPEC)
SETS = (("k5_l31", dict(), False, False, 1),
        ("k7_l31", dict(k=7), False, False, 2),
        ("k5_l31_fold", dict(), True, False, 3),
        ("k5_l30", dict(l=30), False, False, 0),
        ("k8_l31", dict(k=8), False, False, 0),
        ("k5_l31_fast_kh", dict(), False, True, 0))
N_SIM = 300


def _points(L, O, simlib, world, ps, fold):
    """the batch of one parameter set: (name, sequence) points"""
    g, off, names = world
    po = O.params(**ps)
    k, l = po.k, po.l
    rng = np.random.default_rng(1000 * k + l)
    reads = simlib.make_reads(g, off, N_SIM, seed=7 + k, len_mean=3000, len_sd=1500, len_min=20, len_max=9000)
    b, o = reads["bases"], reads["offsets"]
    pts = [("sim %d" % i, b[int(o[i]):int(o[i + 1])].tobytes()) for i in range(N_SIM)]
    pts += [("len=%d" % n, L._cut(g, rng, n)) for n in (l + k - 2, l + k - 1, l + k)]
    for c in (l - 1, l, l + 1):   # compressed length c in 2 c + 1 raw bases (above l + k - 1, so the read is seeded)
        hd = L.heads(rng, c, 0, 0)
        seq = b"".join(bytes([hd[i]]) * (3 if i == 0 else 2) for i in range(c))
        assert L.compressed_length(seq) == c and len(seq) >= l + k - 1
        pts.append(("compressed length %d" % c, seq))
    pts += [("len=%d" % n, L._cut(g, rng, n)) for t in (1, 2) for n in (t * L.SD_TILE_RAW - 1, t * L.SD_TILE_RAW, t * L.SD_TILE_RAW + 1)]
    km1 = O.kminmers(g, O.params(**{**ps, "k": 1}))
    for N in (k - 1, k, L.CHUNK_KMM + k - 1, L.CHUNK_KMM + k):
        pts.append(("N=%d minimizers" % N, L.read_with_minimizers(O, g, ps, N, km1=km1)[0]))
    s = bytearray(L._cut(g, rng, 6000))
    s[2500] = ord("N")
    pts.append(("a read with an N", bytes(s)))
    pts.append(("homopolymer only", b"A" * 500))
    if fold:   # lower case: a whole read, the second half of one, single bases of one (each a copy of a simulated read, which stays in the batch)
        pts.append(("lower case", pts[3][1].lower()))
        h = pts[4][1]
        pts.append(("lower-case half", h[:len(h) // 2] + h[len(h) // 2:].lower()))
        a = bytearray(pts[5][1])
        for i in range(0, len(a), 7):
            a[i] = ord(chr(a[i]).lower())
        pts.append(("lower-case bases", bytes(a)))
        n = bytearray(pts[6][1].lower())
        n[len(n) // 2] = ord("n")
        pts.append(("lower case with an n", bytes(n)))
    return pts


def child(path_in, path_out):
    """every parameter set of path_in through both entry forms; the records as they came back, the spec ids and the path counts"""
    import ctypes as C
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(HERE))
    import mapquik_amd as mq
    from hipmem import DevBuf, device_sync, memset
    d = np.load(path_in)
    out = {}
    for name, ps, fold, fast_kh, _ in SETS:
        bases, offs, g = d[name + "/bases"], d[name + "/offs"], d["genome"]
        ix = mq.Index(mq.Params(fold_case=fold, fast_kh=fast_kh, **ps))
        ix.add_ref(0, "ref0", g)
        ix.finalize()
        n = offs.size - 1
        db, do, dh = DevBuf.from_numpy(bases), DevBuf.from_numpy(offs), DevBuf(n * mq.hit_dtype.itemsize)
        memset(dh, 0xFF)
        ix.reserve(n, int(offs[-1]))
        ix.map_batch_device(db.ptr, do.ptr, n, int(offs[-1]), dh.ptr)
        device_sync()
        out[name + "/device"] = dh.to_numpy(mq.hit_dtype, n)
        out[name + "/device_spec"] = np.array([ix.last_map_spec()])
        out[name + "/paths"] = np.array(ix.last_map_path_counts())
        ctx = ix.context()
        hh = np.frombuffer(b"\xff" * (n * mq.hit_dtype.itemsize), dtype=mq.hit_dtype).copy()
        vp = C.c_void_p
        assert ctx._L.mq_ctx_submit(ctx._h, vp(bases.ctypes.data), vp(offs.ctypes.data), n, vp(hh.ctypes.data)) == 0
        assert ctx._L.mq_ctx_wait(ctx._h) == 0
        out[name + "/host"] = hh
        out[name + "/host_spec"] = np.array([ctx.last_map_spec()])
        ctx.close()
        for x in (db, do, dh):
            x.free()
        ix.close()
    np.savez(path_out, **out)


@pytest.fixture(scope="module")
def runs(oracle, simlib, tmp_path_factory):
    """the batches, the oracle's answers and the two children's records, computed once"""
    import lattice as L
    tmp = tmp_path_factory.mktemp("spec")
    world = simlib.make_genome([300_000], seed=4242)
    g = world[0]
    data, want = {"genome": g}, {}
    for name, ps, fold, _, _ in SETS:
        pts = _points(L, oracle, simlib, world, ps, fold)
        bases, offs = L.batch(pts)
        po = oracle.params(**ps)
        ox = oracle.Index()
        ox.add_ref(0, "ref0", g, po)
        ub = np.frombuffer(bases.tobytes().upper(), dtype=np.uint8) if fold else bases   # the reference folds before it seeds (src/closures.rs:63,106)
        want[name] = (pts, po, ox.map_batch_diag(ub, offs, po, threads=8))
        data[name + "/bases"], data[name + "/offs"] = bases, offs
    path_in = str(tmp / "in.npz")
    np.savez(path_in, **data)
    got = {}
    for tag, env in (("spec", {}), ("none", {"MQ_NO_SPEC": "1"})):
        e = {k: v for k, v in os.environ.items() if k != "MQ_NO_SPEC"}
        e.update(env)
        path_out = str(tmp / (tag + ".npz"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), path_in, path_out], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-4000:])
        got[tag] = dict(np.load(path_out))
    return want, got


@pytest.mark.parametrize("name", [s[0] for s in SETS])
def test_spec_pair_writes_the_same_records(runs, name):
    import mapquik_amd as mq
    want, got = runs
    pts, po, (w, diag) = want[name]
    spec_id = [s[4] for s in SETS if s[0] == name][0]
    a, b = got["spec"], got["none"]
    # which pair ran, which seeding path the reads took
    assert int(a[name + "/device_spec"][0]) == spec_id and int(a[name + "/host_spec"][0]) == spec_id, (a[name + "/device_spec"], a[name + "/host_spec"])
    assert int(b[name + "/device_spec"][0]) == 0 and int(b[name + "/host_spec"][0]) == 0
    seeded = [s for _, s in pts if len(s) >= po.l + po.k - 1]
    ok = b"ACGTacgt" if "fold" in name else b"ACGT"
    n_general = sum(1 for s in seeded if any(c not in ok for c in set(s)))
    assert n_general == (2 if "fold" in name else 1)
    for r in (a, b):
        assert tuple(r[name + "/paths"]) == (len(seeded) - n_general, n_general), (name, r[name + "/paths"])
    # byte-equal records: spec against none, device form against host form
    ref = a[name + "/device"]
    for r, form in ((a, "host"), (b, "device"), (b, "host")):
        assert r[name + "/" + form].tobytes() == ref.tobytes(), (name, form, np.flatnonzero(r[name + "/" + form] != ref)[:10])
    assert set(np.unique(ref["status"]).tolist()) <= {0, 1, 2}, np.unique(ref["status"])
    # ... and they are the oracle's
    assert np.array_equal(ref["n_kminmers"].astype(np.uint64), diag["n_kminmers"].astype(np.uint64))
    m = w["mapped"] != 0
    assert np.array_equal(ref["status"] == 1, m) and m.sum() > N_SIM // 2
    for f in COLUMNS:
        assert np.array_equal(mq.hit_column(ref, f)[m], w[f][m].astype(np.uint64)), (name, f)
    short = np.array([len(s) < po.l + po.k - 1 for _, s in pts])
    assert short.any() and (ref["status"][short] == 0).all() and (ref["n_kminmers"][short] == 0).all()


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
