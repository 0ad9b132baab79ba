"""GPU: the device-resident entry points (mq_map_batch_device, mq_ctx_map_batch_device, mq_map_probe_stats, the redo arena) and the index's
staging buffer at the edges of their contract that no other module reaches: d_offsets[0] other than 0, reads across and behind 2^32 and
2^33 of the caller's buffer, a d_bases that is not 64-byte aligned, a read of 2^32 bases or more, reference records staged behind 4 GiB.
The cases are tests/offset_cases.py's (proved on the CPU by tests/test_offset_cases.py).  The expected records throughout are those of
the same batch at first offset 0, which the fixture `base` ties to the host-buffer form (byte for byte) and to the CPU oracle (status, the
eight PAF columns, n_kminmers).  Every hit buffer is filled with 0xFF before each call; the bytes in front of a shifted batch, inside a
read past the length limit and between the staged records are never written.  A failed hipMalloc fails its test (the largest case takes
about 20 GB: 8.6 GB of bases, and the minimizer lists that total_bases sizes for the index's default context and for a Context).

What each family guards (mapquik_amd/csrc), i.e. what would have to be wrong for it to fail:
  1 shifted first offset    mq_map_kernels.hpp: order_reads_kernel packing o0 into two words of the work descriptor; take_now and the
                            hand-over in map_kernel's loop rebuilding o0 from d.x | d.y << 32 (twice); list_region(A, o0 - o_base, ...) placing
                            a read's list relative to A.offsets[0] (a list placed by o0 itself lies beyond the lists' allocation at S >= 2^32);
                            A.bases + o0 in 64 bits; map_declined_kernel's own o_base / o0 for the read with an N
  2 skewed base pointer     the seeders' 16-byte loads through uint4_unaligned, order_reads_kernel's win() rounding the OFFSET, not the address
  3 every kernel pair       the same arithmetic in seed_reads_kernel, seed_general_kernel and map_lists_kernel (MQ_PIPELINE=split), the
                            chunk-4, SpecNone and seeding-variant instantiations of map_kernel / map_declined_kernel, mz_last's regions
  4 launch order            order_reads_kernel's win(): (o0 + at) & ~63 on 64 bits, the flagged reads' descriptors in front of the work array
  5 instrumented launch     the TIMING instantiations of the pair (mq_map_probe_stats), read_cycles / read_start indexed by read number
  6 redo arena              mq_redo.hpp: redo_collect_kernel's src[slot] = o0 (64 bits, absolute), redo_copy_kernel's bases + src[j] from an
                            odd address to a 64-aligned slot
  7 length limit            order_reads_kernel's WORK_TOO_LONG bit and map_kernel's `len >> 32` turning the read into LIST_OVERFLOW before a
                            byte of it is read; list_region for the reads behind it (o0 - o_base >= 2^32); redo_collect_kernel leaving it
                            (len > max_read_len); the host forms' checks in ctx_submit and mq_kminmers_batch (mq_capi_map.hpp)
  8 staged reference        mq_host_state.hpp StageState::piece / region at `at` >= 2^32; mq_capi_index.hpp join_lines_locked's tile count
                            and mq_join.hpp's 64-bit begin / end; seed_ref_kernel reading the staging buffer across 2^32

Each test prints "offsets timing <family>: <launches> launches <seconds> s" (allocations, copies and this module's Python included).
The first run on an MI355X (a record, not a bound; hipMalloc of 4 to 9 GB that nobody touches is not what costs): 4-6 ms for each S of
family 1 and each j of family 2, 9-10 ms for a configuration of family 3 (25 ms with seeding variant 16), 39 ms for family 4, 2 ms for
family 5, 36 ms for family 6, 12-15 ms for a length of family 7's device form and 6 ms for its host forms, 38 ms for family 8; the `base`
fixture 0.29 s; the module's 26 tests 1.0 s."""
import ctypes as C
import time

import hipmem
import numpy as np
import pytest

import offset_cases as K

pytestmark = pytest.mark.gpu

MQ_EINVAL = -1
MQ_HIT_OVERFLOW = 2
MATCH_PS = dict(k=3, l=15, density=0.03)  # the MQ_MATCH_CAP=1 recipe of test_gpu_device_redo.py


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


@pytest.fixture()
def O(oracle):
    yield oracle
    oracle.lib().mqo_set_variant(0)


@pytest.fixture(scope="module")
def b(simlib, oracle):
    return K.batch(simlib, oracle)


def _timing(family, n, t0):
    print("offsets timing %s: %d launches %.3f s" % (family, n, time.perf_counter() - t0))


def _index(mq, b, **kw):
    ix = mq.Index(mq.Params(**kw))
    ix.add_ref(0, b["gnames"][0], b["g"])
    ix.finalize()
    return ix


def _cmp(mq, hits, want, diag):
    """status, the eight PAF columns of the mapped reads and n_kminmers against the oracle's records"""
    m = want["mapped"] != 0
    assert np.array_equal(hits["status"] == 1, m)
    assert not (hits["status"] == MQ_HIT_OVERFLOW).any()
    for a in ("ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score"):
        assert np.array_equal(mq.hit_column(hits, a)[m], want[a][m].astype(np.uint64)), a
    assert np.array_equal(hits["n_kminmers"].astype(np.uint64), diag["n_kminmers"].astype(np.uint64))


class Placed:
    """A batch in caller-owned device memory, shifted by `shift` and skewed by `skew` (tests/offset_cases.py): an allocation of exactly
    skew + shift + bases.size bytes of which only the batch's own are written."""

    def __init__(self, mq, bases, offs, shift=0, skew=0):
        self.mq, self.n, self.total = mq, offs.size - 1, int(offs[-1] - offs[0])
        assert self.total == bases.size and int(offs[0]) == 0
        self.alloc = hipmem.DevBuf(skew + shift + bases.size)
        hipmem.copy_in(self.alloc, skew + shift, bases)
        self.d_bases = self.alloc.ptr + skew
        self.do = hipmem.DevBuf.from_numpy((offs.astype(object) + shift).astype(np.uint64))
        self.dout = hipmem.DevBuf(self.n * 48)

    def run(self, mapper):
        """poisons the hit array, maps through mapper.map_batch_device (an Index or a Context), returns the records"""
        hipmem.memset(self.dout, 0xFF)
        mapper.map_batch_device(self.d_bases, self.do.ptr, self.n, self.total, self.dout.ptr)
        hipmem.device_sync()
        return self.dout.to_numpy(self.mq.hit_dtype, self.n)

    def probe(self, ix):
        """... through the instrumented launch: (records, lookups, extra steps)"""
        hipmem.memset(self.dout, 0xFF)
        lookups, extra = ix.probe_stats(self.d_bases, self.do.ptr, self.n, self.total, self.dout.ptr)
        hipmem.device_sync()
        return self.dout.to_numpy(self.mq.hit_dtype, self.n), lookups, extra

    def free(self):
        for buf in (self.alloc, self.do, self.dout):
            buf.free()


@pytest.fixture(scope="module")
def base(mq, b):
    """The index at default parameters and the batch's records at first offset 0: the host-buffer form's, the device form's through the
    default context and through a Context -- byte for byte the same, and the oracle's column by column -- with the launch's path counts,
    spec id and order."""
    ix = _index(mq, b)
    host = ix.map_batch(b["bases"], b["offs"])
    _cmp(mq, host, b["want"], b["diag"])
    p0 = Placed(mq, b["bases"], b["offs"])
    dev = p0.run(ix)
    assert dev.tobytes() == host.tobytes()
    fx = dict(ix=ix, hits=dev, paths=ix.last_map_path_counts(), spec=ix.last_map_spec(), order=ix.last_map_order())
    n = len(b["names"])
    assert fx["paths"] == (n - 3, 1)  # all but the empty read and the one of l + k - 2 bases; the read with an N is the declined one
    assert fx["spec"] == 1            # default parameters: the pair compiled for them
    ctx = ix.context()
    assert p0.run(ctx).tobytes() == host.tobytes() and ctx.last_map_spec() == 1
    ctx.close()
    p0.free()
    yield fx
    ix.close()


def _same_launch(ix, fx):
    assert ix.last_map_path_counts() == fx["paths"]
    assert ix.last_map_spec() == fx["spec"]
    assert ix.last_map_order() == fx["order"]


@pytest.mark.parametrize("name", K.SHIFT_NAMES)
def test_shifted_first_offset(mq, b, base, name):
    """Families 1 and 4: the same bytes, path counts, spec id and (n_flagged, n_first) at every S, through both entry points."""
    t0 = time.perf_counter()
    s = K.shift_of(b, name)
    p = Placed(mq, b["bases"], b["offs"], shift=s)
    assert p.alloc.nbytes == s + b["bases"].size
    got = p.run(base["ix"])
    assert got.tobytes() == base["hits"].tobytes()
    _same_launch(base["ix"], base)
    ctx = base["ix"].context()
    assert p.run(ctx).tobytes() == base["hits"].tobytes() and ctx.last_map_spec() == base["spec"]
    ctx.close()
    p.free()
    _timing("1_shift_" + name, 2, t0)


@pytest.mark.parametrize("j", K.POINTER_SKEWS)
def test_skewed_base_pointer(mq, b, base, j):
    """Family 2: offsets as they are, d_bases = allocation + j."""
    t0 = time.perf_counter()
    p = Placed(mq, b["bases"], b["offs"], skew=j)
    assert p.d_bases % 64 == j  # (hipMalloc's allocations are at least 64-byte aligned)
    assert p.run(base["ix"]).tobytes() == base["hits"].tobytes()
    _same_launch(base["ix"], base)
    ctx = base["ix"].context()
    assert p.run(ctx).tobytes() == base["hits"].tobytes()
    ctx.close()
    p.free()
    _timing("2_skew_%d" % j, 2, t0)


@pytest.mark.parametrize("case", ["split", "chunk4", "nospec", "variant16", "fast_kh"])
def test_every_kernel_pair(mq, O, b, monkeypatch, case):
    """Family 3: a fresh index per configuration (the hooks are read at mq_index_new and at the index's first map call), the oracle
    switched alike; S = 63 and the straddling S against the same configuration at S = 0."""
    t0 = time.perf_counter()
    env = dict(split=("MQ_PIPELINE", "split"), chunk4=("MQ_CHAIN_CHUNK", "4"), nospec=("MQ_NO_SPEC", "1")).get(case)
    if env:
        monkeypatch.setenv(*env)
    variant, fast_kh = (16 if case == "variant16" else 0), case == "fast_kh"
    O.lib().mqo_set_variant(variant | (64 if fast_kh else 0))
    po, ox = O.params(), O.Index()
    ox.add_ref(0, b["gnames"][0], b["g"], po)
    want, diag = ox.map_batch_diag(b["bases"], b["offs"], po, threads=4)
    ix = _index(mq, b, seeding_variant=variant, fast_kh=fast_kh)
    host = ix.map_batch(b["bases"], b["offs"])
    _cmp(mq, host, want, diag)
    p0 = Placed(mq, b["bases"], b["offs"])
    dev0 = p0.run(ix)
    assert dev0.tobytes() == host.tobytes()
    paths, spec = ix.last_map_path_counts(), ix.last_map_spec()
    assert paths == (len(b["names"]) - 3, 1) and spec == 0  # (none of these configurations takes a compiled-for-its-parameters pair)
    p0.free()
    for s in (63, K.shift_of(b, "straddle_sim")):
        p = Placed(mq, b["bases"], b["offs"], shift=s)
        assert p.run(ix).tobytes() == dev0.tobytes(), s
        assert ix.last_map_path_counts() == paths and ix.last_map_spec() == spec
        p.free()
    ix.close()
    _timing("3_" + case, 3, t0)


def test_launch_order_with_the_tandem_reads_behind_4g(mq, b, base):
    """Family 4: the reads the ordering pass flags are the ones the restatement of its rule flags (the six tandem reads and the homopolymer
    read), all of them go first -- and the same with every one of them wholly behind 2^32 (the first beginning exactly there) and with
    one of them across it.  (Every S of family 1 asserts the pair as well.)"""
    t0 = time.perf_counter()
    want = int(K.flagged(b["bases"], b["offs"]).sum())
    assert base["order"] == (want, want) and want >= 6
    for s in (K.tandem_behind_shift(b), K.shift_of(b, "straddle_tandem")):
        assert int(K.flagged(b["bases"], b["offs"], s).sum()) == want
        p = Placed(mq, b["bases"], b["offs"], shift=s)
        assert p.run(base["ix"]).tobytes() == base["hits"].tobytes()
        assert base["ix"].last_map_order() == base["order"]
        p.free()
    _timing("4_order", 2, t0)


def test_instrumented_launch(mq, b, base):
    """Family 5: mq_map_probe_stats at S = 0 and with a read across 2^32."""
    t0 = time.perf_counter()
    ix, n = base["ix"], len(b["names"])
    lens = np.diff(b["offs"].astype(np.int64))
    seeded = lens >= b["l"] + b["k"] - 1
    res = []
    for s in (0, K.shift_of(b, "straddle_sim"), K.shift_of(b, "straddle_tandem")):
        p = Placed(mq, b["bases"], b["offs"], shift=s)
        hits, lookups, extra = p.probe(ix)
        cyc, start = ix.last_read_cycles(n)
        assert np.all(cyc[seeded] != 0), s
        assert ix.last_map_path_counts() == base["paths"]
        res.append((hits.tobytes(), lookups, extra))
        p.free()
    assert res[0][0] == base["hits"].tobytes()
    assert res[0][1] == int(base["hits"]["n_kminmers"].astype(np.uint64).sum()) and res[0][1] > 0
    assert res[1] == res[0] and res[2] == res[0]
    _timing("5_instrumented", 3, t0)


def test_redo_arena_at_a_shift(mq, O, simlib, monkeypatch):
    """Family 6: MQ_MATCH_CAP=1 -- nearly every read has more Match runs than its wave's window.  The first overflow read lies across 2^32,
    every other one behind it."""
    t0 = time.perf_counter()
    monkeypatch.setenv("MQ_MATCH_CAP", "1")
    g, off, names = simlib.make_genome([200000], seed=5, repeat_frac=0.3)
    reads = simlib.make_reads(g, off, 20, seed=2, len_mean=12000, err=0.03)
    bases, offs = reads["bases"], reads["offsets"]
    n = offs.size - 1
    po, ox = O.params(**MATCH_PS), O.Index()
    ix = mq.Index(mq.Params(**MATCH_PS))
    assert ix.add_ref(0, names[0], g) == ox.add_ref(0, names[0], g, po)
    assert ix.finalize() == ox.count()
    host = ix.map_batch(bases, offs)  # complete: its overflow reads are redone through the host
    want, diag = ox.map_batch_diag(bases, offs, po, threads=4)
    _cmp(mq, host, want, diag)
    p0 = Placed(mq, bases, offs)
    plain0 = p0.run(ix)
    over = plain0["status"] == MQ_HIT_OVERFLOW
    m = int(over.sum())
    assert m >= 2 and plain0[~over].tobytes() == host[~over].tobytes()
    first = int(np.flatnonzero(over)[0])
    s = K.straddle_shift(offs, first, residue=9)
    assert K.straddling(offs, s) == [first] and set(np.flatnonzero(over)[1:].tolist()) <= set(K.wholly_behind(offs, s))
    placed = [p0, Placed(mq, bases, offs, shift=s), Placed(mq, bases, offs, skew=3), Placed(mq, bases, offs, shift=s, skew=3)]
    # without an arena: the same reads come back MQ_HIT_OVERFLOW, the others are done
    for p in placed[1:]:
        assert p.run(ix).tobytes() == plain0.tobytes()
    lmax = int(np.diff(offs.astype(np.int64)).max())
    ix.reserve_redo(20, lmax)
    ctx = ix.context()
    ctx.reserve_redo(20, lmax)
    for p in placed:
        for mapper in (ix, ctx):
            raw = p.run(mapper)
            assert not (raw["status"] == MQ_HIT_OVERFLOW).any()
            assert raw.tobytes() == host.tobytes()
            assert mapper.redo_counts() == (m, 0)
    ctx.close()
    for p in placed:
        p.free()
    ix.close()
    _timing("6_redo", 3 + 8, t0)


@pytest.mark.parametrize("long_len", K.LONG_READS, ids=["2^32", "2^32+1", "2^33"])
def test_a_read_past_the_length_limit_device_form(mq, b, base, long_len):
    """Family 7: one read of long_len bytes in the middle of the batch, in an allocation that covers it and is never filled there.  That
    record comes back MQ_HIT_OVERFLOW, every other one as without it, the call returns 0; an arena leaves it (redo_counts: left)."""
    t0 = time.perf_counter()
    o, pieces = K.with_long_read(b, long_len)
    n1, total = o.size - 1, int(o[-1] - o[0])
    assert total == b["bases"].size + long_len
    alloc = hipmem.DevBuf(total)
    for at, piece in pieces:
        hipmem.copy_in(alloc, at, piece)
    do, dout = hipmem.DevBuf.from_numpy(o), hipmem.DevBuf(n1 * 48)
    ix = _index(mq, b)  # (an index of its own: the lists that total_bases sizes go with it)
    others = np.arange(n1) != K.LONG_AT

    def run(mapper):
        hipmem.memset(dout, 0xFF)
        mapper.map_batch_device(alloc.ptr, do.ptr, n1, total, dout.ptr)  # (raises unless the call returns 0)
        hipmem.device_sync()
        hits = dout.to_numpy(mq.hit_dtype, n1)
        assert hits["status"][K.LONG_AT] == MQ_HIT_OVERFLOW
        assert hits[others].tobytes() == base["hits"].tobytes()
        return hits

    run(ix)
    _same_launch(ix, base)  # the long read is seeded by neither seeder and is not looked at by the ordering pass
    ctx = ix.context()
    run(ctx)
    lmax = int(np.diff(b["offs"].astype(np.int64)).max())
    for mapper in (ix, ctx):
        mapper.reserve_redo(8, lmax)
        run(mapper)
        assert mapper.redo_counts() == (0, 1)
    ctx.close()
    ix.close()
    for buf in (alloc, do, dout):
        buf.free()
    _timing("7_long_%d" % long_len, 4, t0)


def test_a_read_past_the_length_limit_host_forms(mq, b, base):
    """Family 7, host forms: mq_map_batch, mq_ctx_submit and mq_kminmers_batch answer MQ_EINVAL for an offsets array that holds such a
    length -- before a byte is copied: the bases buffer has eight bytes -- and the context maps the ordinary batch afterwards."""
    t0 = time.perf_counter()
    L, ix = mq.load_library(), base["ix"]
    few = np.frombuffer(b"ACGTACGT", dtype=np.uint8).copy()
    ctx = ix.context()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for long_len in K.LONG_READS:
        offs = np.array([0, 4, 4 + long_len, 8 + long_len], dtype=np.uint64)
        out = np.zeros(3, dtype=mq.hit_dtype)
        assert L.mq_map_batch(ix.handle, p(few), p(offs), 3, p(out)) == MQ_EINVAL
        assert b"2^32" in L.mq_last_error()
        assert L.mq_ctx_submit(ctx._h, p(few), p(offs), 3, p(out)) == MQ_EINVAL
        assert L.mq_ctx_map_batch(ctx._h, p(few), p(offs), 3, p(out)) == MQ_EINVAL
        koff, counts = np.array([0, 4, 8, 12], dtype=np.uint64), np.zeros(3, dtype=np.uint32)
        kout = np.zeros(12, dtype=mq.kminmer_dtype)
        assert L.mq_kminmers_batch(ix.handle, p(few), p(offs), 3, p(koff), p(kout), p(counts)) == MQ_EINVAL
        assert not out.view(np.uint8).any() and not counts.any()
        assert L.mq_ctx_wait(ctx._h) == 0  # nothing was submitted
        assert ctx.map_batch(b["bases"], b["offs"]).tobytes() == base["hits"].tobytes()
    assert ix.map_batch(b["bases"], b["offs"]).tobytes() == base["hits"].tobytes()
    ctx.close()
    _timing("7_host_forms", 4, t0)


def test_staged_reference_behind_4g(mq, oracle, b):
    """Family 8: three records in a staging buffer of 2^32 + 3 MiB bytes -- one across 2^32, two behind it -- against add_ref on the joined
    sequences in a second index."""
    t0 = time.perf_counter()
    recs = K.staged_records(b["g"])
    po, ox = oracle.params(), oracle.Index()
    ix, ix2 = mq.Index(mq.Params()), mq.Index(mq.Params())
    ix.stage_begin(K.STAGE_BYTES)
    for _, at, region, _, _ in recs:
        ix.stage_piece(at, np.frombuffer(region, dtype=np.uint8))  # (pieces only where the records lie)
    for r, (name, at, region, seq, lines) in enumerate(recs):
        assert ix.staged_sequence(at, len(region)).tobytes() == seq == K.join_lines(region), name
        want_n = ix2.add_ref(r, name, np.frombuffer(seq, dtype=np.uint8))
        assert want_n == ox.add_ref(r, name, np.frombuffer(seq, dtype=np.uint8), po) and want_n > 100
        if lines:
            assert ix.add_ref_staged_lines(r, name, at, len(region)) == (want_n, len(seq)), name
        else:
            assert ix.add_ref_staged(r, name, at, len(region)) == want_n, name
        assert ix.ref_info(r) == ix2.ref_info(r) == (name, len(seq))
    assert ix.finalize() == ix2.finalize() == ox.count()
    assert ix.stats() == ix2.stats()
    want, diag = ox.map_batch_diag(b["bases"], b["offs"], po, threads=4)
    hits = ix.map_batch(b["bases"], b["offs"])
    assert hits.tobytes() == ix2.map_batch(b["bases"], b["offs"]).tobytes()
    _cmp(mq, hits, want, diag)
    assert (hits["status"] == 1).sum() >= 100 and set(hits["ref_id"][hits["status"] == 1].tolist()) == {0, 1, 2}
    ix.close()
    ix2.close()
    _timing("8_staged", 2, t0)
