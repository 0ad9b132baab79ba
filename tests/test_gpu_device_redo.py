"""GPU: the device-resident entry points with a redo arena (mq_ctx_reserve_redo / mq_map_reserve_redo, include/mapquik_hip.h).  Without a
reservation mq_map_batch_device / mq_ctx_map_batch_device report MQ_HIT_OVERFLOW for a read with more Match runs than its wave's window or
with a minimizer list that fits neither its region nor the pool; with one, those reads are collected, copied into the arena, mapped with
worst-case regions and windows and written back, all behind the call's launch sequence on the caller's stream.  Every device output buffer
is filled with 0xFF before the call; the records are compared byte for byte with the host-buffer form's (which redoes its overflow reads
through the host) and column by column with the CPU oracle's."""
import ctypes as C

import hipmem
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MQ_ESTATE, MQ_EINVAL = -5, -1
MATCH_PS = dict(k=3, l=15, density=0.03)


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


def _index_both(mq, O, g, off, names, ps, variant=0, fast_kh=False):
    O.lib().mqo_set_variant(variant | (64 if fast_kh else 0))
    P, po = mq.Params(seeding_variant=variant, fast_kh=fast_kh, **ps), O.params(**ps)
    ix, ox = mq.Index(P), O.Index()
    for r in range(off.size - 1):
        s = g[int(off[r]):int(off[r + 1])]
        assert ix.add_ref(r, names[r], s) == ox.add_ref(r, names[r], s, po)
    assert ix.finalize() == ox.count()
    return ix, ox, po


def _cmp(mq, hits, want):
    assert np.array_equal(hits["status"] == 1, want["mapped"] != 0)
    m = want["mapped"] != 0
    for a in ("ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score"):
        assert np.array_equal(mq.hit_column(hits, a)[m], want[a][m].astype(np.uint64)), a


class DeviceBatch:
    """A batch in caller-owned device memory: the bases in an allocation of exactly bases.size bytes, the offsets, a hit array."""

    def __init__(self, mq, bases, offs):
        self.mq, self.n, self.total = mq, offs.size - 1, int(offs[-1] - offs[0])
        self.db = hipmem.DevBuf.from_numpy(bases)
        assert self.db.nbytes == bases.size
        self.do = hipmem.DevBuf.from_numpy(offs)
        self.dout = hipmem.DevBuf(self.n * 48)

    def launch(self, mapper, stream=0):
        """poisons the hit array and queues mapper.map_batch_device (an Index or a Context) on `stream`"""
        hipmem.memset(self.dout, 0xFF)
        mapper.map_batch_device(self.db.ptr, self.do.ptr, self.n, self.total, self.dout.ptr, stream)

    def hits(self):
        hipmem.device_sync()
        return self.dout.to_numpy(self.mq.hit_dtype, self.n)

    def run(self, mapper):
        self.launch(mapper)
        return self.hits()

    def free(self):
        for b in (self.db, self.do, self.dout):
            b.free()


def _assert_redone(raw, host):
    """no record left with status 2, none with a poisoned byte pattern, all equal to the host-buffer form's"""
    assert not (raw["status"] == 2).any()
    assert raw.tobytes() == host.tobytes()


@pytest.fixture(scope="module")
def matchcap(mq, oracle, simlib):
    """MQ_MATCH_CAP=1 (read when the index works out its launch geometry, at its first map call): 50 reads of which almost every one has more
    Match runs than the window.  The index, the oracle's answer, the host-buffer form's records (complete: redone through the host) and the
    device form's without a reservation, computed once."""
    mp = pytest.MonkeyPatch()
    mp.setenv("MQ_MATCH_CAP", "1")
    try:
        g, off, names = simlib.make_genome([200000], seed=5, repeat_frac=0.3)
        reads = simlib.make_reads(g, off, 50, seed=2, len_mean=12000, err=0.03)
        bases, offs = reads["bases"], reads["offsets"]
        ix, ox, po = _index_both(mq, oracle, g, off, names, MATCH_PS)
        host = ix.map_batch(bases, offs)
        want = ox.map_batch(bases, offs, po, threads=4)
    finally:
        mp.undo()
    _cmp(mq, host, want)
    dev = DeviceBatch(mq, bases, offs)
    plain = dev.run(ix)
    fx = dict(ix=ix, ox=ox, po=po, genome=(g, off, names), bases=bases, offs=offs, lens=(offs[1:] - offs[:-1]).astype(np.int64), host=host, want=want,
              dev=dev, plain=plain, over=plain["status"] == 2)
    yield fx
    dev.free()
    ix.close()


def test_match_window_overflow_is_redone_in_stream(mq, matchcap):
    """Case 1, through the index-level entry points (the default context)."""
    fx = matchcap
    ix, dev, over = fx["ix"], fx["dev"], fx["over"]
    assert over.any()  # the precondition: without a reservation status 2 leaves the library
    ok = ~over
    assert fx["plain"][ok].tobytes() == fx["host"][ok].tobytes()
    ix.reserve_redo(50, int(fx["lens"].max()))
    try:
        raw = dev.run(ix)
        _assert_redone(raw, fx["host"])
        _cmp(mq, raw, fx["want"])
        assert ix.redo_counts() == (int(over.sum()), 0)
    finally:
        ix.reserve_redo(0, 0)


def test_pool_exhaustion_is_redone_in_stream(mq, O, simlib, monkeypatch):
    """Case 2: lists so dense that the pool behind the list regions runs out.  Which reads find the pool empty depends on the order in which
    the waves arrive, so the arena has a slot for every read of the batch."""
    monkeypatch.setenv("MQ_LIST_F16", "1")
    g, off, names = simlib.make_genome([900000, 600000], seed=41, repeat_frac=0.1, tandem_frac=0.02)
    ix, ox, po = _index_both(mq, O, g, off, names, dict(k=3, l=14, density=0.5))
    reads = simlib.make_reads(g, off, 400, seed=6, len_mean=12000)
    bases, offs = reads["bases"], reads["offsets"]
    assert bases.size * 0.3 > (1 << 20)
    want = ox.map_batch(bases, offs, po, threads=4)
    host = ix.map_batch(bases, offs)
    _cmp(mq, host, want)
    dev = DeviceBatch(mq, bases, offs)
    over = dev.run(ix)["status"] == 2
    assert over.any() and not over.all()
    ix.reserve_redo(400, int((offs[1:] - offs[:-1]).max()))
    raw = dev.run(ix)
    _assert_redone(raw, host)
    _cmp(mq, raw, want)
    redone, left = ix.redo_counts()
    assert left == 0 and 0 < redone < 400
    dev.free()
    ix.close()


def test_arena_edges(mq, matchcap):
    """Case 3: one slot too few leaves exactly one read with status 2; one base too few leaves exactly the longest overflow reads."""
    fx = matchcap
    ix, dev, over, lens, host = fx["ix"], fx["dev"], fx["over"], fx["lens"], fx["host"]
    m, lmax = int(over.sum()), int(lens[over].max())
    assert m >= 2
    c = ix.context()
    c.reserve_redo(m, lmax)
    raw = dev.run(c)
    _assert_redone(raw, host)
    assert c.redo_counts() == (m, 0)
    c.reserve_redo(m - 1, lmax)
    raw = dev.run(c)
    left = raw["status"] == 2
    assert left.sum() == 1 and over[left].all()
    assert raw[~left].tobytes() == host[~left].tobytes()
    assert c.redo_counts() == (m - 1, 1)
    c.reserve_redo(m, lmax - 1)
    raw = dev.run(c)
    left = raw["status"] == 2
    longest = over & (lens == lmax)
    assert longest.any() and np.array_equal(left, longest)
    assert raw[~left].tobytes() == host[~left].tobytes()
    assert c.redo_counts() == (m - int(longest.sum()), int(longest.sum()))
    c.close()


def test_copy_kernel_residues(mq, O, matchcap, simlib, monkeypatch):
    """Case 4: the overflow reads begin at every residue mod 16 of the caller's buffer and have every length mod 16; the last read is an overflow
    read that ends at the last byte of an allocation of exactly that many bytes.  (120 reads of case 1's recipe: its 50 hold fewer than 16
    overflow reads.)"""
    monkeypatch.setenv("MQ_MATCH_CAP", "1")
    g, off, names = matchcap["genome"]
    ix, ox, po = _index_both(mq, O, g, off, names, MATCH_PS)
    uncut = simlib.make_reads(g, off, 120, seed=2, len_mean=12000, err=0.03)
    ub, uo = uncut["bases"], uncut["offsets"]
    n = uo.size - 1
    d0 = DeviceBatch(mq, ub, uo)
    guess = d0.run(ix)["status"] == 2  # which reads overflow before they are cut
    d0.free()
    order = list(range(n))
    order.append(order.pop(int(np.flatnonzero(guess)[-1])))  # an overflow read last
    # every read is cut at its end by 0..15 bases: the q-th overflow read to a length of residue q mod 16, every other read to a multiple of
    # 16 -- the overflow reads then begin at the residues of q (q - 1) / 2, which are all 16 within q <= 16
    seqs, q = [], 0
    for r in order:
        s = ub[int(uo[r]):int(uo[r + 1])]
        want = q % 16 if guess[r] else 0
        q += int(guess[r])
        seqs.append(s[:s.size - ((s.size - want) % 16)])
    assert q >= 17
    bases = np.concatenate(seqs)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([s.size for s in seqs])
    host = ix.map_batch(bases, offs)
    _cmp(mq, host, ox.map_batch(bases, offs, po, threads=4))
    dev = DeviceBatch(mq, bases, offs)
    over = dev.run(ix)["status"] == 2
    starts, lens = offs[:-1][over].astype(np.int64), (offs[1:] - offs[:-1])[over].astype(np.int64)
    assert set(int(x) for x in starts % 16) == set(range(16)) and set(int(x) for x in lens % 16) == set(range(16))
    assert over[-1] and int(offs[-1]) == bases.size == dev.db.nbytes
    ix.reserve_redo(n, int(lens.max()))
    raw = dev.run(ix)
    _assert_redone(raw, host)
    assert ix.redo_counts() == (int(over.sum()), 0)
    dev.free()
    ix.close()


def test_nothing_overflows(mq, O, simlib):
    """Case 5: default hooks.  The arena changes no record, and the launch diagnostics keep describing the batch's launch, not the arena's."""
    g, off, names = simlib.make_genome(simlib.ECOLI_LEN, seed=913)
    reads = simlib.make_reads(g, off, 300, seed=4)
    bases, offs = reads["bases"], reads["offsets"]
    ix, ox, po = _index_both(mq, O, g, off, names, dict())
    dev = DeviceBatch(mq, bases, offs)
    plain = dev.run(ix)
    assert not (plain["status"] == 2).any()
    paths, spec = ix.last_map_path_counts(), ix.last_map_spec()
    assert sum(paths) == 300
    ix.reserve_redo(64, 30000)
    raw = dev.run(ix)
    assert raw.tobytes() == plain.tobytes()
    _cmp(mq, raw, ox.map_batch(bases, offs, po, threads=4))
    assert ix.redo_counts() == (0, 0)
    assert ix.last_map_path_counts() == paths and ix.last_map_spec() == spec  # (the arena's 64 empty reads are seeded by neither seeder)
    assert ix.last_map_ms() > 0
    dev.free()
    ix.close()


@pytest.mark.parametrize("case", ["split", "chunk4", "nospec", "variant16", "fast_kh"])
def test_every_kernel_pair_redoes(mq, O, matchcap, monkeypatch, case):
    """Case 6: the redo goes through the launch sequence as it stands, whichever kernels it selects.  Case 1 at 20 reads, against the oracle
    switched alike."""
    fx = matchcap
    monkeypatch.setenv("MQ_MATCH_CAP", "1")
    env = dict(split=("MQ_PIPELINE", "split"), chunk4=("MQ_CHAIN_CHUNK", "4"), nospec=("MQ_NO_SPEC", "1")).get(case)
    if env:
        monkeypatch.setenv(*env)
    g, off, names = fx["genome"]
    offs = (fx["offs"][:21] - fx["offs"][0]).astype(np.uint64)
    bases = fx["bases"][int(fx["offs"][0]):int(fx["offs"][20])]
    ix, ox, po = _index_both(mq, O, g, off, names, MATCH_PS, variant=16 if case == "variant16" else 0, fast_kh=case == "fast_kh")
    host = ix.map_batch(bases, offs)
    want = ox.map_batch(bases, offs, po, threads=4)
    _cmp(mq, host, want)
    dev = DeviceBatch(mq, bases, offs)
    over = dev.run(ix)["status"] == 2
    assert over.any()
    ix.reserve_redo(20, int((offs[1:] - offs[:-1]).max()))
    raw = dev.run(ix)
    _assert_redone(raw, host)
    _cmp(mq, raw, want)
    assert ix.redo_counts() == (int(over.sum()), 0)
    dev.free()
    ix.close()


def test_two_contexts_with_arenas_in_flight_together(mq, matchcap):
    """Case 6, second half: two contexts of one index, each with its own arena and its own stream, queued before either is waited for."""
    fx = matchcap
    ix, host, over = fx["ix"], fx["host"], fx["over"]
    ctxs = [ix.context(), ix.context()]
    devs = [DeviceBatch(mq, fx["bases"], fx["offs"]) for _ in ctxs]
    streams = [hipmem.new_stream() for _ in ctxs]
    for c in ctxs:
        c.reserve_redo(50, int(fx["lens"].max()))
    for c, d, s in zip(ctxs, devs, streams):
        d.launch(c, s)
    for c, d, s in zip(ctxs, devs, streams):
        assert hipmem.hip().hipStreamSynchronize(s) == 0
        _assert_redone(d.hits(), host)
        assert c.redo_counts() == (int(over.sum()), 0)
    for c, d, s in zip(ctxs, devs, streams):
        c.close()
        d.free()
        hipmem.hip().hipStreamDestroy(s)


def test_states_and_errors(mq, matchcap, simlib):
    """Case 7."""
    fx = matchcap
    ix, dev, host = fx["ix"], fx["dev"], fx["host"]
    L = mq.load_library()
    c = ix.context()
    with pytest.raises(mq.MapquikError):
        c.redo_counts()  # no arena
    a, b = C.c_uint32(), C.c_uint32()
    assert L.mq_ctx_redo_counts(c._h, C.byref(a), C.byref(b)) == MQ_ESTATE
    # a submitted batch: MQ_ESTATE, and the context is as it was
    c.submit(fx["bases"], fx["offs"])
    assert L.mq_ctx_reserve_redo(c._h, 5, 100) == MQ_ESTATE
    assert c.wait().tobytes() == host.tobytes()
    # arguments
    assert L.mq_ctx_reserve_redo(c._h, 5, 0) == MQ_EINVAL
    assert L.mq_ctx_reserve_redo(c._h, (1 << 30) - 1, (1 << 32) - 1) == MQ_EINVAL
    assert (dev.run(c)["status"] == 2).any()  # ... none of which left an arena behind
    # two reservations of different sizes, one after the other
    lmax = int(fx["lens"].max())
    c.reserve_redo(7, 1000)
    assert c.redo_counts() == (0, 0)  # no device-form call yet
    c.reserve_redo(50, lmax)
    _assert_redone(dev.run(c), host)
    # off again: status 2 is back
    c.reserve_redo(0, 0)
    assert np.array_equal(dev.run(c)["status"] == 2, fx["over"])
    c.close()
    # free order with arenas: a context before its index, and an index whose default context holds one
    g, off, names = simlib.make_genome([50000], seed=3)
    ix2 = mq.Index(mq.Params())
    ix2.add_ref(0, names[0], g)
    ix2.finalize()
    c2 = ix2.context()
    c2.reserve_redo(4, 5000)
    ix2.reserve_redo(4, 5000)
    reads = simlib.make_reads(g, off, 8, seed=1, len_mean=3000)
    d2 = DeviceBatch(mq, reads["bases"], reads["offsets"])
    want2 = ix2.map_batch(reads["bases"], reads["offsets"])
    assert d2.run(c2).tobytes() == want2.tobytes() and d2.run(ix2).tobytes() == want2.tobytes()
    c2.close()
    ix2.close()
    d2.free()
