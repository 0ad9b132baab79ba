"""GPU: the per-read timing of the instrumented launch (mq_map_probe_stats, then mq_last_read_cycles).  map_kernel leaves every read's
cycles and the tick at which its wave took it up; map_declined_kernel overwrites both for a read the fast seeder declined: its cycles
there, and in the tick's place bit 63 plus the seeding split in units of 256 cycles -- stretch finder | fast seeder << 21 | general
seeder << 42 (decoded by tools/read_tail.py).  The counters of the same launch go with it: fast / general reads, lookups."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_READS = 64
DECLINED = (3, 9, 17, 22, 38, 41, 55, 63)  # these reads carry a run of 100 N: the fast seeder declines them
UNIT = 256  # cycles per unit of a declined read's three packed fields
F21 = (1 << 21) - 1


@pytest.fixture(scope="module")
def mq():
    import mapquik_amd
    if mapquik_amd.device_count() <= 0:
        pytest.fail("no HIP device visible: GPU tests must run on the GPU box")
    return mapquik_amd


def test_read_cycles_of_an_instrumented_launch(mq, simlib):
    from hipmem import DevBuf
    g, off, names = simlib.make_genome([200_000], seed=31)
    reads = simlib.make_reads(g, off, N_READS, seed=8, len_mean=2500, len_sd=200, len_min=2100, len_max=2900)  # (the simulated errors move a length by a few bases)
    bases, offs = np.array(reads["bases"], dtype=np.uint8), np.ascontiguousarray(reads["offsets"], dtype=np.uint64)
    lens = np.diff(offs).astype(np.int64)
    assert offs.size == N_READS + 1 and lens.min() >= 2000 and lens.max() <= 3000
    for r in DECLINED:
        at = int(offs[r]) + int(lens[r]) // 2
        bases[at:at + 100] = ord("N")
    ix = mq.Index(mq.Params())
    ix.add_ref(0, names[0], g)
    ix.finalize()
    d_b, d_o, d_h = DevBuf.from_numpy(bases), DevBuf.from_numpy(offs), DevBuf(N_READS * 48)
    lookups, extra = ix.probe_stats(d_b.ptr, d_o.ptr, N_READS, int(offs[-1] - offs[0]), d_h.ptr)
    cyc, start = ix.last_read_cycles(N_READS)
    hits = d_h.to_numpy(mq.hit_dtype, N_READS)
    n_fast, n_general = ix.last_map_path_counts()
    ix.close()

    assert np.all(cyc != 0) and np.all(cyc < 0xFFFFFFFF), cyc
    declined = (start >> np.uint64(63)) != 0
    assert sorted(np.flatnonzero(declined).tolist()) == sorted(DECLINED)
    for r in DECLINED:
        w = int(start[r])
        fields = [w & F21, (w >> 21) & F21, (w >> 42) & F21]
        assert sum(fields) * UNIT <= int(cyc[r]) + len(fields) * UNIT, (r, fields, int(cyc[r]))
    assert np.all(start[~declined] != 0)  # plain timestamps: bit 63 clear (not declined), and a clock that has been running
    assert (n_fast, n_general) == (N_READS - len(DECLINED), len(DECLINED))
    assert lookups == int(hits["n_kminmers"].astype(np.uint64).sum()) and lookups > 0
