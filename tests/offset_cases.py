"""Constructors for the device-form batches of tests/test_gpu_offsets.py: one batch of reads, and the places it is put at in device memory --
a first offset other than 0 (SHIFTS: the residues mod 64, a read across 2^32, everything behind 2^32 and 2^33), a base pointer that is not
64-byte aligned (POINTER_SKEWS), a read of 2^32 bases or more in the middle (LONG_READS), and reference records staged behind 4 GiB
(staged_records).  numpy only, deterministic; tests/test_offset_cases.py proves on the CPU that every case has the property it is named
after.

A device batch "shifted by S": an allocation of S + bases.size bytes, the bases copied to offset S, the offsets uploaded as offs + S,
d_bases = the allocation, total_bases = bases.size (= d_offsets[n] - d_offsets[0]).  The bytes in front of S are never written.
A batch "skewed by j": an allocation of j + bases.size bytes, the bases at j, the offsets as they are, d_bases = the allocation + j."""
import numpy as np

P32 = 1 << 32
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N_SIM = 200            # simulated reads: the first half in front of the named shapes, the second half behind them
TANDEM_PERIODS = (2, 3, 5, 7, 11, 16)
STRADDLE_SIM = "sim57"  # the simulated read that the shift "straddle_sim" lays across 2^32

# S by name, in the order of the issue: plain numbers, and two that depend on the batch (shift_of)
SHIFTS = (("1", 1), ("63", 63), ("64", 64), ("4096+17", 4096 + 17), ("straddle_sim", None), ("straddle_tandem", None), ("2^32", P32), ("2^32+1", P32 + 1),
          ("2^33+5", (1 << 33) + 5))
SHIFT_NAMES = tuple(n for n, _ in SHIFTS)
STRADDLE_RESIDUES = {"straddle_sim": 37, "straddle_tandem": 21}  # S mod 64 of the two (residues no plain shift has)
POINTER_SKEWS = (1, 3, 16, 63)
LONG_READS = (P32, P32 + 1, 1 << 33)  # lengths past the documented limit (len >> 32 != 0)
LONG_AT = N_SIM // 2                  # the long read goes in front of this read: the named shapes and half the simulated reads lie behind it


def world(simlib):
    """one 300-kb genome of uniform A C G T: (genome, contig offsets, names)"""
    return simlib.make_genome([300_000], seed=2024)


def periodic(win):
    """window_periodic of mq_map_kernels.hpp on 48 bases: some lag 1..16 matches in >= 27 of the first 32 positions (compared as the 2-bit
    codes (c >> 1) & 3, which are distinct for A C G T)"""
    c = (np.asarray(win, dtype=np.uint8) >> 1) & 3
    assert c.size == 48
    return any(int((c[:32] == c[lag:lag + 32]).sum()) >= 27 for lag in range(1, 17))


def windows(o0, ln):
    """order_reads_kernel's three windows of a read of ln >= 512 bases at offset o0 of its buffer: 48 bytes from a multiple of 64 of the OFFSET"""
    return [((o0 + at) // 64) * 64 for at in (ln // 6, ln // 2, (ln // 6) * 5)]


def flagged(bases, offs, shift=0):
    """the reads order_reads_kernel takes for short-period tandem arrays when the batch is shifted by `shift`"""
    out = np.zeros(offs.size - 1, dtype=bool)
    for r in range(offs.size - 1):
        o0, ln = int(offs[r]), int(offs[r + 1] - offs[r])
        if ln >= 512:
            out[r] = any(periodic(bases[w - shift:w - shift + 48]) for w in windows(o0 + shift, ln))
    return out


def batch(simlib, oracle):
    """The batch: dict(bases, offs, names, idx) -- names[r] of every read, idx[name] = r -- plus the genome (g, goff, gnames) and, from the
    oracle at default parameters, want (paf records) and diag (n_kminmers ...).  Order: sim0..sim99, the named shapes, sim100..sim199."""
    g, goff, gnames = world(simlib)
    po = oracle.params()
    l, k = int(po.l), int(po.k)
    rng = np.random.default_rng(77)
    sim = simlib.make_reads(g, goff, N_SIM, seed=9, len_mean=3000, len_sd=600, len_min=600, len_max=6000)
    so = sim["offsets"].astype(np.int64)

    def cut(n):
        a = int(rng.integers(0, g.size - n))
        return g[a:a + n].copy()

    named = [("short_l+k-2", cut(l + k - 2)), ("short_l+k-1", cut(l + k - 1)), ("short_l+k", cut(l + k)), ("empty", np.zeros(0, dtype=np.uint8))]
    with_n = cut(5001)
    with_n[2500] = ord("N")
    named.append(("with_N", with_n))
    named.append(("homopolymer", np.full(700, ord("A"), dtype=np.uint8)))
    named += [("len12287", cut(12287)), ("len12289", cut(12289))]
    for p in TANDEM_PERIODS:
        unit = ACGT[rng.integers(0, 4, p)]
        while np.all(unit == unit[0]):  # (a unit of one letter would be the homopolymer read again)
            unit = ACGT[rng.integers(0, 4, p)]
        ln = int(rng.integers(2000, 6001))
        named.append(("tandem%d" % p, np.tile(unit, ln // p + 1)[:ln].copy()))
    reads = [("sim%d" % i, sim["bases"][so[i]:so[i + 1]]) for i in range(N_SIM // 2)] + named + \
            [("sim%d" % i, sim["bases"][so[i]:so[i + 1]]) for i in range(N_SIM // 2, N_SIM)]
    names = [n for n, _ in reads]
    bases = np.concatenate([s for _, s in reads]).astype(np.uint8)
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([s.size for _, s in reads])
    ox = oracle.Index()
    ox.add_ref(0, gnames[0], g, po)
    want, diag = ox.map_batch_diag(bases, offs, po, threads=4)
    return dict(bases=bases, offs=offs, names=names, idx={n: r for r, n in enumerate(names)}, g=g, goff=goff, gnames=gnames, want=want, diag=diag, l=l, k=k)


def straddle_shift(offs, r, residue=None):
    """S = 2^32 - m with offs[r] + S < 2^32 < offs[r + 1] + S: 2^32 falls into the middle of read r (and S mod 64 == residue, if given)"""
    o0, o1 = int(offs[r]), int(offs[r + 1])
    assert o1 - o0 >= 256
    s = P32 - (o0 + (o1 - o0) // 2)
    if residue is not None:
        s -= (s - residue) % 64
    assert o0 + s < P32 < o1 + s
    return s


def shift_of(b, name):
    """the S of a SHIFTS entry for the batch b"""
    fixed = dict(SHIFTS)[name]
    if fixed is not None:
        return fixed
    r = b["idx"][STRADDLE_SIM if name == "straddle_sim" else "tandem7"]
    return straddle_shift(b["offs"], r, STRADDLE_RESIDUES[name])


def tandem_behind_shift(b):
    """S with the first tandem read beginning exactly at 2^32: every tandem read lies wholly behind 2^32, the reads in front of them do not"""
    return P32 - int(b["offs"][b["idx"]["tandem%d" % TANDEM_PERIODS[0]]])


def straddling(offs, shift):
    """the reads r with offs[r] + S < 2^32 < offs[r + 1] + S"""
    lo, hi = offs[:-1].astype(object) + shift, offs[1:].astype(object) + shift
    return [r for r in range(offs.size - 1) if lo[r] < P32 < hi[r]]


def wholly_behind(offs, shift):
    """the reads whose every byte lies at or behind 2^32 (reads of 0 bytes included when they lie there)"""
    return [r for r in range(offs.size - 1) if int(offs[r]) + shift >= P32]


def with_long_read(b, long_len, at=LONG_AT):
    """The batch with one more read of long_len bytes in front of read `at`: (offsets of the n + 1 reads, pieces) -- pieces: the
    (device offset, host bytes) copies that place every ordinary read; the long read's bytes are never written."""
    offs, bases = b["offs"], b["bases"]
    cut = int(offs[at])
    o = np.concatenate([offs[:at + 1], offs[at:] + np.uint64(long_len)]).astype(np.uint64)
    return o, [(0, bases[:cut]), (cut + long_len, bases[cut:])]


def join_lines(region):
    """mq_join.hpp's rule on the bytes between a header's line end and the next record: split at every '\\n', one trailing '\\r' cut from
    each piece (the last one, which has no '\\n', included), the pieces concatenated"""
    return b"".join(p[:-1] if p.endswith(b"\r") else p for p in bytes(region).split(b"\n"))


def wrap(seq, cols, nl, final=True):
    s = bytes(seq)
    return nl.join(s[i:i + cols] for i in range(0, len(s), cols)) + (nl if final else b"")


STAGE_BYTES = P32 + 3 * (1 << 20)


def staged_records(g):
    """Three references cut from the genome and where their records lie in a staging buffer of STAGE_BYTES bytes:
    [(name, at, region bytes, joined sequence, lines?)] -- a one-line record across 2^32, a 60-column record and an 80-column CRLF record
    whose last line has no line end, both behind 2^32."""
    a, b_, c = g[0:120_000], g[120_000:200_017], g[200_017:245_020]
    return [("one_line", P32 - 50_000, bytes(a), bytes(a), False),
            ("wrap60", P32 + (1 << 20) + 1, wrap(b_, 60, b"\n"), bytes(b_), True),
            ("wrap80_crlf_nofinal", P32 + 2 * (1 << 20) + 15, wrap(c, 80, b"\r\n", final=False), bytes(c), True)]
