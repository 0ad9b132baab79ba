"""Parameter sweep: every window length l = 1 .. 64 and every k = 1 .. 32 through both seeders, the index build and the map phase.  The
boundary lattice (lattice.py) pins the SIZE axis; this file is the PARAMETER axis: a given l or k selects code no other value runs
(window_hash's forms by l >> 2 and l & 3, the seed tables' rotations by l - 1, stage B's in-pointer at (s0 + l) mod 16, the 32-step frame
of seeding variant 4 for l > 32, the general seeder's l - 1 predecessors, kminmer_hash's fixed forms and their `decided` flag).
Constructors only (numpy + the oracle module, no GPU); test_param_sweep_cases.py proves on the CPU that every point has the property it
is named after, test_gpu_param_sweep.py compares the HIP path with the oracle on exactly these inputs.

A point is (name, sequence bytes).  Every constructor is deterministic; one that cannot build a point raises SweepError naming it.
"""
import numpy as np

import lattice as L

LS = tuple(range(1, 65))        # MAX_L = 64
KS = tuple(range(1, 33))        # MAX_K = 32
L_AXIS_K = 3                    # the k of the L axis
K_AXIS_LS = (14, 31)            # the l of the K axis: window_hash_q<3> with rem 2 (the reference's second pass), window_hash_fixed<31>
K_AXIS_DENSITY = 0.05
SEED = 77


class SweepError(L.LatticeError):
    """a constructor gave up on a point of the sweep"""


# ------------------------------------------------------------------ the density rule
# An l-mer of l <= 3 bases has 2, 10 or 32 canonical hashes, and a density picks whole l-mers: 0.05 selects none of them.  The values
# below keep some and not all (test_param_sweep_cases.py: at least 50 minimizers, fewer than windows, at every point).
#   64-bit hashes: l = 1: A and T hash to 0x2955... (0.161 * 2^64), C and G to 0x2032... (0.126 * 2^64): 0.14 keeps C and G only
#                  l = 2: 0.3;  l = 3: 0.6 (0.3 selects nothing)
#   32-bit hashes (seeding variant 4: the seeds' low halves): l = 1: A and T -> 0x4be24456 (0.296), C and G -> 0x62a02b4c (0.385): 0.3
#                  keeps A and T only;  l = 2 and l = 3: 0.3 keeps some l-mers and not all
DENSITY = 0.05
DENSITY_SHORT = {(1, False): 0.14, (2, False): 0.3, (3, False): 0.6, (1, True): 0.3, (2, True): 0.3, (3, True): 0.3}


def density(l, h32=False):
    return DENSITY_SHORT.get((l, bool(h32)), DENSITY)


def l_params(l, use_hpc, k=L_AXIS_K, h32=False):
    return dict(k=k, l=l, density=density(l, h32), use_hpc=bool(use_hpc))


def k_params(k, l):
    return dict(k=k, l=l, density=K_AXIS_DENSITY, use_hpc=True)


# ------------------------------------------------------------------ small tools
def compressed_length(seq, use_hpc):
    return L.compressed_length(seq) if use_hpc else len(seq)


def windows(seq, l, use_hpc):
    """l-mers of the (compressed) sequence"""
    return max(0, compressed_length(seq, use_hpc) - l + 1)


def lanes_chunk(seq, l, use_hpc):
    """stage B's lc = ceil(windows / 64) of a read of one tile (mq_seed.hpp, seed_stage_b)"""
    return -(-windows(seq, l, use_hpc) // 64)


_SEED64 = {65: 0x3c8bfbb395c60474, 67: 0x3193c18562a02b4c, 71: 0x20323ed082572324, 84: 0x295549f54be24456}


def window_hashes32(seq, l, use_hpc):
    """canonical ntHash of every window in 32-bit words (seeding variant 4: the seeds' low halves, rotations mod 32), in plain numpy: the
    oracle lists such hashes only behind the density test.  uint32 array, one per window."""
    s = np.frombuffer(seq, dtype=np.uint8)
    if use_hpc and s.size:
        keep = np.ones(s.size, dtype=bool)
        keep[1:] = s[1:] != s[:-1]
        s = s[keep]
    w = s.size - l + 1
    if w <= 0:
        return np.zeros(0, dtype=np.uint32)
    fw, rv = np.zeros(256, dtype=np.uint32), np.zeros(256, dtype=np.uint32)
    for c, v in _SEED64.items():
        fw[c] = v & 0xFFFFFFFF
        rv[int(L._COMP[c])] = v & 0xFFFFFFFF
    hf, hr = fw[s], rv[s]

    def rol(x, r):
        r &= 31
        return x if r == 0 else (x << np.uint32(r)) | (x >> np.uint32(32 - r))
    f, r = np.zeros(w, dtype=np.uint32), np.zeros(w, dtype=np.uint32)
    for j in range(l):
        f ^= rol(hf[j:j + w], l - 1 - j)
        r ^= rol(hr[j:j + w], j)
    return np.minimum(f, r)


def bound_ties(O, seq, ps, h32=False):
    """windows whose hash has the bound's high word: the fast seeder's stage B passes such a window on its high word and stage R's exact test
    may then fail it, which hands the whole read to the general seeder (mq_seed.hpp's header).  64-bit: oracle.minimizers at density 1.0
    lists every window's hash, variant 0; 32-bit: the whole hash is the `high word` (the caller has set variant 4 for the bound)."""
    b = int(O.lib().mqo_density_bound(ps["density"]))
    if h32:
        return int((window_hashes32(seq, ps["l"], ps["use_hpc"]) == np.uint32(b)).sum())
    h = O.minimizers(seq, O.params(**dict(ps, density=1.0)))["hash"]
    return int(((h >> np.uint64(32)) == np.uint64(b >> 32)).sum())


# ------------------------------------------------------------------ L axis: one batch for every l
LC_STRETCH = 3000               # the two reads below a super-row are prefixes of stretches of this length
HP_RUN = 70                     # the homopolymer run: under compression l bases around it span more than 64 raw ones
HP_AT = 1500


def fixed_reads(g):
    """the reads of the L-axis batch that do not depend on l, and the stretches the others are cut from (ACGT only, from lattice.world)"""
    rng = np.random.default_rng(SEED)
    hp, _ = L.plant_run(g, rng, HP_AT, HP_RUN, min_len=LC_STRETCH)
    return dict(tile=L._cut(g, rng, L.SD_TILE_RAW + L.SD_SR_RAW + 37),      # crosses the tile border: the carry of l - 1 codes
                two_tiles=L._cut(g, rng, 2 * L.SD_TILE_RAW + 1),
                odd=L._cut(g, rng, LC_STRETCH), even=L._cut(g, rng, LC_STRETCH),
                seam=L._cut(g, rng, max(LS) + max(KS)), hp=hp)


def lc_read(stretch, l, use_hpc, parity):
    """the longest prefix of the stretch whose window count w makes lc = ceil(w / 64) odd (parity 1) or even (parity 0), lc >= 1"""
    for n in range(len(stretch), 0, -1):
        lc = lanes_chunk(stretch[:n], l, use_hpc)
        if lc >= 1 and lc % 2 == parity:
            return stretch[:n]
    raise SweepError("no prefix with lc %s for l = %d hpc = %s" % ("odd" if parity else "even", l, use_hpc))


def l_axis_points(fx, l, use_hpc, k=L_AXIS_K):
    """the batch of one point of the L axis (and, with k, of the K axis): five reads that are the same at every l, two whose length sets lc's
    parity, three at the seam's lengths l + k - 2, l + k - 1, l + k"""
    pts = [("tile + super-row + 37", fx["tile"]), ("two tiles + 1", fx["two_tiles"]),
           ("lc odd", lc_read(fx["odd"], l, use_hpc, 1)), ("lc even", lc_read(fx["even"], l, use_hpc, 0))]
    pts += [("len=l+k%+d" % d, fx["seam"][:l + k + d]) for d in (-2, -1, 0)]
    pts.append(("run of %d in 3 kb" % HP_RUN, fx["hp"]))
    return pts


# ------------------------------------------------------------------ the declined batch (seed_read_hybrid)
DECLINED_LEN = 6500
DECLINED_N = (50 * L.BLOCK, 50 * L.BLOCK + 32)   # on a 64-byte block border of the read / in the middle of a block


def declined_points(g):
    """two reads with ONE N each and a clean stretch of at least HYB_MIN_CLEAN + 64 bytes on either side: the fast seeder takes both
    stretches as views, the general seeder the windows around the N and the last l - 1 run heads of the first stretch"""
    rng = np.random.default_rng(SEED + 1)
    pts = []
    for at in DECLINED_N:
        s = bytearray(L._cut(g, rng, DECLINED_LEN))
        s[at] = ord("N")
        pts.append(("N at %d" % at, bytes(s)))
    return pts


def clean_sides(seq):
    """whole 64-byte blocks of A C G T in front of and behind the read's one N, in bytes"""
    at = seq.index(b"N")
    return L.clean_blocks(0, at), L.clean_blocks(at + 1, len(seq) - at - 1)


# ------------------------------------------------------------------ K axis: tuples that equal their reverse, tuples decided late
PAL_HALF = 1500                 # bases of s at the most
PAL_TRIES = 60                  # (seed, length, middle base) combinations tried per (k, l)
DEEP_TRIES = 3000               # substitutions tried per (k, l)


def tuple_decisions(h, k):
    """for every k-tuple of the hash list h: the first pair (i, k - 1 - i), i < k / 2, whose elements differ; k / 2 (integer) where none does,
    i.e. the tuple equals its reverse.  int array, one per tuple."""
    h = np.asarray(h, dtype=np.uint64)
    n = h.size - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    half = k // 2
    if half == 0:
        return np.zeros(n, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(h, k)
    ne = win[:, :half] != win[:, ::-1][:, :half]
    return np.where(ne.any(axis=1), ne.argmax(axis=1), half)


def palindromic_tuples(h, k):
    return np.flatnonzero(tuple_decisions(h, k) == k // 2)


def deep_tuples(h, k):
    """tuples whose first differing pair is the innermost one, i = k / 2 - 1 (k >= 4: at k = 2 and 3 the innermost pair is pair 0)"""
    return np.flatnonzero(tuple_decisions(h, k) == k // 2 - 1) if k >= 4 else np.zeros(0, dtype=np.int64)


def _pal_candidates(g, k, l):
    """s + m + revcomp(s): canonical hashes and compression are strand-symmetric, so the minimizer list of s + revcomp(s) is its own reverse.
    Its compressed length is even, so at odd l it has an even number of windows in mirror pairs and an even number of minimizers: a k-tuple
    equal to its reverse then needs an even k.  One base m between the halves (neither s's last base nor its complement, so no run forms)
    breaks the symmetry for the l windows that hold it only; where exactly one of them is listed the count is odd and the list still its
    own reverse."""
    rng = np.random.default_rng(SEED * 1000 + 64 * k + l)
    for t in range(PAL_TRIES):
        n = PAL_HALF - 40 * (t % 8)
        s = L._cut(g, rng, n)
        mids = [b""] + [bytes([c]) for c in b"ACGT" if c != s[-1] and c != int(L._COMP[s[-1]])]
        yield s + mids[t % len(mids)] + L.revcomp(s)


def palindromic_read(O, g, k, l):
    """a read that holds a k-tuple of minimizer hashes equal to its reverse (rev = 0 under `<`, 1 under `<=`: seeding variant 32)"""
    po = O.params(**k_params(k, l))
    for seq in _pal_candidates(g, k, l):
        if palindromic_tuples(O.minimizers(seq, po)["hash"], k).size:
            return seq
    raise SweepError("no palindromic read for k = %d l = %d in %d tries" % (k, l, PAL_TRIES))


def deep_read(O, g, k, l):
    """the palindromic read with one base substituted behind its centre, such that some k-tuple's outer pairs are all equal and its innermost
    pair differs: kminmer_hash_fixed's `decided` flag is set by its last comparison, the loop form breaks out in its last round"""
    if k < 4:
        raise SweepError("k = %d has no pair inside pair 0" % k)
    po = O.params(**k_params(k, l))
    tries = 0
    for seq in _pal_candidates(g, k, l):
        if not palindromic_tuples(O.minimizers(seq, po)["hash"], k).size:
            continue
        mid = len(seq) // 2
        for p in range(mid + 1, min(len(seq), mid + 12 * l + 200)):
            for c in b"ACGT":
                if c == seq[p]:
                    continue
                s = seq[:p] + bytes([c]) + seq[p + 1:]
                tries += 1
                if deep_tuples(O.minimizers(s, po)["hash"], k).size:
                    return s
                if tries >= DEEP_TRIES:
                    raise SweepError("no deep-decision read for k = %d l = %d in %d tries" % (k, l, DEEP_TRIES))
    raise SweepError("no deep-decision read for k = %d l = %d: no palindromic read to start from" % (k, l))


def k_axis_points(O, g, fx, k, l):
    """the L-axis batch at (k, l) plus the two constructed reads"""
    pts = l_axis_points(fx, l, True, k=k) + [("palindromic", palindromic_read(O, g, k, l))]
    if k >= 4:
        pts.append(("deep decision", deep_read(O, g, k, l)))
    return pts


# ------------------------------------------------------------------ the reference of the build and map legs
REF_LEN = 2 * L.REF_SEG + L.REF_HALO + 123     # three segments of the index build
REF_AT = 100_000
MAP_READS = 12


def reference(g):
    return g[REF_AT:REF_AT + REF_LEN].tobytes()


def reference_with_n(ref, l):
    """an N l bases in front of the first segment border: that segment's view is declined and goes to the general seeder over [a, b)"""
    s = bytearray(ref)
    s[L.REF_SEG - l] = ord("N")
    return bytes(s)


def map_reads(ref):
    """12 reads of 2 - 6 kb cut from the reference, every second one reverse-complemented, four with 1 % substituted bases"""
    rng = np.random.default_rng(SEED + 2)
    pts = []
    for i in range(MAP_READS):
        n = int(rng.integers(2000, 6001))
        a = int(rng.integers(0, len(ref) - n))
        s = bytearray(ref[a:a + n])
        if i % 3 == 0:
            for p in rng.choice(n, size=n // 100, replace=False):
                s[p] = L._other(s[p])
        s = bytes(s)
        pts.append(("read %d at %d%s%s" % (i, a, " rc" if i % 2 else "", " 1%" if i % 3 == 0 else ""), L.revcomp(s) if i % 2 else s))
    return pts
