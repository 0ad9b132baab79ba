"""Boundary lattice for the seeders and for the list -> k-min-mer -> Match-run part of the map phase: inputs that sit ON the kernels'
compile-time sizes (and one element to either side), constructed by searching with the CPU oracle.  Constructors only (numpy + the
oracle module, no GPU); test_lattice_cases.py proves on the CPU that every point has the property it is named after, and
test_gpu_lattice.py compares the HIP path with the oracle on exactly these inputs.

A point is (name, sequence bytes).  Every constructor is deterministic; one that cannot build a point raises LatticeError naming it.
"""
import numpy as np

# ---- the sizes the lattice is about (all compile-time constants of the kernels; kept by hand, the headers are not parsed)
WORD = 16                      # mq_seed.hpp:165  load_piece, 16 raw bases per piece
BLOCK = 64                     # mq_seed.hpp:31   one lane's 64-base block (SD_BLOCKS, mq_seed.hpp:37)
SD_SR_RAW = 4096               # mq_seed.hpp:31   raw bases per super-row
SD_TILE_RAW = 12288            # mq_seed.hpp:36   raw bases per tile (the carry into the next one: l - 1 compressed bases)
SD_STEPS_FLAG = 32             # mq_seed.hpp stage B: one flag word per 32 steps
SD_STEPS_GROUP = 64            # mq_seed.hpp stage B: straight-line groups of 64 steps
SD_OWNER_CAP = 256             # mq_seed.hpp:54   stage R: candidates listed per round
GEN_LANE_BYTES = 16            # mq_seed_general.hpp:145 general seeder: 16 bytes per lane
GEN_STEP = 1024                # mq_seed_general.hpp:146 one step of the general seeder's walk
GEN_AHEAD = 2                  # mq_seed_general.hpp:138 steps in flight behind the current one
GEN_RING = 512                 # mq_seed_general.hpp:14  ring entries per wave
GEN_HASH_HEADS = 64            # mq_seed_general.hpp     hashing per 64 run heads
HYB_MIN_CLEAN = 2048           # mq_map_kernels.hpp:188 clean stretch of a declined read the fast seeder takes (whole 64-byte blocks)
LANE_BATCH = 64                # mq_map_kernels.hpp:383 k-min-mers of one lane-batch
ML_NB = 6                      # mq_map_kernels.hpp:382 lane-batches per chunk: a chunk is 64 * ML_NB + k - 1 minimizers, overlap k - 1
CHUNK_KMM = LANE_BATCH * ML_NB  # 384 k-min-mers per chunk
MAP_LDS_RECS = 48              # mq_probe.hpp:48   Match records kept in LDS
CHAIN_CH = 64                  # mq_chain.hpp:57   chain chunk (the CH of map_pair<CH, ...>, mq_host_state.hpp:473; MQ_CHAIN_CHUNK=4: 4)
REF_HALO = 2048                # mq_build_kernels.hpp:12
REF_SEG = 2 * SD_TILE_RAW - REF_HALO  # mq_build_kernels.hpp:13  22528
LIST_SLACK = 64                # mq_host_state.hpp:579 list region of a read: (len * f16 >> 16) + LIST_SLACK (list_region, mq_map_kernels.hpp:125)

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.zeros(256, dtype=np.uint8)
_COMP[[65, 67, 71, 84]] = [84, 71, 67, 65]


class LatticeError(AssertionError):
    """a constructor gave up on a lattice point"""


def world(sim, seed=4242):
    """the one random genome every family cuts its reads from (600 kb, no repeats): (genome, contig offsets, names)"""
    return sim.make_genome([600_000], seed=seed)


def batch(points):
    """(bases, offsets) of a list of points"""
    seqs = [p[1] for p in points]
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(s) for s in seqs])
    return bases, offs


def revcomp(seq):
    return _COMP[np.frombuffer(seq, dtype=np.uint8)[::-1]].tobytes()


def kminmers_or_none(O, seq, po):
    """oracle.kminmers with the seam's rule in front: a sequence below l + k - 1 bases has none (src/mers.rs:79)"""
    if len(seq) < po.l + po.k - 1:
        return np.zeros(0, dtype=O.kminmer_dtype)
    return O.kminmers(seq, po)


def _cut(g, rng, n):
    a = int(rng.integers(0, g.size - n)) if n < g.size else 0
    return g[a:a + n].tobytes()


def _other(*avoid):
    """a base that differs from every byte in `avoid`"""
    for c in b"ACGT":
        if c not in avoid:
            return c
    raise LatticeError("no base left")


# ------------------------------------------------------------------ A: raw lengths
A_BASES = (0, BLOCK, SD_SR_RAW, 2 * SD_SR_RAW, SD_TILE_RAW, SD_TILE_RAW + SD_SR_RAW, 2 * SD_TILE_RAW, 3 * SD_TILE_RAW)
A_LS = (2, 12, 31, 32, 33, 63, 64)
A_PARAMS = dict(k=3, density=0.05, use_hpc=False)        # + l
A_DENSE = dict(k=2, l=4, density=1.0, use_hpc=False)     # every window a candidate


def a_params(l):
    """density 0.05 gives a read of a tile's length a few minimizers -- except at l = 2, where it selects none of the 16 l-mers: 0.3 there"""
    return dict(A_PARAMS, l=l, density=0.3 if l == 2 else A_PARAMS["density"])


def length_offsets(l):
    d = set(range(-(l + 1), l + 2))
    for x in (15, 16, 17, 63, 64, 65):
        d.update((x, -x))
    return sorted(d)


def length_lattice(l, bases=A_BASES, offsets=None):
    """the lengths B + d of family A, negative ones dropped (offsets: the d, length_offsets(l) unless given)"""
    ds = length_offsets(l) if offsets is None else offsets
    return sorted({B + d for B in bases for d in ds if B + d >= 0})


def raw_length_points(g, l, bases=A_BASES, seed=1, offsets=None):
    rng = np.random.default_rng(seed * 1000 + l)
    return [("len=%d" % n, _cut(g, rng, n)) for n in length_lattice(l, bases, offsets)]


# ------------------------------------------------------------------ B: homopolymer runs on the borders
B_RUNS = (2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 12287, 12288, 12289, 24577)
B_BASES = (BLOCK * 7, SD_SR_RAW, 2 * SD_SR_RAW, SD_TILE_RAW, 2 * SD_TILE_RAW)
B_PARAMS = (dict(), dict(k=3, l=12, density=0.05), dict(k=7, l=64, density=0.02))
B_VARIANTS = (8, 16)   # on the default leg: positions from run ends / second position lists
B_TAIL = 1000          # random bases behind a run that leaves the three tiles


def plant_run(g, rng, start, r, min_len=3 * SD_TILE_RAW):
    """a random read of min_len bases (longer when the run needs it: B_TAIL random bases follow it) with ONE run of r equal bases written at
    [start, start + r); the base on either side differs from it.  Returns (sequence, base of the run)."""
    n = max(min_len, start + r + B_TAIL)
    s = bytearray(_cut(g, rng, n))
    c = _other(s[start - 1] if start > 0 else 0, s[start + r] if start + r < n else 0)
    s[start:start + r] = bytes([c]) * r
    return bytes(s), c


def run_is_exact(seq, start, r):
    """the planted run is exactly [start, start + r): one letter, and the base on either side differs from it"""
    c = seq[start]
    return (seq[start:start + r] == bytes([c]) * r and (start == 0 or seq[start - 1] != c)
            and (start + r == len(seq) or seq[start + r] != c))


def heads(rng, j, before, after):
    """j bases, no two neighbours equal, the first differing from `before` and the last from `after`: j run heads"""
    out = []
    for i in range(j):
        avoid = [out[-1] if out else before]
        if i == j - 1:
            avoid.append(after)
        out.append(int(rng.choice([c for c in b"ACGT" if c not in avoid])))
    return bytes(out)


def run_border_points(g, l, runs=B_RUNS, bases=B_BASES, seed=2):
    """family B: (name, sequence, (start, r) of the planted run or None).  A run that would have to start in front of the read does
    not exist (r > B + d for the `ends at` form); everything else is built."""
    rng = np.random.default_rng(seed * 1000 + l)
    pts = []
    for r in runs:
        for B in bases:
            for d in (-1, 0, 1):
                s, _ = plant_run(g, rng, B + d, r)
                pts.append(("run r=%d starts at %d%+d" % (r, B, d), s, (B + d, r)))
                if B + d - r >= 0:
                    s, _ = plant_run(g, rng, B + d - r, r)
                    pts.append(("run r=%d ends at %d%+d" % (r, B, d), s, (B + d - r, r)))
        s, _ = plant_run(g, rng, 0, r)
        pts.append(("run r=%d at the start of the read" % r, s, (0, r)))
        n = max(3 * SD_TILE_RAW, r + B_TAIL)
        s, _ = plant_run(g, rng, n - r, r, min_len=n)
        s = s[:n]
        pts.append(("run r=%d at the end of the read" % r, s, (n - r, r)))
    # two whole-tile runs with j run heads between them: the carry (l - 1 compressed bases) reaches back over more than one tile
    for j in sorted({0, 1, l - 2, l - 1, l}):
        if j < 0:
            continue
        pre = _cut(g, rng, SD_TILE_RAW)
        post = _cut(g, rng, SD_TILE_RAW // 2)
        c1 = _other(pre[-1])
        c2 = _other(c1, post[0])
        mid = heads(rng, j, c1, c2)
        room = SD_TILE_RAW - (j % SD_TILE_RAW)
        seq = pre + bytes([c1]) * SD_TILE_RAW + mid + bytes([c2]) * (room + SD_TILE_RAW) + post  # the second run covers all of tile 3 too
        pts.append(("two whole-tile runs, %d heads between" % j, seq, None))
    # compressed length l - 1, l, l + 1 in a raw length of several tiles
    for c in (l - 1, l, l + 1):
        if c < 2:
            continue
        hd = heads(rng, c, 0, 0)
        total = 3 * SD_TILE_RAW + 100
        lens = [total // c + (1 if i < total % c else 0) for i in range(c)]
        seq = b"".join(bytes([hd[i]]) * lens[i] for i in range(c))
        pts.append(("compressed length %d in %d raw bases" % (c, total), seq, None))
    return pts


def compressed_length(seq):
    a = np.frombuffer(seq, dtype=np.uint8)
    return int(a.size > 0) + int((a[1:] != a[:-1]).sum())


# ------------------------------------------------------------------ C: where a read sits
C_PARAMS = (dict(), dict(k=3, l=12, density=0.05))


def placement_reads(g, seed=3):
    """the four fixed reads: shorter than a block, exactly 64 n bytes, a tile + 1, ending inside a run"""
    rng = np.random.default_rng(seed)
    in_run = bytearray(_cut(g, rng, 5000))
    c = _other(in_run[-8])
    in_run[-7:] = bytes([c]) * 7
    return [("shorter than a block", _cut(g, rng, 50)), ("64 * 40 bytes", _cut(g, rng, BLOCK * 40)),
            ("a tile + 1", _cut(g, rng, SD_TILE_RAW + 1)), ("ends inside a run", bytes(in_run))]


def placement_offsets_batch(g, reads, seed=4):
    """(i) every read behind a padding read of 1 .. 64 bytes that itself starts on a block border: the read at every offset mod 64.  Returns (points, index of each placed read ->
    (which read, residue))"""
    rng = np.random.default_rng(seed)
    pts, where, cur = [], {}, 0
    for p in range(BLOCK):
        for w, (name, s) in enumerate(reads):
            fill = -cur % BLOCK or BLOCK               # up to the next block border, then the padding read of p + 1 bytes
            pts.append(("fill %d" % fill, _cut(g, rng, fill)))
            pts.append(("pad %d" % (p + 1), _cut(g, rng, p + 1)))
            cur += fill + p + 1
            where[len(pts)] = (w, cur % BLOCK)
            pts.append((name, s))
            cur += len(s)
    return pts, where


def placement_neighbour_batch(g, reads, seed=5):
    """(ii) the read in front ends with the read's first base, the read behind starts with its last base"""
    rng = np.random.default_rng(seed)
    pts, where = [], {}
    for w, (name, s) in enumerate(reads):
        pts.append(("front", _cut(g, rng, 300) + s[:1]))
        where[len(pts)] = (w, None)
        pts.append((name, s))
        pts.append(("behind", s[-1:] + _cut(g, rng, 300)))
    return pts, where


def placement_n_batch(g, reads, seed=6):
    """(iii) the byte behind the read is N (the read behind starts with it)"""
    rng = np.random.default_rng(seed)
    pts, where = [], {}
    for w, (name, s) in enumerate(reads):
        where[len(pts)] = (w, None)
        pts.append((name, s))
        pts.append(("N first", b"N" + _cut(g, rng, 300)))
    return pts, where


def fastq_buffer(points):
    """(v) the points as four-line FASTQ records: (buffer, starts, lens); the byte in front of every read is a newline"""
    parts, starts, lens, pos = [], [], [], 0
    for i, (_, s) in enumerate(points):
        hdr = b"@r%d\n" % i
        rec = hdr + s + b"\n+\n" + b"I" * len(s) + b"\n"
        starts.append(pos + len(hdr))
        lens.append(len(s))
        parts.append(rec)
        pos += len(rec)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), np.array(starts, dtype=np.uint64), np.array(lens, dtype=np.uint32)


# ------------------------------------------------------------------ D: minimizer counts
D_PARAMS = (dict(), dict(k=8, l=16), dict(k=7, l=64, density=0.02), dict(k=3, l=12, density=0.05), dict(k=32, l=5, density=0.2),
            dict(use_hpc=False), dict(k=1, l=15, density=0.05))
D_J = (1, 2, 6, 7, 12, 18)


def minimizer_counts(k):
    """the N of family D: a count below 1 does not exist"""
    ns = {k - 1, k, k + 1}
    for j in D_J:
        for e in (-1, 0, 1):
            ns.add(LANE_BATCH * j + k - 1 + e)
    return sorted(n for n in ns if n >= 1)


def read_with_minimizers(O, g, ps, N, first=50, tries=40, km1=None):
    """a stretch of the genome with exactly N minimizers: opened at the start of minimizer i, closed one base behind minimizer
    i + N - 1 and grown base by base until oracle.minimizers counts N (under homopolymer compression the tuple's `end` is
    start + l - 1 in RAW bases and cuts the last window short).  Returns (sequence, start in the genome)."""
    po = O.params(**ps)
    if km1 is None:
        km1 = O.kminmers(g, O.params(**{**ps, "k": 1}))
    for i in range(first, first + tries):
        if i + N >= len(km1):
            break
        a, b = int(km1[i]["start"]), int(km1[i + N - 1]["end"]) + 1
        stop = int(km1[i + N]["end"]) + 1
        while b <= stop:
            c = len(O.minimizers(g[a:b], po))
            if c >= N:
                break
            b += 1
        if b <= stop and c == N and len(kminmers_or_none(O, g[a:b], po)) == max(0, N - po.k + 1):
            return g[a:b].tobytes(), a
    raise LatticeError("no read with %d minimizers for %r" % (N, ps))


def minimizer_count_points(O, g, ps):
    po = O.params(**ps)
    km1 = O.kminmers(g, O.params(**{**ps, "k": 1}))
    return [("N=%d" % N, read_with_minimizers(O, g, ps, N, km1=km1)[0]) for N in minimizer_counts(po.k)]


# ------------------------------------------------------------------ E: where a Match run breaks
E_PARAMS = (dict(), dict(k=8, l=16))
E_BREAKS = (62, 63, 64, CHUNK_KMM - 1, CHUNK_KMM, CHUNK_KMM + 1, 2 * CHUNK_KMM - 1, 2 * CHUNK_KMM)
E_RUNS = (1, 2, MAP_LDS_RECS - 1, MAP_LDS_RECS, MAP_LDS_RECS + 1, CHAIN_CH - 1, CHAIN_CH, CHAIN_CH + 1)


def hit_mask(O, ox, seq, po):
    """for every k-min-mer of the read: is its hash in the oracle index (oracle.Index.get)"""
    get, h = O.lib().mqo_index_get, ox.h    # (oracle.Index.get without the copy of the entry: the search asks a million times)
    return np.array([get(h, int(x)) is not None for x in kminmers_or_none(O, seq, po)["hash"]], dtype=bool)


def _substitutions(seq, lo, hi):
    for p in range(lo, hi):
        for c in b"ACGT":
            if c != seq[p]:
                yield p, seq[:p] + bytes([c]) + seq[p + 1:]


def break_after(O, ox, seq, po, j):
    """one substituted base such that k-min-mers 0 .. j of the damaged read all hit and number j + 1 does not: the LAST hit before the
    break is number j (numbers count the damaged read's own k-min-mers from 0)"""
    km = kminmers_or_none(O, seq, po)
    if j + 1 >= len(km):
        raise LatticeError("break behind k-min-mer %d: the read has %d" % (j, len(km)))
    # around the last minimizer of k-min-mer j + 1 (under compression `end` is short of the window's true end); the hits decide
    for p, s in _substitutions(seq, max(0, int(km[j]["end"]) - po.l), min(len(seq), int(km[j + 1]["end"]) + 2 * po.l + 2)):
        m = hit_mask(O, ox, s, po)
        if m.size > j + 1 and m[:j + 1].all() and not m[j + 1] and m[j + 1:].any():
            return s
    raise LatticeError("no substitution makes k-min-mer %d the last hit before a break" % j)


def break_before(O, ox, seq, po, j):
    """one substituted base such that k-min-mer j - 1 of the damaged read misses and number j and all behind it hit: the FIRST hit
    after the break is number j"""
    km = kminmers_or_none(O, seq, po)
    if j < 1 or j >= len(km):
        raise LatticeError("break in front of k-min-mer %d: the read has %d" % (j, len(km)))
    for p, s in _substitutions(seq, int(km[j - 1]["start"]), min(len(seq), int(km[j]["start"]) + po.l)):  # the first minimizer of k-min-mer j - 1
        m = hit_mask(O, ox, s, po)
        if m.size > j and not m[j - 1] and m[j:].all() and m[:j - 1].any():
            return s
    raise LatticeError("no substitution makes k-min-mer %d the first hit after a break" % j)


def n_matches(ox, seq, po):
    b = np.frombuffer(seq, dtype=np.uint8)
    return int(ox.map_batch_diag(b, np.array([0, b.size], dtype=np.uint64), po)[1]["n_matches"][0])


def reads_with_match_runs(O, ox, seq, po, wanted=E_RUNS, from_own=False):
    """substitutions added one at a time, each kept only if it raises the oracle's Match-run count by exactly one: {M: read with M runs}.
    from_own: the undamaged read may have any count below min(wanted) (dense lists of short l-mers: it misses here and there without
    any damage); the search starts from that count"""
    out = {}
    cur, m = seq, n_matches(ox, seq, po)
    if (m >= min(wanted)) if from_own else (m != 1):
        raise LatticeError("the undamaged read has %d Match runs" % m)
    out[m] = cur
    km = kminmers_or_none(O, seq, po)
    step = po.k + 3
    at = step
    while m < max(wanted) and at + 1 < len(km):
        for p, s in _substitutions(cur, int(km[at]["start"]), int(km[at]["start"]) + po.l):
            if n_matches(ox, s, po) == m + 1:
                cur, m = s, m + 1
                out[m] = cur
                break
        at += step
    missing = [w for w in wanted if w not in out]
    if missing:
        raise LatticeError("no read with %s Match runs (reached %d)" % (missing, m))
    return {w: out[w] for w in wanted}


E_RETRIES = 4   # other stretches of the genome tried for a point that one substitution cannot make in the first


def match_break_points(O, ox, g, ps):
    """family E from family D's reads of two chunks and of three chunks (+ one k-min-mer), forward and reverse-complemented.  Where no
    single substitution makes a point in the read (dense lists of short l-mers: the windows of neighbouring minimizers overlap, and a
    substitution that ends one lists another), the same read cut E_RETRIES times further along the genome is tried for that point."""
    po = O.params(**ps)
    km1 = O.kminmers(g, O.params(**{**ps, "k": 1}))
    made = {}

    def read(chunks, t):
        if (chunks, t) not in made:
            made[(chunks, t)] = read_with_minimizers(O, g, ps, LANE_BATCH * 6 * chunks + po.k - 1 + 1, first=(50 if chunks == 2 else 60) + 100 * t, km1=km1)[0]
        return made[(chunks, t)]

    def point(make, chunks, f, *args):
        for t in range(E_RETRIES + 1):
            try:
                return make(O, ox, f(read(chunks, t)), po, *args)
            except LatticeError as e:
                err = e
        raise err
    pts = []
    for strand, f in (("fwd", lambda s: s), ("rc", revcomp)):
        for chunks in (2, 3):
            for j in E_BREAKS:
                if chunks == 2 and j > CHUNK_KMM + 1:   # the breaks at the end of the second chunk are the three-chunk read's
                    continue
                pts.append(("%s %d chunks: last hit before the break is %d" % (strand, chunks, j), point(break_after, chunks, f, j), ("after", j)))
                pts.append(("%s %d chunks: first hit after the break is %d" % (strand, chunks, j), point(break_before, chunks, f, j), ("before", j)))
        for M, s in point(reads_with_match_runs, 3, f).items():
            pts.append(("%s: %d Match runs" % (strand, M), s, ("runs", M)))
    return pts


CORE_RUNS = (MAP_LDS_RECS - 1, MAP_LDS_RECS, MAP_LDS_RECS + 1, CHAIN_CH - 1, CHAIN_CH, CHAIN_CH + 1)


def match_run_points(O, ox, g, ps, wanted=CORE_RUNS):
    """family E's Match-run reads alone, for a parameter set whose undamaged reads do not hit at every k-min-mer: the read of three
    chunks, forward and reverse-complemented, damaged from its own count upwards (reads_with_match_runs, from_own).  (name, sequence,
    ("runs", M))"""
    po = O.params(**ps)
    km1 = O.kminmers(g, O.params(**{**ps, "k": 1}))
    pts = []
    for strand, f in (("fwd", lambda s: s), ("rc", revcomp)):
        for t in range(E_RETRIES + 1):
            try:
                read = read_with_minimizers(O, g, ps, LANE_BATCH * 18 + po.k - 1 + 1, first=60 + 100 * t, km1=km1)[0]
                made = reads_with_match_runs(O, ox, f(read), po, wanted, from_own=True)
                break
            except LatticeError as e:
                if t == E_RETRIES:
                    raise e
        pts += [("%s: %d Match runs" % (strand, M), s, ("runs", M)) for M, s in made.items()]
    return pts


# ------------------------------------------------------------------ F: general seeder
F_BASES = (0, GEN_STEP, 2 * GEN_STEP, 3 * GEN_STEP, SD_TILE_RAW)
F_RUNS = (1023, 1024, 1025, 2047, 2048, 2049, 4097)
F_RUN_STARTS = (2 * GEN_STEP, 2 * GEN_STEP + 1, 3 * GEN_STEP - 1)   # = 0, 1, 1023 mod 1024
F_CLEAN = (2047, 2048, 2049, 2048 + 63, 2048 + 64, 2048 + 65)
F_HEADS = (63, 64, 65, 511, 512, 513, 1024)
F_PARAMS = (dict(), dict(k=3, l=12, density=0.05), dict(k=7, l=64, density=0.02))


def general_run_points(g, seed=7, starts=F_RUN_STARTS):
    rng = np.random.default_rng(seed)
    pts = []
    for r in F_RUNS:
        for st in starts:
            s, _ = plant_run(g, rng, st, r, min_len=st + r + 3000)
            pts.append(("general: run of A-like r=%d at %d" % (r, st), s, (st, r)))
            sn = bytearray(s)
            sn[st:st + r] = b"N" * r
            pts.append(("general: run of N r=%d at %d" % (r, st), bytes(sn), (st, r)))
    return pts


def declined_stretch_points(g, seed=8, ds=(-1, 0, 1)):
    """a non-ACGT byte at 192 + d, a clean stretch of c bytes behind it, another non-ACGT byte, sequence: the stretch's whole 64-byte
    blocks number 2048 / 64 or one fewer or more depending on d and c.  (name, sequence, (first clean byte, c))"""
    rng = np.random.default_rng(seed)
    pts = []
    for c in F_CLEAN:
        for d in ds:
            a = 3 * BLOCK + d
            pts.append(("declined: N at %d, %d clean bytes" % (a, c), _cut(g, rng, a) + b"N" + _cut(g, rng, c) + b"N" + _cut(g, rng, 3000), (a + 1, c)))
    return pts


def clean_blocks(start, c):
    """bytes of [start, start + c) that lie in whole 64-byte blocks"""
    lo, hi = -(-start // BLOCK) * BLOCK, (start + c) // BLOCK * BLOCK
    return max(0, hi - lo)


def dense_step(h, cycle=b"ACGN"):
    """one 1-KB step of h runs (alternating bytes, run lengths as even as 1024 / h allows)"""
    lens = [GEN_STEP // h + (1 if i < GEN_STEP % h else 0) for i in range(h)]
    return b"".join(bytes([cycle[i % len(cycle)]]) * lens[i] for i in range(h))


def dense_step_points(g, seed=9):
    """reads whose 1-KB steps 2, 3 and 4 hold exactly h run heads each (h a multiple of the cycle or not: the step's first byte differs from
    the last of the one in front either way, asserted by the CPU test through count_heads)"""
    rng = np.random.default_rng(seed)
    pts = []
    for h in F_HEADS:
        cyc = b"nN" if h == GEN_STEP else b"ACGN"
        steps = []
        for i in range(3):
            k = (i * h) % len(cyc)
            steps.append(dense_step(h, cyc[k:] + cyc[:k]))
        pre, post = bytearray(_cut(g, rng, 2 * GEN_STEP)), bytearray(_cut(g, rng, 2 * GEN_STEP))
        mid = b"".join(steps)
        if pre[-1] == mid[0]:
            pre[-1] = _other(pre[-2], mid[0])
        if post[0] == mid[-1]:
            post[0] = _other(post[1], mid[-1])
        pts.append(("dense: %d run heads per 1-KB step" % h, bytes(pre) + mid + bytes(post), h))
    return pts


def count_heads(seq, a, b):
    """run heads among bytes [a, b) of seq"""
    s = np.frombuffer(seq, dtype=np.uint8)
    hd = np.ones(s.size, dtype=bool)
    hd[1:] = s[1:] != s[:-1]
    return int(hd[a:b].sum())


# ------------------------------------------------------------------ G: the same sequences as references
G_BASES = (REF_SEG, 2 * REF_SEG, REF_SEG + REF_HALO)
G_LS = (12, 31, 64)
G_PARAMS = (dict(), dict(k=3, l=12, density=0.05), dict(k=7, l=64, density=0.02))


def reference_length_points(g, l, seed=10):
    return raw_length_points(g, l, bases=G_BASES, seed=seed)


def reference_run_points(g, l, seed=11):
    """family B's runs around the segment borders of the index build, in sequences of three segments; plus halos (the REF_HALO bases
    behind a segment) that hold j < l - 1 run heads: the segment's view cannot complete its last windows (the redo path)"""
    rng = np.random.default_rng(seed * 1000 + l)
    pts = []
    for r in B_RUNS:
        for B in G_BASES:
            for d in (-1, 0, 1):
                s, _ = plant_run(g, rng, B + d, r, min_len=3 * REF_SEG)
                pts.append(("ref: run r=%d starts at %d%+d" % (r, B, d), s, (B + d, r)))
                if B + d - r >= 0:
                    s, _ = plant_run(g, rng, B + d - r, r, min_len=3 * REF_SEG)
                    pts.append(("ref: run r=%d ends at %d%+d" % (r, B, d), s, (B + d - r, r)))
    for hh in sorted({1, 2, l - 2, l - 1, l}):   # run heads in the halo: hh - 1 single bases and the head of one run that fills the rest
        if hh < 1:
            continue
        pre = _cut(g, rng, REF_SEG)
        post = _cut(g, rng, REF_SEG)
        c2 = _other(post[0], pre[-1])
        mid = heads(rng, hh - 1, pre[-1], c2)
        pts.append(("ref: halo with %d run heads" % hh, pre + mid + bytes([c2]) * (REF_HALO - (hh - 1) + 300) + post, ("halo", hh)))
    return pts


# ------------------------------------------------------------------ core: one batch per parameter set for the instantiation matrix
CORE_A_BASES = (0, BLOCK, SD_SR_RAW, SD_TILE_RAW, 2 * SD_TILE_RAW)
CORE_B_RUNS = (WORD - 1, WORD, WORD + 1, BLOCK - 1, BLOCK, BLOCK + 1, SD_SR_RAW - 1, SD_SR_RAW, SD_SR_RAW + 1,
               SD_TILE_RAW - 1, SD_TILE_RAW, SD_TILE_RAW + 1)
CORE_B_BASES = (SD_SR_RAW, SD_TILE_RAW)
CORE_F_START = 2 * GEN_STEP      # the one run start of the core's general-seeder reads (= 0 mod 1024)
CORE_F_D = -1                    # declined_stretch_points' d at which F_CLEAN gives 2048 - 64, 2048 and 2048 + 64 bytes in whole blocks


def core_length_offsets(l):
    """the d of the core's family A: the size itself, one to either side, the carry of l - 1 codes and one more"""
    return (-1, 0, 1, -(l - 1), l - 1, l)


def core_points(O, ox, g, ps, families="ABDEF"):
    """A named subset of families A, B, D, E and F that hits every size of the module header exactly and one element to either side
    (test_lattice_cases.py proves it per constant), small enough that twenty-odd kernel configurations can each map it: (name, sequence,
    family letter).  Names are prefixed with the family, so they are unique within the batch.  D and E come forward and reverse-complemented.
    SD_OWNER_CAP and the 32- / 64-step words of stage B are not the core's: family H (list_capacity_points) and family A's full length
    lattice carry them.
    families: family E's break search damages a read that hits the index at EVERY k-min-mer; at k = 3, l = 12 an error-free read of two
    chunks already misses at a dozen of them (short l-mers, dense lists), so CORE_PARAMS gives that set "R" in E's place: the Match-run
    reads of CORE_RUNS alone (match_run_points), counted up from the undamaged read's own number of runs."""
    po = O.params(**ps)
    l = int(po.l)
    pts = []
    if "A" in families:
        pts += [("A " + n, s, "A") for n, s in raw_length_points(g, l, bases=CORE_A_BASES, offsets=core_length_offsets(l))]
    if "B" in families:
        pts += [("B " + n, s, "B") for n, s, _ in run_border_points(g, l, runs=CORE_B_RUNS, bases=CORE_B_BASES)]
    if "D" in families:
        d = minimizer_count_points(O, g, ps)
        pts += [("D " + n, s, "D") for n, s in d] + [("D " + n + " rc", revcomp(s), "D") for n, s in d]
    if "E" in families:
        pts += [("E " + n, s, "E") for n, s, _ in match_break_points(O, ox, g, ps)]      # (both strands already)
    if "R" in families:
        pts += [("E " + n, s, "E") for n, s, _ in match_run_points(O, ox, g, ps)]
    if "F" in families:
        pts += [("F " + n, s, "F") for n, s, _ in general_run_points(g, starts=(CORE_F_START,)) + declined_stretch_points(g, ds=(CORE_F_D,))
                + dense_step_points(g)]
    return pts


# the parameter sets of the matrix and the families each one's core batch holds
CORE_PARAMS = {"default": (dict(), "ABDEF"), "k3l12": (dict(k=3, l=12, density=0.05), "ABDRF"), "k7": (dict(k=7), "ABDEF")}


# ------------------------------------------------------------------ H: the list region's own edge
H_F16 = 1                                   # MQ_LIST_F16=1: every read below 65,536 bases has cap = LIST_SLACK
H_COUNTS = (LIST_SLACK - 1, LIST_SLACK, LIST_SLACK + 1, LIST_SLACK + SD_OWNER_CAP - 1, LIST_SLACK + SD_OWNER_CAP, LIST_SLACK + SD_OWNER_CAP + 1)
H_NEIGHBOUR = 3000                          # bases of the fixed neighbour read
H_BLOCK = 65536                             # bases per unit of a region's start at f16 = 1


def default_f16(density):
    """list_f16 (mq_host_state.hpp:570): list entries reserved per base, in 1 / 65536"""
    f = min(1.0, 4.0 * max(0.0, density) + 1.0 / 512.0)
    return int(np.ceil(f * 65536.0))


def list_cap(length, f16):
    """list_region's cap (mq_map_kernels.hpp:125)"""
    return ((length * f16) >> 16) + LIST_SLACK


def with_one_n(O, seq, po, N, tries=200):
    """the read with ONE byte replaced by N, chosen near the middle so that the read still lists exactly N minimizers"""
    mid = len(seq) // 2
    for t in range(tries):
        p = mid + t
        if p >= len(seq):
            break
        s = seq[:p] + b"N" + seq[p + 1:]
        if len(O.minimizers(s, po)) == N and len(kminmers_or_none(O, s, po)) == max(0, N - po.k + 1):
            return s
    raise LatticeError("no N keeps %d minimizers" % N)


def read_at_default_cap(O, g, ps, km1, first=50, tries=40):
    """a stretch of the genome whose minimizer count equals its own list capacity at the default f16: (sequence, N)"""
    po = O.params(**ps)
    f16 = default_f16(po.density)
    for i in range(first, first + tries):
        for N in range(LIST_SLACK + 1, LIST_SLACK + 2 * SD_OWNER_CAP):
            if i + N >= len(km1):
                break
            a, b = int(km1[i]["start"]), int(km1[i + N - 1]["end"]) + 1
            if list_cap(b - a, f16) != N:   # (the exact read may be a few bases longer: read_with_minimizers grows it, the cap is asked again)
                continue
            try:
                s, _ = read_with_minimizers(O, g, ps, N, first=i, tries=1, km1=km1)
            except LatticeError:
                continue
            if list_cap(len(s), f16) == N:
                return s, N
    raise LatticeError("no read whose minimizer count equals its default list capacity (f16 = %d) for %r" % (f16, ps))


def list_capacity_points(O, g, ps, tries=40, default_too=True):
    """family H: for every N of H_COUNTS a read with exactly N minimizers and the same read with one N byte (the declined / general
    path), each followed by the fixed neighbour read, so that list regions are adjacent: (name, sequence, N or None for a neighbour).
    default_too: one more pair whose read's count equals its own capacity at the default f16 -- LatticeError if the genome has none."""
    po = O.params(**ps)
    km1 = O.kminmers(g, O.params(**{**ps, "k": 1}))
    rng = np.random.default_rng(12)
    neighbour = _cut(g, rng, H_NEIGHBOUR)
    pts, cur = [], 0

    def pair(name, seq, N):
        # at f16 = 1 a region starts at (offset >> 16) + LIST_SLACK * r: the neighbour's region lies directly behind the read's only if both
        # start in the same 65,536 bases of the batch (the points are meant to open it).  A padding read moves a pair that would not.
        nonlocal cur
        if len(seq) >= H_BLOCK:
            raise LatticeError("%s: %d bases do not fit one block of %d" % (name, len(seq), H_BLOCK))
        if (cur + len(seq)) // H_BLOCK != cur // H_BLOCK:
            fill = -cur % H_BLOCK
            pts.append(("pad %d in front of %s" % (fill, name), _cut(g, rng, fill), "pad"))
            cur += fill
        pts.append((name, seq, N))
        pts.append(("neighbour of " + name, neighbour, None))
        cur += len(seq) + len(neighbour)
    for N in H_COUNTS:
        s, _ = read_with_minimizers(O, g, ps, N, tries=tries, km1=km1)
        pair("N=%d" % N, s, N)
        pair("N=%d with an N" % N, with_one_n(O, s, po, N), N)
    if default_too:
        s, N = read_at_default_cap(O, g, ps, km1, tries=tries)
        pair("N=%d = default cap" % N, s, N)
    return pts


def regions_adjacent(pts, f16=H_F16):
    """for every (read, neighbour) pair of family H at the head of a batch: does the neighbour's list region begin exactly where the
    read's ends (list_region, mq_map_kernels.hpp:125)"""
    _, offs = batch(pts)
    ok = []
    for i, p in enumerate(pts):
        if isinstance(p[2], int):
            o0, o1 = int(offs[i]), int(offs[i + 1])
            base0, base1 = ((o0 * f16) >> 16) + LIST_SLACK * i, ((o1 * f16) >> 16) + LIST_SLACK * (i + 1)
            ok.append(base1 == base0 + list_cap(len(p[1]), f16))
    return ok


# ------------------------------------------------------------------ I: lower case on the borders (fold_case)
I_BYTES = (WORD - 1, WORD, WORD + 1, BLOCK - 1, BLOCK, BLOCK + 1, SD_SR_RAW - 1, SD_SR_RAW, SD_SR_RAW + 1,
           SD_TILE_RAW - 1, SD_TILE_RAW, SD_TILE_RAW + 1)
I_LEN = 3 * SD_TILE_RAW
I_RUN = 64                     # the mixed-case run: bytes [12288 - 32, 12288 + 32)
I_N_RUN = 40                   # the lower-case n run of the general seeder's points


def _lower_at(seq, positions):
    s = bytearray(seq)
    for p in positions:
        s[p] |= 0x20
    return bytes(s)


def fold_border_points(g, seed=13):
    """family I: reads of three tiles whose lower-case bytes sit on the seeders' borders: (name, sequence, (lower-case positions, the
    upper-case read it was made from)).  The oracle gets the upper-case read (the reference folds before it seeds)."""
    rng = np.random.default_rng(seed)
    pts = []
    for p in I_BYTES + (0, I_LEN - 1):
        up = _cut(g, rng, I_LEN)
        pts.append(("lower-case byte %d" % p, _lower_at(up, [p]), ([p], up)))
    st = SD_TILE_RAW - I_RUN // 2
    up, _ = plant_run(g, rng, st, I_RUN)
    odd = list(range(st, st + I_RUN, 2))
    pts.append(("mixed-case run aAaA across %d" % SD_TILE_RAW, _lower_at(up, odd), (odd, up)))
    for a in (GEN_STEP - 1, GEN_STEP, GEN_STEP + 1):   # general seeder: a lower-case n run
        s = bytearray(_cut(g, rng, I_LEN))
        s[a:a + I_N_RUN] = b"N" * I_N_RUN
        up = bytes(s)
        where = list(range(a, a + I_N_RUN))
        pts.append(("lower-case n run starts at %d" % a, _lower_at(up, where), (where, up)))
    a = 3 * BLOCK        # a stretch of HYB_MIN_CLEAN lower-case bases in whole blocks, an N on either side
    up = _cut(g, rng, a - 1) + b"N" + _cut(g, rng, HYB_MIN_CLEAN) + b"N" + _cut(g, rng, I_LEN - a - HYB_MIN_CLEAN - 1)
    where = list(range(a, a + HYB_MIN_CLEAN))
    pts.append(("%d lower-case bases between two N" % HYB_MIN_CLEAN, _lower_at(up, where), (where, up)))
    return pts
