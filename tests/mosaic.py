"""Mosaic reads: reads assembled from error-free slices of DIFFERENT contigs, strands and positions, so that the chain side of the
mapper (Match runs, per-reference anchor and filter, best-of-two with its tie rule, find_coords) sees what simulated reads never
give it: dozens of candidate references spread over several 64-lane chunks of the Match list, many-way ties, a reference whose
only Match lies in a later chunk, gap differences of exactly g, and more Match runs than the default scratch holds.

Plain numpy, seeded; nothing here needs a GPU, and only n_way_tie() asks the oracle (to keep the reads that really tie).
The CPU tests (test_mosaic_cases.py) show that the committed seeds reach those regimes; the GPU tests (test_gpu_mosaic.py) compare
the HIP path with the oracle on exactly these reads.
"""
import numpy as np

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMP[_a] = _b


def revcomp(s):
    return _COMP[s[::-1]]


def concat(seqs):
    bases = np.concatenate(seqs) if seqs else np.zeros(0, dtype=np.uint8)
    offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([s.size for s in seqs])
    return np.ascontiguousarray(bases, dtype=np.uint8), offs


def select(bases, offs, keep):
    """Sub-batch of the reads whose indices are in `keep`."""
    return concat([bases[int(offs[i]):int(offs[i + 1])] for i in keep])


# ------------------------------------------------------------------ the genome
N_BIG, BIG_LEN, N_MID, MID_LEN, N_TINY, TINY_LEN = 40, 60_000, 40, 8_000, 240, 500


def mosaic_genome(sim, seed=7001):
    """320 contigs: 40 of 60 kb, 40 of 8 kb (so that 65 different contigs can each give a 1.5-kb slice) and 240 of 500 bases (shorter than
    most segments: find_coords clips at both ends), shuffled, so that a three-digit ref_id is as likely to be a long contig as a tiny one.  Uniform random sequence without planted
    repeats: every k-min-mer is unique, an error-free slice gives ONE Match run.  Returns (genome, ctg_off, names)."""
    lens = np.array([BIG_LEN] * N_BIG + [MID_LEN] * N_MID + [TINY_LEN] * N_TINY, dtype=np.int64)
    np.random.default_rng(seed).shuffle(lens)
    return sim.make_genome([int(x) for x in lens], seed=seed, threads=2)


def _slice(genome, ctg_off, ctg, pos, length, rc):
    """(bases, ref start, ref end) of up to `length` bases of contig `ctg` from contig position `pos`, clipped to the contig"""
    lo, hi = int(ctg_off[ctg]), int(ctg_off[ctg + 1])
    a = min(max(lo + int(pos), lo), hi)
    b = min(a + int(length), hi)
    s = genome[a:b]
    return (revcomp(s) if rc else s), a - lo, b - lo


# ------------------------------------------------------------------ the generator
def mosaic_reads(genome, ctg_off, rng, n_reads, max_segments, seg_len_range, p_jump, deltas, err=0.0, short_frac=0.0):
    """n_reads reads of 1 .. max_segments segments.  Segment by segment: with probability p_jump a new (contig, position, strand) drawn
    uniformly (contig uniform over the CONTIGS, so tiny contigs are picked as often as long ones); otherwise the same contig and
    strand, the reference position moved on by a value drawn from `deltas` while the query stays contiguous (an exact deletion of that
    many reference bases, or for a negative value an insertion of a copy of the last ones).  On the reverse strand "on" means towards
    lower reference positions, so that a co-linear chain results there too.  Slices are clipped to their contig.
    err > 0 substitutes that fraction of the read's bases afterwards; short_frac of the reads have 1 .. 3 segments only (weak winners:
    mapq 0).
    Returns (bases, offsets, truth); truth[i] = [(contig, ref_start, ref_end, rc), ...] per segment of read i (contig-relative)."""
    n_ctg = ctg_off.size - 1
    deltas = np.asarray(deltas, dtype=np.int64)
    seqs, truth = [], []
    for _ in range(n_reads):
        nseg = int(rng.integers(1, max_segments + 1))
        if short_frac > 0 and rng.random() < short_frac:
            nseg = int(rng.integers(1, 4))
        parts, tr = [], []
        ctg = pos = rc = None
        for s in range(nseg):
            ln = int(rng.integers(seg_len_range[0], seg_len_range[1] + 1))
            if ctg is None or rng.random() < p_jump:
                ctg = int(rng.integers(0, n_ctg))
                clen = int(ctg_off[ctg + 1] - ctg_off[ctg])
                pos = int(rng.integers(0, max(1, clen - 1)))
                rc = bool(rng.integers(0, 2))
            else:
                d = int(deltas[int(rng.integers(0, deltas.size))])
                pos = (tr[-1][1] - d - ln) if rc else (tr[-1][2] + d)
            seg, a, b = _slice(genome, ctg_off, ctg, pos, ln, rc)
            if b <= a:  # ran off the contig: start over somewhere else
                ctg = None
                continue
            parts.append(seg)
            tr.append((ctg, a, b, rc))
        if not parts:
            seg, a, b = _slice(genome, ctg_off, 0, 0, seg_len_range[1], False)
            parts, tr = [seg], [(0, a, b, False)]
        r = np.concatenate(parts)
        if err > 0:
            at = np.flatnonzero(rng.random(r.size) < err)
            r = r.copy()
            r[at] = np.frombuffer(b"ACGT", dtype=np.uint8)[(np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), r[at]) + rng.integers(1, 4, size=at.size)) % 4]
        seqs.append(r)
        truth.append(tr)
    bases, offs = concat(seqs)
    return bases, offs, truth


def big_contigs(ctg_off, min_len=20_000):
    return [c for c in range(ctg_off.size - 1) if int(ctg_off[c + 1] - ctg_off[c]) >= min_len]


# ------------------------------------------------------------------ directed: gap ladder
GAP_GS = (0, 1, 50, 2000, 0x7FFFFFFF, 0xFFFFFFFF)
GAP_FAR = 20_000    # a jump far beyond every small g (and, backwards, behind the anchor's own start)
GAP_SEG = 5_000     # segment length: longer than g + 2 for every small g, so only a backward jump of GAP_FAR lands in front of the
                    # previous segment's start (the order test of check_match_compatible, which no g lets pass)


def gap_jumps(g):
    """the reference jumps tried for one g: 0, g-2 .. g+2 and their negatives (those that are non-zero and fit a contig), +-GAP_FAR"""
    js = {0, GAP_FAR, -GAP_FAR}
    for e in range(-2, 3):
        j = g + e
        if 0 < j <= 4000:
            js.update((j, -j))
    if g > 4000:  # g at the ends of i32 / u32: no jump on a 60-kb contig comes near it; a ladder of ordinary jumps must all pass
        js.update((1, -1, 50, -50, 2000, -2000))
    return sorted(js)


def gap_ladder(genome, ctg_off, g, rng, per_jump=12):
    """Co-linear reads of one contig whose consecutive segments are separated on the reference by `jump` more bases than in the read:
    two-segment reads (5 kb | 5 kb) and three-segment reads (3 kb | 6 kb | 3 kb: the middle segment is the anchor, the same jump on
    both sides), each as it is and reverse-complemented.  Match coordinates are raw positions of the same windows on both sides, so
    without homopolymer compression |gap difference| = |jump| exactly; under compression it holds give or take a few bases (see
    test_mosaic_cases.test_gap_ladder_filters_exactly_beyond_g).
    Returns (bases, offsets, meta); meta[i] = dict(jump, nseg, rc, ctg, segs=[(ref_start, ref_end), ...])."""
    big = big_contigs(ctg_off, 12_000 + 2 * GAP_FAR + 1)
    seqs, meta = [], []
    for jump in gap_jumps(g):
        for rep in range(per_jump):
            for lens in ((GAP_SEG, GAP_SEG), (3000, 6000, 3000)):
                ctg = int(big[int(rng.integers(0, len(big)))])
                clen = int(ctg_off[ctg + 1] - ctg_off[ctg])
                span = sum(lens) + (len(lens) - 1) * abs(jump)
                x = int(rng.integers(0, clen - span)) + (0 if jump >= 0 else (len(lens) - 1) * -jump)
                segs = []
                for ln in lens:
                    segs.append((x, x + ln))
                    x += ln + jump
                assert all(0 <= a and b <= clen for a, b in segs)
                fw = np.concatenate([genome[int(ctg_off[ctg]) + a:int(ctg_off[ctg]) + b] for a, b in segs])
                for rc in (False, True):
                    seqs.append(revcomp(fw) if rc else fw)
                    meta.append(dict(jump=jump, nseg=len(lens), rc=rc, ctg=ctg, segs=segs))
    bases, offs = concat(seqs)
    return bases, offs, meta


# ------------------------------------------------------------------ directed: n-way ties
TIE_NS = (2, 3, 5, 17, 65)


def n_way_tie(genome, ctg_off, ox, po, n, rng, n_want=6, n_pool=2400, seg_len=1500, ahead=0):
    """Reads of n equal-length error-free slices of n DIFFERENT contigs (random strands, random order), each slice ONE Match.  Equal
    lengths do not give equal k-min-mer counts, so: map every slice of a pool alone with the oracle, group the slices by the score it
    gives them, and build each read from slices of n different contigs with the SAME score -- then ask the oracle again and keep the
    reads it reports as ties with at least n candidates.  With ahead = 1 one of the n slices is taken from the group whose score is
    one higher (near-ties: mapped, to that slice's contig); kept are the reads with n candidates of one Match each.
    Returns (bases, offsets, winners); winners[i] = the contig that is ahead (None for a tie)."""
    n_ctg = ctg_off.size - 1
    wide = [c for c in range(n_ctg) if int(ctg_off[c + 1] - ctg_off[c]) >= 4 * seg_len]
    pool = []
    for _ in range(n_pool):
        ctg = int(wide[int(rng.integers(0, len(wide)))])
        clen = int(ctg_off[ctg + 1] - ctg_off[ctg])
        pool.append((ctg, _slice(genome, ctg_off, ctg, int(rng.integers(0, clen - seg_len)), seg_len, bool(rng.integers(0, 2)))[0]))
    pb, poffs = concat([s for _, s in pool])
    out, diag = ox.map_batch_diag(pb, poffs, po, threads=4)
    by_score = {}  # score -> contig -> pool indices
    for i, (ctg, _) in enumerate(pool):
        if out["mapped"][i] and int(diag["n_matches"][i]) == 1 and int(out["ref_id"][i]) == ctg:
            by_score.setdefault(int(out["score"][i]), {}).setdefault(ctg, []).append(i)
    usable = sorted(sc for sc, d in by_score.items() if len(d) >= n and (not ahead or by_score.get(sc + 1)))
    seqs, winners = [], []
    for _ in range(3 * n_want if usable else 0):
        sc = int(usable[int(rng.integers(0, len(usable)))])
        win, ctgs = None, list(by_score[sc])
        picked = []
        if ahead:
            win = int(rng.choice(list(by_score[sc + 1])))
            picked.append(int(rng.choice(by_score[sc + 1][win])))
            ctgs = [c for c in ctgs if c != win]
        if len(ctgs) < n - len(picked):
            continue
        for c in rng.choice(ctgs, size=n - len(picked), replace=False):
            picked.append(int(rng.choice(by_score[sc][int(c)])))
        seqs.append(np.concatenate([pool[picked[j]][1] for j in rng.permutation(n)]))  # the slice that is ahead takes any place
        winners.append(win)
    bases, offs = concat(seqs)
    if not seqs:
        return bases, offs, winners
    out, diag = ox.map_batch_diag(bases, offs, po, threads=4)
    if ahead:
        keep = [i for i in range(len(seqs)) if diag["n_candidates"][i] == n and diag["n_matches"][i] == n and diag["tie"][i] == 0]  # (a slice's count
        # inside a read can differ by one from its count alone: the minimizers next to a junction change)
    else:
        keep = [i for i in range(len(seqs)) if diag["tie"][i] != 0 and diag["n_candidates"][i] >= n]
    keep = keep[:n_want]
    b2, o2 = select(bases, offs, keep)
    return b2, o2, [winners[i] for i in keep]


# ------------------------------------------------------------------ directed: the winner's first Match in a later chunk
def late_candidate(genome, ctg_off, rng, n_reads=12, n_short=(130, 200), short_len=1200, long_len=12_000):
    """n_short error-free slices of contig A, each just long enough for a Match of a few k-min-mers and far from one another (so the
    anchor's filter throws most of them out), then ONE long slice of contig B -- and the mirror image (B first).  In the first form the
    winning reference's only Match is record 70 or later: it is first seen in the second or third 64-lane chunk of the Match list and
    is a reference with a single Match.  In the mirror image it is record 0 and everything behind it belongs to the loser.
    Returns (bases, offsets, meta); meta[i] = dict(a, b, n_short, mirror)."""
    big = big_contigs(ctg_off)
    seqs, meta = [], []
    for r in range(n_reads):
        a, b = (int(x) for x in rng.choice(big, size=2, replace=False))
        la, lb = int(ctg_off[a + 1] - ctg_off[a]), int(ctg_off[b + 1] - ctg_off[b])
        ns = int(rng.integers(n_short[0], n_short[1] + 1))
        rc_a, rc_b = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        shorts = [_slice(genome, ctg_off, a, int(rng.integers(0, la - short_len)), short_len, rc_a)[0] for _ in range(ns)]
        long_ = _slice(genome, ctg_off, b, int(rng.integers(0, lb - long_len)), long_len, rc_b)[0]
        mirror = bool(r % 2)
        seqs.append(np.concatenate(([long_] + shorts) if mirror else (shorts + [long_])))
        meta.append(dict(a=a, b=b, n_short=ns, mirror=mirror))
    bases, offs = concat(seqs)
    return bases, offs, meta


# ------------------------------------------------------------------ the legs (committed seeds and arguments)
DEFAULT_DELTAS = (0, 0, 1, -1, 7, -7, 150, -150, 1999, 2000, 2001, -1999, -2000, -2001, 6000, -6000, 25_000)

LEGS = {
    # name: (params, generator arguments, seed)
    "default": (dict(), dict(n_reads=400, max_segments=400, seg_len_range=(300, 2600), p_jump=0.5, deltas=DEFAULT_DELTAS, short_frac=0.12), 11),
    "k3": (dict(k=3, l=15, density=0.03, c=2, s=5, g=500), dict(n_reads=300, max_segments=400, seg_len_range=(100, 1200), p_jump=0.5, deltas=DEFAULT_DELTAS), 12),
    "k1": (dict(k=1, l=15, density=0.05), dict(n_reads=120, max_segments=400, seg_len_range=(100, 1200), p_jump=0.5, deltas=DEFAULT_DELTAS), 13),
    "k12": (dict(k=12, l=12, density=0.1, g=0), dict(n_reads=300, max_segments=400, seg_len_range=(150, 1500), p_jump=0.5, deltas=DEFAULT_DELTAS), 14),
    "mixed": (dict(), dict(n_reads=200, max_segments=120, seg_len_range=(500, 4000), p_jump=0.3, deltas=DEFAULT_DELTAS, err=0.01), 15),
}


def leg(name, genome, ctg_off):
    """(params dict, bases, offsets, truth) of a committed leg"""
    ps, args, seed = LEGS[name]
    bases, offs, truth = mosaic_reads(genome, ctg_off, np.random.default_rng(seed), **args)
    return dict(ps), bases, offs, truth


_WORLD = None


def world(O, sim):
    """Everything the mosaic tests share, built once per process: (genome, ctg_off, names, sets).  sets[name] = dict(ps = the
    parameters the set was made for, bases, offs, meta).  Names: the LEGS, "gap_<g>" for g in GAP_GS, "tie_<n>" and "near_<n>" for n
    in TIE_NS, "late"."""
    global _WORLD
    if _WORLD is not None:
        return _WORLD
    g, off, names = mosaic_genome(sim)
    sets = {}
    for name in LEGS:
        ps, b, o, tr = leg(name, g, off)
        sets[name] = dict(ps=ps, bases=b, offs=o, meta=tr)
    for gg in GAP_GS:
        b, o, meta = gap_ladder(g, off, gg, np.random.default_rng(2000 + gg % 997))
        sets["gap_%d" % gg] = dict(ps=dict(g=gg), bases=b, offs=o, meta=meta)
    po = O.params()
    ox = O.Index()
    ox.build_mt(g, off, names, po, 4)
    for n in TIE_NS:
        for ahead in (0, 1):
            b, o, win = n_way_tie(g, off, ox, po, n, np.random.default_rng(3000 + 2 * n + ahead), ahead=ahead)
            sets["%s_%d" % ("near" if ahead else "tie", n)] = dict(ps=dict(), bases=b, offs=o, meta=win)
    b, o, meta = late_candidate(g, off, np.random.default_rng(4000))
    sets["late"] = dict(ps=dict(), bases=b, offs=o, meta=meta)
    _WORLD = (g, off, names, sets)
    return _WORLD
