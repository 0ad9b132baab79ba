"""Depth and coverage cases at the tile counts where the one-workgroup scans change their path (depth_scan_kernel, cover_scan_kernel:
SCAN threads, each with per = ceil(n_tiles / SCAN) consecutive tiles) and at id ranges beyond the workgroup histograms (n_ids > 4096:
depth_add_kernel and cover_mark_kernel count per reference with global atomics).  Pure numpy; what a case must answer comes from
tests/depth_model.py and tests/coverage_model.py.  tests/test_scale_cases.py proves on the CPU that every case has the property it is
named after; tests/test_gpu_scale.py runs them through the library.

Every builder takes the tile size T it is built for (windows per depth tile, bits per coverage tile) and the tile count n it must reach
by the documented layout rule: the windows (bits) of the existing references lie behind one another in id order, and tiles never span two
references (tiles_of)."""
import numpy as np

import coverage_model as CM
import depth_model as DM

SCAN = 1024  # threads of the two scan kernels
TILE_COUNTS = (1024, 1025, 2049, 3 * 1024 + 7)  # per = 1 (every thread busy), 2 (one thread behind 1,024 busy, the rest clamped), 3, 4
MAPPED = DM.MAPPED


def per_of(n):
    return -(-n // SCAN)


def live_refs(refs):
    """the existing references as (id, length), in id order"""
    return sorted((int(i), int(ln)) for i, _, ln in refs if int(ln) > 0)


def tiles_of(refs, unit, T):
    """(tile count, per tile (index of its reference among the existing ones, the tile's number inside it)): per existing reference
    ceil(ceil(len / unit) / T) tiles; unit = the window (depth) or 1 bit (coverage)"""
    per_ref = np.array([-(-(-(-ln // unit)) // T) for _, ln in live_refs(refs)], dtype=np.int64)
    ref = np.repeat(np.arange(per_ref.size), per_ref)
    first = np.cumsum(per_ref) - per_ref
    return int(ref.size), np.stack([ref, np.arange(ref.size) - first[ref]], axis=1)


def boundaries(n):
    """the tile numbers at which one scan thread's range ends and the next one's begins"""
    return list(range(per_of(n), n, per_of(n)))


def chosen_boundaries(n):
    """the first, a middle and the last of them"""
    b = boundaries(n)
    return sorted({b[0], b[len(b) // 2], b[-1]})


# ------------------------------------------------------------------ depth: geometries
def depth_one_reference(n, T, w):
    """a single reference of n tiles whose last one is short"""
    return [(1, "one", (n * T - 5) * w + 1)]


def depth_one_tile_each(n, T, w):
    """n references of one tile each (1, 63, 64, 65, T - 1 and T windows in turn, none above T) on the ids 5 c + 2: n_ids > 4096 from
    n = 820 on.  Of the four ids between two of them every second gap holds a reference of length 0 at 5 c + 4 -- it does not exist --
    and the others stay holes.  No length is a multiple of w where w > 1."""
    counts = [min(c, T) for c in (1, 63, 64, 65, T - 1, T)]
    refs = []
    for c in range(n):
        nw = counts[c % 6]
        refs.append((5 * c + 2, "t%d" % c, nw if w == 1 else (nw - 1) * w + 1 + c % (w - 1)))
        if c & 1:
            refs.append((5 * c + 4, "z%d" % c, 0))
    return refs


def depth_mixed(n, T, w):
    """references of 1, 2, 3 and 5 tiles in turn (the last one trimmed: n tiles in all) on the ids 3 c + 1, their last tiles full or 7
    or 14 windows short"""
    refs, left, c = [], n, 0
    while left:
        k = min((1, 2, 3, 5)[c % 4], left)
        nw = k * T - 7 * (c % 3)
        refs.append((3 * c + 1, "m%d" % c, nw if w == 1 else (nw - 1) * w + 1 + c % w))
        left -= k
        c += 1
    return refs


DEPTH = {"one_reference": depth_one_reference, "one_tile_each": depth_one_tile_each, "mixed": depth_mixed}


# ------------------------------------------------------------------ depth: hits
def quiet_successors(refs, w, T):
    """indexes (among the existing references) of the "untouched successors": references whose first tile gets no hit although hits end
    in the last window of the reference in front of them.  About a dozen, never the first or the last reference, never two in a row, none
    that owns a tile at one of the chosen thread-range boundaries."""
    n, tl = tiles_of(refs, w, T)
    L = len(live_refs(refs))
    if L < 4:
        return []
    taken = {int(tl[t][0]) for b in chosen_boundaries(n) for t in (b - 1, b)}
    return [c for c in range(2, L - 1, max(2, L // 12)) if c not in taken]


def depth_hits(refs, T, w, seed):
    """about 20,000 hit records for a depth geometry: random ones (the reference in proportion to its length, the start uniform, lengths of
    one base, less than a window, less than a tile, several tiles, up to the reference's last base; 3 % of them with r_end behind the
    reference), the deterministic ones that carry a running count through the thread ranges of the scan, and about 3 % that the rules
    turn away (depth_model.crafted's kinds)."""
    rng = np.random.default_rng(seed)
    live = live_refs(refs)
    ids, lens = np.array([i for i, _ in live], dtype=np.int64), np.array([ln for _, ln in live], dtype=np.int64)
    nws = -(-lens // w)
    n, tl = tiles_of(refs, w, T)
    L, tile = len(live), T * w
    # random
    N = 19000
    ends = np.cumsum(lens)
    pos = rng.integers(0, int(ends[-1]), N)
    c = np.searchsorted(ends, pos, side="right")
    s = pos - (ends[c] - lens[c])
    kind = rng.integers(0, 5, N)
    span = np.ones(N, dtype=np.int64)
    span = np.where(kind == 1, rng.integers(1, max(w, 2), N), span)
    span = np.where(kind == 2, rng.integers(1, tile, N), span)
    span = np.where(kind == 3, rng.integers(tile, 6 * tile, N), span)
    e = np.where(kind == 4, lens[c] - 1, s + span - 1)
    e = np.where(rng.random(N) < 0.03, lens[c] + rng.integers(0, 5 * w + 1, N), e)
    mapq = rng.choice(np.array([0, 0, 0, 1, 59, 60, 60, 60, 60, 60, 60, 61, 255]), N)
    rows = [np.stack([np.full(N, MAPPED), ids[c], mapq, s, np.minimum(e, 0xFFFFFFFF)], axis=1)]
    det = []
    whole = lambda k, q=60: (MAPPED, ids[k], q, 0, lens[k] - 1)  # noqa: E731
    det += [whole(0), whole(L - 1), whole(0, 0)]
    if L == 1:  # from the middle of tile 0 into the last tile: the running count crosses every thread range
        det += [(MAPPED, ids[0], 60, tile // 2, (n - 1) * tile + w), (MAPPED, ids[0], 60, 0, 0xFFFFFFFF)]
    for b in chosen_boundaries(n):
        (rb, rt), (ra, _) = tl[b], tl[b - 1]
        g = int(rt) * T  # the boundary's first window, counted inside its reference
        if rt > 0:  # both sides in one reference: from the window before into the window behind, and from three before to three behind
            det.append((MAPPED, ids[rb], 60, (g - 1) * w + w // 2, min(g * w + w // 2, lens[rb] - 1)))
            det.append((MAPPED, ids[rb], 60, max(g - 3, 0) * w, min((g + 3) * w, lens[rb] - 1)))
        last = g - 1 if rt > 0 else int(nws[ra]) - 1  # the window in front of the boundary: a hit that ends on its last base
        det.append((MAPPED, ids[ra], 60, max(last - 5, 0) * w, min(last * w + w - 1, lens[ra] - 1)))
        det.append((MAPPED, ids[rb], 60, g * w, min((g + 4) * w, lens[rb] - 1)))  # and one that begins with the boundary
    # what the rules turn away
    all_ids = {int(i) for i, _, _ in refs}
    zero = sorted(int(i) for i, _, ln in refs if int(ln) == 0)
    holes = [i for i in range(int(ids[-1]) + 1) if i not in all_ids][:200]
    beyond = [int(ids[-1]) + 1, int(ids[-1]) + 2, 1 << 24, 0xFFFFFFFF]
    for j in range(600):
        k = int(rng.integers(0, L))
        rid, ln = ids[k], lens[k]
        what = j % 8
        if what == 0:
            det.append((0, rid, 60, 0, ln - 1))                        # unmapped
        elif what == 1:
            det.append((2, rid, 60, 0, ln - 1))                        # overflow
        elif what == 2:
            det.append((MAPPED, rid, 0, ln // 3, ln - 1))              # mapq 0
        elif what == 3 and holes:
            det.append((MAPPED, holes[j % len(holes)], 60, 0, 10))     # a hole
        elif what == 4:
            det.append((MAPPED, beyond[j // 8 % 4], 60, 0, 10))        # beyond the snapshot
        elif what == 5:
            det.append((MAPPED, rid, 60, ln + (j & 8), ln + 20))       # r_start >= len
        elif what == 6:
            det.append((MAPPED, rid, 60, min(ln - 1, 5) + (ln == 1), min(ln - 1, 5) - (ln > 1)))  # r_start > r_end
        else:
            det.append((MAPPED, zero[j % len(zero)] if zero else beyond[0], 60, 0, 0))  # a reference of length 0
    rows.append(np.array(det, dtype=np.int64))
    rows = np.concatenate(rows)
    # the untouched successors: nothing in their first tile; hits that end in the last window of the reference in front of each
    quiet = quiet_successors(refs, w, T)
    rows = rows[~(np.isin(rows[:, 1], ids[quiet]) & (rows[:, 3] < tile))] if quiet else rows
    front = [(MAPPED, ids[k - 1], 60, max(int(nws[k - 1]) - 4, 0) * w, lens[k - 1] - 1 + 2 * (k & 1)) for k in quiet]
    if front:
        rows = np.concatenate([rows, np.array(front, dtype=np.int64)])
    return DM.hits_of(rows[rng.permutation(rows.shape[0])])


def many_ids_hits(refs, w):
    """one hit on every existing reference (its whole length), and a burst of 50,000 identical hits on the one with the largest id"""
    live = live_refs(refs)
    rows = [(MAPPED, i, 60, 0, ln - 1) for i, ln in live]
    i, ln = live[-1]
    return DM.hits_of(rows + [(MAPPED, i, 60, ln // 2, ln + w)] * 50000)


def grouped_wording(refs, hits, window, min_mapq):
    """depth_model.window_wording with the hits grouped by reference once instead of one pass per reference:
    (window_bases, window_starts, diff, first window per existing reference).  diff is the difference array over the windows of all
    references behind one another; +1 and -1 of a hit land inside its reference (a + 1 < b <= its last window), so every reference's
    part sums to 0 and the running sum over the whole array is every reference's own."""
    w = int(window)
    hits = np.asarray(hits)
    cls, _ = DM.classify(refs, hits, min_mapq)
    live = live_refs(refs)
    ids, lens = np.array([i for i, _ in live], dtype=np.int64), np.array([ln for _, ln in live], dtype=np.int64)
    nws = -(-lens // w)
    first = np.cumsum(nws) - nws
    mine = hits[cls == 0]
    c = np.searchsorted(ids, mine["ref_id"].astype(np.int64))
    s = mine["r_start"].astype(np.int64)
    e = np.minimum(mine["r_end"].astype(np.int64), lens[c] - 1)
    a, b, at = s // w, e // w, first[c]
    total = int(nws.sum())
    edge, diff, starts = np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64), np.zeros(total, dtype=np.int64)
    np.add.at(starts, at + a, 1)
    one = a == b
    np.add.at(edge, (at + a)[one], (e - s + 1)[one])
    np.add.at(edge, (at + a)[~one], ((a + 1) * w - s)[~one])
    np.add.at(edge, (at + b)[~one], (e - b * w + 1)[~one])
    far = b > a + 1
    np.add.at(diff, (at + a + 1)[far], 1)
    np.add.at(diff, (at + b)[far], -1)
    return (np.cumsum(diff) * w + edge).astype(np.uint64), starts.astype(np.uint32), diff, first


# ------------------------------------------------------------------ coverage: geometries
STEP = 128 * 64  # bits a wave takes per step of a coverage tile


def cover_long_run(n, T):
    """(first tile, whole tiles) of one_reference's long run: it begins in the middle of tile `first`, covers the next `whole` tiles
    entirely and ends in the middle of the tile behind them.  More than SCAN whole tiles wherever n leaves room for them."""
    return 3, SCAN + 5 if n >= SCAN + 11 else n // 2


def cover_one_reference(n, T, seed=11):
    """one reference of n tiles, about 20,000 entries: random short intervals, intervals across word, step and tile borders at the first,
    a middle and the last thread-range boundary of the scan, duplicates, nested and dead entries, entries out of range, and the long run
    (cover_long_run) built from overlapping entries of one tile's length each"""
    rng = np.random.default_rng(seed)
    rid, ln = 2, n * T - 100
    s = rng.integers(1, ln - 200, 18500)
    e = s + rng.integers(1, 201, 18500) - 1
    ents = [(rid, int(a), int(b)) for a, b in zip(s, e)]
    ents += ents[:200]                                                              # duplicates
    ents += [(rid, a + 1, b - 1) for _, a, b in ents[200:500] if b - a > 2]        # nested
    for m in sorted({1, 2, n // 2, n - 2, n - 1} | set(chosen_boundaries(n))):
        P = m * T
        ents += [(rid, P - 5, P + 5), (rid, P - 300, P - 200), (rid, P - 190, P - 1), (rid, P + 1000, P + 1030)]
        if m & 1:
            ents.append((rid, P, P + 30))                                           # ends on P - 1, starts on P: one run
        for q in (STEP, 3 * STEP):
            if q < T:
                ents += [(rid, P - q - 10, P - q + 10), (rid, P - q + 64, P - q + 64)]
        for q in (5, 77):
            ents.append((rid, P - 64 * q - 3, P - 64 * q + 5))
    d = rng.integers(1, ln - T, 300)
    ents += [(rid, int(a), int(a) + int(x), 2) for a, x in zip(d, rng.integers(1000, T, 300))]  # dead: inserted twice
    ents += [(rid, 3000, 0), (rid, 0, 0)]                                           # born dead
    ents += [(rid, ln, ln + 5), (rid, ln + 1000, ln + 1000), (rid, 500, 400), (rid, 2**32 - 1, 2**32 - 1)]  # out of range
    ents += [(rid, ln - 30, ln + 50), (rid, 0, 7)]                                  # clamped to the last base; the first bases
    t0, whole = cover_long_run(n, T)
    a, stop = t0 * T + T // 2 + 7, (t0 + 1 + whole) * T + T // 2 - 9
    while a + T - 1 < stop:
        ents.append((rid, a, a + T - 1))
        a += T - 37
    ents.append((rid, a, stop))
    return CM.Case("one_reference %d" % n, [(rid, "one", ln)], ents)


COVER_LENGTHS = (1, 63, 64, 65, 128, 200)


def cover_silent(c):
    """one_tile_each: reference number c has no entry -- two of every six, and every length in turn"""
    return (c // 6 + c) % 3 == 2


def cover_one_tile_each(n, T):
    """n references of 1, 63, 64, 65, 128 and 200 bases in turn on the ids 5 c + 2 (n_ids > 4096); a third of them without an entry, the
    others with one to three; of those, every one whose length is a multiple of 64 is covered up to its last base (the end at len), and
    the ones of length 1 by a clamped entry"""
    refs, ents = [], []
    for c in range(n):
        rid, ln = 5 * c + 2, COVER_LENGTHS[c % 6]
        refs.append((rid, "t%d" % c, ln))
        if cover_silent(c):
            continue
        head, tail, mid = (rid, 0, min(5, ln + 2)), (rid, max(ln - 40, 0), ln + 3), (rid, ln // 2, ln // 2 + 3)
        if ln == 1:
            cand = [(rid, 0, 3), (rid, 0, 0), (rid, 0, 9, 2)]
        elif ln % 64 == 0:
            cand = [tail, head, mid]
        else:
            cand = [head, mid, tail]
        ents += cand[:1 + (c // 6) % 3]
    return CM.Case("one_tile_each %d" % n, refs, ents)


def cover_mixed(n, T):
    """references of T - 1, T, T + 1, 2 T + 65 and 64 bases in turn (1, 1, 2, 3 and 1 tiles; the last one trimmed: n tiles in all) on the
    ids 2 c + 1 (below 4,096: the workgroup histogram with more than a thousand references), with entries at each one's first bases,
    across each of its tile borders and up to its last base, and c % 7 short runs of their own in the first tile of the long ones: the
    tiles' run counts differ from one tile to the next"""
    refs, ents, left, c = [], [], n, 0
    while left:
        ln = (T - 1, T, T + 1, 2 * T + 65, 64)[c % 5]
        k = -(-ln // T)
        if k > left:
            k, ln = left, (left - 1) * T + 70
        rid = 2 * c + 1
        refs.append((rid, "m%d" % c, ln))
        ents.append((rid, 0, 5))
        for j in range(1, k + 1):  # (behind the reference's last tile the border is its end: the entry is clamped there)
            if j * T - 10 >= ln:
                continue
            if c % 4 == 3:
                ents += [(rid, j * T - 10, j * T - 1), (rid, j * T, j * T + 10)]  # ends on the border, begins on it: one run
            else:
                ents.append((rid, j * T - 10, j * T + 10))
        ents.append((rid, max(ln - 40, 0), ln + 3))
        if c & 1 and ln > 200:
            ents.append((rid, ln // 2, ln // 2 + 70))
        if ln > 4000:
            ents += [(rid, 1000 + 300 * i, 1000 + 300 * i + c % 50) for i in range(c % 7)]
        left -= k
        c += 1
    return CM.Case("mixed %d" % n, refs, ents)


def cover_comb(T):
    """one reference of 2 T + 65 bases with a one-base entry at every even position of [T - 4096, T + 4096): 32 runs per word, 4,096 per
    step of a wave, across a tile border; where a tile has room for it (T >= 4 steps) the same comb at the odd positions of
    [STEP - 64, STEP + 64), across the step border inside tile 0.  (Position 0 is avoided: [0, 0] is born dead.)"""
    ents = [(0, p, p) for p in range(T - 4096, T + 4096, 2)]
    if T >= 4 * STEP:
        ents += [(0, p, p) for p in range(STEP - 63, STEP + 64, 2)]
    return CM.Case("comb", [(0, "comb", 2 * T + 65)], ents)


COVERAGE = {"one_reference": cover_one_reference, "one_tile_each": cover_one_tile_each, "mixed": cover_mixed}
