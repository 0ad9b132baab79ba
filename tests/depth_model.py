"""A numpy model of the depth accumulator (mq_depth), written from the rules in include/mapquik_hip.h and from nothing else: a count per
BASE of every reference (one difference array per reference over its bases, then a prefix sum), and window sums of that.  The
kernels never hold a per-base array; tests/test_depth_model.py holds this model against a second wording (the difference array over
WINDOWS that the kernels use) on the crafted cases below, which the GPU tests then run through the library.

    model(refs, hits, window, min_mapq) -> (records, window_bases, window_starts, totals)
refs: (id, name, length) triples (tests/mqx.py's); hits: api.hit_dtype records.  records has the layout of api.ref_depth_dtype."""
import numpy as np

MAPPED = 1
hit_dtype = np.dtype([(n, "<u4") for n in ("status", "ref_id", "rc", "mapq", "q_start", "q_end", "r_start", "r_end", "score", "n_kminmers", "q_start_hi", "q_end_hi")])
ref_depth_dtype = np.dtype([("ref_id", "<u4"), ("reserved", "<u4"), ("len", "<u8"), ("n_windows", "<u8"), ("first_window", "<u8"), ("reads", "<u8"),
                            ("bases", "<u8"), ("zero_windows", "<u8"), ("max_window_bases", "<u8")])
TOTALS = ("offered", "counted", "not_mapped", "below_mapq", "out_of_range")


def classify(refs, hits, min_mapq):
    """per hit: 0 counted, 1 not_mapped, 2 below_mapq, 3 out_of_range -- in the header's order of the tests"""
    lens = {int(i): int(n) for i, _, n in refs if int(n) > 0}
    ln = np.array([lens.get(int(i), 0) for i in hits["ref_id"]], dtype=np.int64)
    s, e = hits["r_start"].astype(np.int64), hits["r_end"].astype(np.int64)
    cls = np.zeros(hits.size, dtype=np.int64)
    oor = (ln == 0) | (s > e) | (s >= ln)
    cls[oor] = 3
    cls[hits["mapq"] < min_mapq] = 2
    cls[hits["status"] != MAPPED] = 1
    return cls, ln


def model(refs, hits, window, min_mapq):
    w = int(window)
    assert 1 <= w <= 1 << 24
    hits = np.asarray(hits)
    cls, ln = classify(refs, hits, min_mapq)
    totals = dict(offered=int(hits.size), counted=int((cls == 0).sum()), not_mapped=int((cls == 1).sum()), below_mapq=int((cls == 2).sum()),
                  out_of_range=int((cls == 3).sum()))
    live = sorted((int(i), int(n)) for i, _, n in refs if int(n) > 0)
    recs = np.zeros(len(live), dtype=ref_depth_dtype)
    wb, ws = [], []
    first = 0
    for c, (rid, length) in enumerate(live):
        mine = hits[(cls == 0) & (hits["ref_id"] == rid)]
        s = mine["r_start"].astype(np.int64)
        e = np.minimum(mine["r_end"].astype(np.int64), length - 1)
        d = np.zeros(length + 1, dtype=np.int64)
        np.add.at(d, s, 1)
        np.add.at(d, e + 1, -1)
        per_base = np.cumsum(d[:length])
        at = np.zeros(length, dtype=np.int64)
        np.add.at(at, s, 1)
        edges = np.arange(0, length, w)
        bases, starts = np.add.reduceat(per_base, edges), np.add.reduceat(at, edges)
        recs[c] = (rid, 0, length, edges.size, first, mine.size, int(bases.sum()), int((bases == 0).sum()), int(bases.max()))
        first += edges.size
        wb.append(bases.astype(np.uint64))
        ws.append(starts.astype(np.uint32))
    return recs, (np.concatenate(wb) if wb else np.zeros(0, np.uint64)), (np.concatenate(ws) if ws else np.zeros(0, np.uint32)), totals


def window_wording(refs, hits, window, min_mapq):
    """The same result worded on WINDOWS: per counted hit a = s // w, b = e // w; the bases in a and in b are added where they fall, +1 /
    -1 go into a difference array over the windows strictly between, and window_bases = running count * w + those edge bases."""
    w = int(window)
    hits = np.asarray(hits)
    cls, _ = classify(refs, hits, min_mapq)
    live = sorted((int(i), int(n)) for i, _, n in refs if int(n) > 0)
    wb, ws = [], []
    for rid, length in live:
        nw = -(-length // w)
        mine = hits[(cls == 0) & (hits["ref_id"] == rid)]
        s = mine["r_start"].astype(np.int64)
        e = np.minimum(mine["r_end"].astype(np.int64), length - 1)
        a, b = s // w, e // w
        edge, diff, starts = np.zeros(nw, dtype=np.int64), np.zeros(nw + 1, dtype=np.int64), np.zeros(nw, dtype=np.int64)
        np.add.at(starts, a, 1)
        one = a == b
        np.add.at(edge, a[one], (e - s + 1)[one])
        np.add.at(edge, a[~one], ((a + 1) * w - s)[~one])
        np.add.at(edge, b[~one], (e - b * w + 1)[~one])
        far = b > a + 1
        np.add.at(diff, (a + 1)[far], 1)
        np.add.at(diff, b[far], -1)
        assert int(diff.sum()) == 0
        wb.append((np.cumsum(diff[:nw]) * w + edge).astype(np.uint64))
        ws.append(starts.astype(np.uint32))
    return (np.concatenate(wb) if wb else np.zeros(0, np.uint64)), (np.concatenate(ws) if ws else np.zeros(0, np.uint32))


def hits_of(rows):
    """hit records from (status, ref_id, mapq, r_start, r_end) rows; the other fields carry a pattern no rule reads"""
    h = np.zeros(len(rows), dtype=hit_dtype)
    if len(rows):
        a = np.array(rows, dtype=np.int64)
        for j, f in enumerate(("status", "ref_id", "mapq", "r_start", "r_end")):
            h[f] = a[:, j].astype(np.uint32)
        h["rc"] = np.arange(len(rows)) & 1
        h["q_start"], h["q_end"], h["score"], h["n_kminmers"] = 0xDEAD, 0xBEEF, 11, 0xFFFFFFFF
        h["q_start_hi"], h["q_end_hi"] = 0xFFFFFFFF, 0xFFFFFFFF
    return h


IDS = (0, 2, 3, 7, 8, 12, 13, 20)  # sparse: holes at 1, 4-6, 9-11, 14-19


def crafted(T, w):
    """(refs, hits) for window w and tile size T: references of length 1, w-1, w, w+1, T*w-1, T*w, T*w+1 and 2*T*w+1 on sparse ids, and
    on each of them hits whose ends sit on the borders of its first, its tile-border and its last windows and one base to either side,
    one-base hits, the whole reference, ends behind the reference (clipped), and everything the rules turn away."""
    lens = []
    for n in (1, w - 1, w, w + 1, T * w - 1, T * w, T * w + 1, 2 * T * w + 1):
        if n >= 1 and n not in lens:
            lens.append(n)
    refs = [(IDS[j], "ref%d" % IDS[j], n) for j, n in enumerate(lens)]
    rows = []
    k = 0
    for rid, _, n in refs:
        nw = -(-n // w)
        pts = {0, n - 1}
        for j in (0, 1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, nw - 1, nw):
            for d in (-1, 0, 1):
                p = j * w + d
                if 0 <= p < n:
                    pts.add(p)
        pts = sorted(pts)
        for s in pts:
            for e in pts:
                if s <= e:
                    rows.append((MAPPED, rid, 60 if k % 3 else 0, s, e))
                    k += 1
            rows.append((MAPPED, rid, 60, s, s))           # one base
            rows.append((MAPPED, rid, 60, s, n))           # r_end == len: clipped
            rows.append((MAPPED, rid, 0, s, n + 5 * w))    # far behind: clipped
        rows.append((MAPPED, rid, 60, 0, n - 1))           # the whole reference
        rows.append((MAPPED, rid, 60, 0, 0xFFFFFFFF))
        rows.append((MAPPED, rid, 60, n, n + 3))           # r_start >= len
        rows.append((MAPPED, rid, 60, n + 7, n + 7))
        if n > 1:
            rows.append((MAPPED, rid, 60, n - 1, n - 2))   # r_start > r_end
            rows.append((MAPPED, rid, 0, 1, 0))
        rows.append((0, rid, 60, 0, n - 1))                # unmapped, overflow
        rows.append((2, rid, 60, 0, n - 1))
        rows.append((0, rid, 0, 0, 0))
    for rid in (1, 5, 19):                                 # holes
        rows.append((MAPPED, rid, 60, 0, 0))
    for rid in (21, 22, 1 << 24, 0xFFFFFFFF):              # beyond the snapshot
        rows.append((MAPPED, rid, 60, 0, 10))
    return refs, hits_of(rows)


def carry_case(T, w):
    """A hit from tile 0 of one reference into its tile 2 (the count crosses two tile borders), hits that end in that reference's last
    window, and, next in id order, a reference whose first windows nobody touches: no carry may leak into it."""
    refs = [(4, "a", 3 * T * w), (5, "b", 2 * T * w + 3), (9, "c", w)]
    rows = [(MAPPED, 4, 60, w // 2, 2 * T * w + w + 1), (MAPPED, 4, 60, 5 * w, 3 * T * w - 1), (MAPPED, 4, 60, 0, 3 * T * w + 9),
            (MAPPED, 5, 60, T * w, T * w + 3 * w), (MAPPED, 9, 60, 0, 0)]
    return refs, hits_of(rows)


def bed_bytes(refs, recs, window_bases, window_starts, window):
    """<prefix>.depth.bed as both drivers write it"""
    names = {int(i): n for i, n, _ in refs}
    out = []
    for r in recs:
        f, n = int(r["first_window"]), int(r["len"])
        for j in range(int(r["n_windows"])):
            a, b = j * window, min((j + 1) * window, n)
            v = int(window_bases[f + j])
            out.append("%s\t%d\t%d\t%d\t%d\t%.2f\n" % (names[int(r["ref_id"])], a, b, v, int(window_starts[f + j]), v / (b - a)))
    return "".join(out).encode()


TSV_HEAD = "#ref\tlen\treads\tbases\tmean\tzero_windows\tmax_window_mean\n"


def tsv_bytes(refs, recs, window):
    names = {int(i): n for i, n, _ in refs}
    out = [TSV_HEAD]
    for r in recs:
        n = int(r["len"])
        out.append("%s\t%d\t%d\t%d\t%.2f\t%d\t%.2f\n" % (names[int(r["ref_id"])], n, int(r["reads"]), int(r["bases"]), int(r["bases"]) / n, int(r["zero_windows"]),
                                                      int(r["max_window_bases"]) / min(window, n)))
    return "".join(out).encode()


def log_line(recs, totals, window, min_mapq):
    return "Depth: %d of %d hits counted (%d not mapped, %d below mapq %d, %d out of range): %d bases in %d windows of %d" % (
        totals["counted"], totals["offered"], totals["not_mapped"], totals["below_mapq"], min_mapq, totals["out_of_range"], int(recs["bases"].sum()),
        int(recs["n_windows"].sum()), window)


def hits_of_paf(paf_text, refs):
    """the hits a PAF's lines stand for: one mapped hit per line (columns 6, 8, 9 and 12)"""
    ids = {n: int(i) for i, n, _ in refs}
    rows = []
    for ln in paf_text.splitlines():
        f = ln.split("\t")
        rows.append((MAPPED, ids[f[5]], int(f[11]), int(f[7]), int(f[8])))
    return hits_of(rows)
