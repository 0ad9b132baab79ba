"""A model of the index coverage (mq_index_coverage) and crafted index files for it.

Written from the semantics the feature freezes, in plain numpy, by sorting and merging intervals -- not from the kernels, which keep a
bitmap.  A slot is live iff count == 1 and end != 0.  A live entry of a reference of length len covers [start, min(end, len - 1)], both
inclusive; one with start > end or start >= len covers nothing and counts as out of range.  A reference's coverage is the union of its
live entries' intervals: the maximal runs, half-open, sorted by reference id and start, never running from one reference into the next.
References of length 0 do not exist.  test_coverage_model.py holds this against a per-base boolean array and against the oracle.

`crafted_cases(T)`: index files (mqx.write) whose interval sets sit on every edge of a layout that keeps one bit per base in 64-bit
words, cut into tiles of T bits that never span two references.
"""
import numpy as np

import mqx

ref_coverage_dtype = np.dtype([("ref_id", "<u4"), ("reserved", "<u4"), ("len", "<u8"), ("live_kminmers", "<u8"), ("covered_bases", "<u8"),
                               ("n_intervals", "<u8"), ("first_interval", "<u8")])
cov_interval_dtype = np.dtype([("start", "<u4"), ("end", "<u4")])


def live_in_range(slots, refs):
    """(per-slot reference id, live mask, in-range mask, clamped inclusive end) of a slot array under a reference list"""
    lens = {int(i): int(ln) for i, _, ln in refs if int(ln) > 0}
    ids = (slots["id_rc"] >> np.uint32(1)).astype(np.int64)
    ln = np.array([lens.get(int(i), 0) for i in ids], dtype=np.int64)
    live = (slots["count"] == 1) & (slots["end"] != 0)
    start, end = slots["start"].astype(np.int64), slots["end"].astype(np.int64)
    ok = live & (ln > 0) & (start <= end) & (start < ln)
    return ids, live, ok, np.minimum(end, ln - 1)


def model(slots, refs):
    """(records, intervals, out_of_range) of a slot array (mqx.slot_dtype) and a reference list of (id, name, length)"""
    ids, live, ok, last = live_in_range(slots, refs)
    recs, ivs = [], []
    for rid, _, ln in sorted((int(i), n, int(ln)) for i, n, ln in refs):
        if ln == 0:
            continue
        m = ok & (ids == rid)
        spans = sorted(zip(slots["start"][m].astype(np.int64).tolist(), (last[m] + 1).tolist()))
        first, covered = len(ivs), 0
        for a, b in spans:
            if len(ivs) > first and a <= ivs[-1][1]:
                ivs[-1][1] = max(ivs[-1][1], b)
            else:
                ivs.append([a, b])
        covered = sum(b - a for a, b in ivs[first:])
        recs.append((rid, 0, ln, int(m.sum()), covered, len(ivs) - first, first))
    return (np.array(recs, dtype=ref_coverage_dtype), np.array([tuple(x) for x in ivs], dtype=cov_interval_dtype).reshape(-1), int((live & ~ok).sum()))


def brute(slots, refs):
    """the same from one boolean per base: {id: covered array}, and the live in-range entries per id"""
    ids, _, ok, last = live_in_range(slots, refs)
    out, n = {}, {}
    for rid, _, ln in refs:
        if int(ln) == 0:
            continue
        c = np.zeros(int(ln), dtype=bool)
        for i in np.flatnonzero(ok & (ids == int(rid))):
            c[int(slots["start"][i]):int(last[i]) + 1] = True
        out[int(rid)], n[int(rid)] = c, int((ok & (ids == int(rid))).sum())
    return out, n


def runs_of(c):
    """half-open maximal runs of a boolean array"""
    d = np.diff(np.concatenate([[0], c.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def bed_bytes(refs, recs, ivs):
    names = {int(i): n for i, n, _ in refs}
    return b"".join(b"%s\t%d\t%d\n" % (names[int(r["ref_id"])].encode(), int(v["start"]), int(v["end"]))
                    for r in recs for v in ivs[int(r["first_interval"]):int(r["first_interval"]) + int(r["n_intervals"])])


def tsv_bytes(refs, recs):
    names = {int(i): n for i, n, _ in refs}
    return b"#ref\tlen\tlive_kminmers\tcovered\tfraction\tintervals\n" + b"".join(
        b"%s\t%d\t%d\t%d\t%.6f\t%d\n" % (names[int(r["ref_id"])].encode(), int(r["len"]), int(r["live_kminmers"]), int(r["covered_bases"]),
                                        int(r["covered_bases"]) / int(r["len"]), int(r["n_intervals"])) for r in recs)


# ------------------------------------------------------------------ crafted files
P = mqx.params(k=3, l=12, density=0.05)


class Case:
    """refs: (id, name, len); ents: (id, start, end) or (id, start, end, count) or (id, start, end, count, key)"""

    def __init__(self, name, refs, ents, table_slots=None):
        self.name, self.refs = name, [(int(i), n, int(ln)) for i, n, ln in refs]
        s = np.zeros(len(ents), dtype=mqx.slot_dtype)
        for j, e in enumerate(ents):
            e = tuple(e) + (1, None)[len(e) - 3:]
            key = (0x9E3779B97F4A7C15 * (j + 1)) % 2**64 if e[4] is None else e[4]
            s[j] = (e[1], e[2], j, (e[0] << 1) | (j & 1), key, e[3], 1 if key == 0 else 0)
        self.slots = s
        self.table_slots = table_slots or mqx.pow2_above(max(len(ents), 1))
        self.params = P

    def write(self, path):
        mqx.write(str(path), self.params, self.table_slots, self.refs, self.slots)
        return str(path)


def _from_table(t):
    c = Case(t.name, t.refs, [])
    c.slots, c.table_slots, c.params = t.slots(), t.table_slots, t.params
    return c


LENGTHS = lambda T: (1, 63, 64, 65, 128, T - 1, T, T + 1, 2 * T + 65)  # noqa: E731


def crafted_cases(T, src=None):
    """The cases of the issue, by name.  src: an mqx.Source ("small" leg) for the table shapes; None leaves them out."""
    R = lambda *lens: [(i, "r%d" % i, ln) for i, ln in enumerate(lens)]  # noqa: E731
    big = 2 * T + 65
    cases = []
    # reference lengths: every one covered at its first bases and up to its last base (the entry that reaches the end is clamped there;
    # a reference of length 1 can only be covered by a clamped entry, [0, 0] itself is born dead)
    lens = LENGTHS(T)
    ents = []
    for i, ln in enumerate(lens):
        ents += [(i, 0, min(5, ln + 2))] + ([(i, max(ln - 40, 0), ln + 3)] if ln > 1 else [])
    cases.append(Case("reference lengths", R(*lens), ents))
    cases.append(Case("start == end", R(1000), [(0, 5, 5), (0, 700, 700)]))
    cases.append(Case("[1, 1]", R(1000), [(0, 1, 1)]))
    cases.append(Case("words apart", R(1000, 1000, 1000), [(0, 0, 63), (1, 63, 64), (2, 64, 127)]))
    cases.append(Case("adjacent", R(1000), [(0, 0, 63), (0, 63, 64), (0, 64, 127)]))
    cases.append(Case("adjacent without overlap", R(1000), [(0, 0, 63), (0, 64, 127), (0, 128, 128), (0, 130, 140)]))
    cases.append(Case("inside one word", R(1000), [(0, 70, 90)]))
    cases.append(Case("three words", R(1000), [(0, 60, 130)]))
    cases.append(Case("more than a tile", R(big), [(0, 10, T + 100)]))
    cases.append(Case("ends on T - 1", R(big), [(0, T - 50, T - 1)]))
    cases.append(Case("starts on T", R(big), [(0, T, T + 30)]))
    cases.append(Case("ends on T - 1, starts on T", R(big), [(0, T - 50, T - 1), (0, T, T + 30)]))
    cases.append(Case("crosses T", R(big), [(0, T - 10, T + 10), (0, 3, 4)]))
    cases.append(Case("crosses two tile borders", R(big), [(0, T - 10, 2 * T + 10), (0, 2 * T + 40, 2 * T + 64)]))
    cases.append(Case("whole tiles", R(big), [(0, 0, 2 * T - 1)]))
    cases.append(Case("whole reference", R(2 * T), [(0, 0, 2 * T - 1)]))
    cases.append(Case("no run across references", R(64, 50, T, 100, 128, 70), [(0, 10, 63), (1, 0, 20), (2, T - 20, T - 1), (3, 0, 9), (4, 64, 127), (5, 0, 69)]))
    cases.append(Case("overlapping and nested", R(1000), [(0, 100, 300), (0, 200, 400), (0, 250, 260), (0, 500, 600), (0, 500, 600), (0, 601, 650)]))
    cases.append(Case("dead entries", R(5000), [(0, 10, 50), (0, 1000, 1100, 2), (0, 2000, 2100, 7), (0, 0, 0), (0, 3000, 0), (0, 30, 1050, 2)]))
    cases.append(Case("key 0 live", R(1000), [(0, 10, 50, 1, 0), (0, 100, 120)]))
    cases.append(Case("key 0 dead", R(1000), [(0, 10, 50, 2, 0), (0, 100, 120)]))
    cases.append(Case("key 0 alone", R(1000), [(0, 10, 50, 1, 0)], table_slots=2))
    cases.append(Case("out of range", R(100, 100), [(0, 90, 150), (0, 100, 120), (0, 200, 300), (1, 50, 40), (1, 99, 99), (1, 2**32 - 1, 2**32 - 1), (0, 4, 2**32 - 1, 2)]))
    cases.append(Case("a reference with no live entry", R(500, 500, 500), [(0, 10, 50), (1, 10, 50, 2), (2, 400, 499)]))
    cases.append(Case("no entry at all", R(500), []))
    top = mqx.MAX_REF_ID - 1
    cases.append(Case("sparse ids", [(5, "five", 300), (1000, "", 64), (top, "top", T + 1)], [(5, 0, 10), (5, 290, 299), (1000, 0, 63), (top, T - 1, T), (top, 3, 9)]))
    # 4,097 ids: one past the range the kernel counts through a workgroup histogram
    cases.append(Case("4097 ids", [(0, "a", 200), (4095, "b", 200), (4096, "c", 200)], [(0, 1, 100), (4095, 2, 150), (4096, 3, 199), (4096, 5, 7)]))
    if src is not None:
        cases += [_from_table(t) for t in mqx.tiny_tables(src)] + [_from_table(mqx.one_empty(src)), _from_table(mqx.table_end(src))]
    return cases
