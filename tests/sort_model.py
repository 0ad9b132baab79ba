"""A numpy model of the coordinate sorter (mq_sorter), written from the rules in include/mapquik_hip.h and from nothing else: filter, then
np.lexsort((ordinal, r_start, ref_id)).  tests/test_sort_model.py holds it against a second wording (Python's sorted on tuples) and proves
that every crafted case below has the property it is named after; the GPU tests then run the cases through the library.

    model(refs, hits, ordinals, min_mapq) -> (order, records, totals)
refs: (id, name, length) triples (tests/mqx.py's); hits: api.hit_dtype records; ordinals: one u32 per hit.  records has the layout of
api.sort_ref_dtype.  passes(...) says how many of the key's 11 digits a sort of the kept records cannot skip."""
import numpy as np

from depth_model import hit_dtype, hits_of_paf  # noqa: F401  (the record layout; a PAF's lines as hits)

MAPPED, UNMAPPED, OVERFLOW = 1, 0, 2
sort_ref_dtype = np.dtype([("ref_id", "<u4"), ("reserved", "<u4"), ("first", "<u8"), ("count", "<u8")])
TOTALS = ("offered", "kept", "not_mapped", "below_mapq", "out_of_range")
DIGITS = 11
SCAN_THREADS = 256  # the workgroup of sort_scan_kernel takes this many tiles per step; one case has more tiles than that


def make_hits(ref_id, r_start, status=MAPPED, mapq=60):
    """hit records with these columns (scalars broadcast); every field the rules do not read is filled with noise"""
    ref_id = np.asarray(ref_id, dtype=np.uint32)
    h = np.zeros(ref_id.size, dtype=hit_dtype)
    h["ref_id"], h["r_start"], h["status"], h["mapq"] = ref_id, r_start, status, mapq
    h["rc"] = np.arange(h.size) & 1
    h["q_start"], h["q_end"], h["r_end"], h["score"], h["n_kminmers"] = 0xDEAD, 0xBEEF, 0xFFFFFFFF, 11, 0xFFFFFFFF
    h["q_start_hi"], h["q_end_hi"] = 0xFFFFFFFF, 0xFFFFFFFF
    return h


def classify(refs, hits, min_mapq):
    """per hit: 0 kept, 1 not_mapped, 2 below_mapq, 3 out_of_range -- in the header's order of the tests"""
    live = np.array(sorted(int(i) for i, _, n in refs if int(n) > 0), dtype=np.int64)
    cls = np.zeros(hits.size, dtype=np.int64)
    cls[~np.isin(hits["ref_id"].astype(np.int64), live)] = 3
    cls[hits["mapq"] < min_mapq] = 2
    cls[hits["status"] != MAPPED] = 1
    return cls


def model(refs, hits, ordinals, min_mapq):
    hits, ordinals = np.asarray(hits), np.asarray(ordinals, dtype=np.uint32)
    assert hits.size == ordinals.size
    cls = classify(refs, hits, min_mapq)
    totals = dict(offered=int(hits.size), kept=int((cls == 0).sum()), not_mapped=int((cls == 1).sum()), below_mapq=int((cls == 2).sum()),
                  out_of_range=int((cls == 3).sum()))
    k = cls == 0
    rid, rs, od = hits["ref_id"][k], hits["r_start"][k], ordinals[k]
    perm = np.lexsort((od, rs, rid))
    live = sorted(int(i) for i, _, n in refs if int(n) > 0)
    recs = np.zeros(len(live), dtype=sort_ref_dtype)
    srt = rid[perm]
    for c, i in enumerate(live):
        a, b = np.searchsorted(srt, i, "left"), np.searchsorted(srt, i, "right")
        recs[c] = (i, 0, a, b - a)
    return od[perm].astype(np.uint32), recs, totals


def digits(ref_id, r_start, ordinal):
    """[11, n]: the 8-bit digits of the 88-bit key, least significant first"""
    key = (np.asarray(ref_id, dtype=np.uint64) << np.uint64(32)) | np.asarray(r_start, dtype=np.uint64)
    o = np.asarray(ordinal, dtype=np.uint64)
    return np.stack([(o >> np.uint64(8 * d)) & np.uint64(255) for d in range(4)] + [(key >> np.uint64(8 * d)) & np.uint64(255) for d in range(7)])


def passes(refs, hits, ordinals, min_mapq):
    """the digit positions in which the kept records differ: what mqdiag_sort_passes must report"""
    k = classify(refs, np.asarray(hits), min_mapq) == 0
    if not k.any():
        return 0
    dg = digits(hits["ref_id"][k], hits["r_start"][k], np.asarray(ordinals)[k])
    return int(sum(np.unique(dg[d]).size > 1 for d in range(DIGITS)))


def runs(ordinals):
    """[(begin, end)]: the maximal stretches of consecutive ordinals -- each can go into one add call"""
    o = np.asarray(ordinals, dtype=np.int64)
    if o.size == 0:
        return []
    cut = np.flatnonzero(np.diff(o) != 1) + 1
    return list(zip(np.concatenate([[0], cut]).tolist(), np.concatenate([cut, [o.size]]).tolist()))


# ------------------------------------------------------------------ crafted cases
REFS = [(0, "a", 1000), (2, "b", 5), (3, "c", 1 << 20), (7, "d", 999), (300, "e", 70000), (70000, "f", 9)]  # holes at 1, 4-6, ...
LIVE = [r[0] for r in REFS]
# ref_id digits: 256 ids that differ in ONE byte of the id, the other two bytes all ones, so the largest is 2^24 - 1
DIGIT_IDS = {8: [0xFFFF00 | v for v in range(256)], 9: [0xFF00FF | (v << 8) for v in range(256)], 10: [0x00FFFF | (v << 16) for v in range(256)]}
DIGIT_REFS = [(i, "s%06x" % i, 10 + (i & 7)) for i in sorted(set(sum(DIGIT_IDS.values(), [])))]


def border_counts(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, SCAN_THREADS * T + T + 5]


def sized(n, seed=1):
    """n kept hits on REFS, random keys with many repeats, ordinals 0 .. n - 1"""
    rng = np.random.default_rng(seed + n)
    return make_hits(rng.choice(LIVE, n), rng.integers(0, 1 << 12, n) << rng.integers(0, 21, n)), np.arange(n, dtype=np.uint32)


def digit_case(d, tagged=False):
    """(refs, hits, ordinals): 256 records that differ in digit d of the key and in nothing else, shuffled.  Digits 0 .. 3 are the
    ordinal's bytes (one key; the other ordinal bytes as large as they go, so the ordinals reach 2^32 - 2), 4 .. 7 r_start's, 8 .. 10
    ref_id's -- with ONE ordinal for all (legal: the keys differ), so the order that comes back cannot show where a record went; tagged
    gives such a case ordinals whose lowest byte is a second permutation: two digits differ, and the order shows digit d deciding."""
    rng = np.random.default_rng(40 + d)
    v = rng.permutation(256).astype(np.uint64)
    if d < 4:
        fixed = 0xFFFFFE00 if d == 0 else 0xFFFFFFFE & ~(0xFF << (8 * d))
        return REFS, make_hits(np.full(256, 3), 0x01020304), ((v << np.uint64(8 * d)) | np.uint64(fixed)).astype(np.uint32)
    ords = (np.uint32(0x01020300) | rng.permutation(256).astype(np.uint32)) if tagged else np.full(256, 0x01020304, dtype=np.uint32)
    if d < 8:
        fixed = 0xA5C3F00F & ~(0xFF << (8 * (d - 4)))
        return REFS, make_hits(np.full(256, 300), ((v << np.uint64(8 * (d - 4))) | np.uint64(fixed)).astype(np.uint32)), ords
    return DIGIT_REFS, make_hits(np.array(DIGIT_IDS[d], dtype=np.uint32)[v.astype(np.int64)], 0x80000001), ords


def stability_cases(T):
    """name -> (hits, ordinals) on REFS, each 3 T + 17 records with ordinals 0 .. n - 1"""
    n = 3 * T + 17
    i = np.arange(n)
    rng = np.random.default_rng(9)
    rnd_id, rnd_rs = rng.choice(LIVE, n), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    by_key = np.lexsort((rnd_rs, rnd_id))
    return {
        "all_keys_equal": make_hits(np.full(n, 7), 123456),               # the order must be the ordinals'
        "two_keys_lane_by_lane": make_hits(np.full(n, 3), (i & 1) * 256),  # neighbours in a wave alternate between two bins
        "one_bin_but_low_byte": make_hits(np.full(n, 3), (i % 251) << 8),  # digit 4 is one bin for all, digit 5 spreads them
        "one_per_bin": make_hits(np.full(n, 3), i % 256),                  # every round of a wave meets 64 different bins
        "sorted": make_hits(rnd_id[by_key], rnd_rs[by_key]),
        "reversed": make_hits(rnd_id[by_key][::-1], rnd_rs[by_key][::-1]),
        "random": make_hits(rnd_id, rnd_rs),
    }, np.arange(n, dtype=np.uint32)


def filter_case(T):
    """2 T + 130 hits on REFS, kept but for the ones the rules turn away, which sit on the wave and tile borders and at random places:
    unmapped, overflow, every mapq around the thresholds 1 and 60, ids in holes and beyond the snapshot"""
    n = 2 * T + 130
    rng = np.random.default_rng(12)
    h = make_hits(rng.choice(LIVE, n), rng.integers(0, 1 << 20, n), mapq=rng.choice([0, 1, 59, 60, 255], n))
    at = np.unique(np.concatenate([[0, 1, 62, 63, 64, 65, 127, 128, T - 1, T, T + 1, 2 * T - 1, 2 * T, n - 1], rng.integers(0, n, n // 5)]))
    kind = rng.integers(0, 4, at.size)
    h["status"][at[kind == 0]] = UNMAPPED
    h["status"][at[kind == 1]] = OVERFLOW
    h["ref_id"][at[kind == 2]] = rng.choice([1, 4, 6, 299, 69999], int((kind == 2).sum()))          # holes
    h["ref_id"][at[kind == 3]] = rng.choice([70001, 1 << 24, 0xFFFFFFFF], int((kind == 3).sum()))  # beyond the snapshot
    return h, np.arange(5, n + 5, dtype=np.uint32)


# ------------------------------------------------------------------ the drivers' files
TSV_HEAD = "#ref\tlen\tlines\tfirst_line\toffset\n"


def sorted_files(refs, paf_bytes, min_mapq):
    """(<prefix>.sorted.paf, <prefix>.sorted.tsv, records, totals of the kept lines) for a <prefix>.paf: line j of the PAF is the hit of
    the j-th mapped read, and reads that wrote no line sort nowhere, so the PAF's own line numbers serve as ordinals"""
    lines = paf_bytes.splitlines(keepends=True)
    hits = hits_of_paf(paf_bytes.decode(), refs)
    order, recs, tot = model(refs, hits, np.arange(hits.size), min_mapq)
    out = [lines[int(o)] for o in order]
    offs = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64)
    names = {int(i): (n, ln) for i, n, ln in refs}
    tsv = TSV_HEAD + "".join("%s\t%d\t%d\t%d\t%d\n" % (names[int(r["ref_id"])][0], names[int(r["ref_id"])][1], int(r["count"]), int(r["first"]), int(offs[int(r["first"])]))
                             for r in recs)
    return b"".join(out), tsv.encode(), recs, tot


def log_line(recs, totals, min_mapq):
    return "Sorted: %d of %d hits kept (%d not mapped, %d below mapq %d, %d out of range): %d lines on %d references" % (
        totals["kept"], totals["offered"], totals["not_mapped"], totals["below_mapq"], min_mapq, totals["out_of_range"], int(recs["count"].sum()),
        int((recs["count"] > 0).sum()))
