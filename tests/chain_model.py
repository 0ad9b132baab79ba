"""A slow, independently worded model of the chain side of the mapper, on Python ints with every wrap written out.

What it states (DESIGN.md, and the behaviour tests/golden/kat_intree.json documents):
  runs      a hit opens a run; the following k-min-mers extend it while `extends()` holds; a miss is swallowed and ends the run, a hit
            that does not extend ends the run and opens the next one.  `extends()` is the reference's test as its operators bind:
            (same reference AND same strand AND reverse run AND offset one lower) OR (forward run AND offset one higher) -- so a forward
            run takes any hit whose offset is one higher, on whichever reference and strand.
  grouping  a run belongs to the reference of the hit that opened it.
  chain     per reference: one run => taken as it is.  Several => the anchor is the first run with the largest count, and a run stays iff
            it is the anchor's equal in every field, or has the anchor's strand, lies on the right side of it on the reference
            (strictly, by r_start, ordered by q_start) and the query gap and the reference gap between the two differ by at most g,
            both gaps and their difference computed in wrapping 32-bit two's complement, |.| wrapping too, then widened with its sign.
  score     sum of the kept runs' counts; mapq 60 iff c != 0 and s != 0 and (kept runs >= c or score >= s), else 0.
  best      the candidate with the strictly largest score in first-seen order; if the runner-up's score equals it: unmapped.
  coords    extend the chain's ends by the unaligned read ends, clipped to the reference; unsigned 64-bit arithmetic that wraps.

Input is the oracle's own k-min-mer list of the read and its index answers (oracle.kminmers, Index.get): only the stages above are
modelled.  The output has the oracle's paf_dtype columns as a dict, or None for an unmapped read.
"""
import ctypes

U64 = (1 << 64) - 1


class _Entry(ctypes.Structure):  # oracle.entry_dtype
    _fields_ = [("id", ctypes.c_uint64), ("start", ctypes.c_uint64), ("end", ctypes.c_uint64), ("offset", ctypes.c_uint64), ("rc", ctypes.c_int32)]


def i32(x):
    """two's-complement reading of the low 32 bits"""
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def abs_widened(x):
    """|x| of a 32-bit value that wraps (|-2^31| = -2^31), then sign-extended to 64 bits and read as unsigned"""
    a = i32(-x) if x < 0 else x
    return a & U64


class Run:
    __slots__ = ("q_start", "q_end", "r_start", "r_end", "count", "rc", "ref")

    def same(self, o):
        return (self.q_start, self.q_end, self.r_start, self.r_end, self.count, self.rc) == (o.q_start, o.q_end, o.r_start, o.r_end, o.count, o.rc)


def extends(run, q_rev, hit, prev):
    """may `hit` (the index entry of the next k-min-mer, whose strand flag in the read is q_rev) extend `run`, whose last entry is `prev`?"""
    step_down = i32(i32(prev["offset"]) - i32(hit["offset"])) == 1
    step_up = i32(i32(hit["offset"]) - i32(prev["offset"])) == 1
    same_ref = hit["id"] == prev["id"]
    same_strand = (q_rev != hit["rc"]) == run.rc
    return (same_ref and same_strand and run.rc and step_down) or ((not run.rc) and step_up)


def runs_of(kmers, entries):
    """kmers: [(start, end, rev)], entries: the index answer per k-min-mer (dict id/start/end/offset/rc, or None) -> [Run] in read order"""
    out, i, n = [], 0, len(kmers)
    while i < n:
        e = entries[i]
        if e is None:
            i += 1
            continue
        r = Run()
        r.q_start, r.q_end, r.r_start, r.r_end, r.count = kmers[i][0], kmers[i][1], e["start"], e["end"], 1
        r.rc = kmers[i][2] != e["rc"]
        r.ref = e["id"]
        prev = e
        i += 1
        while i < n:
            h = entries[i]
            if h is None:
                i += 1  # the miss is used up
                break
            if not extends(r, kmers[i][2], h, prev):
                break   # this hit opens the next run
            if r.rc:
                r.r_start = h["start"]
            else:
                r.r_end = h["end"]
            r.q_end = kmers[i][1]
            r.count += 1
            prev = h
            i += 1
        out.append(r)
    return out


def gaps_differ_too_much(q_gap_from, q_gap_to, r_gap_from, r_gap_to, g):
    gq = i32(i32(q_gap_to) - i32(q_gap_from))
    gr = i32(i32(r_gap_to) - i32(r_gap_from))
    return abs_widened(i32(gq - gr)) > g


def stays(anchor, x, g):
    if anchor.same(x):
        return True
    if anchor.rc != x.rc:
        return False
    u, v = (anchor, x) if anchor.q_start < x.q_start else (x, anchor)  # u: the one that starts earlier in the read
    if u.rc:  # reverse strand: the later run lies at LOWER reference positions
        if not u.r_start > v.r_start:
            return False
        return not gaps_differ_too_much(u.q_end, v.q_start, v.r_end, u.r_start, g)
    if not v.r_start > u.r_start:
        return False
    return not gaps_differ_too_much(u.q_end, v.q_start, u.r_end, v.r_start, g)


def candidate(runs, c, s, g):
    """one reference's runs -> (rc, q_start, q_end, r_start, r_end, score, mapq)"""
    kept = runs
    if len(runs) > 1:
        anchor = runs[0]
        for r in runs[1:]:
            if r.count > anchor.count:
                anchor = r
        kept = [r for r in runs if stays(anchor, r, g)]
    if not kept:
        return None
    score = sum(r.count for r in kept)
    mapq = 60 if (c != 0 and s != 0 and (len(kept) >= c or score >= s)) else 0
    a, z = kept[0], kept[-1]
    if a.rc and len(kept) > 1:
        r_start, r_end = z.r_start, (a.r_end - 1) & U64
    else:
        r_start, r_end = a.r_start, (z.r_end - 1) & U64
    return a.rc, a.q_start, (z.q_end - 1) & U64, r_start, r_end, score, mapq


def place(q_len, r_len, cand):
    rc, q_start, q_end, r_start, r_end, score, mapq = cand
    tail = (q_len - q_end - 1) & U64  # read bases behind the chain
    last = (r_len - 1) & U64
    if not rc:
        if r_start >= q_start:
            out_rs, head_used = (r_start - q_start) & U64, q_start
        else:
            out_rs, head_used = 0, r_start
        if (r_end + tail) & U64 <= last:
            out_re, tail_used = (r_end + tail) & U64, tail
        else:
            out_re, tail_used = last, (r_len - r_end - 1) & U64
    else:  # the read's head lies towards the reference's end
        if (r_end + q_start) & U64 <= last:
            out_re, head_used = (r_end + q_start) & U64, q_start
        else:
            out_re, head_used = last, (r_len - r_end - 1) & U64
        if r_start >= tail:
            out_rs, tail_used = (r_start - tail) & U64, tail
        else:
            out_rs, tail_used = 0, r_start
    return dict(rc=int(rc), q_len=q_len, q_start=(q_start - head_used) & U64, q_end=(q_end + tail_used) & U64, r_len=r_len,
                r_start=out_rs, r_end=out_re, score=score, mapq=mapq)


def map_read(kmers, entries, q_len, ref_len, c, s, g):
    """ref_len: function reference id -> length.  Returns (result dict with ref_id, or None; counters dict)"""
    runs = runs_of(kmers, entries)
    per_ref = {}
    for r in runs:
        per_ref.setdefault(r.ref, []).append(r)
    cands = []
    for ref, rs in per_ref.items():
        cd = candidate(rs, c, s, g)
        if cd is not None:
            cands.append((ref, cd))
    info = dict(n_matches=len(runs), n_candidates=len(cands))
    if not cands:
        return None, info
    best = 0
    if len(cands) > 1:
        top = top_score = runner_up = 0
        for i, (_, cd) in enumerate(cands):
            if cd[5] > top_score:
                runner_up, top, top_score = top_score, i, cd[5]
            elif cd[5] > runner_up:
                runner_up = cd[5]
        if top_score == runner_up:
            return None, info
        best = top
    ref, cd = cands[best]
    res = place(q_len, ref_len(ref), cd)
    res["ref_id"] = ref
    return res, info


def map_with_oracle(O, ox, po, seq):
    """the model on one read, fed with the oracle's k-min-mers and index answers"""
    if len(seq) < po.l + po.k - 1:
        return None, dict(n_matches=0, n_candidates=0)
    km = O.kminmers(seq, po)
    kmers = list(zip(km["start"].tolist(), km["end"].tolist(), (km["rev"] != 0).tolist()))
    get, entries = O.lib().mqo_index_get, []  # (Index.get without the numpy record per call)
    for h in km["hash"].tolist():
        p = get(ox.h, h)
        if not p:
            entries.append(None)
            continue
        e = _Entry.from_address(p)
        entries.append(dict(id=e.id, start=e.start, end=e.end, offset=e.offset, rc=bool(e.rc)))
    return map_read(kmers, entries, len(seq), lambda r: int(ox.ref_len(r)), int(po.c), int(po.s), int(po.g))
