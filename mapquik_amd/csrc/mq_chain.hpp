// mq_chain.hpp -- the chain stage: a read's Match records -> its mq_hit (Chain::get_match and helpers, src/chain.rs; find_largest_two_chains,
// determine_best_match, find_coords, src/mers.rs:104-183).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mapquik_hip.h"
#include "mq_device.hpp"
#include "mq_wave.hpp"

namespace mq {

// ------------------------------------------------------------------ chain helpers (src/chain.rs)
__device__ __forceinline__ uint64_t abs_as_usize(int32_t x) {
    int32_t a = x < 0 ? (int32_t)(0u - (uint32_t)x) : x;  // i32::MIN.abs() wraps in release
    return (uint64_t)(int64_t)a;
}
// fwd_gap_too_long / rc_gap_too_long (src/chain.rs:132-142): `as i32` casts, wrapping subtraction
__device__ __forceinline__ bool gap_too_long(uint32_t v_q_s, uint32_t u_q_e, uint32_t x, uint32_t y, uint32_t g) {
    int32_t g1 = (int32_t)(v_q_s - u_q_e);
    int32_t g2 = (int32_t)(x - y);
    return abs_as_usize((int32_t)((uint32_t)g1 - (uint32_t)g2)) > (uint64_t)g;
}
// check_match_compatible (src/chain.rs:43-63), h1 = anchor
__device__ __forceinline__ bool match_compatible(const MatchRec &h1, const MatchRec &h2, uint32_t g) {
    if (h1.q_start == h2.q_start && h1.q_end == h2.q_end && h1.r_start == h2.r_start && h1.r_end == h2.r_end &&
        h1.count == h2.count && h1.rc == h2.rc)
        return true;
    if (h1.rc != h2.rc) return false;
    const bool h1_first = h1.q_start < h2.q_start;
    const MatchRec &u = h1_first ? h1 : h2;
    const MatchRec &v = h1_first ? h2 : h1;
    if (u.rc) {
        if (u.r_start <= v.r_start || gap_too_long(v.q_start, u.q_end, u.r_start, v.r_end, g)) return false;
    } else if (v.r_start <= u.r_start || gap_too_long(v.q_start, u.q_end, v.r_start, u.r_end, g)) {
        return false;
    }
    return true;
}

__device__ __forceinline__ MatchRec rd_match(const MatchRec &m, int l) {
    MatchRec r;
    r.q_start = rdlane(m.q_start, l);
    r.q_end = rdlane(m.q_end, l);
    r.r_start = rdlane(m.r_start, l);
    r.r_end = rdlane(m.r_end, l);
    r.count = rdlane(m.count, l);
    r.ref = rdlane(m.ref, l);
    r.rc = rdlane(m.rc, l);
    r.done = 0;
    return r;
}

// The anchor output of a launch (ANCH instantiations only: mq_ctx_reserve_anchors): the pool the winning chains' runs go to, and the
// batch's counters (mq_blocks.hpp)
struct AnchorOut {
    mq_anchor *pool;
    uint32_t cap;  // entries of the pool
    AnchorCounters *counters;
};

// Per-reference Chain::get_match + best-of + find_coords.  CH = lanes used per chunk (64; smaller only in tests
// so that ordinary inputs exercise the multi-chunk path).
// first: lane i's record i already in a register (the caller read the first chunk itself); with nm <= CH nothing is read here then
// ANCH: the runs of the winning chain -- the list filter_matches_max leaves, src/chain.rs:123-129 -- go to ao's pool as well, and `span`
// says where ({0, 0} for a read that is not mapped).  Every line of that sits under `if constexpr (ANCH)`: the instantiations without it
// are the code they were.
template <int CH, bool ANCH = false>
__device__ __forceinline__ void chain_stage(MatchRec *__restrict__ scratch, uint32_t nm, const DevParams &P, uint64_t q_len,
                                            const uint64_t *__restrict__ ref_lens, mq_hit &out, const MatchRec *first = nullptr,
                                            const AnchorOut *ao = nullptr, mq_anchor_span *span = nullptr) {
    const uint32_t lane = lane_id();
    // find_largest_two_chains state (src/mers.rs:110-129)
    uint32_t max_count = 0, second_count = 0, n_cand = 0;
    MatchRec bfirst = {}, blast = {};
    uint32_t b_ref = 0, b_score = 0, b_mapq = 0, b_len = 0;
    MatchRec b_anchor = {};  // (ANCH) the anchor of the reference that becomes b_ref: wave-uniform, like bfirst / blast
    for (uint32_t c0 = 0; c0 < nm; c0 += CH) {
        const bool v0 = lane < (uint32_t)CH && c0 + lane < nm;
        MatchRec m = {};
        if (first && c0 == 0) m = *first;
        else if (v0) m = scratch[c0 + lane];
        uint64_t pending = __ballot(v0 && !m.done);
        while (pending) {
            const int lead = __ffsll((long long)pending) - 1;
            const uint32_t r = rdlane(m.ref, lead);
            // pass A: Chain::len and find_largest_match (src/chain.rs:93-104): first index with the largest count
            uint32_t n_in = 0, best_cnt = 0;
            MatchRec anchor = {};
            for (uint32_t c = c0; c < nm; c += CH) {
                const bool v = lane < (uint32_t)CH && c + lane < nm;
                MatchRec x = {};
                if (c == c0) x = m;
                else if (v) x = scratch[c + lane];
                const bool in = v && x.ref == r && !x.done;
                const uint64_t im = __ballot(in);
                if (!im) continue;
                n_in += (uint32_t)__popcll(im);
                const uint32_t cnt = in ? x.count : 0u;
                const uint32_t mx = wave_max_u32(cnt);
                if (mx > best_cnt) {
                    const int fl = __ffsll((long long)__ballot(in && cnt == mx)) - 1;
                    best_cnt = mx;
                    anchor = rd_match(x, fl);
                }
            }
            // pass B: filter_matches_max (src/chain.rs:123-129) when len > 1; first/last kept, score
            uint32_t nkept = 0, score = 0;
            MatchRec first = {}, last = {};
            if (n_in == 1u) {
                // a reference with ONE Match (the stray hit of a repeat copy: most of the extra candidates of a repetitive genome): Chain::len
                // == 1, nothing to filter -- that Match (the anchor: this chunk's lead lane) is the first and the last, its count the score
                nkept = 1u;
                score = best_cnt;
                first = last = anchor;
            } else
            for (uint32_t c = c0; c < nm; c += CH) {
                const bool v = lane < (uint32_t)CH && c + lane < nm;
                MatchRec x = {};
                if (c == c0) x = m;
                else if (v) x = scratch[c + lane];
                const bool in = v && x.ref == r && !x.done;
                const uint64_t im = __ballot(in);
                if (!im) continue;
                if (c != c0 && in) scratch[c + lane].done = 1u;
                const bool keep = in && match_compatible(anchor, x, P.g);
                const uint64_t km = __ballot(keep);
                if (!km) continue;
                if (nkept == 0) first = rd_match(x, __ffsll((long long)km) - 1);
                last = rd_match(x, 63 - __clzll((long long)km));
                nkept += (uint32_t)__popcll(km);
                score += wave_sum_u32(keep ? x.count : 0u);
            }
            pending &= ~__ballot(v0 && m.ref == r);
            if (nkept == 0) continue;  // len_f == 0 => None (cannot happen: the anchor is compatible with itself)
            // find_largest_two_chains update (strict >)
            n_cand++;
            if (score > max_count) {
                second_count = max_count;
                max_count = score;
                bfirst = first;
                blast = last;
                b_ref = r;
                b_score = score;
                b_len = nkept;
                if constexpr (ANCH) b_anchor = anchor;
                b_mapq = ((P.s != 0 && P.c != 0) && (nkept >= P.c || score >= P.s)) ? 60u : 0u;
            } else if (score > second_count) {
                second_count = score;
            }
        }
    }
    out.status = MQ_HIT_UNMAPPED;
    out.ref_id = 0;
    out.rc = 0;
    out.mapq = 0;
    out.q_start = out.q_end = out.r_start = out.r_end = out.score = out.q_start_hi = out.q_end_hi = 0;
    if (n_cand == 0) return;
    if (n_cand > 1 && max_count == second_count) return;  // determine_best_match: tie => None (src/mers.rs:106)
    // get_match coordinates (src/chain.rs:162-168), usize arithmetic
    const bool rc = bfirst.rc != 0;
    const uint64_t q_start = bfirst.q_start;
    const uint64_t q_end = (uint64_t)blast.q_end - 1;
    uint64_t r_start, r_end;
    if (rc && b_len > 1) {
        r_start = blast.r_start;
        r_end = (uint64_t)bfirst.r_end - 1;
    } else {
        r_start = bfirst.r_start;
        r_end = (uint64_t)blast.r_end - 1;
    }
    // find_coords (src/mers.rs:131-183)
    const uint64_t r_len = ref_lens[b_ref];
    const uint64_t tail = q_len - q_end - 1;
    uint64_t frs, fre, exc_s, exc_e;
    if (!rc) {
        if (r_start >= q_start) { frs = r_start - q_start; exc_s = q_start; }
        else { frs = 0; exc_s = r_start; }
        if (r_end + tail <= r_len - 1) { fre = r_end + tail; exc_e = tail; }
        else { fre = r_len - 1; exc_e = r_len - r_end - 1; }
    } else {
        if (r_end + q_start <= r_len - 1) { fre = r_end + q_start; exc_s = q_start; }
        else { fre = r_len - 1; exc_s = r_len - r_end - 1; }
        if (r_start >= tail) { frs = r_start - tail; exc_e = tail; }
        else { frs = 0; exc_e = r_start; }
    }
    out.status = MQ_HIT_MAPPED;
    out.ref_id = b_ref;
    out.rc = rc ? 1u : 0u;
    out.mapq = b_mapq;
    // usize arithmetic, wrapping like a release build: exc_s / exc_e wrap when the run's r_end lies beyond THIS reference's end
    // (a run the precedence quirk extended onto another, longer reference); all 64 bits go out
    const uint64_t qs64 = q_start - exc_s, qe64 = q_end + exc_e;
    out.q_start = (uint32_t)qs64;
    out.q_end = (uint32_t)qe64;
    out.q_start_hi = (uint32_t)(qs64 >> 32);
    out.q_end_hi = (uint32_t)(qe64 >> 32);
    out.r_start = (uint32_t)frs;
    out.r_end = (uint32_t)fre;
    out.score = b_score;
    if constexpr (ANCH) {
        // pass C, for a mapped read only: the winner's kept runs once more, in read order.  The records are loaded again (the `done` flags
        // no longer matter; one chunk in LDS: lane i still holds record i in *first); a run stays by pass B's test against the winner's
        // anchor, so the list has b_len entries -- for a reference with a single run that run equals the anchor.
        // The claim first: ONE atomic add of b_len on the pool cursor, in front of the first store.  The cursor counts on past the capacity.
        unsigned long long at = 0;
        if (lane == 0) at = atomicAdd(&ao->counters->cursor, (unsigned long long)b_len);
        at = rdlane64(at, 0);
        const bool fits = at + b_len <= (unsigned long long)ao->cap;
        if (!fits) {
            if (lane == 0) atomicAdd(&ao->counters->dropped_reads, 1u);
            span->first = MQ_ANCHORS_DROPPED;
            span->count = b_len;
            return;
        }
        mq_anchor *dst = ao->pool + at;
        uint32_t running = 0;
        for (uint32_t c = 0; c < nm; c += CH) {
            const bool v = lane < (uint32_t)CH && c + lane < nm;
            MatchRec x = {};
            if (first && c == 0) x = *first;
            else if (v) x = scratch[c + lane];
            const bool keep = v && x.ref == b_ref && match_compatible(b_anchor, x, P.g);
            const uint64_t km = __ballot(keep);
            if (!km) continue;
            const uint32_t rank = running + mbcnt64(km);  // kept runs in front of this lane's: earlier chunks, lower lanes
            if (keep && rank < b_len) {  // (rank < b_len always: pass B counted the same runs)
                mq_anchor a;
                a.q_start = x.q_start;
                a.q_end = x.q_end;
                a.r_start = x.r_start;
                a.r_end = x.r_end;
                a.count = x.count;
                dst[rank] = a;
            }
            running += (uint32_t)__popcll(km);
        }
        span->first = (uint32_t)at;
        span->count = b_len;
    }
}

}  // namespace mq
