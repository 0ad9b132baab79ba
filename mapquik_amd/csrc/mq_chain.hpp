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

// The chains output of a launch (CHN instantiations only: mq_ctx_reserve_chains).  A candidate as the candidate loop leaves it, staged
// until the read's number of candidates is known: 32 bytes, two 16-byte words
struct ChainRec {
    uint32_t ref, rc_mapq;   // rc in bit 0, mapq == 60 in bit 1
    uint32_t q_start, q_end; // first.q_start, last.q_end (as Match stores it)
    uint32_t r_a, r_b;       // the two r ends get_match takes (chain_r_ends), r_b as Match stores it
    uint32_t score, nkept;
};
static_assert(sizeof(ChainRec) == 32 && sizeof(mq_chain) == 48 && sizeof(mq_chain) == sizeof(mq_hit), "chain records");
using ChainOut = ChainLaunch;  // (mq_blocks.hpp: the launch's arguments live in its counter block)

// get_match's choice of reference ends (src/chain.rs:162-168) as a candidate is staged: r_start, and r_end as Match stores it.  A staged
// record comes back through find_coords as a chain of ONE run whose first and last are the same record -- the choice is made once, here.
__device__ __forceinline__ void chain_r_ends(bool rc, uint32_t nkept, const MatchRec &first, const MatchRec &last, uint32_t &r_a, uint32_t &r_b) {
    if (rc && nkept > 1) {
        r_a = last.r_start;
        r_b = first.r_end;
    } else {
        r_a = first.r_start;
        r_b = last.r_end;
    }
}

// get_match's `- 1`s and choice of reference ends (src/chain.rs:162-168) and find_coords (src/mers.rs:131-183) for one chain of N_RUNS kept
// runs, from the ends of its first and last run: declares qs64, qe64 (columns 3, 4, 64-bit), frs, fre (columns 8, 9) in the scope it
// stands in.  usize arithmetic, wrapping like a release build: exc_s / exc_e wrap when the run's r_end lies beyond THIS reference's end (a
// run the precedence quirk extended onto another, longer reference); all 64 bits go out.
// ONE copy of the arithmetic, as a statement macro and not only as a function: the hit takes it in place, the chains output through
// find_coords below.  Five wordings of a __forceinline__ function called from the hit path each moved the SGPR spill counts of three to
// six existing map_declined_kernel instantiations (kernels that spill 200-350 SGPRs; which ones moved changed with the wording), and
// the kernels' code is held identical across changes; these statements in place leave all of them as they were.
#define MQ_FIND_COORDS(RC, FIRST_Q_START, LAST_Q_END, FIRST_R_START, FIRST_R_END, LAST_R_START, LAST_R_END, N_RUNS, Q_LEN, R_LEN) \
    const uint64_t q_start = (FIRST_Q_START);                                                                                    \
    const uint64_t q_end = (uint64_t)(LAST_Q_END) - 1;                                                                           \
    uint64_t r_start, r_end;                                                                                                     \
    if ((RC) && (N_RUNS) > 1) {                                                                                                  \
        r_start = (LAST_R_START);                                                                                                \
        r_end = (uint64_t)(FIRST_R_END) - 1;                                                                                     \
    } else {                                                                                                                     \
        r_start = (FIRST_R_START);                                                                                               \
        r_end = (uint64_t)(LAST_R_END) - 1;                                                                                      \
    }                                                                                                                            \
    const uint64_t r_len = (R_LEN);                                                                                              \
    const uint64_t tail = (Q_LEN) - q_end - 1;                                                                                   \
    uint64_t frs, fre, exc_s, exc_e;                                                                                             \
    if (!(RC)) {                                                                                                                 \
        if (r_start >= q_start) { frs = r_start - q_start; exc_s = q_start; }                                                    \
        else { frs = 0; exc_s = r_start; }                                                                                       \
        if (r_end + tail <= r_len - 1) { fre = r_end + tail; exc_e = tail; }                                                     \
        else { fre = r_len - 1; exc_e = r_len - r_end - 1; }                                                                     \
    } else {                                                                                                                     \
        if (r_end + q_start <= r_len - 1) { fre = r_end + q_start; exc_s = q_start; }                                            \
        else { fre = r_len - 1; exc_s = r_len - r_end - 1; }                                                                     \
        if (r_start >= tail) { frs = r_start - tail; exc_e = tail; }                                                             \
        else { frs = 0; exc_e = r_start; }                                                                                       \
    }                                                                                                                            \
    const uint64_t qs64 = q_start - exc_s, qe64 = q_end + exc_e;

// ... as the device function of (rc, first / last ends, n_runs, q_len, r_len): what the chains output's copy-out calls per candidate
struct ChainCoords {
    uint64_t qs64, qe64, frs, fre;
};
__device__ __forceinline__ ChainCoords find_coords(bool rc, uint32_t first_q_start, uint32_t last_q_end, uint32_t first_r_start, uint32_t first_r_end,
                                                   uint32_t last_r_start, uint32_t last_r_end, uint32_t n_runs, uint64_t q_len, uint64_t r_len_of_ref) {
    MQ_FIND_COORDS(rc, first_q_start, last_q_end, first_r_start, first_r_end, last_r_start, last_r_end, n_runs, q_len, r_len_of_ref)
    ChainCoords o;
    o.qs64 = qs64;
    o.qe64 = qe64;
    o.frs = frs;
    o.fre = fre;
    return o;
}

// Per-reference Chain::get_match + best-of + find_coords.  CH = lanes used per chunk (64; smaller only in tests
// so that ordinary inputs exercise the multi-chunk path).
// first: lane i's record i already in a register (the caller read the first chunk itself); with nm <= CH nothing is read here then
// ANCH: the runs of the winning chain -- the list filter_matches_max leaves, src/chain.rs:123-129 -- go to ao's pool as well, and `span`
// says where ({0, 0} for a read that is not mapped).  Every line of that sits under `if constexpr (ANCH)`: the instantiations without it
// are the code they were.
// CHN: every candidate chain goes to co's pool (mq_ctx_reserve_chains), in the order the loop below visits the references -- that of each
// reference's first run in the read -- and `cspan` says where.  The number of candidates is known only when the loop ends and a read's
// entries are contiguous, claimed with ONE atomic add: so the loop stages each candidate in the wave's chain window `cwin`, and the copy-out
// behind the loop finishes them (find_coords against each chain's own reference length, MQ_CHAIN_TOP) with a lane per candidate.  Every
// line of that sits under `if constexpr (CHN)`.
template <int CH, bool ANCH = false, bool CHN = false>
__device__ __forceinline__ void chain_stage(MatchRec *__restrict__ scratch, uint32_t nm, const DevParams &P, uint64_t q_len,
                                            const uint64_t *__restrict__ ref_lens, mq_hit &out, const MatchRec *first = nullptr,
                                            const AnchorOut *ao = nullptr, mq_anchor_span *span = nullptr, const ChainOut *co = nullptr,
                                            ChainRec *__restrict__ cwin = nullptr, mq_chain_span *cspan = nullptr) {
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
            if constexpr (CHN) {
                // candidate n_cand's tuple (wave-uniform) into the chain window, by lane 0: two 16-byte vector stores.  A candidate has at
                // least one run of its own, so n_cand < nm <= the window's records here (ChainOut::win_cap): the stage cannot overflow.
                if (lane == 0) {
                    const bool crc = first.rc != 0;
                    ChainRec cr;
                    cr.ref = r;
                    cr.rc_mapq = (crc ? 1u : 0u) | (((P.s != 0 && P.c != 0) && (nkept >= P.c || score >= P.s)) ? 2u : 0u);
                    cr.q_start = first.q_start;
                    cr.q_end = last.q_end;
                    chain_r_ends(crc, nkept, first, last, cr.r_a, cr.r_b);
                    cr.score = score;
                    cr.nkept = nkept;
                    uint4 *w = reinterpret_cast<uint4 *>(cwin + n_cand);
                    w[0] = make_uint4(cr.ref, cr.rc_mapq, cr.q_start, cr.q_end);
                    w[1] = make_uint4(cr.r_a, cr.r_b, cr.score, cr.nkept);
                }
            }
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
    if constexpr (CHN) {
        // the copy-out, for every read with a candidate (mapped or tied).  This wave's staged records are read back by this wave: the
        // ordering the Match window has between the runs' stores and this stage's loads (map_read) -- the stores acknowledged, the wave
        // together -- and plain loads.  The claim first: ONE atomic add of n_cand on the pool cursor, which counts on past the capacity.
        if (n_cand) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (map_read's statement in front of this stage, verbatim: not a new fence)
            wave_sync();
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(&co->counters->cursor, (unsigned long long)n_cand);
            at = rdlane64(at, 0);
            cspan->count = n_cand;
            if (at + n_cand > (unsigned long long)co->cap) {
                if (lane == 0) atomicAdd(&co->counters->dropped_reads, 1u);
                cspan->first = MQ_CHAINS_DROPPED;
            } else {
                cspan->first = (uint32_t)at;
                for (uint32_t c = lane; c < n_cand; c += 64u) {  // rounds of 64, lane = candidate
                    const uint4 *w = reinterpret_cast<const uint4 *>(cwin + c);
                    const uint4 w0 = w[0], w1 = w[1];
                    // (the staged ends are the ones get_match chose: as a chain of one run they come through the choice unchanged)
                    const ChainCoords fc = find_coords((w0.y & 1u) != 0, w0.z, w0.w, w1.x, w1.y, w1.x, w1.y, 1u, q_len, ref_lens[w0.x]);
                    uint4 *dst = reinterpret_cast<uint4 *>(co->pool + at + c);  // 48 bytes: three 16-byte vector stores
                    dst[0] = make_uint4(w1.z == max_count ? MQ_CHAIN_TOP : 0u, w0.x, w0.y & 1u, (w0.y & 2u) ? 60u : 0u);
                    dst[1] = make_uint4((uint32_t)fc.qs64, (uint32_t)fc.qe64, (uint32_t)fc.frs, (uint32_t)fc.fre);
                    dst[2] = make_uint4(w1.z, w1.w, (uint32_t)(fc.qs64 >> 32), (uint32_t)(fc.qe64 >> 32));
                }
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
    // get_match coordinates (src/chain.rs:162-168) and find_coords (src/mers.rs:131-183)
    MQ_FIND_COORDS(rc, bfirst.q_start, blast.q_end, bfirst.r_start, bfirst.r_end, blast.r_start, blast.r_end, b_len, q_len, ref_lens[b_ref])
    out.status = MQ_HIT_MAPPED;
    out.ref_id = b_ref;
    out.rc = rc ? 1u : 0u;
    out.mapq = b_mapq;
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
