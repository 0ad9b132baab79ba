// mq_probe.hpp -- the index probe (ReadOnlyIndex::get) and MapSink, the map stage's consumer of an ordered minimizer list: k-min-mers ->
// tuple hashes -> probes of a whole chunk resolved together -> Match runs (Match::new/update/check/extend, chain_matches).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mapquik_hip.h"
#include "mq_device.hpp"
#include "mq_hash.hpp"
#include "mq_wave.hpp"

namespace mq {

// ------------------------------------------------------------------ index probe (ReadOnlyIndex::get, src/index.rs:118-126)
// table has nslots = mask + 1 slots (nslots / 2 buckets) plus one extra bucket [nslots / 2] for the key 0.
__device__ __forceinline__ uint4 ld_u4(const void *p) { return *reinterpret_cast<const uint4 *>(p); }
__device__ __forceinline__ uint64_t u64_of(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }
__device__ __forceinline__ bool probe_table(const Bucket *__restrict__ table, uint64_t mask, uint64_t key, Entry &out) {
    const uint64_t nb = (mask + 1) >> 1;
    if (key == 0) {
        out = table[nb].pay[0];
        return entry_live(out);
    }
    const uint64_t s0 = key & mask;
    uint64_t b = s0 >> 1;
    uint32_t w = (uint32_t)s0 & 1u;
    for (uint32_t step = 0;; ++step) {
        const unsigned long long k = table[b].key[w];
        if (k == key) {
            out = table[b].pay[w];
            return entry_live(out);
        }
        if (k == 0) return false;
        if (step == 0) {
            w ^= 1u;  // the other way of the home bucket
        } else if (step == 1 || w == 1u) {
            b = b + 1 == nb ? 0 : b + 1;
            w = 0;
        } else {
            w = 1u;
        }
    }
}

// ------------------------------------------------------------------ the map stage's consumer of an ordered minimizer list
// Match records a wave keeps in LDS next to the staged list (the space the seed phase's larger LDS leaves unused during the map phase):
// an ordinary read has a handful, and chaining them from LDS saves the wait for their stores and the loads' round trip through L2
constexpr uint32_t MAP_LDS_RECS = 48;
static_assert(MAP_LDS_RECS <= 64, "records_to_scratch: one record per lane");
struct MapSink {
    const Bucket *__restrict__ table;
    uint64_t mask;
    const DevParams &P;
    MatchRec *__restrict__ scratch;
    uint32_t cap_matches;
    MatchRec *lds_rec;  // the first MAP_LDS_RECS Match records also go to LDS: a read with no more than that is chained from there
    mq_kminmer *__restrict__ dump;  // optional k-min-mer dump window for this read
    uint32_t dump_cap;
    bool rev_eq;  // seeding variant 32: a palindromic tuple counts as reversed (a constant false in code built without the variants)
    // wave-uniform state
    uint32_t kmm_count = 0;
    uint32_t n_matches = 0;
    bool c_open = false;  // a run is open across the batch boundary; M holds it so far
    MatchRec M = {};
    uint32_t c_hit = 0, c_id = 0, c_off = 0, c_sigma = 0;  // last element of the previous batch
    uint32_t probe_steps = 0;  // per lane: slots visited beyond the home slot (diagnostic: mean probes per lookup)

    __device__ MapSink(const Bucket *t, uint64_t m, const DevParams &p, MatchRec *s, uint32_t cap, MatchRec *lr, mq_kminmer *d, uint32_t dc, bool re)
        : table(t), mask(m), P(p), scratch(s), cap_matches(cap), lds_rec(lr), dump(d), dump_cap(dc), rev_eq(re) {}
    // record i of the read: the first MAP_LDS_RECS stay in LDS, later ones go to their place in the wave's scratch in device memory
    // (records_to_scratch() then moves the LDS ones there too).  An ordinary read's records never leave LDS: no store's
    // acknowledgement is outstanding when the map phase ends.
    __device__ __forceinline__ void put_rec(uint32_t i, const MatchRec &m) const {
        // a typed LDS store: left generic, the compiler folds the two branches into ONE flat store through a selected pointer (26 flat stores
        // in round 5's map_kernel) -- which goes the memory path's way even when it lands in LDS and counts on both wait counters
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) u32x4 lds_u4;
        if (i < MAP_LDS_RECS) {
            lds_u4 *d = (lds_u4 *)(&lds_rec[i]);
            d[0] = u32x4{m.q_start, m.q_end, m.r_start, m.r_end};
            d[1] = u32x4{m.count, m.ref, m.rc, m.done};
        } else if (i < cap_matches) {
            scratch[i] = m;
        }
    }
    __device__ __forceinline__ void records_to_scratch() const {
        const uint32_t n = n_matches < MAP_LDS_RECS ? n_matches : MAP_LDS_RECS, i = lane_id();
        if (i < n && i < cap_matches) scratch[i] = lds_rec[i];
    }

    // k-min-mer `base + lane` of a minimizer list: canonical orientation, tuple hash, query coordinates
    // (a SpecFixed holds its own k's tuple hash, SipHash only; SpecNone holds every supported k's and the opt-in kh_fast)
    template <class Spec = SpecNone>
    __device__ __forceinline__ void batch_keys(const unsigned long long *mzh, const uint32_t *mzp, uint32_t base, bool act,
                                               uint64_t &key, bool &rev, uint32_t &q_start, uint32_t &q_end) const {
        const uint32_t i0 = base + lane_id();
        const uint32_t k = spec_k<Spec>(P), l = spec_l<Spec>(P);
        key = 0;
        rev = false;
        q_start = q_end = 0;
        if (act) {
            auto get = [&](uint32_t i) { return (uint64_t)mzh[i0 + i]; };
            const bool re = rev_eq, fk = spec_fast_kh<Spec>(P);
            if constexpr (Spec::FIXED) {
                key = kminmer_hash_fixed<Spec::K>(get, rev, re, fk);
            } else {
                // 5: the reference's default k (src/main.rs: -k 5); 7: experiments/table1.sh:50; 8: example/run_ecoli.sh:26
                key = k == 5u ? kminmer_hash_fixed<5>(get, rev, re, fk) : k == 7u ? kminmer_hash_fixed<7>(get, rev, re, fk)
                      : k == 8u ? kminmer_hash_fixed<8>(get, rev, re, fk) : kminmer_hash(k, get, rev, re, fk);
            }
            q_start = mzp[i0];
            q_end = mzp[i0 + k - 1] + l - 1u;
        }
    }

    // ---- index probes of a whole chunk of lane-batches, resolved together (ReadOnlyIndex::get, src/index.rs:118-126).
    // Per (lane, batch) one 16-byte load fetches both keys of the home bucket; every batch's load is in flight before the first is
    // looked at.  A key that matches gets its 16 payload bytes fetched at once (same 64-byte line: the L2 has it); the few lookups
    // whose home bucket is full of other keys walk on bucket by bucket in rounds shared by all batches.  Memory latencies a chunk
    // exposes: one for the keys, one for the payloads, one per extra round (rare) -- not one or more per batch.
    // state of a lookup, two bits per batch in `st`: 0 = miss, 1 = key found (payload load issued into kk[c]), 3 = walking on
    __device__ __forceinline__ const Bucket *home_bucket(uint64_t key) const {
        return table + (key == 0 ? (mask + 1) >> 1 : (key & mask) >> 1);
    }
    template <int NB>
    __device__ __forceinline__ void probe_all(const uint64_t (&key)[NB], uint4 (&kk)[NB], uint32_t actbits, uint32_t &st) {
        st = 0;
        const uint64_t nb = (mask + 1) >> 1;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if ((actbits >> c) & 1u) {
                const uint64_t k = key[c];
                const Bucket *B = home_bucket(k);
                uint32_t way, s2;
                if (k == 0) {  // the extra bucket's way 0: its payload says whether the key 0 is present
                    s2 = 1u;
                    way = 0;
                } else {
                    const uint32_t w0 = (uint32_t)k & (uint32_t)mask & 1u;
                    const uint64_t ka = u64_of(kk[c].x, kk[c].y), kb = u64_of(kk[c].z, kk[c].w);
                    const uint64_t kh = w0 ? kb : ka, kp = w0 ? ka : kb;
                    if (kh == k) { s2 = 1u; way = w0; }
                    else if (kh == 0) { s2 = 0u; way = 0; }
                    else if (kp == k) { s2 = 1u; way = w0 ^ 1u; probe_steps++; }
                    else if (kp == 0) { s2 = 0u; way = 0; probe_steps++; }
                    else { s2 = 3u; way = 0; probe_steps++; }
                }
                if (s2 == 1u) kk[c] = ld_u4(&B->pay[way]);
                st |= s2 << (2 * c);
            }
        }
#ifdef MQ_STAGE_MAP_SPLIT
        mq_clk(12);
#endif
        // walking on (about one lookup in a hundred: both ways of the home bucket hold other keys).  Every lane takes ONE of its
        // walking lookups at a time -- its key by a select over the batches, a loop over the following buckets shared by all lanes,
        // the outcome written back by a select -- so the rare path holds six registers instead of looping over all NB batches.
        while (__ballot((st & 0xAAAAAAAAu) != 0)) {
            const bool walking = (st & 0xAAAAAAAAu) != 0;
            const uint32_t wc = walking ? ((uint32_t)__builtin_ctz(st & 0xAAAAAAAAu) >> 1) : 0xFFu;  // the lane's first batch in state 3
            uint64_t k = 0;
#pragma unroll
            for (int c = 0; c < NB; ++c) k = wc == (uint32_t)c ? key[c] : k;
            uint64_t b = (k & mask) >> 1;
            uint4 res = make_uint4(0, 0, 0, 0);
            uint32_t s2 = walking ? 3u : 0u;
            while (__ballot(s2 == 3u)) {
                if (s2 == 3u) {
                    b = (b + 1) & (nb - 1);  // a power of two of buckets
                    const uint4 v = ld_u4(&table[b].key[0]);
                    const uint64_t ka = u64_of(v.x, v.y), kb = u64_of(v.z, v.w);
                    uint32_t way = 0;
                    probe_steps++;
                    if (ka == k) { s2 = 1u; }
                    else if (ka == 0) { s2 = 0u; }
                    else {
                        probe_steps++;
                        if (kb == k) { s2 = 1u; way = 1u; }
                        else if (kb == 0) { s2 = 0u; }
                    }
                    if (s2 == 1u) res = ld_u4(&table[b].pay[way]);
                }
            }
#pragma unroll
            for (int c = 0; c < NB; ++c) {
                if (wc == (uint32_t)c) {
                    kk[c] = res;
                    st = (st & ~(3u << (2 * c))) | (s2 << (2 * c));
                }
            }
        }
    }

    // one batch of n <= 64 consecutive k-min-mers (lane = k-min-mer) with their index entries: dump + Match runs
    __device__ __forceinline__ void batch_runs(uint32_t n, uint64_t key, bool rev, uint32_t q_start, uint32_t q_end, bool hit, const Entry &e) {
        const uint32_t lane = lane_id();
        if (dump && lane < n && kmm_count + lane < dump_cap) {
            mq_kminmer d;
            d.hash = key;
            d.start = q_start;
            d.end = q_end;
            d.offset = kmm_count + lane;
            d.rev = rev ? 1u : 0u;
            dump[kmm_count + lane] = d;
        }
        kmm_count += n;
        // chain_matches + Match::extend (src/mers.rs:57-73, src/match.rs:45-58), lane = k-min-mer.
        // Run state after element i: 0 = no open run (miss), 1 = forward run, 2 = reverse run (Match.rc of the run's
        // first element).  Element i maps the previous state to the next one; the maps compose associatively, so a wave
        // scan resolves every state.  Match::check (src/match.rs:39-43) parses as (A && B && C) || D:
        //   reverse run continues iff same ref id && (q.rev != r.rc) && p.offset - r.offset == 1   (cr)
        //   forward run continues iff r.offset - p.offset == 1                                      (cf)
        const uint32_t r_id = e.id_rc >> 1;
        const uint32_t srel = (hit && (rev != ((e.id_rc & 1u) != 0))) ? 1u : 0u;  // q.rev != r.rc
        // previous element's entry: DPP wave shift right by one lane; lane 0 has no source lane and keeps `old` = the carried element
        const uint32_t hit_p = (uint32_t)__builtin_amdgcn_update_dpp((int)c_hit, (int)(hit ? 1u : 0u), 0x138, 0xf, 0xf, false);
        const uint32_t id_p = (uint32_t)__builtin_amdgcn_update_dpp((int)c_id, (int)r_id, 0x138, 0xf, 0xf, false);
        const uint32_t off_p = (uint32_t)__builtin_amdgcn_update_dpp((int)c_off, (int)e.offset, 0x138, 0xf, 0xf, false);
        const bool both = hit && hit_p;
        const bool cf = both && ((int32_t)(e.offset - off_p) == 1);
        const bool cr = both && r_id == id_p && srel == 1u && ((int32_t)(off_p - e.offset) == 1);
        // Element i maps the previous state to: miss -> 0; hit -> sv = (srel ? 2 : 1) unless it continues a run
        // (state 1 && cf -> 1, state 2 && cr -> 2).  cr implies sv == 2 and cf with sv == 1 gives 1 either way, so every
        // element is a CONSTANT map except "cf && srel" (1 -> 1, anything else -> 2), which is idempotent under
        // composition: the state after it is 1 iff the nearest preceding constant element (or the carry) left state 1.
        const uint32_t sv = srel ? 2u : 1u;
        const bool nonconst = cf && srel == 1u;
        uint32_t sigma = hit ? sv : 0u;
        if (__ballot(nonconst)) {  // rare (a forward step between entries whose strands disagree with the read's): most batches skip this
            const uint64_t constmask = __ballot(!nonconst);
            const uint64_t constF = __ballot(!nonconst && hit && sv == 1u);
            const uint64_t lt_mask = lane ? (~0ull >> (64u - lane)) : 0ull;  // lanes below this one
            const uint64_t below = constmask & lt_mask;
            const bool baseF = below ? ((constF >> (63 - __clzll((long long)below))) & 1ull) != 0 : (c_sigma == 1u);
            if (nonconst) sigma = baseF ? 1u : 2u;
        }
        const uint32_t sigma_p = (uint32_t)__builtin_amdgcn_update_dpp((int)c_sigma, (int)sigma, 0x138, 0xf, 0xf, false);  // lane 0: the carried state
        const bool prevF = sigma_p == 1u, prevR = sigma_p == 2u;
        const bool isnew = hit && !((prevF && cf) || (prevR && cr));
        const uint64_t hitmask = __ballot(hit);
        const uint64_t newmask = __ballot(isnew);
        // the run carried in from the previous batch ends unless element 0 continues it
        const bool cont0 = (hitmask & 1ull) && !(newmask & 1ull);
        if (c_open && n > 0 && !cont0) {
            if (lane == 0) put_rec(n_matches, M);
            n_matches++;
            c_open = false;
        }
        if (n > 0) {
            // element i ends a run iff it is a hit and the next element is a miss or starts a new run;
            // the last element of the batch never ends one here (its run stays open for the next batch / finish()).
            const uint64_t next_breaks = ((~hitmask | newmask) >> 1);
            const bool is_end = hit && lane + 1u < n && ((next_breaks >> lane) & 1ull);
            const uint64_t endmask = __ballot(is_end);
            const uint64_t below = newmask & ((lane >= 63u) ? ~0ull : ((2ull << lane) - 1ull));
            const int fl = below ? 63 - __clzll((long long)below) : -1;  // first element of this lane's run
            const int src = fl < 0 ? 0 : fl;
            const uint32_t f_qs = (uint32_t)__shfl((int)q_start, src, 64);
            const uint32_t f_rs = (uint32_t)__shfl((int)e.start, src, 64);
            const uint32_t f_re = (uint32_t)__shfl((int)e.end, src, 64);
            const uint32_t f_id = (uint32_t)__shfl((int)r_id, src, 64);
            const uint32_t f_rc = (uint32_t)__shfl((int)srel, src, 64);
            MatchRec m;
            if (fl >= 0) {
                m.q_start = f_qs;
                m.rc = f_rc;
                m.ref = f_id;
                m.count = lane - (uint32_t)fl + 1u;
                m.r_start = f_rc ? e.start : f_rs;  // Match::update: rc moves r_start, forward moves r_end
                m.r_end = f_rc ? f_re : e.end;
            } else {  // the run began in an earlier batch: extend the carried Match
                m.q_start = M.q_start;
                m.rc = M.rc;
                m.ref = M.ref;
                m.count = M.count + lane + 1u;
                m.r_start = M.rc ? e.start : M.r_start;
                m.r_end = M.rc ? M.r_end : e.end;
            }
            m.q_end = q_end;
            m.done = 0;
            if (is_end) {
                const uint32_t mi = n_matches + mbcnt64(endmask);
                put_rec(mi, m);
            }
            n_matches += (uint32_t)__popcll(endmask);
            // carry out: state of the last element
            const int last = (int)n - 1;
            c_hit = (uint32_t)((hitmask >> last) & 1ull);
            c_id = rdlane(r_id, last);
            c_off = rdlane(e.offset, last);
            c_sigma = rdlane(sigma, last);
            if (c_hit) {
                M.q_start = rdlane(m.q_start, last);
                M.q_end = rdlane(m.q_end, last);
                M.r_start = rdlane(m.r_start, last);
                M.r_end = rdlane(m.r_end, last);
                M.count = rdlane(m.count, last);
                M.ref = rdlane(m.ref, last);
                M.rc = rdlane(m.rc, last);
                M.done = 0;
                c_open = true;
            } else {
                c_open = false;
            }
        }
    }

    // All k-min-mers of an ordered minimizer list (have <= 64*NB + k - 1 entries) in one go: every tuple hash first, every home
    // bucket's keys in flight together, the probes resolved together (probe_all), then the runs batch by batch.
    // hashes_done(): called once the minimizers' hashes (mzh) have all been read -- the positions (mzp) are still needed
    // mzq (variant 16 only, else nullptr): the minimizers' second positions (the window's last compressed base), valid once
    // hashes_done() has returned (the caller stages them where the hashes were)
    template <int NB, class Spec = SpecNone, class F>
    __device__ __forceinline__ void consume_list(const unsigned long long *mzh, const uint32_t *mzp, uint32_t have, const F &hashes_done,
                                                 const uint32_t *mzq = nullptr) {
        const uint32_t k = spec_k<Spec>(P), l = spec_l<Spec>(P);
        if (have < k) return;
        const uint32_t lane = lane_id();
        const uint32_t K = have - k + 1u;
        uint64_t key[NB];
        uint4 kk[NB];
        uint32_t revbits = 0, actbits = 0;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            key[c] = 0;
            kk[c] = make_uint4(0, 0, 0, 0);
            if ((uint32_t)c * 64u < K) {
                const bool act = (uint32_t)c * 64u + lane < K;
                bool rev;
                uint32_t qs, qe;
                batch_keys<Spec>(mzh, mzp, (uint32_t)c * 64u, act, key[c], rev, qs, qe);
                revbits |= (rev ? 1u : 0u) << c;
                if (act) {
                    actbits |= 1u << c;
                    kk[c] = ld_u4(&home_bucket(key[c])->key[0]);
                }
                __builtin_amdgcn_sched_barrier(0);  // one tuple hash at a time: interleaving NB of them costs ~10 registers each
            }
        }
        hashes_done();
        mq_clk(6);
        uint32_t st;
        probe_all<NB>(key, kk, actbits, st);
#ifdef MQ_STAGE_MAP_SPLIT
        mq_clk(13);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        mq_clk(14);
#endif
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if ((uint32_t)c * 64u < K) {
                const uint32_t n = K - (uint32_t)c * 64u < 64u ? K - (uint32_t)c * 64u : 64u;
                const bool act = lane < n;
                const uint32_t i0 = (uint32_t)c * 64u + lane;
                uint32_t qs = 0, qe = 0;
                if (act) {
                    qs = mzp[i0];
                    qe = mzq ? mzq[i0 + k - 1] : mzp[i0 + k - 1] + l - 1u;
                }
                Entry e;
                e.start = kk[c].x;
                e.end = kk[c].y;
                e.offset = kk[c].z;
                e.id_rc = kk[c].w;
                const bool hit = ((st >> (2 * c)) & 3u) == 1u && entry_live(e);
                batch_runs(n, key[c], ((revbits >> c) & 1u) != 0, qs, qe, hit, e);
            }
        }
        mq_clk(7);
    }

    // the run still open after the last k-min-mer of the read ends there
    __device__ __forceinline__ void finish_runs() {
        if (c_open) {
            if (lane_id() == 0) put_rec(n_matches, M);
            n_matches++;
            c_open = false;
        }
    }

};

}  // namespace mq
