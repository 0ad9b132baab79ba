// mq_device.hpp -- gfx950 device code for mapquik's hot path (seeding, index probe, Match runs, pseudo-chain).
//
// One wavefront (64 lanes) owns one sequence (or one segment of a long reference).  Everything is
// integer / byte work: no MFMA.  This header holds what the parts share: the parameters (DevParams, the seeding variants, Spec), the
// index table's types and the Match record.  The parts: mq_wave.hpp (wave helpers, stage clocks), mq_hash.hpp (ntHash seeds, tuple
// hashes), mq_seed.hpp (the fast seeder for ACGT-only sequences), mq_seed_general.hpp (the GENERAL streaming seeder: any length, any
// bytes), mq_probe.hpp (index probe and Match-run builder: MapSink), mq_chain.hpp (chain stage).
// Structure of the streaming seeder (lanes = consecutive positions):
//   raw bytes --(head flags, ballot/mbcnt compaction)--> HPC ring in LDS --(64-wide XOR prefix scan of
//   rotated ntHash seeds)--> canonical l-mer hashes --(density predicate, ballot compaction)--> ordered
//   minimizer list in LDS --> sink (k-min-mers -> probe -> runs, or a global minimizer list).
//
// ntHash without a serial roll: with X(t) = XOR_{u<=t} ror(h(c_u), u) and Y(t) = XOR_{u<=t} rol(hc(c_u), u),
//   fh(window ending at e) = rol(X(e) ^ X(e-l), e)        rh = ror(Y(e) ^ Y(e-l), e-l+1)
// (all rotation amounts mod 64; blocks of 64 HPC positions are 64-aligned so amounts are lane constants).
//
// Reference semantics restated here (citations relative to the reference tree):
//   KminmersIterator (rust-seq2kminmers, call sites src/mers.rs:27,53)   -> seed_segment (mq_seed_general.hpp) / seed_sequence_fast (mq_seed.hpp) + kminmer_hash (mq_hash.hpp)
//   ReadOnlyIndex::get (src/index.rs:118-126)                           -> probe_table (mq_probe.hpp)
//   Match::new/update/check/extend (src/match.rs:20-58), chain_matches (src/mers.rs:57-73) -> MapSink::batch_runs (mq_probe.hpp)
//   Chain::get_match (src/chain.rs:147-169) and helpers                  -> chain_stage (mq_chain.hpp)
//   find_largest_two_chains/determine_best_match/find_coords (src/mers.rs:104-183) -> chain_stage
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mapquik_hip.h"
#include "../../include/mapquik_hip_diag.h"

namespace mq {

constexpr int WAVE = 64;
constexpr int MAX_K = 32;
constexpr int MAX_L = 64;

struct DevParams {
    uint64_t bound;  // density bound: keep l-mer iff min(fh,rh) <= bound
    uint32_t k, l, use_hpc, c, s, g;
    uint32_t fold;  // 1: a-z count as A-Z (to_ascii_uppercase of src/closures.rs:63,106 done here instead of by the caller)
    // Seeding variant (MQ_SEEDVAR_* bits, include/mapquik_hip.h; 0 = the frozen reading).  What the kernels see of each bit:
    //   1, 2   nothing: `bound` already is what `hash <= bound` must be compared with (bound - 1 for the strict test; keep_none when
    //          even that cannot say it: strict test against a bound of 0)
    //   4      the seeds are the low halves of the 64-bit seeds, DUPLICATED into both halves of a 64-bit word: rol64 of such a word
    //          is rol32 of its half in both halves, XOR keeps the form, and dup(a) <= dup(b) <=> a <= b -- so every kernel runs
    //          unchanged on dup(h32) against bound = dup(bound32), and only a hash on its way into a list is cut to its low word
    //   8      a minimizer's listed position is (raw position of the NEXT run head) - 1
    //   16     a minimizer carries a second position (raw position of its window's last compressed base) in a list of its own
    //   32     kminmer_hash: an undecided (palindromic) tuple counts as reversed
    uint32_t variant;
    uint32_t keep_none;  // 1: no l-mer passes the density test at all
    uint32_t fast_kh;    // 1: MQ_FLAG_FAST_KH -- the tuple hash is kh_fast() instead of SipHash-1-3 (index and reads alike)
};
// VAR = false: code built for the frozen reading only -- the variant bits are not even looked at, so map_kernel's instantiation for
// variant 0 (every timed launch) carries none of the variants' code or registers; every other kernel is built with VAR = true and
// decides at run time (wave-uniform branches), with identical results for variant 0
template <bool VAR> __device__ __forceinline__ bool var_h32(const DevParams &P) { return VAR && (P.variant & MQ_SEEDVAR_HASH32) != 0; }
template <bool VAR> __device__ __forceinline__ bool var_pos_end(const DevParams &P) { return VAR && (P.variant & MQ_SEEDVAR_POS_RUN_END) != 0; }
template <bool VAR> __device__ __forceinline__ bool var_end_compressed(const DevParams &P) { return VAR && (P.variant & MQ_SEEDVAR_END_COMPRESSED) != 0; }
template <bool VAR> __device__ __forceinline__ bool var_rev_eq(const DevParams &P) { return VAR && (P.variant & MQ_SEEDVAR_REV_ON_EQUAL) != 0; }
template <bool VAR> __device__ __forceinline__ bool var_keep_none(const DevParams &P) { return VAR && P.keep_none != 0; }
// a hash as it goes into a minimizer list: the 32-bit variant's value zero-extended
template <bool VAR> __device__ __forceinline__ uint64_t list_hash(const DevParams &P, uint64_t h) { return var_h32<VAR>(P) ? (h & 0xFFFFFFFFull) : h; }

// Spec: the parameters a map kernel instantiation is COMPILED for.  k, l, use_hpc, fold and fast_kh reach the hot code of the fused pair
// through the spec_* accessors below and nowhere else: with SpecNone they are DevParams' wave-uniform run-time values (any parameters,
// every other kernel), with a SpecFixed they are constants -- immediates instead of SGPR operands, one tuple hash and one window hash
// instead of a dispatch over all of them, and no kh_fast code (a SpecFixed is built for SipHash only).  The host launches a SpecFixed
// pair only for an index whose DevParams equal it field by field (mq_host_state.hpp, MAP_SPECS): same source path, same results.
struct SpecNone {
    static constexpr bool FIXED = false;
};
template <uint32_t K_, uint32_t L_, bool HPC_, bool FOLD_>
struct SpecFixed {
    static constexpr bool FIXED = true;
    static constexpr uint32_t K = K_, L = L_;
    static constexpr bool HPC = HPC_, FOLD = FOLD_, FAST_KH = false;
    static_assert(K_ >= 1 && K_ <= MAX_K && L_ >= 1 && L_ <= MAX_L, "k and l within MAX_K, MAX_L");
};
template <class Spec> __device__ __forceinline__ uint32_t spec_k(const DevParams &P) {
    if constexpr (Spec::FIXED) return Spec::K;
    else return P.k;
}
template <class Spec> __device__ __forceinline__ uint32_t spec_l(const DevParams &P) {
    if constexpr (Spec::FIXED) return Spec::L;
    else return P.l;
}
template <class Spec> __device__ __forceinline__ bool spec_hpc(const DevParams &P) {
    if constexpr (Spec::FIXED) return Spec::HPC;
    else return P.use_hpc != 0;
}
template <class Spec> __device__ __forceinline__ bool spec_fold(const DevParams &P) {
    if constexpr (Spec::FIXED) return Spec::FOLD;
    else return P.fold != 0;
}
template <class Spec> __device__ __forceinline__ bool spec_fast_kh(const DevParams &P) {
    if constexpr (Spec::FIXED) return Spec::FAST_KH;
    else return P.fast_kh != 0;
}

// Index table: 64-byte buckets of two 32-byte slots, both keys first so that ONE 16-byte load decides most lookups.
//   slot s = bucket s >> 1, way s & 1;  key == 0 <=> empty (a real key 0 lives in way 0 of one extra bucket behind the table).
// Probe sequence of a key (insert and lookup walk the same one; src/index.rs:11-39's identity hasher gives the home slot):
//   home slot (key & mask), the other way of the home bucket, then the following buckets way 0, way 1, ...
// A slot is live iff its key matches, pay.end != 0 and ENTRY_DUP is not set in pay.id_rc: a key inserted more than once gets the
// bit while the table is built (the order-independent form of "second insert => tombstone", src/index.rs:94-104; is_empty <=>
// end == 0, src/index.rs:67-69), so a lookup needs the 16 payload bytes only, and only for a key that matched.
struct alignas(16) Entry {
    uint32_t start, end, offset, id_rc;
};
struct alignas(64) Bucket {
    unsigned long long key[2];
    Entry pay[2];
    uint32_t claims;    // extra bucket only: insertions of the key 0 (its key field cannot tell "present" from "empty")
    uint32_t pad[3];
};
static_assert(sizeof(Bucket) == 64, "bucket size");
// Entry::id_rc bit 31: the key was inserted more than once (or its entry's end is 0): the reference's tombstone, an entry that
// compares as empty (src/index.rs:67-69, 94-104).  Set while the table is built (table_insert); reference ids stay below 2^24.
constexpr uint32_t ENTRY_DUP = 0x80000000u;
__device__ __forceinline__ bool entry_live(const Entry &e) { return e.end != 0u && !(e.id_rc & ENTRY_DUP); }
constexpr uint32_t SLOT_BYTES = 32;  // table bytes per slot

// reference k-min-mer waiting for insertion (same layout as mq_kminmer, rev field = id<<1|rc)
struct alignas(8) RefKmm {
    unsigned long long hash;
    uint32_t start, end, offset, id_rc;
};
static_assert(sizeof(RefKmm) == 24, "RefKmm size");

// src/match.rs:10-18 plus the ref id of the run's first entry (src/mers.rs:68) and a "grouped" flag
struct alignas(16) MatchRec {
    uint32_t q_start, q_end, r_start, r_end, count, ref, rc, done;
};

}  // namespace mq
