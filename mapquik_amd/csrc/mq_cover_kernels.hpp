// mq_cover_kernels.hpp -- index coverage (mq_index_coverage): which bases of which reference the live k-min-mers of a finished table
// span, and how many live k-min-mers each reference owns (part of the one translation unit mq_capi.hip).
//
// What counts.  A slot is live as everywhere else (entry_live: end != 0 and no ENTRY_DUP).  A live entry of reference `id` with reference
// length `len` covers the bases [start, min(end, len - 1)], both ends inclusive: the interval the entry itself records, what a Match of
// that k-min-mer alone reports as r_start and r_end.  (With homopolymer compression end = pos[k - 1] + l - 1 counts l COMPRESSED bases
// from the last minimizer's raw position and may stop short of the l-mer's true last raw base; the coverage reports what the index
// records and does not repair it.)  A live entry with start > end or start >= len covers nothing and is counted in out_of_range (only a
// crafted file holds one; so is one that names a reference the index does not have, which no loader lets in).  Dead entries contribute
// nothing; the key 0 in the extra bucket counts like any other key.  A base whose only possible entry would have end == 0 can never be
// covered: such an entry is born dead (table_insert), so base 0 of a reference is covered only by an entry that ends behind it.
//
// Layout.  A bitmap of 64-bit words, one bit per base; every reference that exists (len > 0 in the dense length array) starts on a word
// boundary, at cover base word `base[id]` (a dense array beside the lengths: holes in the id range own no word of the bitmap), and
// takes ceil(len / 64) words.  The bitmap is cut into tiles of MQ_COV_TILE_WORDS words that never span two references; the host builds
// the descriptors (CovTile).  Bits at and behind `len` in a reference's last word are never set.
//
//   cover_mark_kernel    the table as a stream (retable_kernel's source side): 64-bit atomic ORs whose result nobody reads
//   cover_count_kernel   one wave per tile: covered bases and run starts per tile and per reference
//   cover_scan_kernel    exclusive prefix of the tiles' run starts (one workgroup, scan_counts_kernel's pattern), first_interval per reference
//   cover_emit_kernel    the count's pass again: a start and an end stored per run, at base + rank
//
// Runs across tiles.  A run START is a set bit whose predecessor in the same reference is clear: w & ~((w << 1) | carry), carry = bit 63
// of the previous word, 0 at a reference's first word.  A run END is kept as the first clear bit behind a run, ~w & ((w << 1) | carry),
// whose position is the interval's half-open end, so both need the PREVIOUS word only and one scan serves both: the ends that lie in
// front of tile t are the starts in front of it minus one if the carry into the tile is set (that run's end lies in t or behind it).
// A reference's last word ends its run whatever follows: when its bit 63 is set (len a multiple of 64) the lane that holds it adds the
// end `len` behind the word's own.
#pragma once
#include "../../include/mapquik_hip.h"  // mq_cov_interval
#include "mq_device.hpp"                // Bucket, Entry, entry_live
#include "mq_probe.hpp"                 // ld_u4, u64_of
#include "mq_wave.hpp"                  // lane_id, rdlane, rdfirst, the DPP scans
// (RETABLE_AHEAD, the slots a lane loads ahead of its first use, is mq_build_kernels.hpp's: the part in front of this one)

constexpr uint32_t MQ_COV_TILE_WORDS = 1024;  // 65,536 bases per tile: about 48 k tiles for a 3.1-Gbp genome
static_assert(MQ_COV_TILE_WORDS % 128u == 0, "a wave takes 128 words per step");
constexpr uint32_t MQ_COV_LDS_IDS = 4096;     // dense id ranges up to here count live entries in a workgroup histogram

struct alignas(8) CovTile {
    uint64_t first_word;  // of the bitmap
    uint32_t ref;         // index into the existing references, in id order (not the id)
    uint32_t n_words;     // 1 .. MQ_COV_TILE_WORDS
    uint32_t ref_word;    // the tile's first word, counted from its reference's first
    uint32_t flags;       // COV_FIRST / COV_LAST: the reference's first / last tile
};
static_assert(sizeof(CovTile) == 24, "tile descriptor size");
constexpr uint32_t COV_FIRST = 1u, COV_LAST = 2u;
struct alignas(8) CovWords {  // a lane's two words of a step: one 16-byte load (a reference's first word may be an odd one)
    unsigned long long a, b;
};

// acc: [0] entries out of range.  live: one counter per reference id (dense).  n_ids: max id + 1.
__global__ __launch_bounds__(256) void cover_mark_kernel(const Bucket *__restrict__ table, uint64_t n_buckets_plus1, const uint64_t *__restrict__ ref_lens,
                                                         const uint64_t *__restrict__ base, uint32_t n_ids, unsigned long long *__restrict__ bitmap,
                                                         unsigned long long *__restrict__ live, unsigned long long *__restrict__ acc) {
    __shared__ uint32_t hist[MQ_COV_LDS_IDS];
    const bool lds = n_ids <= MQ_COV_LDS_IDS;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < n_ids; i += blockDim.x) hist[i] = 0;
        __syncthreads();
    }
    uint32_t out_of_range = 0;
    const uint64_t n = 2 * n_buckets_plus1;  // slots, the extra bucket's two included
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x * RETABLE_AHEAD;
    for (uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u)) * RETABLE_AHEAD + (threadIdx.x & 63u); i0 < n; i0 += step) {
        uint4 kk[RETABLE_AHEAD], pp[RETABLE_AHEAD];
        uint32_t claims[RETABLE_AHEAD];
#pragma unroll
        for (uint32_t u = 0; u < RETABLE_AHEAD; ++u) {  // (a slot past the end reads the last one again: no branch around a load)
            const uint64_t i = i0 + 64u * u < n ? i0 + 64u * u : n - 1;
            const Bucket &B = table[i >> 1];
            kk[u] = ld_u4(B.key);
            pp[u] = ld_u4(&B.pay[i & 1u]);
            claims[u] = B.claims;
        }
#pragma unroll
        for (uint32_t u = 0; u < RETABLE_AHEAD; ++u) {
            const uint64_t i = i0 + 64u * u;
            const uint32_t w = (uint32_t)i & 1u;
            const bool extra = (i >> 1) == n_buckets_plus1 - 1;
            const unsigned long long key = w ? u64_of(kk[u].z, kk[u].w) : u64_of(kk[u].x, kk[u].y);
            const bool occupied = i < n && (extra ? (w == 0 && claims[u] != 0) : key != 0);  // slot_occupied, on the loaded words
            Entry e;
            e.start = pp[u].x, e.end = pp[u].y, e.offset = pp[u].z, e.id_rc = pp[u].w;
            if (!occupied || !entry_live(e)) continue;
            const uint32_t id = e.id_rc >> 1;
            const uint64_t len = id < n_ids ? ref_lens[id] : 0;
            if (len == 0 || e.start > e.end || e.start >= len) {
                out_of_range++;
                continue;
            }
            if (lds) atomicAdd(&hist[id], 1u);
            else atomicAdd(&live[id], 1ull);
            const uint32_t last = e.end < len ? e.end : (uint32_t)(len - 1);
            unsigned long long *const words = bitmap + base[id];
            const uint32_t w0 = e.start >> 6, w1 = last >> 6;  // (w1 < ceil(len / 64): inside the reference's words)
            const unsigned long long m0 = ~0ull << (e.start & 63u), m1 = ~0ull >> (63u - (last & 63u));
            if (w0 == w1) {
                atomicOr(&words[w0], m0 & m1);
            } else {
                atomicOr(&words[w0], m0);
                for (uint32_t x = w0 + 1; x < w1; ++x) atomicOr(&words[x], ~0ull);
                atomicOr(&words[w1], m1);
            }
        }
    }
    out_of_range = wave_sum_u32(out_of_range);
    if (lane_id() == 0 && out_of_range) atomicAdd(&acc[0], (unsigned long long)out_of_range);
    if (lds) {  // at most one global atomic per (workgroup, reference)
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_ids; i += blockDim.x) {
            const uint32_t c = hist[i];
            if (c) atomicAdd(&live[i], (unsigned long long)c);
        }
    }
}

// What both passes over a tile share: a step's two words per lane with the words behind the tile's last masked off, the bit that
// precedes each word in its reference, the run starts and the run ends (header comment).
struct CovStep {
    unsigned long long a, b;    // the lane's words 2 * lane and 2 * lane + 1 of the step (0 behind the tile's end)
    unsigned long long sa, sb;  // run starts
    unsigned long long ea, eb;  // run ends: the first clear bit behind a run
    bool tail;                  // this lane holds the reference's last word and its bit 63 is set: one more end, at `len`
    bool tail_in_b;
};
// carry: bit 63 of the word in front of the step's first (wave-uniform); returns the carry into the next step
__device__ __forceinline__ uint32_t cov_step(const unsigned long long *__restrict__ words, const CovTile &T, uint32_t w_step, uint32_t lane, uint32_t carry, CovStep &S) {
    const uint32_t wa = w_step + 2u * lane;
    CovWords v = {0ull, 0ull};
    if (wa < T.n_words) v = *reinterpret_cast<const CovWords *>(words + wa);  // (the bitmap has two words of padding behind its last)
    S.a = v.a;
    S.b = wa + 1u < T.n_words ? v.b : 0ull;
    const uint32_t top_b = (uint32_t)(S.b >> 63);
    uint32_t prev = (uint32_t)__shfl_up((int)top_b, 1, 64);  // bit 63 of the previous lane's second word
    if (lane == 0) prev = carry;
    const unsigned long long pa = (S.a << 1) | prev, pb = (S.b << 1) | (S.a >> 63);
    S.sa = S.a & ~pa, S.sb = S.b & ~pb;
    S.ea = ~S.a & pa, S.eb = ~S.b & pb;
    // words behind the tile's end are 0 here, so the word behind the tile's last shows an end at its bit 0 when the run reaches the
    // tile's last bit: that end belongs to the next tile (or, in a reference's last tile, is the tail) -- not to this one
    if (wa >= T.n_words) S.ea = 0;
    if (wa + 1u >= T.n_words) S.eb = 0;
    const bool last_tile = (T.flags & COV_LAST) != 0;
    S.tail_in_b = wa + 2u == T.n_words;
    S.tail = last_tile && ((S.tail_in_b && top_b) || (wa + 1u == T.n_words && (S.a >> 63)));
    return rdlane(top_b, 63);  // (0 once the step runs past the tile: nobody reads it then)
}
// the bit in front of a tile's first word: 0 at a reference's first tile
__device__ __forceinline__ uint32_t cov_tile_carry(const unsigned long long *__restrict__ bitmap, const CovTile &T) {
    return (T.flags & COV_FIRST) ? 0u : (uint32_t)(bitmap[T.first_word - 1] >> 63);
}

// One wave per tile.  tile_runs[t]: run starts of tile t; ref_sums[2 * ref]: covered bases, [2 * ref + 1]: run starts (one atomic each per tile).
__global__ __launch_bounds__(256) void cover_count_kernel(const unsigned long long *__restrict__ bitmap, const CovTile *__restrict__ tiles, uint32_t n_tiles,
                                                          uint32_t *__restrict__ tile_runs, unsigned long long *__restrict__ ref_sums) {
    const uint32_t lane = lane_id();
    const uint32_t t = rdfirst(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (t >= n_tiles) return;
    const CovTile T = tiles[t];
    const unsigned long long *words = bitmap + T.first_word;
    uint32_t carry = cov_tile_carry(bitmap, T);
    uint32_t covered = 0, runs = 0;
    for (uint32_t w = 0; w < T.n_words; w += 128u) {
        CovStep S;
        carry = cov_step(words, T, w, lane, carry, S);
        covered += (uint32_t)__popcll(S.a) + (uint32_t)__popcll(S.b);
        runs += (uint32_t)__popcll(S.sa) + (uint32_t)__popcll(S.sb);
    }
    covered = wave_sum_u32(covered);
    runs = wave_sum_u32(runs);
    if (lane == 0) {
        tile_runs[t] = runs;
        if (covered) atomicAdd(&ref_sums[2 * T.ref], (unsigned long long)covered);
        if (runs) atomicAdd(&ref_sums[2 * T.ref + 1], (unsigned long long)runs);
    }
}

// Exclusive prefix of the tiles' run starts: tile_off[t], tile_off[n_tiles] = the number of intervals; first_interval[ref] at every
// reference's first tile.  One workgroup.
__global__ __launch_bounds__(1024) void cover_scan_kernel(const uint32_t *__restrict__ tile_runs, const CovTile *__restrict__ tiles, uint32_t n_tiles,
                                                          unsigned long long *__restrict__ tile_off, unsigned long long *__restrict__ first_interval) {
    __shared__ unsigned long long part[1024];
    const uint32_t t = threadIdx.x, per = (n_tiles + 1023u) / 1024u;
    const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    unsigned long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += tile_runs[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const unsigned long long v = t >= d ? part[t - d] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = part[t] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        tile_off[i] = run;
        if (tiles[i].flags & COV_FIRST) first_interval[tiles[i].ref] = run;
        run += tile_runs[i];
    }
    if (t == 1023u) tile_off[n_tiles] = part[1023];
}

// The count's pass again, lane = word pair: the r-th start of the tile goes to intervals[tile_off + r].start, the r-th end to
// intervals[tile_off - carry + r].end.  ref_lens_c: the existing references' lengths, by CovTile::ref.  n_intervals bounds every store.
__device__ __forceinline__ void cov_store_bits(unsigned long long m, uint32_t bit0, uint32_t *__restrict__ field, unsigned long long at, unsigned long long n_intervals) {
    while (m) {
        const uint32_t b = (uint32_t)__builtin_ctzll(m);
        m &= m - 1;
        if (at < n_intervals) field[2 * at] = bit0 + b;
        ++at;
    }
}
__global__ __launch_bounds__(256) void cover_emit_kernel(const unsigned long long *__restrict__ bitmap, const CovTile *__restrict__ tiles, uint32_t n_tiles,
                                                         const unsigned long long *__restrict__ tile_off, const uint64_t *__restrict__ ref_lens_c,
                                                         mq_cov_interval *__restrict__ intervals, unsigned long long n_intervals) {
    const uint32_t lane = lane_id();
    const uint32_t t = rdfirst(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (t >= n_tiles) return;
    const CovTile T = tiles[t];
    const unsigned long long *words = bitmap + T.first_word;
    uint32_t carry = cov_tile_carry(bitmap, T);
    unsigned long long s_at = tile_off[t], e_at = s_at - carry;  // (carry set: at least one start lies in front of this tile)
    uint32_t *const starts = &intervals[0].start, *const ends = &intervals[0].end;
    const uint32_t len = (uint32_t)ref_lens_c[T.ref];
    for (uint32_t w = 0; w < T.n_words; w += 128u) {
        CovStep S;
        carry = cov_step(words, T, w, lane, carry, S);
        const uint32_t ns = (uint32_t)__popcll(S.sa) + (uint32_t)__popcll(S.sb);
        const uint32_t ne = (uint32_t)__popcll(S.ea) + (uint32_t)__popcll(S.eb) + (S.tail ? 1u : 0u);
        const uint32_t is = wave_incl_scan_u32(ns), ie = wave_incl_scan_u32(ne);
        const uint32_t bit0 = (T.ref_word + w + 2u * lane) * 64u;  // the position of the lane's first bit in its reference
        unsigned long long at = s_at + (is - ns);
        cov_store_bits(S.sa, bit0, starts, at, n_intervals);
        cov_store_bits(S.sb, bit0 + 64u, starts, at + (uint32_t)__popcll(S.sa), n_intervals);
        at = e_at + (ie - ne);
        cov_store_bits(S.ea, bit0, ends, at, n_intervals);
        cov_store_bits(S.eb, bit0 + 64u, ends, at + (uint32_t)__popcll(S.ea), n_intervals);
        if (S.tail && at + ne - 1u < n_intervals) ends[2 * (at + ne - 1u)] = len;
        s_at += rdlane(is, 63);
        e_at += rdlane(ie, 63);
    }
}
