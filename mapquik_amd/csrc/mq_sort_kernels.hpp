// mq_sort_kernels.hpp -- coordinate order of finished hits (mq_sorter): a stable least-significant-digit radix sort of (ref_id, r_start,
// ordinal) written for wave64 (part of the one translation unit mq_capi.hip).  The rules are the header's (include/mapquik_hip.h):
//
// What is kept.  Hit i of an add with first_ordinal o carries the ordinal o + i.  It is kept iff status == MQ_HIT_MAPPED, mapq >= min_mapq
// and ref_id exists in the snapshot (id < n_ids and lens[id] > 0); any other status is tallied not_mapped, a mapped hit below min_mapq
// below_mapq, a mapped hit at or above it on an id beyond the snapshot or in a hole out_of_range.  r_start is not range-checked.
//
// Layout.  Kept records lie compactly in two arrays, key[] (u64 = ref_id << 32 | r_start) and ord[] (u32): 12 bytes per record.  The order
// is that of the 88-bit number (ref_id : 24, r_start : 32, ordinal : 32), eleven 8-bit digits: digits 0 .. 3 are the ordinal's bytes, 4 .. 7
// r_start's, 8 .. 10 ref_id's.  The append order of the adds is not deterministic and need not be: the ordinal is part of the key, so the
// sorted order is a function of the multiset of records alone.
//
//   sort_add_kernel      one lane per hit: filter, then ONE atomic on the cursor per wave (ballot, popcount, the leader adds, every kept
//                        lane takes its rank among the kept lanes below it); tallies wave-summed, one atomic per counter and workgroup
//   sort_hist_kernel     one pass over the kept records: all 11 digit histograms, privatised in LDS per workgroup, then added to the
//                        global 11 x 256 block.  The host reads it and skips every digit in which all kept records agree.
//   per digit that remains, least significant first, from one key / ordinal set to the other:
//   sort_count_kernel    a workgroup per tile of MQ_SORT_TILE records: the tile's 256 digit counts, stored digit-major [256][n_tiles]
//   sort_scan_kernel     a workgroup per digit VALUE: exclusive scan of that value's row of n_tiles counts in place (chunks of 256 with a
//                        carry: any tile count), and the row's total
//   sort_scatter_kernel  a workgroup per tile: the exclusive scan of the 256 row totals (where each digit value's records begin), plus the
//                        tile's row prefix, plus a STABLE rank inside the tile; then every record is stored to its place
//   sort_refs_kernel     one lane per existing reference: first / count in the sorted keys by two binary searches (the three ref_id byte
//                        histograms do not say how sparse ids combine, the sorted keys do)
//
// Stability inside a tile.  Wave w of the workgroup owns the tile's records [w * T / 4, (w + 1) * T / 4), 64 consecutive ones per round, so
// "lower index" is (wave, round, lane) in that order.  Per round a lane finds its peers -- the lanes with its digit -- from eight ballots
// (match-any); its rank among them is the popcount of the peers below it, and the wave's running count of the digit (wave-private LDS,
// read before the round's first peer writes it back increased) is the rank of the round among the wave's earlier rounds.  After the
// rounds one thread per digit value turns the four waves' counts into the waves' first positions.  No atomics: the rank is a function of
// the tile's content.
#pragma once
#include "../../include/mapquik_hip.h"  // mq_hit, MQ_HIT_MAPPED
#include "mq_wave.hpp"                  // lane_id, rdlane64, mbcnt64, wave_sync, the DPP scan

constexpr uint32_t MQ_SORT_TILE = 2048;   // records per tile: 24 KB of keys and ordinals against the tile's 1 KB of counts
constexpr uint32_t MQ_SORT_DIGITS = 11;   // 8-bit digits of the 88-bit key
constexpr uint32_t MQ_SORT_ROUNDS = MQ_SORT_TILE / 256u;  // records per thread of the count / scatter workgroup
static_assert(MQ_SORT_TILE % 256u == 0, "a tile is whole rounds of a 256-thread workgroup");

// acc: [0] the append cursor = kept, [1] not_mapped, [2] below_mapq, [3] out_of_range (`offered` is the host's: it knows every n).
constexpr uint32_t SORT_ACC_WORDS = 4;

__device__ __forceinline__ uint32_t sort_digit(uint64_t key, uint32_t ord, uint32_t d) {  // d is wave-uniform
    return d < 4u ? (ord >> (8u * d)) & 255u : (uint32_t)(key >> (8u * (d - 4u))) & 255u;
}

// One lane per hit, whole waves per trip (lanes behind n keep nothing, so all 64 lanes reach the ballot).  Only the first two 16-byte
// words of a hit are loaded (status, ref_id, rc, mapq | q_start, q_end, r_start, r_end).  lens: dense by reference id, n_ids entries.
// The host has made sure that offered + n <= cap before the launch; the store is bounded by cap all the same.
__global__ __launch_bounds__(256) void sort_add_kernel(const mq_hit *__restrict__ hits, uint32_t n, uint32_t first_ordinal, uint32_t min_mapq, const uint64_t *__restrict__ lens,
                                                       uint32_t n_ids, unsigned long long *__restrict__ key, uint32_t *__restrict__ ord, uint64_t cap,
                                                       unsigned long long *__restrict__ acc) {
    __shared__ uint32_t tally[3][4];
    uint32_t not_mapped = 0, below_mapq = 0, out_of_range = 0;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += step) {
        const uint64_t i = i0 + lane;
        bool keep = false;
        uint64_t k = 0;
        if (i < n) {
            const uint4 *const p = reinterpret_cast<const uint4 *>(hits + i);
            const uint4 h0 = p[0], h1 = p[1];
            if (h0.x != MQ_HIT_MAPPED) not_mapped++;
            else if (h0.w < min_mapq) below_mapq++;
            else if (h0.y >= n_ids || lens[h0.y] == 0) out_of_range++;
            else {
                keep = true;
                k = ((uint64_t)h0.y << 32) | h1.z;
            }
        }
        const uint64_t kept = __ballot(keep);
        if (kept) {  // (wave-uniform)
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(&acc[0], (unsigned long long)__popcll(kept));  // one atomic per wave
            at = rdlane64(at, 0);
            const uint64_t pos = at + mbcnt64(kept);  // the kept lanes below this one
            if (keep && pos < cap) {
                key[pos] = k;
                ord[pos] = first_ordinal + (uint32_t)i;
            }
        }
    }
    not_mapped = wave_sum_u32(not_mapped);
    below_mapq = wave_sum_u32(below_mapq);
    out_of_range = wave_sum_u32(out_of_range);
    if (lane == 0) {
        tally[0][threadIdx.x >> 6] = not_mapped;
        tally[1][threadIdx.x >> 6] = below_mapq;
        tally[2][threadIdx.x >> 6] = out_of_range;
    }
    __syncthreads();
    if (threadIdx.x < 3) {  // one atomic per counter and workgroup
        const uint32_t c = tally[threadIdx.x][0] + tally[threadIdx.x][1] + tally[threadIdx.x][2] + tally[threadIdx.x][3];
        if (c) atomicAdd(&acc[1 + threadIdx.x], (unsigned long long)c);
    }
}

// All 11 digit histograms of the n kept records: hist[d * 256 + v] += the records whose digit d is v.
__global__ __launch_bounds__(256) void sort_hist_kernel(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ ord, uint64_t n, unsigned long long *__restrict__ hist) {
    __shared__ uint32_t h[MQ_SORT_DIGITS * 256];
    for (uint32_t j = threadIdx.x; j < MQ_SORT_DIGITS * 256u; j += 256u) h[j] = 0;
    __syncthreads();
    const uint64_t step = (uint64_t)gridDim.x * 256u;  // (a workgroup sees fewer than 2^32 records: the bins are 32 bits wide)
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += step) {
        const uint64_t k = key[i];
        const uint32_t o = ord[i];
#pragma unroll
        for (uint32_t d = 0; d < MQ_SORT_DIGITS; ++d) atomicAdd(&h[d * 256u + sort_digit(k, o, d)], 1u);
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < MQ_SORT_DIGITS * 256u; j += 256u) {
        const uint32_t c = h[j];
        if (c) atomicAdd(&hist[j], (unsigned long long)c);
    }
}

// A workgroup per tile: counts[v * n_tiles + tile] = the tile's records whose digit d is v.
__global__ __launch_bounds__(256) void sort_count_kernel(const unsigned long long *__restrict__ key, const uint32_t *__restrict__ ord, uint64_t n, uint32_t d, uint32_t n_tiles,
                                                         uint32_t *__restrict__ counts) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t first = (uint64_t)blockIdx.x * MQ_SORT_TILE;
#pragma unroll
    for (uint32_t r = 0; r < MQ_SORT_ROUNDS; ++r) {
        const uint64_t i = first + r * 256u + threadIdx.x;
        if (i < n) atomicAdd(&h[sort_digit(key[i], ord[i], d)], 1u);
    }
    __syncthreads();
    counts[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

// the exclusive prefix of x over the workgroup's 256 threads and the workgroup's total; part: four words of LDS (two barriers)
__device__ __forceinline__ uint32_t sort_block_excl_scan(uint32_t x, uint32_t *part, uint32_t *total) {
    const uint32_t incl = wave_incl_scan_u32(x), w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) part[w] = incl;
    __syncthreads();
    const uint32_t p0 = part[0], p1 = part[1], p2 = part[2], p3 = part[3];
    __syncthreads();  // (part may be written again at once)
    *total = p0 + p1 + p2 + p3;
    return incl - x + (w > 0 ? p0 : 0u) + (w > 1 ? p1 : 0u) + (w > 2 ? p2 : 0u);
}

// A workgroup per digit value v (grid 256): row v of the counts becomes its own exclusive prefix over the tiles, in chunks of 256 with a
// carry, so for any tile count; totals[v] = the row's sum.  (A thread reads and writes its own elements only.)
__global__ __launch_bounds__(256) void sort_scan_kernel(uint32_t *counts, uint32_t n_tiles, uint32_t *__restrict__ totals) {
    __shared__ uint32_t part[4];
    uint32_t *const row = counts + (uint64_t)blockIdx.x * n_tiles;
    uint32_t carry = 0;
    for (uint32_t c = 0; c < n_tiles; c += 256u) {  // (c + 255 cannot wrap: n_tiles <= 2^32 / MQ_SORT_TILE)
        const uint32_t t = c + threadIdx.x;
        const uint32_t x = t < n_tiles ? row[t] : 0u;
        uint32_t total;
        const uint32_t excl = sort_block_excl_scan(x, part, &total);
        if (t < n_tiles) row[t] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// A workgroup per tile.  pref: the scanned counts; totals: the 256 row sums.  A record with digit v goes to
// (the sum of totals[< v]) + pref[v][tile] + its stable rank among the tile's records with digit v.
__global__ __launch_bounds__(256) void sort_scatter_kernel(const unsigned long long *__restrict__ key_in, const uint32_t *__restrict__ ord_in, uint64_t n, uint32_t d, uint32_t n_tiles,
                                                           const uint32_t *__restrict__ pref, const uint32_t *__restrict__ totals, unsigned long long *__restrict__ key_out,
                                                           uint32_t *__restrict__ ord_out) {
    __shared__ uint32_t cnt[4][256];  // per wave: the running count of every digit value, then the wave's first position for it
    __shared__ uint32_t part[4];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) cnt[j][threadIdx.x] = 0;
    uint32_t total;
    const uint32_t digit_first = sort_block_excl_scan(totals[threadIdx.x], part, &total);  // (its barriers also cover the zeroing)
    const uint64_t first = (uint64_t)blockIdx.x * MQ_SORT_TILE + (uint64_t)w * (MQ_SORT_TILE / 4u);
    uint64_t k[MQ_SORT_ROUNDS];
    uint32_t o[MQ_SORT_ROUNDS], rank[MQ_SORT_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < MQ_SORT_ROUNDS; ++r) {
        const uint64_t i = first + r * 64u + lane;
        const bool in = i < n;
        k[r] = in ? key_in[i] : 0ull;
        o[r] = in ? ord_in[i] : 0u;
    }
#pragma unroll
    for (uint32_t r = 0; r < MQ_SORT_ROUNDS; ++r) {
        const bool in = first + r * 64u + lane < n;
        const uint32_t v = sort_digit(k[r], o[r], d);
        uint64_t peers = __ballot(in);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {  // match-any: the lanes that agree with this one in every bit of the digit
            const uint64_t m = __ballot((v >> b) & 1u);
            peers &= ((v >> b) & 1u) ? m : ~m;
        }
        const uint32_t below = mbcnt64(peers);  // peers in lower lanes
        const uint32_t before = cnt[w][v];      // the wave's earlier rounds
        wave_sync();
        if (in && below == 0) cnt[w][v] = before + (uint32_t)__popcll(peers);  // one lane per digit value present
        wave_sync();
        rank[r] = before + below;
    }
    __syncthreads();
    {
        const uint32_t v = threadIdx.x;  // one thread per digit value: the waves' counts become the waves' first positions
        uint32_t at = digit_first + pref[(uint64_t)v * n_tiles + blockIdx.x];
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j) {
            const uint32_t c = cnt[j][v];
            cnt[j][v] = at;
            at += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < MQ_SORT_ROUNDS; ++r) {
        if (first + r * 64u + lane < n) {
            const uint64_t pos = (uint64_t)cnt[w][sort_digit(k[r], o[r], d)] + rank[r];
            if (pos < n) {  // (a permutation of [0, n) by construction; no store leaves the arrays whatever the counts hold)
                key_out[pos] = k[r];
                ord_out[pos] = o[r];
            }
        }
    }
}

// One lane per existing reference c (ids ascending): out[2c] = the first sorted record of ids[c], out[2c + 1] = how many.
__device__ __forceinline__ uint64_t sort_lower_bound(const unsigned long long *__restrict__ key, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__global__ __launch_bounds__(256) void sort_refs_kernel(const unsigned long long *__restrict__ key, uint64_t n, const uint32_t *__restrict__ ids, uint32_t n_refs,
                                                        unsigned long long *__restrict__ out) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= n_refs) return;
    const uint64_t id = ids[c];
    const uint64_t a = sort_lower_bound(key, n, id << 32), b = sort_lower_bound(key, n, (id + 1) << 32);
    out[2 * c] = a;
    out[2 * c + 1] = b - a;
}
