// mq_depth_kernels.hpp -- mapping depth (mq_depth): how many read bases landed in every window of every reference, accumulated from
// finished mq_hit records (part of the one translation unit mq_capi.hip).  The rules are the header's (include/mapquik_hip.h) and mirror
// the coverage's (mq_cover_kernels.hpp):
//
// What counts.  A hit is counted iff status == MQ_HIT_MAPPED and mapq >= min_mapq; any other status is tallied as not_mapped, a mapped hit
// below min_mapq as below_mapq.  A counted hit on reference `id` of length `len` covers the bases [r_start, min(r_end, len - 1)], both ends
// inclusive; with r_start > r_end, r_start >= len, id >= n_ids or len == 0 (a hole of a sparse id range) it covers nothing and is
// tallied as out_of_range instead.  Window j of a reference is [j * w, min((j + 1) * w, len)), 1 <= w <= 2^24, any integer.
//
// Layout.  Every reference that exists owns ceil(len / w) windows, beginning at window `base[id]` (a dense array beside the lengths, as in
// the coverage plan: holes own nothing); the windows of all references lie behind one another in id order.  Per window three accumulators,
// built so that a hit costs O(1) atomics whatever its length:
//   edge   (u64)  bases of hits in their first and in their last window (a hit inside one window: all of its bases)
//   diff   (i32)  a difference array over the windows of one reference: +1 at the first window strictly between a hit's first and last,
//                 -1 at its last window.  Both land inside the hit's reference, so every reference's diff sums to 0; the running sum at
//                 window j is the number of hits that have j strictly inside, and such a window is always a full one (only a reference's
//                 last window can be shorter, and it is never strictly inside): running * w is exact.  Fewer than 2^31 hits are ever
//                 offered to one accumulator (the host refuses more), so the running sum fits 32 bits.
//   starts (u32)  hits whose r_start lies in the window
//
//   depth_add_kernel    one lane per hit: filter, clip, at most five atomics whose results nobody reads
//   depth_sum_kernel    one wave per tile: the tile's diff summed as i64
//   depth_scan_kernel   one workgroup: exclusive prefix of the tile sums, restarted at every reference's first tile
//   depth_emit_kernel   one wave per tile: running count by a DPP scan, window_bases = running * w + edge, window_starts, and the sums,
//                       empty windows and maximum per reference
// The three result kernels read the accumulators and never change them.  Tiles of MQ_DEPTH_TILE_WINDOWS windows never span two
// references; the host builds the descriptors (DepthTile).
#pragma once
#include "../../include/mapquik_hip.h"  // mq_hit, MQ_HIT_MAPPED
#include "mq_wave.hpp"                  // lane_id, rdlane, rdfirst, shfl64, the DPP scans, ld_sc1_u64

constexpr uint32_t MQ_DEPTH_TILE_WINDOWS = 256;  // four steps of a wave: about 12 k tiles for a 3.1-Gbp genome at w = 1000
static_assert(MQ_DEPTH_TILE_WINDOWS % 64u == 0, "a wave takes 64 windows per step");
constexpr uint32_t MQ_DEPTH_LDS_IDS = 4096;      // dense id ranges up to here count reads per reference in a workgroup histogram
constexpr uint32_t MQ_DEPTH_MAX_WINDOW = 1u << 24;

struct alignas(8) DepthTile {
    uint64_t first_window;  // of the accumulators
    uint32_t ref;           // index into the existing references, in id order (not the id)
    uint32_t n_windows;     // 1 .. MQ_DEPTH_TILE_WINDOWS
    uint32_t ref_tile;      // the tile's number inside its reference: tile t - ref_tile is the reference's first
    uint32_t reserved;
};
static_assert(sizeof(DepthTile) == 24, "tile descriptor size");

// acc: [0] counted [1] not_mapped [2] below_mapq [3] out_of_range (`offered` is the host's: it knows every n).
constexpr uint32_t DEPTH_ACC_WORDS = 4;

__device__ __forceinline__ uint64_t depth_wave_sum_u64(uint64_t v) {
    for (uint32_t d = 32; d; d >>= 1) v += shfl64(v, (int)(lane_id() ^ d));
    return v;
}
__device__ __forceinline__ uint64_t depth_wave_max_u64(uint64_t v) {
    for (uint32_t d = 32; d; d >>= 1) {
        const uint64_t o = shfl64(v, (int)(lane_id() ^ d));
        v = o > v ? o : v;
    }
    return v;
}

// One lane per hit, whole waves per trip (the trip count is wave-uniform: the wave sums behind the loop see all 64 lanes).  Of a hit's
// three 16-byte words the first two hold every field the rules read (status, ref_id, mapq; r_start, r_end); the third is never loaded,
// and the compiler narrows the two loads to the 20 bytes that are used.
// lens, base: dense by reference id, n_ids entries.  reads: one counter per reference id (dense).
__global__ __launch_bounds__(256) void depth_add_kernel(const mq_hit *__restrict__ hits, uint32_t n, uint32_t w, uint32_t min_mapq, const uint64_t *__restrict__ lens,
                                                        const uint64_t *__restrict__ base, uint32_t n_ids, unsigned long long *__restrict__ edge, int *__restrict__ diff,
                                                        uint32_t *__restrict__ starts, unsigned long long *__restrict__ reads, unsigned long long *__restrict__ acc) {
    __shared__ uint32_t hist[MQ_DEPTH_LDS_IDS];
    const bool lds = n_ids <= MQ_DEPTH_LDS_IDS;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < n_ids; i += blockDim.x) hist[i] = 0;
        __syncthreads();
    }
    uint32_t counted = 0, not_mapped = 0, below_mapq = 0, out_of_range = 0;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += step) {
        const uint64_t i = i0 + (threadIdx.x & 63u);
        if (i >= n) continue;  // lanes behind n do nothing
        const uint4 *const p = reinterpret_cast<const uint4 *>(hits + i);
        const uint4 h0 = p[0], h1 = p[1];  // status, ref_id, rc, mapq | q_start, q_end, r_start, r_end
        if (h0.x != MQ_HIT_MAPPED) {
            not_mapped++;
            continue;
        }
        if (h0.w < min_mapq) {
            below_mapq++;
            continue;
        }
        const uint32_t id = h0.y, s = h1.z, r_end = h1.w;
        const uint64_t len = id < n_ids ? lens[id] : 0;
        if (len == 0 || s > r_end || s >= len) {
            out_of_range++;
            continue;
        }
        counted++;
        if (lds) atomicAdd(&hist[id], 1u);
        else atomicAdd(&reads[id], 1ull);
        const uint32_t e = r_end < len ? r_end : (uint32_t)(len - 1);
        const uint32_t a = s / w, b = e / w;  // (b < ceil(len / w): inside the reference's windows)
        const uint64_t at = base[id];
        atomicAdd(&starts[at + a], 1u);
        if (a == b) {
            atomicAdd(&edge[at + a], (unsigned long long)(e - s) + 1ull);
        } else {
            atomicAdd(&edge[at + a], (unsigned long long)(a + 1u) * w - s);
            atomicAdd(&edge[at + b], (unsigned long long)e - (unsigned long long)b * w + 1ull);
            if (b > a + 1u) {
                atomicAdd(&diff[at + a + 1u], 1);
                atomicAdd(&diff[at + b], -1);
            }
        }
    }
    counted = wave_sum_u32(counted);
    not_mapped = wave_sum_u32(not_mapped);
    below_mapq = wave_sum_u32(below_mapq);
    out_of_range = wave_sum_u32(out_of_range);
    if (lane_id() == 0) {  // one atomic per wave and counter
        if (counted) atomicAdd(&acc[0], (unsigned long long)counted);
        if (not_mapped) atomicAdd(&acc[1], (unsigned long long)not_mapped);
        if (below_mapq) atomicAdd(&acc[2], (unsigned long long)below_mapq);
        if (out_of_range) atomicAdd(&acc[3], (unsigned long long)out_of_range);
    }
    if (lds) {  // at most one global atomic per (workgroup, reference)
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_ids; i += blockDim.x) {
            const uint32_t c = hist[i];
            if (c) atomicAdd(&reads[i], (unsigned long long)c);
        }
    }
}

// One wave per tile: tile_sum[t] = the sum of the tile's diff.
__global__ __launch_bounds__(256) void depth_sum_kernel(const int *__restrict__ diff, const DepthTile *__restrict__ tiles, uint32_t n_tiles, long long *__restrict__ tile_sum) {
    const uint32_t lane = lane_id();
    const uint32_t t = rdfirst(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (t >= n_tiles) return;
    const DepthTile T = tiles[t];
    long long sum = 0;
    for (uint32_t j = lane; j < T.n_windows; j += 64u) sum += diff[T.first_window + j];
    sum = (long long)depth_wave_sum_u64((uint64_t)sum);
    if (lane == 0) tile_sum[t] = sum;
}

// Exclusive prefix of the tile sums over all tiles (tile_pref), and the same restarted at every reference's first tile (tile_off): the
// running count in front of tile t's first window.  One workgroup (cover_scan_kernel's pattern).
__global__ __launch_bounds__(1024) void depth_scan_kernel(const long long *__restrict__ tile_sum, const DepthTile *__restrict__ tiles, uint32_t n_tiles,
                                                          long long *tile_pref, long long *__restrict__ tile_off) {
    __shared__ long long part[1024];
    const uint32_t t = threadIdx.x, per = (n_tiles + 1023u) / 1024u;
    const uint32_t lo = t * per < n_tiles ? t * per : n_tiles, hi = lo + per < n_tiles ? lo + per : n_tiles;
    long long sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += tile_sum[i];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const long long v = t >= d ? part[t - d] : 0ll;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    long long run = part[t] - sum;
    for (uint32_t i = lo; i < hi; ++i) {
        tile_pref[i] = run;
        run += tile_sum[i];
    }
    __syncthreads();  // every tile's prefix is stored; a reference's first tile may be another thread's
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t first = i - tiles[i].ref_tile;
        const long long here = (long long)ld_sc1_u64(reinterpret_cast<const unsigned long long *>(tile_pref + i));
        tile_off[i] = here - (long long)ld_sc1_u64(reinterpret_cast<const unsigned long long *>(tile_pref + first));
    }
}

// One wave per tile, a window per lane and step.  ref_sums[3 * ref]: bases, [3 * ref + 1]: windows with no base, [3 * ref + 2]: the
// largest window_bases (one atomic each per tile).
__global__ __launch_bounds__(256) void depth_emit_kernel(const unsigned long long *__restrict__ edge, const int *__restrict__ diff, const uint32_t *__restrict__ starts,
                                                         const DepthTile *__restrict__ tiles, uint32_t n_tiles, const long long *__restrict__ tile_off, uint32_t w,
                                                         unsigned long long *__restrict__ window_bases, uint32_t *__restrict__ window_starts,
                                                         unsigned long long *__restrict__ ref_sums) {
    const uint32_t lane = lane_id();
    const uint32_t t = rdfirst(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (t >= n_tiles) return;
    const DepthTile T = tiles[t];
    uint32_t running = (uint32_t)tile_off[t];  // (0 <= the true count < 2^31: the arithmetic mod 2^32 is exact)
    unsigned long long sum = 0, largest = 0;
    uint32_t zeros = 0;
    for (uint32_t j0 = 0; j0 < T.n_windows; j0 += 64u) {
        const bool in = j0 + lane < T.n_windows;
        const uint64_t g = T.first_window + j0 + lane;
        const uint32_t d = in ? (uint32_t)diff[g] : 0u;
        const uint32_t incl = wave_incl_scan_u32(d);  // (all 64 lanes: the trip count is wave-uniform)
        if (in) {
            const unsigned long long bases = (unsigned long long)(running + incl) * w + edge[g];
            window_bases[g] = bases;
            window_starts[g] = starts[g];
            sum += bases;
            zeros += bases == 0;
            largest = bases > largest ? bases : largest;
        }
        running += rdlane(incl, 63);
    }
    sum = depth_wave_sum_u64(sum);
    largest = depth_wave_max_u64(largest);
    zeros = wave_sum_u32(zeros);
    if (lane == 0) {
        if (sum) atomicAdd(&ref_sums[3 * T.ref], sum);
        if (zeros) atomicAdd(&ref_sums[3 * T.ref + 1], (unsigned long long)zeros);
        if (largest) atomicMax(&ref_sums[3 * T.ref + 2], largest);
    }
}
