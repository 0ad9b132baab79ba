// mq_join.hpp -- the lines of one line-wrapped FASTA record joined in device memory (RefLoader::prepare, host/ref_loader.hpp, and
// fastx_records.hpp do the same on the host with memmove: the reference reads such records through seq_io, src/closures.rs:46-94).
// The region R = buf[begin, end) is everything between a header's line end and the next record's '>': it is split at every '\n', one
// trailing '\r' is cut from each piece (the last one, which has no '\n', included) and the pieces are concatenated.  Byte-wise: a byte
// is dropped when it is '\n', or when it is '\r' and the next byte of R is '\n' or there is no next byte; everything else is kept.
//   join_count_kernel   kept bytes per 16-KB tile (one wave per tile, 16-byte lane loads; the shape of mq_fastx.hpp)
//   join_scan_kernel    exclusive 64-bit scan of the tile counts (one workgroup); the total = the joined length
//   join_write_kernel   every kept byte to dst[tile_off + rank]: a lane closes the gaps of its 16 bytes in registers and stores what
//                       it keeps at its (unaligned) place -- 16 bytes at once for the 3 lanes in 4 that drop nothing at 60-80 columns
// Tiles start at `begin` rounded down to 16 (never in front of the allocation); loads run to the next multiple of 16 behind `end`.
// Byte work, HBM-stream bound: the region is read twice and written once.
#pragma once
#include "mq_fastx.hpp"  // the scanners' shared tile helpers
#include "mq_wave.hpp"

namespace mq {

// Bit b of the result: byte p0 + b is a kept byte of R.  v: the 16 bytes at p0 (zero when p0 >= end: nothing is loaded there).  The byte
// behind a lane's last one is the first byte of the lane above; the last lane reads that one byte itself.  All 64 lanes call this.
__device__ __forceinline__ uint32_t join_keep16(const uint8_t *__restrict__ buf, uint64_t p0, uint64_t begin, uint64_t end, uint32_t lane, uint4 &v) {
    uint32_t nl = 0xFFFFu, cr = 0;  // behind R every byte counts as a line end: a '\r' that is R's last byte goes
    v = make_uint4(0, 0, 0, 0);
    if (p0 < end) {
        v = *reinterpret_cast<const uint4 *>(buf + p0);
        nl = eq_bits16<'\n'>(v) | (~below16(p0, end) & 0xFFFFu);
        cr = eq_bits16<'\r'>(v);
    }
    uint32_t next = (uint32_t)__shfl_down((int)(nl & 1u), 1, 64);
    if (lane == 63u) next = p0 + 16u >= end ? 1u : (buf[p0 + 16u] == '\n' ? 1u : 0u);
    return ~(nl | (cr & ((nl >> 1) | (next << 15)))) & ~below16(p0, begin) & 0xFFFFu;
}

// buf: 16-byte aligned, readable up to the next multiple of 16 behind `end`; tile t = 16 KB from (begin & ~15) + t * FX_TILE
__global__ __launch_bounds__(256) void join_count_kernel(const uint8_t *__restrict__ buf, uint64_t begin, uint64_t end, uint32_t n_tiles,
                                                         uint32_t *__restrict__ tile_counts) {
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        const uint64_t t0 = (begin & ~15ull) + (uint64_t)t * FX_TILE;
        uint32_t c = 0;
#pragma unroll 4
        for (uint32_t it = 0; it < FX_TILE / 1024u; ++it) {
            uint4 v;
            c += (uint32_t)__popc(join_keep16(buf, t0 + it * 1024u + lane * 16u, begin, end, lane, v));
        }
        c = wave_sum_u32(c);
        if (lane == 0) tile_counts[t] = c;
    }
}

// tile_off[t] = kept bytes in front of tile t; *total = the joined length (written the way scan_tiles_kernel is, on 64 bits)
__global__ __launch_bounds__(1024) void join_scan_kernel(const uint32_t *__restrict__ tile_counts, uint32_t n_tiles, unsigned long long *__restrict__ tile_off,
                                                         unsigned long long *__restrict__ total) {
    __shared__ unsigned long long part[1024];
    uint32_t lo, hi;
    unsigned long long sum = 0;
    tile_span(n_tiles, lo, hi);
    for (uint32_t i = lo; i < hi; ++i) sum += tile_counts[i];
    unsigned long long run = block_excl_scan_1024(part, sum);
    for (uint32_t i = lo; i < hi; ++i) {
        tile_off[i] = run;
        run += tile_counts[i];
    }
    if (threadIdx.x == 1023u) *total = part[1023];
}

// 16 / 8 / 4 / 2 bytes to d, d of any alignment (one store each: the target takes unaligned global accesses)
__device__ __forceinline__ void store_u128(uint8_t *d, uint64_t lo, uint64_t hi) {
    struct __attribute__((packed, aligned(1))) U128 {
        uint64_t lo, hi;
    };
    U128 x{lo, hi};
    __builtin_memcpy(d, &x, 16);
}
__device__ __forceinline__ void store_u64(uint8_t *d, uint64_t x) { __builtin_memcpy(d, &x, 8); }
__device__ __forceinline__ void store_u32(uint8_t *d, uint32_t x) { __builtin_memcpy(d, &x, 4); }
__device__ __forceinline__ void store_u16(uint8_t *d, uint16_t x) { __builtin_memcpy(d, &x, 2); }

// The kept bytes (mask `keep`, `mine` of them, at least one) of the 16 bytes v to d: the gaps are closed in registers, then 16 / 8 / 4 / 2 /
// 1-byte stores at the (unaligned) place -- 16 bytes at once for the 3 lanes in 4 that drop nothing at 60-80 columns
__device__ __forceinline__ void store_kept16(uint8_t *d, const uint4 v, uint32_t keep, uint32_t mine) {
    uint64_t lo = ((uint64_t)v.y << 32) | v.x, hi = ((uint64_t)v.w << 32) | v.z;
    // the dropped bytes below the highest kept one go, highest first: what lies above each moves down by a byte
    uint32_t drop = ~keep & ((2u << (31u - (uint32_t)__clz((int)keep))) - 1u);
    while (drop) {
        const uint32_t b = 31u - (uint32_t)__clz((int)drop);
        drop ^= 1u << b;
        if (b < 8u) {
            const uint64_t below = (1ull << (8u * b)) - 1ull;
            lo = (lo & below) | (((lo >> 8) | (hi << 56)) & ~below);
            hi >>= 8;
        } else {
            const uint64_t below = (1ull << (8u * (b - 8u))) - 1ull;
            hi = (hi & below) | ((hi >> 8) & ~below);
        }
    }
    if (mine == 16u) {
        store_u128(d, lo, hi);
        return;
    }
    if (mine & 8u) {
        store_u64(d, lo);
        d += 8;
        lo = hi;
    }
    if (mine & 4u) {
        store_u32(d, (uint32_t)lo);
        d += 4;
        lo >>= 32;
    }
    if (mine & 2u) {
        store_u16(d, (uint16_t)lo);
        d += 2;
        lo >>= 16;
    }
    if (mine & 1u) *d = (uint8_t)lo;
}

// dst: room for every kept byte (at most end - begin); never the buffer that is read: tiles of one launch would race
__global__ __launch_bounds__(256) void join_write_kernel(const uint8_t *__restrict__ buf, uint64_t begin, uint64_t end, uint32_t n_tiles,
                                                         const unsigned long long *__restrict__ tile_off, uint8_t *__restrict__ dst) {
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        const uint64_t t0 = (begin & ~15ull) + (uint64_t)t * FX_TILE;
        uint64_t at = tile_off[t];
        for (uint32_t it = 0; it < FX_TILE / 1024u; ++it) {
            if (t0 + it * 1024u >= end) break;  // (the whole wave)
            uint4 v;
            const uint32_t keep = join_keep16(buf, t0 + it * 1024u + lane * 16u, begin, end, lane, v);
            const uint32_t mine = (uint32_t)__popc(keep);
            const uint32_t incl = wave_incl_scan_u32(mine);
            if (mine) store_kept16(dst + at + (incl - mine), v, keep, mine);
            at += rdlane(incl, 63);
        }
    }
}

}  // namespace mq
