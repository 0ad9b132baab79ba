// mq_fastx_lines.hpp -- FASTA records whose sequences run over several lines, found AND joined on the device (mq_ctx_submit_fastx with
// MQ_FASTX_FASTA_LINES; parse_chunk, host/fastx_records.hpp, does the same on a host thread with memmove: the reference reads such
// files through seq_io, src/closures.rs:100-123).  The piece is buf[begin, end), buf[begin] == '>'.
//   header start   a '>' at `begin` or directly behind a '\n'; a '>' anywhere else is an ordinary byte
//   header line    from a header start to the next '\n' (or to `end`); record r = header line r + everything up to the next header start
//   kept byte      a byte behind its record's header line that is not '\n' and not a '\r' whose next byte is '\n' or which is the piece's
//                  last byte: the record's sequence is its kept bytes, in order (empty lines contribute nothing)
// One bit of state runs through the piece: "inside a header line" -- a header start sets it, a '\n' clears it, the last event wins.
//   fl_count_kernel   per 16-KB tile (one wave per tile, 16-byte lane loads; the shape of mq_fastx.hpp / mq_join.hpp): header starts, the
//                     tile's effect on the state, kept bytes behind the tile's first event and -- counted apart, since they are kept only
//                     when the tile is entered outside a header line -- candidates in front of it
//   fl_scan_kernel    one workgroup, any number of tiles: the state entering each tile, exclusive sums of kept bytes and header starts,
//                     the result words
//   fl_write_kernel   every kept byte to joined[tile_off + rank] (store_kept16), hdr_begin[r] / offsets[r] at header start r, hdr_end[r] at
//                     the '\n' that closes header line r
//   fl_check_kernel   lens[r] = offsets[r + 1] - offsets[r]; a record without a sequence byte makes the piece IRREGULAR
// Nothing is serial in the number of bytes.  Byte work, HBM-stream bound: the piece is read twice and its sequence bytes written once.
#pragma once
#include "mq_blocks.hpp"  // FxJoined: the scan's result
#include "mq_join.hpp"    // store_kept16 and, through it, mq_fastx.hpp's tile helpers
#include "mq_wave.hpp"

namespace mq {

// What a lane knows of its 16 bytes at p0 (16-bit masks, bit b = byte p0 + b) before the state reaches it
struct FlLane {
    uint4 v;        // the bytes (zero when p0 >= end: nothing is loaded there)
    uint32_t hs;    // header starts
    uint32_t nl;    // '\n' inside [begin, end)
    uint32_t cand;  // bytes of [begin, end) that are kept when they lie outside a header line
};

// The byte in front of a lane's first byte comes from the lane below, the byte behind its last one from the lane above; lanes 0 and 63
// read theirs themselves.  All 64 lanes call this.
__device__ __forceinline__ FlLane fl_lane16(const uint8_t *__restrict__ buf, uint32_t p0, uint32_t begin, uint32_t end, uint32_t lane) {
    FlLane L;
    L.v = make_uint4(0, 0, 0, 0);
    const uint32_t valid = in_range16(p0, begin, end);
    uint32_t nl = 0, cr = 0, gt = 0;
    if (p0 < end) {
        L.v = *reinterpret_cast<const uint4 *>(buf + p0);
        nl = eq_bits16<'\n'>(L.v);
        cr = eq_bits16<'\r'>(L.v);
        gt = eq_bits16<'>'>(L.v);
    }
    // line starts: behind a '\n', and the piece's first byte
    uint32_t prev_nl = (uint32_t)__shfl_up((int)(nl >> 15), 1, 64);
    if (lane == 0u) prev_nl = (p0 > begin && p0 <= end) ? (buf[p0 - 1u] == '\n' ? 1u : 0u) : 0u;
    uint32_t ls = ((nl << 1) | prev_nl) & 0xFFFFu;
    if (begin >= p0 && begin - p0 < 16u) ls |= 1u << (begin - p0);
    // a '\r' goes when a '\n' follows it or nothing does
    const uint32_t nl_ext = nl | (~valid & 0xFFFFu);  // (behind the piece every byte counts as a line end)
    uint32_t next = (uint32_t)__shfl_down((int)(nl_ext & 1u), 1, 64);
    if (lane == 63u) next = p0 + 16u >= end ? 1u : (buf[p0 + 16u] == '\n' ? 1u : 0u);
    const uint32_t drop_cr = cr & ((nl_ext >> 1) | (next << 15));
    L.hs = gt & ls & valid;
    L.nl = nl & valid;
    L.cand = valid & ~(nl | drop_cr);
    return L;
}

// Bit b: byte b lies inside a header line (state behind the events at or below it), s_in = the state in front of byte 0.  A carry
// chain: a header start generates, a '\n' kills, every other byte propagates -- the carries of one addition.
__device__ __forceinline__ uint32_t fl_state16(uint32_t hs, uint32_t nl, uint32_t s_in) {
    const uint32_t a = ~nl & 0xFFFFu, b = hs;  // generate = a & b = hs, propagate = a | b = not '\n'
    return (((a + b + s_in) ^ a ^ b) >> 1) & 0xFFFFu;
}

// The state in front of each lane's first byte: two ballots and a find-MSB over the lanes below.  wave_in: the state in front of lane 0
// (wave-uniform).  below: whether an event lies in a lane below (else s_in is wave_in); wave_ev / wave_out: whether the 64 lanes hold an
// event at all and the state behind the last one.
struct FlWave {
    uint32_t s_in;
    bool below, wave_ev;
    uint32_t wave_out;
};
__device__ __forceinline__ FlWave fl_wave_state(const FlLane &L, uint32_t lane, uint32_t wave_in) {
    const uint32_t ev = L.hs | L.nl;
    const bool last_set = ev && ((L.hs >> (31u - (uint32_t)__clz((int)ev))) & 1u);
    const uint64_t E = __ballot(ev != 0u), S = __ballot(last_set);
    const uint64_t lower = E & ((1ull << lane) - 1ull);
    FlWave W;
    W.below = lower != 0ull;
    W.s_in = W.below ? (uint32_t)((S >> (63 - __clzll((long long)lower))) & 1ull) : wave_in;
    W.wave_ev = E != 0ull;
    W.wave_out = W.wave_ev ? (uint32_t)((S >> (63 - __clzll((long long)E))) & 1ull) : wave_in;
    return W;
}

constexpr uint32_t FL_EV_NONE = 0u, FL_EV_CLEAR = 2u, FL_EV_SET = 3u;  // a tile's effect on the state (bit 1: it has an event, bit 0: the state behind it)

// buf: 16-byte aligned, readable up to the next multiple of 16 behind `end`.  tile_counts[4 t ..]: kept bytes behind the tile's first
// event, candidates in front of it, header starts, effect.
__global__ __launch_bounds__(256) void fl_count_kernel(const uint8_t *__restrict__ buf, uint32_t begin, uint32_t end, uint32_t n_tiles,
                                                       uint32_t *__restrict__ tile_counts) {
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        uint32_t kept = 0, pre = 0, heads = 0;
        bool seen = false;  // an event earlier in this tile (wave-uniform)
        uint32_t st = 0;    // ... and the state behind it; in front of the first event the tile counts as entered outside a header line
        for (uint32_t it = 0; it < FX_TILE / 1024u; ++it) {
            const uint32_t q0 = t * FX_TILE + it * 1024u;
            if (q0 >= end) break;  // (the whole wave)
            const FlLane L = fl_lane16(buf, q0 + lane * 16u, begin, end, lane);
            const FlWave W = fl_wave_state(L, lane, st);
            const uint32_t out = L.cand & ~fl_state16(L.hs, L.nl, W.s_in);
            const uint32_t ev = L.hs | L.nl;
            const uint32_t front = (seen || W.below) ? 0u : (ev ? ((ev & (0u - ev)) - 1u) : 0xFFFFu);  // bytes in front of the tile's first event
            pre += (uint32_t)__popc(out & front);
            kept += (uint32_t)__popc(out & ~front);
            heads += (uint32_t)__popc(L.hs);
            seen = seen || W.wave_ev;
            st = W.wave_out;
        }
        kept = wave_sum_u32(kept);
        pre = wave_sum_u32(pre);
        heads = wave_sum_u32(heads);
        if (lane == 0) {
            tile_counts[4u * t] = kept;
            tile_counts[4u * t + 1u] = pre;
            tile_counts[4u * t + 2u] = heads;
            tile_counts[4u * t + 3u] = seen ? (FL_EV_CLEAR | st) : FL_EV_NONE;
        }
    }
}

// tile_off[3 t ..]: kept bytes in front of tile t, header starts in front of it, the state entering it.
// info: an FxJoined (mq_blocks.hpp) as 32-bit words.  offsets[records] = the joined length; hdr_end of a last record whose header
// line the piece ends in = end.  IRREGULAR (no record reported): the piece does not start with '>', or holds more records than span_cap.
__global__ __launch_bounds__(1024) void fl_scan_kernel(const uint8_t *__restrict__ buf, uint32_t begin, uint32_t end, const uint32_t *__restrict__ tile_counts,
                                                       uint32_t n_tiles, uint32_t *__restrict__ tile_off, unsigned long long *__restrict__ offsets,
                                                       uint32_t *__restrict__ hdr_end, uint32_t span_cap, uint32_t *__restrict__ info) {
    __shared__ uint32_t eff[1024];
    __shared__ uint2 part[1024];  // x: kept bytes, y: header starts
    const uint32_t t = threadIdx.x;
    uint32_t lo, hi;
    tile_span(n_tiles, lo, hi);
    // the state: last event wins, over this thread's tiles, then over the threads
    uint32_t mine = FL_EV_NONE;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t e = tile_counts[4u * i + 3u];
        if (e) mine = e;
    }
    // (FL_EV_NONE: no event in front of this thread's tiles -- outside a header line, as the piece begins)
    const uint32_t st_in = block_excl_scan_1024(eff, mine, [](uint32_t below, uint32_t own) { return own ? own : below; }) & 1u;
    // kept bytes and header starts of this thread's tiles, now that the state entering each is known
    const auto add = [](uint2 a, uint2 b) { return make_uint2(a.x + b.x, a.y + b.y); };
    const auto counted = [&](uint32_t i, uint32_t st) {  // tile i entered in state st
        return make_uint2(tile_counts[4u * i] + (st ? 0u : tile_counts[4u * i + 1u]), tile_counts[4u * i + 2u]);
    };
    uint32_t st = st_in;
    uint2 sum = make_uint2(0u, 0u);
    for (uint32_t i = lo; i < hi; ++i) {
        sum = add(sum, counted(i, st));
        const uint32_t e = tile_counts[4u * i + 3u];
        if (e) st = e & 1u;
    }
    uint2 run = block_excl_scan_1024(part, sum, add);
    st = st_in;
    for (uint32_t i = lo; i < hi; ++i) {
        tile_off[3u * i] = run.x;
        tile_off[3u * i + 1u] = run.y;
        tile_off[3u * i + 2u] = st;
        run = add(run, counted(i, st));
        const uint32_t e = tile_counts[4u * i + 3u];
        if (e) st = e & 1u;
    }
    if (t == 1023u) {
        const uint32_t n = part[1023].y, joined = part[1023].x;
        const bool bad = (end > begin && buf[begin] != '>') || n > span_cap;
        if (!bad) {
            offsets[n] = joined;
            if (n && (eff[1023] & 1u)) hdr_end[n - 1u] = end;  // the piece ends inside the last header line
        }
        info[MQ_WORD(FxJoined, records)] = bad ? 0u : n;
        info[MQ_WORD(FxJoined, joined)] = bad ? 0u : joined;
        info[MQ_WORD(FxJoined, flags)] = bad ? FX_IRREGULAR : 0u;
        info[MQ_WORD(FxJoined, spare)] = 0;
    }
}

// joined: room for every kept byte (at most end - begin), never buf; hdr_begin / hdr_end: span_cap entries, offsets: span_cap + 1
__global__ __launch_bounds__(256) void fl_write_kernel(const uint8_t *__restrict__ buf, uint32_t begin, uint32_t end, uint32_t n_tiles,
                                                       const uint32_t *__restrict__ tile_off, const uint32_t *__restrict__ info, uint8_t *__restrict__ joined,
                                                       uint32_t *__restrict__ hdr_begin, uint32_t *__restrict__ hdr_end, unsigned long long *__restrict__ offsets,
                                                       uint32_t span_cap) {
    if (info[MQ_WORD(FxJoined, flags)] & FX_IRREGULAR) return;  // decided by the scan already: nothing to write (and no record index beyond span_cap is ever formed)
    const uint32_t lane = lane_id();
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t t = wave; t < n_tiles; t += n_waves) {
        uint32_t at = tile_off[3u * t], rec = tile_off[3u * t + 1u], st = tile_off[3u * t + 2u];
        for (uint32_t it = 0; it < FX_TILE / 1024u; ++it) {
            const uint32_t q0 = t * FX_TILE + it * 1024u;
            if (q0 >= end) break;  // (the whole wave)
            const uint32_t p0 = q0 + lane * 16u;
            const FlLane L = fl_lane16(buf, p0, begin, end, lane);
            const FlWave W = fl_wave_state(L, lane, st);
            const uint32_t in_hdr = fl_state16(L.hs, L.nl, W.s_in);
            const uint32_t keep = L.cand & ~in_hdr;
            const uint32_t closes = L.nl & ((in_hdr << 1) | W.s_in);  // '\n' whose byte in front lies inside a header line
            const uint32_t mine = (uint32_t)__popc(keep), heads = (uint32_t)__popc(L.hs);
            const uint32_t incl = wave_incl_scan_u32(mine | (heads << 16));  // (at most 1,024 kept bytes and 512 header starts per iteration)
            const uint32_t my_at = at + (incl & 0xFFFFu) - mine, my_rec = rec + (incl >> 16) - heads;
            if (mine) store_kept16(joined + my_at, L.v, keep, mine);
            for (uint32_t m = L.hs; m; m &= m - 1u) {
                const uint32_t b = (uint32_t)__ffs((int)m) - 1u, below = (1u << b) - 1u;
                const uint32_t r = my_rec + (uint32_t)__popc(L.hs & below);
                if (r < span_cap) {
                    hdr_begin[r] = p0 + b;
                    offsets[r] = my_at + (uint32_t)__popc(keep & below);
                }
            }
            for (uint32_t m = closes; m; m &= m - 1u) {
                const uint32_t b = (uint32_t)__ffs((int)m) - 1u;
                const uint32_t r = my_rec + (uint32_t)__popc(L.hs & ((1u << b) - 1u)) - 1u;  // the header start in front of it
                if (r < span_cap) hdr_end[r] = p0 + b;
            }
            const uint32_t tot = rdlane(incl, 63);
            at += tot & 0xFFFFu;
            rec += tot >> 16;
            st = W.wave_out;
        }
    }
}

// lens[r]: the joined length of record r; a record without a sequence byte makes the piece IRREGULAR (the host parser gives such a
// record a reading of its own -- the line behind a header is sequence even when it starts with '>' -- which is not restated here)
__global__ __launch_bounds__(256) void fl_check_kernel(const unsigned long long *__restrict__ offsets, uint32_t *__restrict__ lens, uint32_t *__restrict__ info) {
    if (info[MQ_WORD(FxJoined, flags)] & FX_IRREGULAR) return;
    const uint32_t n_rec = info[MQ_WORD(FxJoined, records)];
    bool bad = false;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x) {
        const uint32_t len = (uint32_t)(offsets[r + 1u] - offsets[r]);
        lens[r] = len;
        if (len == 0u) bad = true;
    }
    if (__ballot(bad) && lane_id() == 0) atomicOr(&info[MQ_WORD(FxJoined, flags)], FX_IRREGULAR);
}

}  // namespace mq
