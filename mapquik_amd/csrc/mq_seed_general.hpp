// mq_seed_general.hpp -- the GENERAL streaming seeder: any bytes, any length (what the fast seeder of mq_seed.hpp declines, and the
// windows around its clean stretches), and its sink that writes lists.
// Structure (lanes = consecutive positions): mq_device.hpp's head comment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mq_device.hpp"
#include "mq_hash.hpp"
#include "mq_wave.hpp"

namespace mq {

constexpr int RING = 512;    // HPC ring entries kept per wave: l - 1 <= 63 behind the block being hashed + 63 waiting + one write group of the walk (<= 256)
constexpr int MZ_CAP = 160;  // < (64 + k - 1) carried + 64 appended, k <= 32

// Per-wave LDS of the general streaming seeder
struct WaveLds {
    unsigned long long mz_hash[MZ_CAP];
    uint32_t mz_pos[MZ_CAP];
    uint32_t mz_last[MZ_CAP];  // variant 16 only: raw position of the window's last compressed base
    uint32_t ring_pos[RING];
    uint8_t ring_code[RING];
};

// ------------------------------------------------------------------ streaming seeder
// Emits, in order, every minimizer whose l-mer starts at a homopolymer-run head with raw index in [a, b).
// Sink interface: void on_minimizers(WaveLds&, uint32_t &mz_count)  (called after each block, wave-uniform)
// 16 bytes at `at` of a sequence of len bytes (those at or behind len read as 0); n = how many of them are inside
__device__ __forceinline__ uint4 load16_tail(const uint8_t *__restrict__ seq, uint64_t len, uint64_t at, uint32_t &n) {
    typedef uint4 __attribute__((aligned(1))) uint4_u;
    if (at + 16u <= len) {
        n = 16u;
        return *reinterpret_cast<const uint4_u *>(seq + at);
    }
    n = at < len ? (uint32_t)(len - at) : 0u;
    uint64_t lo = 0, hi = 0;  // (the sequence's last piece only; no array: a dynamically indexed one lives in scratch memory)
    for (uint32_t j = 0; j < n; ++j) {
        const uint64_t b = seq[at + j];
        if (j < 8u) lo |= b << (8u * j);
        else hi |= b << (8u * (j - 8u));
    }
    return make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
}
// first position >= from whose byte differs from v (compared as the general seeder compares: a-z as A-Z when folding), or len; 4 KB a step
__device__ __forceinline__ uint64_t next_byte_differing(const uint8_t *__restrict__ seq, uint64_t len, uint64_t from, uint32_t v, bool fold) {
    const uint32_t lane = lane_id();
    const uint32_t m8 = (fold && v - 'A' < 26u) ? 0xDFu : 0xFFu;  // v is what a byte folds TO: a letter matches its lower case too
    const uint32_t mm = m8 * 0x01010101u, vv = (v & 0xFFu) * 0x01010101u;
    if (v > 0xFFu) return from;  // no byte at all (the sequence's start)
    for (uint64_t p = from; p < len; p += 4096u) {
        const uint64_t at = p + 64u * lane;
        uint32_t first = 64u;  // index of the lane's first differing byte
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            uint32_t n;
            const uint4 q = load16_tail(seq, len, at + 16u * (uint32_t)j, n);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 3; i >= 0; --i) {
                const uint32_t d = (w[i] & mm) ^ vv;
                if (d) {
                    const uint32_t k = 16u * (uint32_t)j + 4u * (uint32_t)i + ((uint32_t)__ffs((int)d) - 1u) / 8u;
                    if (k < 16u * (uint32_t)j + n) first = k;  // (bytes behind len read as 0: not a difference)
                }
            }
        }
        const uint64_t m = __ballot(first < 64u);
        if (m) {
            const int l0 = __ffsll((long long)m) - 1;
            return p + 64u * (uint32_t)l0 + rdlane(first, l0);
        }
    }
    return len;
}
// min_last > 0: only windows whose LAST compressed base lies at or behind raw position min_last (seed_read_hybrid: the windows that lie
// wholly in front of it were listed by the fast seeder)
template <bool VAR = true, class Sink>
__device__ __forceinline__ void seed_segment(const uint8_t *__restrict__ seq, uint64_t len, uint64_t a, uint64_t b,
                                             const DevParams &P, WaveLds &S, Sink &sink, uint32_t &mz_count, uint64_t min_last = 0) {
    const uint32_t lane = lane_id();
    const uint32_t l = P.l;
    if (a >= len || a >= b) return;
    uint32_t hbase = 0, hproc = 0;  // HPC positions seen / folded into the scan (segment-local, wave-uniform)
    uint32_t s_elig = 0;            // heads with raw index < b
    uint64_t prevF = 0, prevR = 0;  // per-lane inclusive prefixes of the previous block
    uint64_t carryF = 0, carryR = 0;
    uint32_t prev_byte = a > 0 ? (uint32_t)seq[a - 1] : 0x100u;
    if (P.fold && prev_byte - 'a' < 26u) prev_byte -= 32u;
    // lane constants
    const uint32_t from = (lane - l) & 63u;
    const bool src_cur = lane + l <= 63u;
    const uint32_t rot_r = (lane - l + 1u) & 63u;
    const bool h32 = var_h32<VAR>(P), pos_end = var_pos_end<VAR>(P), with_last = var_end_compressed<VAR>(P);  // seeding variants (wave-uniform)

    auto process_block = [&](uint32_t nvalid) {
        const uint32_t idx = hproc + lane;
        const bool valid = lane < nvalid;
        const uint32_t code = valid ? (uint32_t)S.ring_code[idx & (RING - 1)] : 4u;
        uint64_t tf = rotr64(nt_seed(code, h32), lane);
        uint64_t tr = rotl64(nt_seed(comp_code(code), h32), lane);
        tf = wave_incl_xor_scan_u64(tf);  // DPP row shifts and broadcasts (as ds_bpermute steps each of the six was an LDS round trip)
        tr = wave_incl_xor_scan_u64(tr);
        tf ^= carryF;
        tr ^= carryR;
        const uint64_t of = shfl64(src_cur ? tf : prevF, (int)from);
        const uint64_t orr = shfl64(src_cur ? tr : prevR, (int)from);
        const uint64_t fh = rotl64(tf ^ of, lane);
        const uint64_t rh = rotr64(tr ^ orr, rot_r);
        const uint64_t h = fh < rh ? fh : rh;
        const uint32_t j = idx - (l - 1u);  // HPC index of the window's first base
        const bool sel = valid && idx >= l - 1u && j < s_elig && h <= P.bound && !var_keep_none<VAR>(P) &&
                         (min_last == 0 || (uint64_t)S.ring_pos[idx & (RING - 1)] >= min_last);
        const uint64_t sm = __ballot(sel);
        if (sel) {
            const uint32_t o = mz_count + mbcnt64(sm);
            S.mz_hash[o] = list_hash<VAR>(P, h);
            // variant 8: the last base of the first base's run = the base in front of the next run head (l >= 2: inside the window)
            S.mz_pos[o] = pos_end ? S.ring_pos[(j + 1u) & (RING - 1)] - 1u : S.ring_pos[j & (RING - 1)];
            if (with_last) S.mz_last[o] = S.ring_pos[idx & (RING - 1)];  // variant 16: the window's last compressed base
        }
        mz_count += (uint32_t)__popcll(sm);
        prevF = tf;
        prevR = tr;
        carryF = rdlane64(tf, 63);
        carryR = rdlane64(tr, 63);
        wave_sync();
        sink.on_minimizers(S, mz_count);
    };

    // The walk: 1 KB per step, 16 bytes per lane.  What it looks for are run heads (a byte that differs from the byte in front of it; every byte
    // without HPC) -- the hashing above is per 64 HEADS, not per 64 bytes.  Sequences that come here are what the fast seeder declined: gaps of
    // the reference (N by the ten thousand), reads drawn from inside one (N with a sequencing error every ~140 bytes: two heads per error), the
    // neighbourhood of a stray byte in otherwise clean sequence.  A lane compares its 16 bytes with the same bytes shifted by one (SWAR,
    // exact non-zero-byte mask), the heads' places in the ring come from one wave scan, and each lane writes its own heads, lowest first.
    // (Round 5 walked 64 bytes per step, one per lane: 375 steps for a 24-kb read from inside a gap against 24, each with its ballots, its
    // scalar bookkeeping and a memory round trip: such a read cost 4-5 x an ordinary read, 0.7 % of the maize-like batch.)
    constexpr int AHEAD = 2;  // steps in flight behind the current one
    auto load16 = [&](uint64_t at) -> uint4 {
        uint32_t n;
        return load16_tail(seq, len, at, n);
    };
    uint4 nb[AHEAD + 1];
#pragma unroll
    for (int j = 0; j <= AHEAD; ++j) nb[j] = load16(a + 1024u * (uint32_t)j + 16u * lane);
    for (uint64_t pos = a;; pos += 1024) {
        const uint64_t at = pos + 16u * lane;
        uint4 v = nb[0];
#pragma unroll
        for (int j = 0; j < AHEAD; ++j) nb[j] = nb[j + 1];
        nb[AHEAD] = load16(at + 1024u * (uint32_t)(AHEAD + 1));
        const uint32_t nin = at < len ? (len - at < 16u ? (uint32_t)(len - at) : 16u) : 0u;  // bytes of this lane inside the sequence
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (P.fold) {  // a-z -> A-Z, byte-wise: 0x20 in every byte of 0x61..0x7A (no carry leaves a byte: the tests run on the low seven bits)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t t = w[i] & 0x7F7F7F7Fu;
                w[i] ^= (((t + 0x1F1F1F1Fu) & ~(t + 0x05050505u) & ~w[i]) & 0x80808080u) >> 2;
            }
        }
        // the byte in front of the lane's first: the previous lane's last (DPP wave_shr:1; lane 0 keeps `old` = the byte in front of the step)
        const uint32_t pl = (uint32_t)__builtin_amdgcn_update_dpp((int)(prev_byte & 0xFFu), (int)(w[3] >> 24), 0x138, 0xf, 0xf, false);
        uint32_t hm = 0xFFFFu;  // bit j: byte j is a run head
        if (P.use_hpc) {
            const uint32_t sh[4] = {(w[0] << 8) | pl, __builtin_amdgcn_alignbyte(w[1], w[0], 3), __builtin_amdgcn_alignbyte(w[2], w[1], 3),
                                    __builtin_amdgcn_alignbyte(w[3], w[2], 3)};
            hm = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t d = w[i] ^ sh[i];
                const uint32_t nz = ((((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u) >> 7;  // 1 in every byte that differs from the byte in front of it
                hm |= ((nz * 0x01020408u) >> 24 & 0xFu) << (4 * i);                             // those four bits side by side (no two partial products meet)
            }
            if (prev_byte > 0xFFu && at == 0) hm |= 1u;  // the sequence's first byte has nothing in front of it: a head whatever it is
        }
        hm &= nin >= 16u ? 0xFFFFu : ((1u << nin) - 1u);
        const uint32_t cnt = (uint32_t)__popc(hm);
        // heads with raw index < b (the windows that START there are this segment's)
        const uint32_t eb = at >= b ? 0u : (b - at >= 16u ? 0xFFFFu : ((1u << (uint32_t)(b - at)) - 1u));
        const uint32_t incl2 = wave_incl_scan_u32(cnt | ((uint32_t)__popc(hm & eb) << 16));  // both counts in one scan (<= 1024 each)
        const uint32_t tot2 = rdlane(incl2, 63);
        const uint32_t total = tot2 & 0xFFFFu;
        s_elig += tot2 >> 16;
        const uint32_t excl = (incl2 & 0xFFFFu) - cnt;
        const bool full = pos + 1024u <= len;
        const uint32_t last_byte = rdlane(w[3] >> 24, 63);  // (used only when the step lies inside the sequence)
        // the heads go into the ring in groups the ring has room for: all at once unless the step is dense (then 16 lanes = 256 bytes at a time)
        const uint32_t ngrp = total <= 256u ? 1u : 4u, glanes = 64u / ngrp;
        const uint32_t hb0 = hbase;  // the step's first head goes here
        for (uint32_t gi = 0; gi < ngrp; ++gi) {
            const bool mine = lane / glanes == gi;
            uint32_t m = mine ? hm : 0u;
            uint32_t o = hb0 + excl;
            while (__ballot(m != 0u)) {
                if (m) {
                    const uint32_t bit = (uint32_t)__ffs((int)m) - 1u;
                    const uint32_t wd = bit < 8u ? (bit < 4u ? w[0] : w[1]) : (bit < 12u ? w[2] : w[3]);
                    const uint32_t bt = (wd >> (8u * (bit & 3u))) & 0xFFu;
                    S.ring_code[o & (RING - 1)] = (uint8_t)base_code(bt);
                    S.ring_pos[o & (RING - 1)] = (uint32_t)(at + bit);
                    ++o;
                    m &= m - 1u;
                }
            }
            hbase += ngrp == 1u ? total : (rdlane(incl2, (int)(glanes * (gi + 1u) - 1u)) & 0xFFFFu) - (gi ? (rdlane(incl2, (int)(glanes * gi - 1u)) & 0xFFFFu) : 0u);
            wave_sync();
            while (hbase - hproc >= 64u) {
                process_block(64u);
                hproc += 64u;
            }
        }
        prev_byte = last_byte;
        if (P.use_hpc && total == 0u && full && pos + 2048u <= len) {
            // 1 KB that repeats the byte in front of it (a gap of the reference: tens of thousands of N; a very long homopolymer run): jump to the
            // KB that holds the next different byte -- nothing in between is a run head (bytes are compared as the walk compares them: folded)
            const uint64_t q = next_byte_differing(seq, len, pos + 1024u, prev_byte, P.fold != 0);
            const uint64_t skip = ((q - (pos + 1024u)) >> 10) << 10;
            if (skip) {
                pos += skip;
#pragma unroll
                for (int j = 0; j <= AHEAD; ++j) nb[j] = load16(pos + 1024u * (uint32_t)(j + 1) + 16u * lane);
            }
        }
        const bool end_of_seq = pos + 1024 >= len;
        // behind b: done once the last eligible window is complete -- or at once when no run head lies in [a, b) at all (a segment inside
        // a long homopolymer run has nothing to seed; without this it would read on to the end of the run, however far that is)
        const bool past = (pos + 1024 >= b) && (s_elig == 0u || hbase >= s_elig + l - 1u);
        if (end_of_seq || past) break;
    }
    if (hbase > hproc) process_block(hbase - hproc);
}

// sink of the general seeder when it writes lists: ordered minimizers to an SoA list region (hash[], pos[]) -- the split
// pipeline's reads and the reference segments the fast seeder declined
struct SoaListSink {
    unsigned long long *__restrict__ out_hash;
    uint32_t *__restrict__ out_pos;
    uint32_t *__restrict__ out_last;  // variant 16 only (else nullptr): the second position of every minimizer
    uint32_t cap;
    uint32_t written = 0;  // may exceed cap (the map stage then reports the read as overflowed)
    __device__ SoaListSink(unsigned long long *h, uint32_t *p, uint32_t *q, uint32_t c) : out_hash(h), out_pos(p), out_last(q), cap(c) {}
    __device__ __forceinline__ void on_minimizers(WaveLds &S, uint32_t &mz_count) {
        const uint32_t lane = lane_id();
        for (uint32_t base = 0; base < mz_count; base += 64u) {
            const uint32_t i = base + lane;
            if (i < mz_count && written + i < cap) {
                out_hash[written + i] = S.mz_hash[i];
                out_pos[written + i] = S.mz_pos[i];
                if (out_last) out_last[written + i] = S.mz_last[i];
            }
        }
        written += mz_count;
        mz_count = 0;
        wave_sync();
    }
};

}  // namespace mq
