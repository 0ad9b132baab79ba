// mq_redo.hpp -- the overflow redo of a device-resident batch, on the device and in stream (mq_ctx_reserve_redo): three small kernels around
// an ordinary launch sequence over the context's redo arena.  Needs nothing of the mapper but the hit record.
//   redo_collect_kernel   one lane per read of the batch: the reads that came back MQ_HIT_OVERFLOW claim the arena's slots
//   redo_copy_kernel      one wave per slot: the read's bytes from the caller's buffer to the slot
//   (the launch sequence of launch_map, spans form, over the slots: worst-case list regions and Match windows, hits to the arena's own array)
//   redo_scatter_kernel   one lane per slot: the slot's hit to the read's place in the caller's array
// Slot j is bytes [j * stride, j * stride + max_read_len) of the arena; a slot nobody claimed is a read of length 0 (MQ_HIT_UNMAPPED at once:
// shorter than l + k - 1) that nothing scatters.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mapquik_hip.h"
#include "mq_blocks.hpp"
#include "mq_wave.hpp"

namespace mq {

constexpr uint32_t REDO_COPY_WAVES = 4;  // slots per workgroup of redo_copy_kernel

// Read r of the batch is bases[offsets[r], offsets[r + 1]).  An overflow read of at most max_read_len bytes takes the next slot: one ballot
// and one atomic per wave (every lane of the workgroup stays to the end: no lane leaves in front of the ballots).  The order of the slots
// is the order in which the waves arrive, not the reads'.
__global__ __launch_bounds__(256) void redo_collect_kernel(const mq_hit *__restrict__ out, const uint64_t *__restrict__ offsets, uint32_t n, uint32_t max_reads,
                                                           uint32_t max_read_len, RedoCounters *__restrict__ counters, uint32_t *__restrict__ ids,
                                                           uint64_t *__restrict__ src, uint32_t *__restrict__ lens) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = lane_id();
    bool over = false;
    uint64_t o0 = 0, len = 0;
    if (r < n && out[r].status == MQ_HIT_OVERFLOW) {
        over = true;
        o0 = offsets[r];
        len = offsets[r + 1] - o0;
    }
    const bool wants = over && len <= (uint64_t)max_read_len;
    const uint64_t m = __ballot(wants);
    uint32_t first = 0;
    if (m) {  // (wave-uniform)
        if (lane == 0) first = atomicAdd(&counters->claimed, (uint32_t)__popcll(m));
        first = rdfirst(first);
    }
    const uint32_t slot = first + mbcnt64(m);
    const bool has_slot = wants && slot < max_reads;
    if (has_slot) {
        ids[slot] = r;
        src[slot] = o0;
        lens[slot] = (uint32_t)len;
    }
    const uint64_t stay = __ballot(over && !has_slot);  // longer than a slot, or every slot taken: the record keeps its status
    if (stay && lane == 0) atomicAdd(&counters->left, (uint32_t)__popcll(stay));
}

// Slot j's bytes: 16 per lane per step, loaded from wherever the read begins (any address) and stored to the slot (a multiple of 64).  Every
// load lies inside [src[j], src[j] + lens[j]): whole 16-byte pieces first, the last len % 16 bytes one per lane -- the caller's buffer may
// end at the read's last byte.
typedef uint4 __attribute__((aligned(1))) redo_u4_any;
__global__ __launch_bounds__(64 * REDO_COPY_WAVES) void redo_copy_kernel(const uint8_t *__restrict__ bases, const uint64_t *__restrict__ src,
                                                                         const uint32_t *__restrict__ lens, uint32_t max_reads, uint8_t *__restrict__ arena,
                                                                         uint64_t stride) {
    const uint32_t j = blockIdx.x * REDO_COPY_WAVES + rdfirst(threadIdx.x >> 6);
    if (j >= max_reads) return;
    const uint32_t len = lens[j];
    if (len == 0) return;  // nobody claimed the slot
    const uint32_t lane = lane_id();
    const uint8_t *s = bases + src[j];
    uint8_t *d = arena + (uint64_t)j * stride;
    const uint64_t whole = len & ~15u;
    for (uint64_t at = 16u * lane; at < whole; at += 16u * 64u) *reinterpret_cast<uint4 *>(d + at) = *reinterpret_cast<const redo_u4_any *>(s + at);
    const uint64_t t = whole + lane;
    if (t < len) d[t] = s[t];
}

// The hits of the slots that were claimed, each to its read's record: all 48 bytes
__global__ __launch_bounds__(256) void redo_scatter_kernel(const mq_hit *__restrict__ arena_hits, const uint32_t *__restrict__ ids,
                                                           const RedoCounters *__restrict__ counters, uint32_t max_reads, mq_hit *__restrict__ out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const uint32_t redone = counters->claimed < max_reads ? counters->claimed : max_reads;
    if (j < redone) out[ids[j]] = arena_hits[j];
}

}  // namespace mq
