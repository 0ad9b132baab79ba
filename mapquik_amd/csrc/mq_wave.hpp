// mq_wave.hpp -- what one wavefront (64 lanes) does with itself: the LDS hand-off between its lanes, lane id, cross-lane reads, DPP scans
// and reductions, 64-bit rotations, the L2-served loads of the map phase, and the stage clocks of the diagnostic builds.  Needs nothing
// of the mapper: the record scanners (mq_fastx.hpp, mq_join.hpp, mq_fastx_lines.hpp) include this part alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mq_blocks.hpp"

namespace mq {

// ------------------------------------------------------------------ wave helpers
// LDS hand-off between lanes of ONE wave (waves of a workgroup work on different reads and never rendezvous):
// LDS operations of a wave execute in order; this only stops the compiler from moving them across the point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// The empty asm makes every call site compute its own copy: with a pure lane id the compiler hoists every lane-dependent address
// and mask of EVERY phase out of the persistent per-read loop and keeps them all live (161 VGPRs for the fused kernel, 112 with this).
__device__ __forceinline__ uint32_t lane_id() {
    uint32_t x = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(x));
    return x;
}
// Diagnostic builds only (-DMQ_STAGE_CLOCKS): wave time per stage.  mq_clk(i) charges the cycles since the wave's previous stamp
// to stage i; map_kernel adds every wave's totals to MapCounters::clk (mq_blocks.hpp, MQ_N_CLK of them) at its end (read back by
// mq_last_stage_clocks).
//   0 stage A  1 stage B  2 stage R  3 tile carry  4 list stores acknowledged  5 list -> LDS  6 tuple hashes + probe issue
//   7 probe resolve + runs  8 runs finished, Match records in L2  9 chain + result  10 general seeder  11 next read (atomic, offsets)
//   with -DMQ_STAGE_A_SPLIT stage A's time is charged to: 10 / 13 what precedes the super-row loop in a sequence's first / later
//   tiles; 0 / 14 the wait for the bases of the first super-row of a first / later tile; 12 that wait for the other super-rows;
//   15 the work (decode, look-ups, scan, stream) -- three more stamps per super-row, so only for looking inside stage A
//   with -DMQ_STAGE_MAP_SPLIT stage 7 is split: 12 home buckets' keys arrived and compared, payloads requested; 13 lookups that walk on;
//   14 payloads arrived; 7 the runs
#ifdef MQ_STAGE_CLOCKS
struct StageClkLds {
    unsigned long long acc[16][MQ_N_CLK];  // a workgroup has at most 16 waves (1,024 threads)
    unsigned long long last[16];
};
__device__ __forceinline__ StageClkLds &mq_clk_lds() {
    __shared__ StageClkLds C;
    return C;
}
__device__ __forceinline__ void mq_clk(int i) {
    StageClkLds &C = mq_clk_lds();
    const uint32_t w = threadIdx.x >> 6;
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63u) == 0) {
        if (i >= 0) C.acc[w][i] += now - C.last[w];
        C.last[w] = now;
    }
}
#elif defined(MQ_CODE_MARKS)
// Diagnostic build (tools/code_sizes.sh, never loaded): every stage stamp becomes a symbol in the code object -- mq_mark_<stage>_<n> -- so that
// llvm-readelf can say how many bytes of map_kernel lie between two stamps (which stage owns how much of the instruction cache's 64 KB).
__device__ __forceinline__ void mq_clk(int i) { asm volatile("mq_mark_%c0_%=:" ::"n"(i + 1)); }
#else
__device__ __forceinline__ void mq_clk(int) {}
#endif
__device__ __forceinline__ uint32_t mbcnt64(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
__device__ __forceinline__ uint32_t rdlane(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }
__device__ __forceinline__ uint64_t rdlane64(uint64_t v, int l) {
    return ((uint64_t)rdlane((uint32_t)(v >> 32), l) << 32) | rdlane((uint32_t)v, l);
}
__device__ __forceinline__ uint32_t rdfirst(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
    uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int d) {
    uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t rotl64(uint64_t x, uint32_t r) { return __builtin_rotateleft64(x, (uint64_t)(r & 63u)); }
__device__ __forceinline__ uint64_t rotr64(uint64_t x, uint32_t r) { return __builtin_rotateright64(x, (uint64_t)(r & 63u)); }
// Wave reductions on the DPP network (row_shr inside each row of 16, then row_bcast:15 / row_bcast:31 across rows): VALU-rate
// moves, where __shfl_xor would go through ds_bpermute (~24 cycles of issue each, profiles/r02_valu_issue.txt).  Lanes that
// a shift leaves without a source read `old` = the operation's identity.  All 64 lanes must be active.
__device__ __forceinline__ uint32_t wave_incl_scan_u32(uint32_t x) {
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { return rdlane(wave_incl_scan_u32(v), 63); }
// the same scan with XOR (the general seeder's prefix of rotated seeds), on the two halves of a 64-bit word
__device__ __forceinline__ uint32_t wave_incl_xor_scan_u32(uint32_t x) {
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    x ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ uint64_t wave_incl_xor_scan_u64(uint64_t v) {
    return ((uint64_t)wave_incl_xor_scan_u32((uint32_t)(v >> 32)) << 32) | wave_incl_xor_scan_u32((uint32_t)v);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x) {
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false));
    x = mx(x, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false));
    return rdlane(x, 63);
}

// the map phase's loads of the list its own wave wrote in the seed phase
__device__ __forceinline__ uint64_t ld_sc1_u64(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // L2-served: never a stale L1 line
}
__device__ __forceinline__ uint32_t ld_sc1_u32(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

}  // namespace mq
