// mq_blocks.hpp -- the small blocks of device memory that kernels and host code BOTH address: one type per block, defined here once.
// A kernel that takes the block's type (through MapArgs / RefSeedArgs) names the fields; a kernel whose parameter is a plain word pointer
// indexes it with MQ_WORD / MQ_WORD64 of a field; the host allocates one element, clears sizeof of it and copies fields by offsetof and
// sizeof.  The positions are part of no ABI, but the kernels' code is compared instruction by instruction across changes: the
// static_asserts below say where everything has always been.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mapquik_hip.h"

namespace mq {

// index of a 32-bit / 64-bit field in its block seen as an array of such words
#define MQ_WORD(Type, field) (offsetof(Type, field) / sizeof(uint32_t))
#define MQ_WORD64(Type, field) (offsetof(Type, field) / sizeof(unsigned long long))

constexpr int MQ_N_CLK = 16;  // stage clocks of a -DMQ_STAGE_CLOCKS build (the stages: mq_wave.hpp, mq_clk)

// ------------------------------------------------------------------ a map launch sequence (mq_ctx::d_counter = MapArgs::counters)
// two 64-bit statistics of an instrumented launch (mq_map_probe_stats); MapArgs::stats64 points at MapCounters::probe
struct ProbeStats {
    unsigned long long steps;    // slots visited beyond the home slot
    unsigned long long lookups;  // index lookups
};
// The chains output of a launch (mq_ctx_reserve_chains): what the CHN instantiations of the map kernels need beyond MapArgs.  It rides in
// the launch sequence's counter block, in what used to be spare words, so that MapArgs -- the kernel arguments of EVERY instantiation -- stays
// the size it was.  Written by the host behind the block's clearing, in stream order; all zero for a launch without the output.
struct ChainRec;
struct PoolCounters;
using ChainCounters = PoolCounters;
struct ChainLaunch {
    mq_chain *pool;
    uint32_t cap;      // entries of the pool
    uint32_t win_cap;  // records of a wave's chain window: at least the launch's Match window AND the records the LDS path chains (MAP_LDS_RECS)
    ChainCounters *counters;  // the BATCH's block (below): not cleared per launch
    ChainRec *windows; // per mapping wave: win_cap records, beside the wave's Match window (never IN it: pass C of the anchors reads that again)
    mq_chain_span *spans;     // read r's span goes to spans[ids ? ids[r] : r], as the anchors' does
    const uint32_t *ids;
};
// cleared by the host in front of every launch sequence
struct MapCounters {
    uint32_t seed_work;      // work cursor: map_kernel's items behind every wave's own two; seed_reads_kernel's reads (split)
    uint32_t map_work;       // work cursor of map_lists_kernel (split)
    uint32_t queue_len;      // reads the fast seeder declined (MapArgs::queue)
    uint32_t declined_work;  // work cursor over that queue: map_declined_kernel, seed_general_kernel (split)
    uint32_t n_fast;         // reads seeded by the fast seeder
    uint32_t n_general;      // reads it declined
    uint32_t n_moved;        // lists written again into a pool region
    uint32_t n_flagged;      // order_reads_kernel: reads that go first (may exceed WORK_FRONT_CAP)
    ProbeStats probe;        // instrumented launch only
    unsigned long long pool_cursor;  // entries of the pool handed out (pool_take)
    unsigned long long spare0;
    unsigned long long clk[MQ_N_CLK];  // -DMQ_STAGE_CLOCKS builds: cycles per stage, summed over waves (mq_last_stage_clocks)
    ChainLaunch chains;  // CHN instantiations only
    unsigned long long spare1[2];
};
static_assert(sizeof(MapCounters) == 256, "the counter block of a launch sequence");
static_assert(offsetof(MapCounters, seed_work) == 0 && offsetof(MapCounters, map_work) == 4 && offsetof(MapCounters, queue_len) == 8 &&
                  offsetof(MapCounters, declined_work) == 12,
              "work and queue cursors");
static_assert(offsetof(MapCounters, n_fast) == 16 && offsetof(MapCounters, n_general) == 20 && offsetof(MapCounters, n_moved) == 24 &&
                  offsetof(MapCounters, n_flagged) == 28,
              "read counts");
static_assert(offsetof(MapCounters, probe) == 32 && offsetof(ProbeStats, steps) == 0 && offsetof(ProbeStats, lookups) == 8 && sizeof(ProbeStats) == 16,
              "probe statistics");
static_assert(offsetof(MapCounters, pool_cursor) == 48, "pool cursor");
static_assert(offsetof(MapCounters, clk) == 64 && offsetof(MapCounters, chains) == 64 + 8 * MQ_N_CLK, "stage clocks");
static_assert(sizeof(ChainLaunch) == 48 && offsetof(MapCounters, spare1) == 240, "the chains output's launch arguments");

// ------------------------------------------------------------------ the index build's seeders (BuildScratch::info)
// work cursors of seed_ref_kernel / seed_ref_general_kernel: RefSeedArgs::counters points at RefBuildInfo::work
struct RefSeedWork {
    uint32_t fast_work;     // segments taken by the fast seeder
    uint32_t queue_len;     // segments it declined (RefSeedArgs::queue)
    uint32_t general_work;  // work cursor over that queue
};
// cleared by the host in front of every reference; scan_counts_kernel sees it as 64-bit words
struct RefBuildInfo {
    unsigned long long total;       // minimizers of the reference
    unsigned long long overflowed;  // segments whose list outgrew its region
    RefSeedWork work;
    uint32_t spare;
};
static_assert(sizeof(RefBuildInfo) == 32 && offsetof(RefBuildInfo, total) == 0 && offsetof(RefBuildInfo, overflowed) == 8 &&
                  offsetof(RefBuildInfo, work) == 16,
              "build info");
static_assert(offsetof(RefSeedWork, fast_work) == 0 && offsetof(RefSeedWork, queue_len) == 4 && offsetof(RefSeedWork, general_work) == 8, "seeders' cursors");

// ------------------------------------------------------------------ the record scanners' result (mq_ctx::fx_info, h_fx_info)
// One block, written by whichever scanner ran on the piece; the kernels see it as 32-bit words.  `flags` (FX_IRREGULAR) is read and
// OR-ed by kernels of both, so it sits at one place.
struct FxRecords {  // scan_tiles_kernel: records of one sequence line (mq_fastx.hpp)
    uint32_t lines;    // incl. the virtual end of a last line without '\n'
    uint32_t records;
    uint32_t flags;
    uint32_t spare;
};
struct FxJoined {  // fl_scan_kernel: line-wrapped records (mq_fastx_lines.hpp)
    uint32_t records;
    uint32_t joined;  // bytes of the joined sequences
    uint32_t flags;
    uint32_t spare;
};
union FxResult {
    FxRecords one;
    FxJoined lines;
    uint32_t words[4];
};
static_assert(sizeof(FxRecords) == 16 && sizeof(FxJoined) == 16 && sizeof(FxResult) == 16, "four result words");
static_assert(offsetof(FxRecords, lines) == 0 && offsetof(FxRecords, records) == 4 && offsetof(FxJoined, records) == 0 && offsetof(FxJoined, joined) == 4,
              "result words");
static_assert(offsetof(FxRecords, flags) == 8 && offsetof(FxRecords, flags) == offsetof(FxJoined, flags), "one place for the flags of both scanners");

// ------------------------------------------------------------------ the overflow redo of a device-resident batch (RedoArena::counters)
// cleared by the host in front of every device-form call on a context with a redo arena; written by redo_collect_kernel (mq_redo.hpp)
struct RedoCounters {
    uint32_t claimed;  // overflow reads short enough for a slot: the slot cursor (the first max_reads of them have one and are redone)
    uint32_t left;     // overflow reads that keep MQ_HIT_OVERFLOW: longer than a slot, or no slot left
    uint32_t spare[2];
};
static_assert(sizeof(RedoCounters) == 16 && offsetof(RedoCounters, claimed) == 0 && offsetof(RedoCounters, left) == 4 && offsetof(RedoCounters, spare) == 8,
              "redo counters");

// ------------------------------------------------------------------ a pooled output of a batch (PooledOutput::counters, mq_host_state.hpp)
// One block per output: the anchors' (AnchorOut::counters, written by chain_stage<CH, true>, mq_chain.hpp) and the chains'
// (ChainLaunch::counters, written by chain_stage<CH, ANCH, true>).  Cleared by the host once per BATCH, in front of its main launch sequence --
// not per launch, as MapCounters is: the batch's redo launches go on claiming from the same cursor.
struct PoolCounters {
    unsigned long long cursor;  // pool entries claimed; counts on past the pool's capacity, so it ends as what the batch needed
    uint32_t dropped_reads;     // reads whose claim did not fit (span first = MQ_ANCHORS_DROPPED / MQ_CHAINS_DROPPED)
    uint32_t spare;
};
using AnchorCounters = PoolCounters;
static_assert(sizeof(PoolCounters) == 16 && offsetof(PoolCounters, cursor) == 0 && offsetof(PoolCounters, dropped_reads) == 8 &&
                  offsetof(PoolCounters, spare) == 12,
              "pool counters");

}  // namespace mq
