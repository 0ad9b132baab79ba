// mq_host_state.hpp -- host-side state behind the C ABI (part of the one translation unit mq_capi.hip): mq_ctx (a stream slot) and mq_index
// with the owners of its parts (StageState, TableReservation, BuildScratch; buffers and handles are the owning types of mq_host_buf.hpp),
// the table of map kernels, launch geometry, scratch management.
#pragma once

// =================================================================== host side

constexpr uint32_t MQ_MAX_REF_ID = 1u << 24;
struct mq_index;
using RefMap = std::map<uint32_t, std::pair<std::string, uint64_t>>;  // reference id -> (name, length): ref_map (src/closures.rs:30, 49)

// The MQ_* test and diagnostic hooks.  Each is read where it acts, never cached at mq_index_new: tests change them between calls.
static bool env_set(const char *name) { return getenv(name) != nullptr; }
static int env_int(const char *name, int fallback) {
    const char *e = getenv(name);
    return e ? atoi(e) : fallback;
}

// One kernel launch with its launch error checked.  The arguments are taken as the kernel's own parameter types, so a Buf converts at the call.
template <class... KA>
static int launch(void (*kernel)(KA...), uint32_t grid, uint32_t block, hipStream_t stream, std::common_type_t<KA>... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, stream, args...);
    HIPCHK(hipGetLastError());
    return MQ_OK;
}

// A piece of a FASTX file whose records the device finds (mq_ctx_submit_fastx): none in flight, or its format
enum class FxKind { None, Fasta, Fastq, FastaLines };

struct RedoArena;  // (below: it holds an mq_ctx of its own)
struct mq_ctx;

// A pooled per-read output of a context's batches -- the anchors (mq_ctx_reserve_anchors) and the chains (mq_ctx_reserve_chains): read r's
// items are pool[spans[r].first, + spans[r].count), claimed by the kernels from one cursor (PoolCounters, mq_blocks.hpp).  reads == 0: no
// reservation -- the context runs the kernels it always ran.  Everything is allocated at the reservation, never by a launch; a launch only
// points its arguments here.  What holds for every such output:
//   - the counter block is cleared once per BATCH, by the batch's main launch (begin_batch), not per launch: the batch's redo launches claim
//     from the same cursor, and place each span where an id map says (the arena's slot-to-read array, or `ids` for the host-driven redo);
//   - `done` is recorded on the stream of every launch sequence that delivered (the context's, or the caller's), and whoever reads the
//     arrays or lets them go waits for it;
//   - a reservation is refused while a batch or a piece is pending, and a failed one leaves the reservation that was there.
template <class Item, class Span>
struct PooledOutput {
    const char *const noun, *const adjective;  // "anchors" / "anchor", "chains" / "chains": the error texts, and mq_ctx_reserve_<noun>
    uint32_t reads = 0;              // max_reads
    uint64_t cap = 0;                // max entries of the pool (< 2^32 - 1)
    Buf<Item> pool;
    Buf<Span> spans;
    Buf<PoolCounters> counters;      // one block
    Buf<uint32_t> ids;               // the host-driven redo's read numbers (redo_relaunch)
    PinnedBuf<Item> h_pool;          // read_back's host copies
    PinnedBuf<Span> h_spans;
    PinnedBuf<PoolCounters> h_counters;
    ScopedEvent done;
    bool ran = false;                // `done` has been recorded since the reservation
    uint32_t n = 0;                  // reads of the last batch that delivered

    PooledOutput(const char *noun_, const char *adjective_) : noun(noun_), adjective(adjective_) {}
    // A batch is refused when it has more reads than spans.  The entry points ask before they queue anything (a FASTX piece: before its map
    // launch -- the number of records is known only at the wait); launch_map asks again, where the spans are about to be written.
    int admit(uint32_t batch) const {
        if (reads && batch > reads)
            return set_err(MQ_EINVAL, std::string("more reads in the batch than the context's ") + adjective + " reservation holds (mq_ctx_reserve_" + noun + ": max_reads)");
        return MQ_OK;
    }
    // the main (not a redo) launch of a batch, in front of its kernels: from here on read_back describes this batch
    int begin_batch(uint32_t batch, hipStream_t st) {
        HIPCHK(hipMemsetAsync(counters, 0, sizeof(PoolCounters), st));
        n = batch;
        return MQ_OK;
    }
    // behind the kernels of every launch sequence that delivered
    int mark_done(hipStream_t st) {
        HIPCHK(hipEventRecord(done, st));
        ran = true;
        return MQ_OK;
    }
    int require_reserved() const {
        return reads ? MQ_OK : set_err(MQ_ESTATE, std::string("no ") + noun + " reserved on this context: call mq_ctx_reserve_" + noun + " first");
    }
    int device_pointers(const Span **d_spans, const Item **d_pool) const {
        if (!reads) return require_reserved();
        *d_spans = spans;
        *d_pool = pool;
        return MQ_OK;
    }
    // (mq_capi_map.hpp, beside ctx_require_idle and ctx_wait) (0, 0) releases; alloc_extra() / commit_extra(): what the reservation brings
    // beyond the owner's arrays -- allocated with them, committed with them (a release commits what was never allocated: it goes)
    template <class Alloc, class Commit>
    int reserve(mq_ctx *c, uint32_t max_reads, uint64_t max_entries, Alloc alloc_extra, Commit commit_extra);
    // host copies of the last batch's spans, pool and counters, once everything that writes them is done
    int read_back(mq_ctx *c, const Span **out_spans, const Item **out_pool, uint32_t *n_reads, uint64_t *stored, uint64_t *needed, uint32_t *dropped_reads);
};

// One stream slot: everything a map launch sequence writes (work counters, Match scratch, minimizer lists,
// events) plus the staging buffers of the host-buffer entry points.  Launch sequences of DIFFERENT contexts of one index
// may be in flight together (the index itself is read-only once finalized); one context runs one sequence at a time.
struct mq_ctx {
    mq_index *idx = nullptr;
    // (members are destroyed last to first: the buffers, then the events, then the stream; ctx_release synchronises the stream before)
    ScopedStream stream;            // the context's own stream (host-buffer entry points)
    ScopedEvent ev0, ev1;
    bool ev_valid = false;
    uint32_t last_spec = 0;         // MAP_SPECS id of the pair the last fused launch sequence ran (0: SpecNone)
    Buf<MapCounters> d_counter;     // one block (mq_blocks.hpp): MapArgs::counters, cleared in front of every launch sequence
    Buf<MatchRec> scratch;          // per mapping wave: cap_matches records
    size_t scratch_waves = 0;       // waves it has windows for
    Buf<unsigned long long> mz_hash;
    Buf<uint32_t> mz_pos;
    Buf<uint32_t> mz_last;          // seeding variant 16 only: every minimizer's second position (allocated with mz_pos, else empty)
    uint64_t mz_cap = 0;            // list entries allocated (the three lists are one group)
    Buf<uint32_t> mz_count;
    Buf<uint64_t> mz_base;
    Buf<uint32_t> queue;
    Buf<uint4> work;                // map_kernel's work items (order_reads_kernel): WORK_FRONT_CAP + reads_cap descriptors
    uint64_t reads_cap = 0;         // reads the four per-read arrays above hold (one group)
    uint64_t pool_base = 0, pool_cap = 0;  // of the last ctx_ensure: the pool behind the regular list regions
    // staging for the host-buffer entry points
    Buf<uint8_t> st_bases;
    Buf<uint64_t> st_off;
    Buf<mq_hit> st_out;
    Buf<uint32_t> st_lens;
    PinnedBuf<uint64_t> h_off;      // relative offsets on their way to the device
    PinnedBuf<mq_hit> h_out;        // hits on their way back
    // device-parsed FASTA chunks (mq_ctx_submit_fasta / mq_ctx_wait_fasta): tile counts / offsets, the line ends, the scan's result words
    Buf<uint32_t> fx_tile_counts, fx_tile_off;
    Buf<uint32_t> fx_nl;
    PinnedBuf<uint32_t> h_fx_nl;
    Buf<FxResult> fx_info;          // one block (mq_blocks.hpp): FxRecords or FxJoined, by the scanner that ran (fx_kind)
    PinnedBuf<FxResult> h_fx_info;
    PinnedBuf<uint8_t> h_fx_tail;   // one page: the piece's bytes behind its last page boundary
    // MQ_FASTX_FASTA_LINES (mq_fastx_lines.hpp): the joined sequence bytes, header spans and their mirrors; the joined lengths come back
    // from st_lens, the offsets of the joined reads live in st_off
    Buf<uint8_t> fl_joined;
    Buf<uint32_t> fl_hb, fl_he;
    PinnedBuf<uint32_t> h_fl_hb, h_fl_he, h_fl_lens;
    bool fl_used = false;           // a LINES piece has been submitted on this context: mq_ctx_reserve sizes the buffers above too
    FxKind fx_kind = FxKind::None;  // the piece in flight (mq_ctx_wait_fasta finishes Fasta / Fastq, mq_ctx_wait_fasta_lines FastaLines)
    uint32_t fx_bytes = 0;          // ... and its size
    // a submitted, not yet waited-for batch
    bool pending = false;
    const uint8_t *p_bases = nullptr;
    const uint64_t *p_offsets = nullptr;
    const uint32_t *p_lens = nullptr;
    uint32_t p_n = 0;
    mq_hit *p_out = nullptr;
    // mq_ctx_reserve_anchors / mq_ctx_reserve_chains: the two pooled outputs of the context's batches (PooledOutput above), and the chain
    // windows of the context's launches, which come and go with the chains reservation: a window of chain_win_cap(cap_matches) records for
    // every mapping wave a batch of max_reads reads can employ.  (The windows of the host-driven redo, whose size is the longest redone
    // read's, live as long as that redo's Match windows do: redo_relaunch.)
    PooledOutput<mq_anchor, mq_anchor_span> anchors{"anchors", "anchor"};
    PooledOutput<mq_chain, mq_chain_span> chains{"chains", "chains"};
    Buf<ChainRec> chn_windows;
    // mq_ctx_reserve_redo: what the device form needs to redo its overflow reads in stream (none: they come back MQ_HIT_OVERFLOW).  The
    // last member, so the first to go: it waits for its own last launch, and its buffers go before the context's.
    std::unique_ptr<RedoArena> redo;
};

// The redo arena of a context: room for max_reads overflow reads of a device-form call, and everything a launch sequence over them writes.
// That is a context state of its own (`sub`: lists and per-read arrays from ctx_ensure(max_reads, max_reads * stride, 65536), work
// descriptors, queue, counter block, events; no stream -- it is launched on the caller's), so the main launch's counters, events and spec id
// keep describing the main launch.  Slot j is bases[j * stride, (j + 1) * stride): offsets[j] = j * stride is written once, here;
// lens[j], ids[j], src[j] are redo_collect_kernel's (mq_redo.hpp).  (The owner has selected the index's device when the arena goes.)
struct RedoArena {
    uint32_t max_reads = 0, max_read_len = 0;
    uint64_t stride = 0;           // bytes per slot: max_read_len + 64 rounded up to 64 (what the staging buffers leave behind a batch's last read)
    uint32_t cap = 0, grid = 0;    // LaunchOpt::cap_override, grid_override of the launch: worst-case Match windows on a small grid
    mq_ctx sub;
    Buf<uint8_t> bases;
    Buf<uint64_t> offsets;         // max_reads + 1
    Buf<uint32_t> lens, ids;
    Buf<uint64_t> src;             // where slot j's read begins in the caller's buffer
    Buf<mq_hit> hits;
    Buf<MatchRec> windows;         // grid * max(MAP_WAVES, ML_WAVES) windows of cap records
    Buf<ChainRec> chain_windows;   // as many chain windows of chain_win_cap(cap) records, while the owning context has a chains reservation
    Buf<RedoCounters> counters;    // one block (mq_blocks.hpp), cleared in front of every device-form call
    ScopedEvent done;              // behind redo_scatter_kernel of the last device-form call
    bool ran = false;              // ... recorded at least once
    uint32_t last_n = 0;           // reads of the last device-form call (0: none yet, or an empty one: nothing was queued)
    ~RedoArena() {
        if (ran) (void)hipEventSynchronize(done);  // the caller's stream has passed the arena's last use
    }
};

// Per-read timing of the instrumented launch (mq_last_read_cycles): the fused pair leaves it in the split pipeline's per-read arrays, which
// it does not use otherwise -- the host side of read_cycles() / read_start(), mq_map_kernels.hpp
static const uint32_t *ctx_read_cycles(const mq_ctx *c) { return c->mz_count; }
static const uint64_t *ctx_read_start(const mq_ctx *c) { return c->mz_base; }

// (the caller has selected the index's device: the context's buffers, events and stream go with it)
static void ctx_release(mq_ctx *c) {
    if (!c) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    delete c;
}
struct CtxRelease {
    void operator()(mq_ctx *c) const { ctx_release(c); }
};
using CtxPtr = std::unique_ptr<mq_ctx, CtxRelease>;

struct KmmChunk {
    Buf<RefKmm> d;   // d.cap k-min-mers of room
    uint64_t n = 0;  // k-min-mers of several references share a chunk (assemblies with 10^5 small contigs)
};

// grow-only scratch of mq_index_add_ref (freed by finalize): no allocation per reference once it has grown
struct BuildScratch {
    Buf<uint8_t> seq;
    Buf<unsigned long long> seg_hash;  // per-segment minimizer lists
    Buf<uint32_t> seg_pos;
    Buf<unsigned long long> dense_hash;  // the reference's dense list
    Buf<uint32_t> dense_pos;
    Buf<uint32_t> seg_last, dense_last;  // seeding variant 16 only
    Buf<uint32_t> counts, queue;
    Buf<unsigned long long> seg_off;
    Buf<RefBuildInfo> info;  // one block (mq_blocks.hpp): total, overflowed segments, the seeders' work cursors
    // mq_index_add_ref_staged_lines: kept bytes per tile of the region, their exclusive scan, [0] the joined length (mq_join.hpp)
    Buf<uint32_t> join_counts;
    Buf<unsigned long long> join_off, join_total;
};

// mq_index_stage_*: the reference file's bytes on their way to the device piece by piece (a buffer of the file's size, an upload
// stream, one event per piece); a state of its own behind its own lock, so that pieces keep flowing while a record is being indexed.
// (The caller has selected the index's device.)
struct StageState {
    std::mutex mu;
    Buf<uint8_t> buf;
    uint64_t bytes = 0;
    ScopedStream stream;
    std::vector<ScopedEvent> events;  // ticket t = event t (tickets count from 0): the pieces issued so far, every event RECORDED

    int begin(uint64_t total_bytes) {
        std::lock_guard<std::mutex> lk(mu);
        if (buf) return set_err(MQ_ESTATE, "mq_index_stage_begin: one staging buffer per index");
        // no buffer without its stream (a later piece() must not find one): the buffer becomes the state's only once the stream exists
        Buf<uint8_t> b;
        int rc = b.alloc(total_bytes + 64);
        if (rc) return rc;
        hipStream_t st = nullptr;
        const hipError_t es = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (es != hipSuccess) return set_err(MQ_EHIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(es));
        stream.h = st;
        buf = std::move(b);
        bytes = total_bytes;
        return MQ_OK;
    }
    int piece(uint64_t at, const uint8_t *src, uint64_t n, uint64_t *ticket) {
        std::lock_guard<std::mutex> lk(mu);
        if (!buf) return set_err(MQ_ESTATE, "mq_index_stage_piece before mq_index_stage_begin");
        if (at > bytes || n > bytes - at) return set_err(MQ_EINVAL, "piece outside the staging buffer");
        if (n) HIPCHK(hipMemcpyAsync(buf + at, src, n, hipMemcpyHostToDevice, stream));
        // the event joins the list, and its ticket exists, only once its record has succeeded (a ticket that indexed an event never
        // recorded would let a wait return at once and a record be indexed before its bytes arrive)
        ScopedEvent ev;
        HIPCHK(hipEventCreateWithFlags(&ev.h, hipEventDisableTiming));
        const hipError_t er = hipEventRecord(ev, stream);
        if (er != hipSuccess) return set_err(MQ_EHIP, std::string("hipEventRecord: ") + hipGetErrorString(er));
        events.push_back(std::move(ev));
        *ticket = events.size() - 1;
        return MQ_OK;
    }
    // 1: the piece has arrived, 0: not yet (wait == 0 only)
    int done(uint64_t ticket, int wait) {
        hipEvent_t ev;
        {
            std::lock_guard<std::mutex> lk(mu);
            if (ticket >= events.size()) return set_err(MQ_EINVAL, "unknown ticket");
            ev = events[(size_t)ticket];
        }
        if (wait) {
            HIPCHK(hipEventSynchronize(ev));
            return 1;
        }
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return 1;
        if (e == hipErrorNotReady) {
            (void)hipGetLastError();
            return 0;
        }
        return set_err(MQ_EHIP, std::string("hipEventQuery: ") + hipGetErrorString(e));
    }
    // the state, range and ticket checks of the calls that read the staging buffer, and the null stream made to wait for the pieces;
    // *d_region: buffer + at
    int region(const char *who, uint64_t at, uint64_t n, uint64_t after_ticket, const uint8_t **d_region) {
        std::lock_guard<std::mutex> lk(mu);
        if (!buf) return set_err(MQ_ESTATE, std::string(who) + " before mq_index_stage_begin");
        if (at > bytes || n > bytes - at) return set_err(MQ_EINVAL, "record outside the staging buffer");
        if (after_ticket != MQ_STAGE_ALL_ISSUED && after_ticket >= events.size()) return set_err(MQ_EINVAL, "unknown ticket");
        // the build's kernels run on the null stream: it waits (on the device, not here) for the piece named (pieces complete in issue
        // order, so for every piece up to it), or for every piece issued so far
        const uint64_t upto = after_ticket == MQ_STAGE_ALL_ISSUED ? events.size() : after_ticket + 1;
        if (upto) HIPCHK(hipStreamWaitEvent(0, events[(size_t)upto - 1], 0));
        *d_region = buf + at;
        return MQ_OK;
    }
    // pieces still on their way arrive first; then the events, the stream and the buffer go
    void reset() {
        std::lock_guard<std::mutex> lk(mu);
        if (stream) hipStreamSynchronize(stream);
        events.clear();
        stream.reset();
        buf.reset();
        bytes = 0;
    }
    ~StageState() { reset(); }
};

static size_t table_bytes_of(uint64_t nslots) { return (size_t)(nslots / 2 + 1) * sizeof(Bucket); }

// mq_index_reserve: the table allocated and cleared ahead of time by a thread of its own; finalize takes it when the size fits.
// (Under the index's lock; the thread writes table, err and ms, which nobody reads before join().)
struct TableReservation {
    std::thread thread;
    Buf<Bucket> table;
    uint64_t nslots = 0;
    int err = 0;    // hipError_t of the background allocation
    double ms = 0;  // what hipMalloc + memset + synchronize took there
    bool made() const { return thread.joinable() || table; }
    void start(int device, uint64_t n) {
        nslots = n;
        thread = std::thread([this, device]() {
            hipError_t e = hipSetDevice(device);
            Buf<Bucket> t;
            const auto t0 = std::chrono::steady_clock::now();
            if (e == hipSuccess) e = t.try_alloc(table_bytes_of(nslots) / sizeof(Bucket));
            ScopedStream st;
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.h, hipStreamNonBlocking);  // not the null stream: the build's kernels run there
            if (e == hipSuccess) e = hipMemsetAsync(t, 0, table_bytes_of(nslots), st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (e == hipSuccess) table = std::move(t);
            err = (int)e;
        });
    }
    void join() {
        if (thread.joinable()) thread.join();
    }
    // the reserved table when it has `want` slots, else nothing: an estimate that was off, or an allocation that failed, is given back
    Buf<Bucket> take(uint64_t want) {
        join();
        Buf<Bucket> t = std::move(table);
        if (nslots != want || err != 0) t.reset();
        return t;
    }
    ~TableReservation() { join(); }
};

// mq_index_coverage (mq_cover_kernels.hpp): the device side of one call, all of it given back before the call returns, and the host
// copies the caller reads until the next call that changes the index, or asks again, drops them.
struct CoverState {
    Buf<unsigned long long> bitmap;          // one bit per base, every existing reference on a word boundary, two words of padding
    Buf<uint64_t> base, lens_c;              // the cover base word per reference id (dense, beside d_ref_lens); the existing references' lengths
    Buf<unsigned long long> live;            // live entries per reference id (dense)
    Buf<CovTile> tiles;
    Buf<uint32_t> tile_runs;
    Buf<unsigned long long> tile_off, ref_sums, first_interval, acc;
    Buf<mq_cov_interval> intervals;          // allocated behind the count, at its exact size
    std::vector<mq_ref_coverage> h_refs;
    std::vector<mq_cov_interval> h_intervals;
    uint64_t out_of_range = 0;
    // (the owner has selected the index's device)
    void free_device() { reset_all(bitmap, base, lens_c, live, tiles, tile_runs, tile_off, ref_sums, first_interval, acc, intervals); }
    void drop() {
        free_device();
        std::vector<mq_ref_coverage>().swap(h_refs);
        std::vector<mq_cov_interval>().swap(h_intervals);
        out_of_range = 0;
    }
    uint64_t held() const { return h_refs.capacity() * sizeof(mq_ref_coverage) + h_intervals.capacity() * sizeof(mq_cov_interval); }
};

// mq_depth (mq_depth_kernels.hpp, mq_capi_depth.hpp): a depth accumulator.  Its own object beside the index: it holds a snapshot of the
// reference ids and lengths (plan) and nothing of the index but its device.  Everything but the hit staging and the result arrays is
// allocated at mq_depth_new; mq_depth_add_device only points a launch's arguments here.  (Members go last to first: the buffers, the
// events, then the stream; the owner has selected the device and waited for it.)
struct mq_depth {
    std::mutex mu;  // every entry point locks the accumulator
    int device = 0;
    uint32_t window = 0, min_mapq = 0;
    uint32_t n_ids = 0, n_tiles = 0;
    uint64_t n_windows = 0;
    uint64_t offered = 0;                      // hits offered since creation or the last clear (< 2^31)
    std::vector<mq_ref_depth> plan;            // the existing references in id order: ref_id, len, n_windows, first_window
    ScopedStream stream;                       // the host route's launches and the result pass
    ScopedEvent e0, e1;                        // around the result pass's kernels (mqdiag_depth_result_ms)
    float result_ms = 0;
    Buf<uint64_t> lens, base;                  // dense by reference id: the snapshot's lengths, every reference's first window
    Buf<unsigned long long> edge;              // the three accumulators, n_windows each
    Buf<int> diff;
    Buf<uint32_t> starts;
    Buf<unsigned long long> reads, acc;        // counted hits per reference id (dense); DEPTH_ACC_WORDS totals
    Buf<DepthTile> tiles;
    Buf<long long> tile_sum, tile_pref, tile_off;
    Buf<unsigned long long> ref_sums;          // three words per existing reference
    Buf<unsigned long long> window_bases;      // the result arrays: allocated by the first mq_depth_result
    Buf<uint32_t> window_starts;
    Buf<mq_hit> stage;                         // mq_depth_add's hits on their way in (grows)
    std::vector<mq_ref_depth> h_refs;          // the caller's copies of the last result
    std::vector<uint64_t> h_bases;
    std::vector<uint32_t> h_starts;
};

// mq_sorter (mq_sort_kernels.hpp, mq_capi_sort.hpp): the coordinate order of the hits offered to it.  Its own object beside the index, as
// mq_depth: a snapshot of the reference ids (dense lengths) and the index's device.  The kept records always lie in key / ord, `capacity`
// elements each; key2 / ord2 / counts are the result pass's and come with the first mq_sort_result (a pass sorts from one set into the
// other, and the sets are swapped behind every pass, so the records are in key / ord again).  mq_sort_add_device only points a launch's
// arguments here.  (Members go last to first, as mq_depth's.)
struct mq_sorter {
    std::mutex mu;  // every entry point locks the sorter
    int device = 0;
    uint32_t min_mapq = 0, n_ids = 0;
    uint64_t capacity = 0;                     // records key / ord hold: counted in OFFERED hits
    uint64_t offered = 0;                      // hits offered since creation or the last clear (< 2^32 - 1)
    uint32_t passes = 0;                       // digits the last result sorted (mqdiag_sort_passes)
    std::vector<uint32_t> ref_ids;             // the existing references, ascending
    ScopedStream stream;                       // the host route's launches and the result pass
    ScopedEvent e0, e1;                        // around the result pass (mqdiag_sort_result_ms)
    float result_ms = 0;
    Buf<uint64_t> lens;                        // dense by reference id: the snapshot's lengths
    Buf<uint32_t> ids;                         // ref_ids on the device
    Buf<unsigned long long> acc;               // SORT_ACC_WORDS: the append cursor (= kept) and three tallies
    Buf<unsigned long long> key, key2;         // ref_id << 32 | r_start
    Buf<uint32_t> ord, ord2;                   // the ordinals beside them
    Buf<uint32_t> counts, totals;              // [256][tiles of capacity] per-tile digit counts / their row prefixes; the 256 row sums
    Buf<unsigned long long> hist;              // 11 x 256: the digit histograms
    Buf<unsigned long long> ref_out;           // first, count per existing reference
    Buf<mq_hit> stage;                         // mq_sort_add's hits on their way in (grows)
    std::vector<uint32_t> h_order;             // the caller's copies of the last result
    std::vector<mq_sort_ref> h_refs;
    mq_sort_totals h_totals = {};
};

struct mq_index {
    mq_params params;
    DevParams dp;
    int device = 0;
    int n_cu = 0;
    std::once_flag geometry_once;  // launch geometry is worked out once, by whichever context or entry point maps first
    int geometry_rc = MQ_OK;
    std::mutex mu;  // serialises the index-level entry points (add_ref, finalize, and everything that uses the default context)
    RefMap refs;
    uint64_t n_kmm_total = 0;
    bool finalized = false;
    bool extending = false;     // mq_index_reopen: the table holds the keys of an earlier finalize, the next one inserts into it
    bool extend_failed = false; // a finalize of a reopened index failed with part of the new keys in the table: no retry could be exact
    bool merge_failed = false;  // ... or a merge (mq_index_merge*) did, behind its first insert launch: set with extend_failed, finalized cleared
    // the contexts mq_ctx_new made on this index (not the default one): mq_index_merge* refuses while one of them has a batch in flight
    std::mutex ctx_mu;
    std::vector<mq_ctx *> ctxs;
    uint32_t table_factor = 0;  // mq_index_set_table_factor: slots per inserted k-min-mer (0: the default, 8)
    uint64_t nslots = 0;
    uint64_t n_unique = 0, n_keys = 0;
    int grid_ref = 0;                        // workgroups of seed_ref_kernel that stay resident
    // launch geometry (workgroups) and scratch sizes, fixed at the first map call
    uint32_t grid_fused = 0, grid_seed = 0, grid_map = 0;  // map_kernel; seed_reads_kernel, map_lists_kernel (split)
    // ... of the launches of contexts with an anchors or a chains reservation: the minimum over grid_fused and the output pairs the index can
    // launch (anchors, chains, both), worked out at the first reservation of either kind (an index nobody reserves on keeps its launch geometry)
    std::once_flag outputs_geometry_once;
    int outputs_geometry_rc = MQ_OK;
    uint32_t grid_fused_outputs = 0;
    uint32_t cap_matches = 0;
    bool split = false;             // diagnostic MQ_PIPELINE=split: the two phases as separate launches (a profiler then prices each)
    bool force_general = false;     // test hook MQ_FORCE_GENERAL=1: never take the fast seeding path
    bool heavy_first = true;        // order_reads_kernel puts reads that look like short-period tandem arrays first (MQ_HEAVY_FIRST=0: A/B hook, reads in their own order)
    int chain_chunk = 64;           // test hook: MQ_CHAIN_CHUNK=4 exercises the multi-chunk chain path
    bool no_spec = false;           // A/B and test hook MQ_NO_SPEC=1: product launches take the SpecNone pair whatever the parameters
    uint32_t map_spec = 0;          // MAP_SPECS id of the pair a product launch takes (0: SpecNone); follows dp (set_dev_params)
    double t_add_ms = 0;            // MQ_BUILD_TIMING: wall time spent in mq_index_add_ref[_device] so far
    double table_alloc_ms = 0;      // what allocating + clearing the table that is in use took (hipMalloc + memset + synchronize), wherever it ran
    // What lives on the device.  ~mq_index joins the reservation and selects the device; then the members go last to first: the reserved
    // table, the k-min-mer chunks, the staged pieces (synchronised first), the build scratch, the table, the reference lengths, and
    // last the default context (synchronised, then released).  (The coverage state holds device memory only inside mq_index_coverage.)
    CtxPtr def_ctx;      // the context behind the index-level map entry points
    CoverState cov;      // mq_index_coverage: the last result's host copies
    Buf<uint64_t> d_ref_lens;
    Buf<Bucket> table;   // nslots / 2 buckets + the extra bucket of the key 0
    BuildScratch bld;
    StageState stage;
    std::vector<KmmChunk> chunks;
    TableReservation rsv;

    ~mq_index() {
        rsv.join();
        hipSetDevice(device);
    }
};

constexpr uint64_t MQ_MAX_TABLE_SLOTS = 1ull << 40;
// slots of the table for n inserted k-min-mers at `factor` slots each, rounded up to a power of two (a count that no table could hold,
// a corrupt file's for one, gives twice the largest table: refused where it is used)
static uint64_t table_slots_at(uint64_t factor, uint64_t n_kmm) {
    const uint64_t want = n_kmm > MQ_MAX_TABLE_SLOTS ? 2 * MQ_MAX_TABLE_SLOTS : factor * n_kmm;
    uint64_t nslots = 1024;
    while (nslots < want && nslots <= MQ_MAX_TABLE_SLOTS) nslots <<= 1;
    return nslots;
}
// ... at the index's own factor: MQ_TABLE_FACTOR (default 8: load <= 0.125)
static uint64_t table_slots_for(const mq_index *idx, uint64_t n_kmm) {
    const int lf = env_int("MQ_TABLE_FACTOR", 0);  // (test / experiment hook: overrides the caller's choice)
    const uint64_t factor = lf >= 2 ? (uint64_t)lf : idx->table_factor ? (uint64_t)idx->table_factor : 8ull;  // >= 2: a full table would make a miss walk forever
    return table_slots_at(factor, n_kmm);
}

// The size arguments of mq_index_resize / mq_index_load_sized / mq_index_clone_sized for an index of n_kmm inserted k-min-mers and n_keys
// distinct keys; *out: the table's slots, 0 when both arguments are 0 ("as it is").  An exact size must leave an empty slot (a table
// without one would make a miss walk forever: read_header's rule); a factor gives table_slots_at's size, raised to the smallest legal one.
static int sized_table_slots(uint64_t table_slots, uint32_t slots_per_kminmer, uint64_t n_kmm, uint64_t n_keys, uint64_t *out) {
    *out = 0;
    if (table_slots && slots_per_kminmer) return set_err(MQ_EINVAL, "table size: table_slots or slots_per_kminmer, not both");
    if (table_slots) {
        if (table_slots < 2 || (table_slots & (table_slots - 1)) != 0 || table_slots > MQ_MAX_TABLE_SLOTS)
            return set_err(MQ_EINVAL, "table_slots: a power of two in [2, 2^40]");
        if (table_slots <= n_keys) return set_err(MQ_EINVAL, "table_slots: more slots than the index has keys (a table needs an empty slot)");
        *out = table_slots;
    } else if (slots_per_kminmer) {
        if (slots_per_kminmer < 2 || slots_per_kminmer > 64) return set_err(MQ_EINVAL, "slots per k-min-mer: 2..64");
        uint64_t s = table_slots_at(slots_per_kminmer, n_kmm);
        while (s <= n_keys && s <= MQ_MAX_TABLE_SLOTS) s <<= 1;
        if (s > MQ_MAX_TABLE_SLOTS) return set_err(MQ_EINVAL, "slots per k-min-mer: the table would pass 2^40 slots");
        *out = s;
    }
    return MQ_OK;
}

extern "C" {

const char *mq_last_error(void) { return g_err.c_str(); }
int mq_abi_version(void) { return MQ_ABI_VERSION; }

int mq_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        set_err(MQ_ENODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
        return 0;
    }
    return n;
}

void mq_params_default(mq_params *p) {
    p->k = 5;
    p->l = 31;
    p->density = 0.01;
    p->use_hpc = 1;
    p->c = 4;
    p->s = 11;
    p->g = 2000;
    p->flags = 0;
}

}  // extern "C"

// (density as FH * H::MAX as FH) as H with Rust's saturating float->int cast, for the seeding variant's FH (f64; f32 with bit 2) and H
// (u64; u32 with bit 4)
static uint64_t density_bound(double density, uint32_t variant) {
    if (variant & MQ_SEEDVAR_HASH32) {
        if (variant & MQ_SEEDVAR_F32_BOUND) {
            const float f = (float)density * 4294967295.0f;
            if (!(f > 0.0f)) return 0;
            if (f >= 4294967296.0f) return 0xFFFFFFFFull;
            return (uint64_t)(uint32_t)f;
        }
        const double d = density * 4294967295.0;
        if (!(d > 0.0)) return 0;
        if (d >= 4294967296.0) return 0xFFFFFFFFull;
        return (uint64_t)(uint32_t)d;
    }
    if (variant & MQ_SEEDVAR_F32_BOUND) {
        const float f = (float)density * 18446744073709551615.0f;
        if (!(f > 0.0f)) return 0;
        if (f >= 18446744073709551616.0f) return UINT64_MAX;
        return (uint64_t)f;
    }
    const double d = density * 18446744073709551615.0;
    if (!(d > 0.0)) return 0;
    if (d >= 18446744073709551616.0) return UINT64_MAX;
    return (uint64_t)d;
}
// DevParams of an index: the bound in the form the kernels compare with (`hash <= bound` on 64-bit words; DevParams::variant)
static void set_dev_bound(DevParams &dp, double density, uint32_t variant) {
    uint64_t b = density_bound(density, variant);
    dp.keep_none = 0;
    if (variant & MQ_SEEDVAR_STRICT_BOUND) {  // hash < b  <=>  hash <= b - 1; nothing is below 0
        if (b == 0) dp.keep_none = 1;
        else b -= 1;
    }
    if (variant & MQ_SEEDVAR_HASH32) b = (b & 0xFFFFFFFFull) | (b << 32);  // dup(bound32): compared with dup(hash32)
    dp.bound = b;
    dp.variant = variant;
}

// DevParams of an index with these parameters (mq_index_new, and mq_index_set_map_params for the ones that act at mapping time)
static DevParams dev_params_from(const mq_params &p, uint32_t variant) {
    DevParams dp{};
    set_dev_bound(dp, p.density, variant);
    dp.k = p.k;
    dp.l = p.l;
    dp.use_hpc = p.use_hpc ? 1 : 0;
    dp.c = p.c;
    dp.s = p.s;
    dp.g = p.g;
    dp.fold = (p.flags & MQ_FLAG_FOLD_CASE) ? 1u : 0u;
    dp.fast_kh = (p.flags & MQ_FLAG_FAST_KH) ? 1u : 0u;
    return dp;
}

static int use_device(const mq_index *idx) {
    HIPCHK(hipSetDevice(idx->device));
    return MQ_OK;
}

// workgroups (of 256 threads) of a kernel that walks the table's nb1 buckets, two slots each
static uint32_t bucket_walk_grid(uint64_t nb1) { return (uint32_t)std::min<uint64_t>((2 * nb1 + 255) / 256, 1u << 16); }
// ... of a kernel that takes an array of n saved slots one per lane (unpack_slots_kernel, merge_check_slots_kernel; n >= 1)
static uint32_t slot_array_grid(uint64_t n) { return (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 16); }
// ... of a kernel whose lanes load RETABLE_AHEAD of n slots ahead (retable_kernel, merge_table_kernel, merge_slots_kernel; n >= 1)
static uint32_t ahead_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 256 * RETABLE_AHEAD - 1) / (256 * RETABLE_AHEAD), 1u << 16)); }

// a table of nslots slots, its clearing queued on the null stream: kernels launched there afterwards find it zeroed without a wait
static int new_table(Buf<Bucket> &table, uint64_t nslots) {
    int rc = table.alloc(table_bytes_of(nslots) / sizeof(Bucket));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(table, 0, table_bytes_of(nslots), 0));
    return MQ_OK;
}
static int alloc_table(mq_index *idx, uint64_t nslots) {
    if (nslots < 2) nslots = 2;  // whole buckets
    const auto t0 = std::chrono::steady_clock::now();
    int rc = new_table(idx->table, nslots);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    idx->table_alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    idx->nslots = nslots;
    return MQ_OK;
}

// Every instantiation of the fused launch sequence's two kernels, by [seeding variant != 0][instrumented][chain chunk 4]: launch_map picks
// its pair here or from MAP_SPECS below (map_pair_of), and the launch geometry is the minimum over the pairs the index can launch.  (The
// instrumented launch is built for chunk 64 only.)
using MapFn = void (*)(MapArgs);
struct MapPair {
    MapFn map, declined;
};
template <int CH, bool TIMING, bool VAR, class Spec = SpecNone, bool ANCH = false, bool CHN = false>
constexpr MapPair map_pair() {
    return {map_kernel<CH, TIMING, VAR, Spec, ANCH, CHN>, map_declined_kernel<CH, TIMING, VAR, Spec, ANCH, CHN>};
}
static const MapPair MAP_KERNELS[2][2][2] = {{{map_pair<64, false, false>(), map_pair<4, false, false>()}, {map_pair<64, true, false>(), map_pair<64, true, false>()}},
                                             {{map_pair<64, false, true>(), map_pair<4, false, true>()}, {map_pair<64, true, true>(), map_pair<64, true, true>()}}};
// The output dimensions: the SpecNone, non-instrumented pairs once more with the anchor output, the chains output or both (a context with
// a reservation: mq_ctx_reserve_anchors, mq_ctx_reserve_chains), by [anchors][chains][seeding variant != 0][chain chunk 4].  The [0][0]
// corner is not built: it is MAP_KERNELS.  MAP_SPECS has no such dimension: a reserving context launches SpecNone.
template <bool ANCH, bool CHN>
constexpr MapPair out_pair(bool var, bool ch4) {
    return var ? (ch4 ? map_pair<4, false, true, SpecNone, ANCH, CHN>() : map_pair<64, false, true, SpecNone, ANCH, CHN>())
               : (ch4 ? map_pair<4, false, false, SpecNone, ANCH, CHN>() : map_pair<64, false, false, SpecNone, ANCH, CHN>());
}
#define MQ_OUT_PAIRS(A, C) {{out_pair<A, C>(false, false), out_pair<A, C>(false, true)}, {out_pair<A, C>(true, false), out_pair<A, C>(true, true)}}
static const MapPair MAP_KERNELS_OUTPUTS[2][2][2][2] = {{{{{nullptr, nullptr}, {nullptr, nullptr}}, {{nullptr, nullptr}, {nullptr, nullptr}}}, MQ_OUT_PAIRS(false, true)},
                                                        {MQ_OUT_PAIRS(true, false), MQ_OUT_PAIRS(true, true)}};
#undef MQ_OUT_PAIRS

// The spec dimension of the table: the product pair (chunk 64, not instrumented, frozen reading) compiled for the parameters nearly
// every run uses -- the reference's defaults -k 5 -l 31 with homopolymer compression and SipHash, the -k 7 of its real-data runs, and the
// defaults with case folding (the native driver folds every file-fed run).  Spec id 0 = SpecNone = MAP_KERNELS: every other parameter
// set, the seeding variants, the instrumented launch and chunk 4.  A spec is taken on an EXACT match of all five fields it fixes.
struct MapSpec {
    uint32_t k, l, use_hpc, fold, fast_kh;
    MapPair pair;
};
template <class S>
constexpr MapSpec map_spec() {
    return {S::K, S::L, S::HPC ? 1u : 0u, S::FOLD ? 1u : 0u, S::FAST_KH ? 1u : 0u, map_pair<64, false, false, S>()};
}
static const MapSpec MAP_SPECS[] = {map_spec<SpecFixed<5, 31, true, false>>(), map_spec<SpecFixed<7, 31, true, false>>(),
                                    map_spec<SpecFixed<5, 31, true, true>>()};
constexpr uint32_t N_MAP_SPECS = sizeof(MAP_SPECS) / sizeof(MAP_SPECS[0]);

// id (1-based, 0: none) of the spec whose fields equal dp's; any_fold: the fold field is not compared (mq_index_set_map_params may change
// it between launches: the launch geometry covers both)
static bool spec_matches(const MapSpec &s, const DevParams &dp, bool any_fold) {
    return s.k == dp.k && s.l == dp.l && s.use_hpc == dp.use_hpc && s.fast_kh == dp.fast_kh && (any_fold || s.fold == dp.fold);
}
// The spec a product launch of this index takes (0: SpecNone).  MQ_NO_SPEC=1 (A/B and test hook, read at mq_index_new) forces SpecNone.
static bool specs_allowed(const mq_index *idx) { return !idx->no_spec && idx->dp.variant == 0 && idx->chain_chunk != 4; }
static uint32_t map_spec_of(const mq_index *idx) {
    if (!specs_allowed(idx)) return 0;
    for (uint32_t i = 0; i < N_MAP_SPECS; ++i)
        if (spec_matches(MAP_SPECS[i], idx->dp, false)) return i + 1;
    return 0;
}
// the pair of a fused launch sequence, and the spec id it carries
// anchors, chains: the launching context has that reservation and the launch delivers (never the instrumented one)
static const MapPair &map_pair_of(const mq_index *idx, bool instrumented, uint32_t *spec_id = nullptr, bool anchors = false, bool chains = false) {
    if ((anchors || chains) && !instrumented) {
        if (spec_id) *spec_id = 0;
        return MAP_KERNELS_OUTPUTS[anchors][chains][idx->dp.variant != 0][idx->chain_chunk == 4];
    }
    const uint32_t sid = instrumented ? 0u : idx->map_spec;
    if (spec_id) *spec_id = sid;
    return sid ? MAP_SPECS[sid - 1].pair : MAP_KERNELS[idx->dp.variant != 0][instrumented][idx->chain_chunk == 4];
}
// an index's DevParams change in one place: the pair its launches take is chosen here, once per parameter set
static void set_dev_params(mq_index *idx, const DevParams &dp) {
    idx->dp = dp;
    idx->map_spec = map_spec_of(idx);
}

// launch geometry: persistent waves, as many workgroups as stay resident
static int occ_of(const void *fn, int threads, int &occ) {
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, threads, 0));
    if (occ < 1) occ = 1;
    if (occ > 8) occ = 8;
    const int oe = env_int("MQ_OCC", 0);  // diagnostic: cap workgroups per CU
    if (oe >= 1 && oe < occ) occ = oe;
    return MQ_OK;
}
static int ensure_geometry_once(mq_index *idx) {
    int occ = 0, occ_min = INT_MAX, rc;
    // the grid of a launch sequence = the workgroups that are RESIDENT together, for every instantiation launched on it: wave w's first two
    // work items are its own (items w and n_waves + w, among them the heavy reads that go first), so a workgroup that has to wait for a
    // place would hold them back; map_declined_kernel (more scratch) may fit fewer than map_kernel.  The instantiations launched on THIS
    // index: its SpecNone pair and the instrumented one (its seeding variant and chain chunk are fixed at mq_index_new), and the spec pairs
    // its parameters can select (case folding may change between launches, so a spec and its fold-case twin both count)
    std::vector<MapPair> pairs = {map_pair_of(idx, true), MAP_KERNELS[idx->dp.variant != 0][0][idx->chain_chunk == 4]};
    if (specs_allowed(idx))
        for (const MapSpec &s : MAP_SPECS)
            if (spec_matches(s, idx->dp, true)) pairs.push_back(s.pair);
    for (const MapPair &kp : pairs)
        for (const MapFn fn : {kp.map, kp.declined}) {
            if ((rc = occ_of((const void *)fn, 64 * MAP_WAVES, occ))) return rc;
            occ_min = std::min(occ_min, occ);
        }
    idx->grid_fused = (uint32_t)(occ_min * idx->n_cu);
    if ((rc = occ_of((const void *)seed_reads_kernel<0>, 64 * SEED_WAVES, occ))) return rc;
    idx->grid_seed = (uint32_t)(occ * idx->n_cu);
    if ((rc = occ_of((const void *)map_lists_kernel<64, false>, 64 * ML_WAVES, occ))) return rc;
    idx->grid_map = (uint32_t)(occ * idx->n_cu);
    // Match runs per read held in HBM scratch; a read with more runs is reported MQ_HIT_OVERFLOW (never silently wrong)
    idx->cap_matches = (uint32_t)env_int("MQ_MATCH_CAP", 2048);
    if (idx->cap_matches < 1) idx->cap_matches = 1;
    return MQ_OK;
}

// workgroups of the fused launch sequence for n reads (ensure_geometry must have succeeded)
static uint32_t fused_grid(const mq_index *idx, uint32_t n) { return std::min<uint32_t>(idx->grid_fused, (n + MAP_WAVES - 1) / MAP_WAVES); }

// workgroups (of 4 waves) of a record scanner's tile-walking kernels: a wave per 16-KB tile, at most 8 workgroups per CU
static uint32_t fx_grid(const mq_index *idx, uint32_t n_tiles) { return std::max<uint32_t>(1, std::min<uint32_t>((n_tiles + 3) / 4, (uint32_t)idx->n_cu * 8u)); }

static int ensure_geometry(mq_index *idx) {
    std::call_once(idx->geometry_once, [idx] { idx->geometry_rc = ensure_geometry_once(idx); });  // contexts of one index start concurrently
    return idx->geometry_rc;
}

// ... of a context that reserves anchors or chains: the index's three output pairs (its seeding variant and chain chunk are fixed at
// mq_index_new) join the occupancy minimum -- for the launches of such contexts only, in a second grid
static int ensure_outputs_geometry(mq_index *idx) {
    int rc = ensure_geometry(idx);
    if (rc) return rc;
    std::call_once(idx->outputs_geometry_once, [idx] {
        int occ = 0, occ_min = INT_MAX;
        for (const MapPair *kp : {&map_pair_of(idx, false, nullptr, true, false), &map_pair_of(idx, false, nullptr, false, true), &map_pair_of(idx, false, nullptr, true, true)})
            for (const MapFn fn : {kp->map, kp->declined}) {
                if ((idx->outputs_geometry_rc = occ_of((const void *)fn, 64 * MAP_WAVES, occ))) return;
                occ_min = std::min(occ_min, occ);
            }
        idx->grid_fused_outputs = std::min(idx->grid_fused, (uint32_t)(occ_min * idx->n_cu));
    });
    return idx->outputs_geometry_rc;
}

// records of a chain window beside a Match window of `cap` records: a read chained from LDS (up to MAP_LDS_RECS records, whatever cap is)
// stages there too
static uint32_t chain_win_cap(uint32_t cap) { return std::max(cap, MAP_LDS_RECS); }
// mapping waves a launch over up to n reads can employ, in either pipeline (ctx_ensure's count for the Match windows)
static size_t map_waves_for(const mq_index *idx, uint32_t n) {
    const size_t max_waves = std::max((size_t)idx->grid_fused * MAP_WAVES, (size_t)idx->grid_map * ML_WAVES);
    const size_t wpw = (size_t)std::max(MAP_WAVES, ML_WAVES);
    return std::min(max_waves, ((size_t)n + wpw - 1) / wpw * wpw + wpw);
}

// list entries reserved per base, in 1/65536: 4 d + 1/512 -- canonical selection keeps 1-(1-d)^2 ~ 2 d of the l-mers, so this
// is at least twice the expected count (2.6 times under homopolymer compression); denser lists take the overflow redo
static uint32_t list_f16(const mq_index *idx) {
    double d = idx->params.density;
    if (!(d > 0)) d = 0;
    double f = 4.0 * d + 1.0 / 512.0;
    if (f > 1.0) f = 1.0;
    const int e = env_int("MQ_LIST_F16", -1);  // test hook: force list-region overflows
    if (e >= 0) return (uint32_t)std::min(65536, e);
    return (uint32_t)std::ceil(f * 65536.0);
}
constexpr uint32_t LIST_SLACK = 64;

static int ctx_ensure(mq_ctx *c, uint32_t n, uint64_t total_bases, uint32_t f16) {
    mq_index *idx = c->idx;
    int rc = ensure_geometry(idx);
    if (rc) return rc;
    if (!c->d_counter && (rc = c->d_counter.alloc(1))) return rc;
    if (!c->ev0) {
        HIPCHK(hipEventCreate(&c->ev0.h));
        HIPCHK(hipEventCreate(&c->ev1.h));
    }
    {
        // Match scratch: one window per mapping wave THIS batch can employ (a launch never has more workgroups than reads / waves per
        // workgroup): a context that only ever sees chunks of a thousand reads does not pay for 4,096 waves' windows (268 MB of fresh
        // device memory, ~8 ms, per context)
        const size_t max_waves = std::max((size_t)idx->grid_fused * MAP_WAVES, (size_t)idx->grid_map * ML_WAVES);
        const size_t want = map_waves_for(idx, n);  // (the chain windows of a chains reservation are counted by the same function)
        if (want > c->scratch_waves) {
            c->scratch_waves = 0;
            const size_t nw = std::min(max_waves, want + want / 4);
            if ((rc = c->scratch.alloc(nw * idx->cap_matches))) return rc;
            c->scratch_waves = nw;
        }
    }
    // a group shares one capacity: all of it goes before any of it comes back, and a failure leaves the group empty
    if (n > c->reads_cap) {
        c->reads_cap = 0;
        reset_all(c->mz_count, c->mz_base, c->queue, c->work);
        const uint64_t nc = (uint64_t)n + n / 4 + 64;
        if ((rc = c->mz_count.alloc(nc)) || (rc = c->mz_base.alloc(nc)) || (rc = c->queue.alloc(nc)) || (rc = c->work.alloc(nc + WORK_FRONT_CAP))) {
            reset_all(c->mz_count, c->mz_base, c->queue, c->work);
            return rc;
        }
        c->reads_cap = nc;
    }
    // regular regions, then the pool for lists denser than their region (an eighth of the regular space, at least 1 M entries)
    const uint64_t regular = ((total_bases * f16) >> 16) + (uint64_t)LIST_SLACK * n + 64;
    const uint64_t pool = f16 >= 65536u ? 0 : std::max<uint64_t>(regular / 8, 1ull << 20);
    const uint64_t need = regular + pool;
    c->pool_base = regular;
    c->pool_cap = pool;
    if (need > c->mz_cap) {
        c->mz_cap = 0;
        reset_all(c->mz_hash, c->mz_pos, c->mz_last);
        const uint64_t nc = need + need / 8;
        if ((rc = c->mz_hash.alloc(nc)) || (rc = c->mz_pos.alloc(nc)) || ((idx->dp.variant & MQ_SEEDVAR_END_COMPRESSED) && (rc = c->mz_last.alloc(nc)))) {
            reset_all(c->mz_hash, c->mz_pos, c->mz_last);
            return rc;
        }
        c->mz_cap = nc;
    }
    return MQ_OK;
}

static mq_ctx *ctx_create(mq_index *idx) {
    mq_ctx *c = new (std::nothrow) mq_ctx();
    if (!c) {
        set_err(MQ_ENOMEM, "out of host memory");
        return nullptr;
    }
    c->idx = idx;
    if (hipSetDevice(idx->device) != hipSuccess || hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking) != hipSuccess) {
        set_err(MQ_EHIP, "hipStreamCreate failed");
        c->stream.h = nullptr;
        ctx_release(c);
        return nullptr;
    }
    return c;
}

// ref_map lengths (src/closures.rs:49), dense by ref id: one length per id up to the largest, 0 for an id the map does not have (a
// reference of length 0 cannot own a k-min-mer, so a zero marks a hole)
static uint32_t max_ref_id(const RefMap &refs) { return refs.empty() ? 0 : refs.rbegin()->first; }
static std::vector<uint64_t> dense_ref_lens(const RefMap &refs) {
    std::vector<uint64_t> lens((size_t)max_ref_id(refs) + 1, 0);
    for (auto &kv : refs) lens[kv.first] = kv.second.second;
    return lens;
}
static int upload_ref_lens(const RefMap &refs, Buf<uint64_t> &d_lens) {
    const std::vector<uint64_t> lens = dense_ref_lens(refs);
    int rc = d_lens.alloc(lens.size());
    if (rc) return rc;
    HIPCHK(hipMemcpy(d_lens, lens.data(), lens.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
    return MQ_OK;
}
static int upload_ref_lens(mq_index *idx) { return upload_ref_lens(idx->refs, idx->d_ref_lens); }

static void free_build_scratch(mq_index *idx) {
    idx->stage.reset();
    idx->bld = BuildScratch();
}
