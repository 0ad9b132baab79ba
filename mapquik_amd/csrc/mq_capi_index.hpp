// mq_capi_index.hpp -- C ABI, index side: mq_index_new .. mq_index_finalize (Index::new, ref_extract + add_with_mer, get_count +
// into_read_only; src/index.rs:78-116, src/mers.rs:15-38), reopen / resize, and what an index says of itself (statistics, parameters,
// reference info) and takes for mapping time (mq_index_set_map_params) (part of the one translation unit mq_capi.hip).  Every entry point that can
// throw runs inside guarded(); what a function allocates for itself is a Buf or a Scoped handle, so every early return gives it back.
#pragma once

using IndexPtr = std::unique_ptr<mq_index>;  // a half-built or refused index goes through ~mq_index, like one the caller frees

static int check_params(const mq_params *params) {
    if (!params) return set_err(MQ_EINVAL, "params is NULL");
    if (params->l < 1 || params->l > MAX_L || params->k < 1 || params->k > MAX_K) return set_err(MQ_EINVAL, "unsupported k/l: need 1 <= l <= 64 and 1 <= k <= 32");
    if (params->flags & ~(MQ_FLAG_FOLD_CASE | MQ_FLAG_FAST_KH | MQ_FLAG_SEED_VARIANT_MASK)) return set_err(MQ_EINVAL, "undefined bits in mq_params.flags");
    const uint32_t variant = (params->flags & MQ_FLAG_SEED_VARIANT_MASK) >> MQ_FLAG_SEED_VARIANT_SHIFT;
    if ((variant & MQ_SEEDVAR_POS_RUN_END) && params->l < 2)
        return set_err(MQ_EINVAL, "seeding variant 8 (position = end of the homopolymer run) needs l >= 2: the run's end is read off the window's second base");
    return MQ_OK;
}

extern "C" {

mq_index *mq_index_new(const mq_params *params, int device) {
    return guarded([&]() -> mq_index * {
        if (check_params(params) != MQ_OK) return nullptr;
        const bool init_timing = env_set("MQ_DRIVER_TIMING");  // diagnostic (stderr): where the first index's start-up time goes
        const auto ti0 = std::chrono::steady_clock::now();
        auto stamp = [&](const char *what) {
            if (init_timing) fprintf(stderr, "    mq_index_new: +%.3f s %s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - ti0).count(), what);
        };
        int n = mq_device_count();
        stamp("hipGetDeviceCount (runtime initialised)");
        if (n <= 0) {
            set_err(MQ_ENODEVICE, "no HIP device: the mapquik HIP path has no CPU fallback");
            return nullptr;
        }
        if (device < 0 || device >= n) {
            set_err(MQ_EINVAL, "device ordinal out of range");
            return nullptr;
        }
        IndexPtr idx(new mq_index());
        idx->params = *params;
        idx->device = device;
        if (env_int("MQ_CHAIN_CHUNK", 64) == 4) idx->chain_chunk = 4;
        idx->no_spec = env_int("MQ_NO_SPEC", 0) != 0;
        set_dev_params(idx.get(), dev_params_from(*params, (params->flags & MQ_FLAG_SEED_VARIANT_MASK) >> MQ_FLAG_SEED_VARIANT_SHIFT));
        idx->force_general = env_int("MQ_FORCE_GENERAL", 0) != 0;
        idx->heavy_first = env_int("MQ_HEAVY_FIRST", 1) != 0;
        const char *pl = getenv("MQ_PIPELINE");
        idx->split = pl && strcmp(pl, "split") == 0;
        hipDeviceProp_t prop;
        if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
            set_err(MQ_EHIP, "hipSetDevice/hipGetDeviceProperties failed");
            return nullptr;
        }
        idx->n_cu = prop.multiProcessorCount;
        stamp("hipSetDevice + hipGetDeviceProperties");
        // an empty one-bucket table so that seeding-only calls work before finalize
        if (alloc_table(idx.get(), 2) != MQ_OK) return nullptr;
        stamp("first hipMalloc + hipMemset (code objects loaded)");
        idx->def_ctx.reset(ctx_create(idx.get()));
        stamp("stream created");
        if (!idx->def_ctx) return nullptr;
        return idx.release();
    });
}

void mq_index_free(mq_index *idx) { delete idx; }

}  // extern "C"

// ---- mq_index_add_ref_device in steps (all on the null stream: the next call's kernels, and finalize, are ordered behind them)

// A reopened index whose finalize failed after its first insert launch: the table holds some of the new keys, the counts none of them,
// and inserting the chunks again would turn every new live key dead.  (A fresh build's retry gets a new table; an extension has none.)
static const char *const EXTEND_FAILED = "a finalize of this reopened index failed part way: the table is no longer exact, free the index";
// The same for a merge (mq_index_merge*, mq_capi_index_io.hpp) that failed behind its first insert launch: the only table there is has changed.
static const char *const MERGE_FAILED = "a merge into this index failed part way: the table is no longer exact, free the index";
static int extend_failed_err(const mq_index *idx) { return set_err(MQ_ESTATE, idx->merge_failed ? MERGE_FAILED : EXTEND_FAILED); }

// what every mq_index_add_ref* refuses before anything is registered or overwritten
static int check_new_ref(const mq_index *idx, uint32_t ref_id, uint64_t len) {
    if (idx->finalized) return set_err(MQ_ESTATE, "index already finalized");
    if (idx->extend_failed) return extend_failed_err(idx);
    if (len >= (1ull << 32)) return set_err(MQ_EINVAL, "sequence length must be < 2^32");
    if (ref_id >= MQ_MAX_REF_ID) return set_err(MQ_EINVAL, "ref_id must be < 2^24 (reference lengths are kept in a dense device array)");
    if (idx->refs.count(ref_id)) return set_err(MQ_EINVAL, "duplicate ref_id");
    return MQ_OK;
}

static uint32_t *dense_last_of(mq_index *idx) { return (idx->dp.variant & MQ_SEEDVAR_END_COMPRESSED) ? idx->bld.dense_last.p : nullptr; }

// the scratch of the seeders sized for this sequence (and cleared where they count), and their arguments
static int plan_ref_seed(mq_index *idx, const uint8_t *d_seq, uint64_t len, RefSeedArgs *A) {
    BuildScratch &b = idx->bld;
    const bool with_last = (idx->dp.variant & MQ_SEEDVAR_END_COMPRESSED) != 0;
    const uint32_t n_seg = (uint32_t)((len + REF_SEG - 1) / REF_SEG);
    // expected minimizers per segment: 2 * density of the compressed l-mers; cap with slack, worst case on retry
    double dens = idx->params.density;
    if (!(dens > 0)) dens = 0;
    if (dens > 1) dens = 1;
    uint32_t cap = (uint32_t)std::min<double>((double)REF_SEG, 3.0 * 2.0 * dens * (double)REF_SEG + 256.0);
    if (env_set("MQ_REF_CAP")) cap = (uint32_t)std::max(1, env_int("MQ_REF_CAP", 1));  // test hook: tiny regions, so that segments take the redo path
    int rc;
    if ((rc = b.counts.ensure(n_seg))) return rc;
    if ((rc = b.queue.ensure(n_seg))) return rc;
    if ((rc = b.seg_off.ensure((uint64_t)n_seg + 1))) return rc;
    if (!b.info && (rc = b.info.alloc(1))) return rc;
    if (!idx->grid_ref) {
        int occ = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)seed_ref_kernel, 64 * SEED_WAVES, 0));
        idx->grid_ref = std::max(1, occ) * idx->n_cu;
    }
    if ((rc = b.seg_hash.ensure((uint64_t)n_seg * cap))) return rc;
    if ((rc = b.seg_pos.ensure((uint64_t)n_seg * cap))) return rc;
    if (with_last && (rc = b.seg_last.ensure((uint64_t)n_seg * cap))) return rc;
    HIPCHK(hipMemsetAsync(b.info, 0, sizeof(RefBuildInfo), 0));
    *A = RefSeedArgs{d_seq, len, n_seg, idx->dp, b.seg_hash, b.seg_pos, with_last ? b.seg_last.p : nullptr, cap, b.counts, b.queue,
                     &b.info.p->work, idx->force_general ? 1u : 0u};
    return MQ_OK;
}

// the fast seeder, the general one for the segments it declined, the scan of the counts; *n_mz: minimizers of the sequence, *n_over:
// segments whose list outgrew its region
static int seed_ref_segments(mq_index *idx, const RefSeedArgs &A, uint64_t *n_mz, uint32_t *n_over) {
    BuildScratch &b = idx->bld;
    int rc;
    if ((rc = launch(seed_ref_kernel, std::min<uint32_t>((uint32_t)idx->grid_ref, (A.n_seg + SEED_WAVES - 1) / SEED_WAVES), 64 * SEED_WAVES, 0, A))) return rc;
    // the queue's length lives on the device: a fixed grid, waves that find the queue empty leave at once
    if ((rc = launch(seed_ref_general_kernel, std::min<uint32_t>((uint32_t)idx->n_cu * 32u, A.n_seg), 64, 0, A))) return rc;
    // (the fast seeder's queue is consumed by now: the same array takes the numbers of the segments whose list outgrew its region)
    if ((rc = launch(scan_counts_kernel, 1, 1024, 0, b.counts, A.n_seg, A.cap, b.seg_off, &b.info.p->total, b.queue))) return rc;
    RefBuildInfo h = {};  // total and overflowed: what lies in front of the seeders' cursors
    HIPCHK(hipMemcpy(&h, b.info, offsetof(RefBuildInfo, work), hipMemcpyDeviceToHost));
    *n_mz = h.total;
    *n_over = (uint32_t)h.overflowed;
    return MQ_OK;
}

// the segments' lists into the sequence's dense list; the segments that overflowed seeded again, straight into their place in it
static int compact_and_redo(mq_index *idx, const RefSeedArgs &A, uint64_t n_mz, uint32_t n_over) {
    BuildScratch &b = idx->bld;
    int rc;
    if ((rc = b.dense_hash.ensure(n_mz))) return rc;
    if ((rc = b.dense_pos.ensure(n_mz))) return rc;
    if (A.seg_last && (rc = b.dense_last.ensure(n_mz))) return rc;
    if ((rc = launch(compact_lists_kernel, std::min<uint32_t>(A.n_seg, 65535u), 64, 0, b.seg_hash, b.seg_pos, A.cap, b.counts, b.seg_off, A.n_seg, b.dense_hash, b.dense_pos,
                     A.seg_last, dense_last_of(idx))))
        return rc;
    if (!n_over) return MQ_OK;
    return launch(seed_ref_redo_kernel, std::min<uint32_t>(n_over, (uint32_t)idx->n_cu * 32u), 64, 0, A, b.queue, n_over, b.seg_off, b.dense_hash, b.dense_pos, dense_last_of(idx));
}

// the reference's k-min-mers go behind those of the previous references in the current chunk while it has room
static int append_kminmers(mq_index *idx, uint32_t ref_id, uint64_t n_mz, uint64_t n_kmm) {
    int rc;
    if (idx->chunks.empty() || idx->chunks.back().n + n_kmm > idx->chunks.back().d.cap) {
        KmmChunk ch;
        if ((rc = ch.d.alloc(std::max<uint64_t>(n_kmm, 16ull << 20)))) return rc;
        idx->chunks.push_back(std::move(ch));
    }
    KmmChunk &ch = idx->chunks.back();
    const uint32_t kb = (uint32_t)std::min<uint64_t>((n_kmm + 255) / 256, 65535ull);
    if ((rc = launch(ref_kminmers_kernel, kb, 256, 0, idx->bld.dense_hash, idx->bld.dense_pos, n_mz, idx->dp, ref_id, ch.d + ch.n, dense_last_of(idx)))) return rc;
    ch.n += n_kmm;
    idx->n_kmm_total += n_kmm;
    return MQ_OK;
}

static int64_t add_ref_device_locked(mq_index *idx, uint32_t ref_id, const char *name, const uint8_t *d_seq, uint64_t len) {
    if (!idx || (!d_seq && len)) return set_err(MQ_EINVAL, "bad arguments");
    int rc = check_new_ref(idx, ref_id, len);
    if (rc) return rc;
    if ((rc = use_device(idx))) return rc;
    idx->refs[ref_id] = std::make_pair(std::string(name ? name : ""), len);
    const DevParams &P = idx->dp;
    if (len < (uint64_t)P.l + P.k - 1) return 0;  // src/mers.rs:18
    if (P.keep_none) return 0;                    // (seeding variant 1 with a bound of 0: no l-mer passes `hash < 0`)
    RefSeedArgs A;
    uint64_t n_mz = 0;
    uint32_t n_over = 0;
    if ((rc = plan_ref_seed(idx, d_seq, len, &A))) return rc;
    if ((rc = seed_ref_segments(idx, A, &n_mz, &n_over))) return rc;
    if (n_mz < P.k) return 0;
    const uint64_t n_kmm = n_mz - P.k + 1;
    if ((rc = compact_and_redo(idx, A, n_mz, n_over))) return rc;
    if ((rc = append_kminmers(idx, ref_id, n_mz, n_kmm))) return rc;
    return (int64_t)n_kmm;
}

extern "C" {

int64_t mq_index_add_ref_device(mq_index *idx, uint32_t ref_id, const char *name, const uint8_t *d_seq, uint64_t len) {
    return guarded([&]() -> int64_t {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (!env_set("MQ_BUILD_TIMING")) return add_ref_device_locked(idx, ref_id, name, d_seq, len);
        hipDeviceSynchronize();
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t r = add_ref_device_locked(idx, ref_id, name, d_seq, len);
        hipDeviceSynchronize();
        idx->t_add_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return r;
    });
}

int64_t mq_index_add_ref(mq_index *idx, uint32_t ref_id, const char *name, const uint8_t *seq, uint64_t len) {
    return guarded([&]() -> int64_t {
        if (!idx || (!seq && len)) return set_err(MQ_EINVAL, "bad arguments");
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = use_device(idx);
        if (rc) return rc;
        if (len >= (1ull << 32)) return set_err(MQ_EINVAL, "sequence length must be < 2^32");
        if ((rc = idx->bld.seq.ensure(len + 64))) return rc;
        if (len) HIPCHK(hipMemcpy(idx->bld.seq, seq, len, hipMemcpyHostToDevice));
        return add_ref_device_locked(idx, ref_id, name, idx->bld.seq, len);
    });
}

// ---- the reference file straight from file pieces (the batch form of src/closures.rs:46-94's reader loop for a caller that never holds
// a whole record in host memory): pieces of the file go to a device buffer of the file's size asynchronously, on a stream of their own,
// and a record is indexed from there (add_ref_device_locked on the null stream, made to wait for the pieces issued so far) while the
// pieces behind it are still on their way.  A human reference is 3.1 GB in 25 records: copied record by record from pageable memory
// it took 0.24 s of the driver's 0.31-s reference phase; streamed from page-locked 16-MB pieces it is the PCIe link's 0.07 s, hidden
// behind the file read.
int mq_index_stage_begin(mq_index *idx, uint64_t total_bytes) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        if (idx->finalized) return set_err(MQ_ESTATE, "index already finalized");
        int rc = use_device(idx);
        if (rc) return rc;
        return idx->stage.begin(total_bytes);
    });
}

int mq_index_stage_piece(mq_index *idx, uint64_t at, const uint8_t *src, uint64_t n, uint64_t *ticket) {
    return guarded([&]() -> int {
        if (!idx || (!src && n) || !ticket) return set_err(MQ_EINVAL, "bad arguments");
        int rc = use_device(idx);
        if (rc) return rc;
        return idx->stage.piece(at, src, n, ticket);
    });
}

int mq_index_stage_done(mq_index *idx, uint64_t ticket, int wait) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        int rc = use_device(idx);
        if (rc) return rc;
        return idx->stage.done(ticket, wait);
    });
}

int64_t mq_index_add_ref_staged(mq_index *idx, uint32_t ref_id, const char *name, uint64_t at, uint64_t len, uint64_t after_ticket) {
    return guarded([&]() -> int64_t {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        int rc = use_device(idx);
        if (rc) return rc;
        const uint8_t *d_seq = nullptr;
        if ((rc = idx->stage.region("mq_index_add_ref_staged", at, len, after_ticket, &d_seq))) return rc;
        std::lock_guard<std::mutex> lk(idx->mu);
        return add_ref_device_locked(idx, ref_id, name, d_seq, len);
    });
}

// ---- records whose sequence is spread over lines (every genome FASTA of an archive is wrapped at 60-80 columns): the region between
// the header's line end and the next record's '>' is joined on the device (mq_join.hpp) into bld.seq -- not in place: tiles of one launch
// would race, and the staging buffer still holds the header of the next record -- and indexed from there.

// The lines of d_region[0, bytes) joined into bld.seq, on the null stream (behind the previous record's build kernels, which read
// bld.seq); *joined: the joined length, read back once the last kernel is queued.  d_region lies `at` bytes into the staging buffer,
// whose base is 16-byte aligned and which has 64 bytes of slack behind it.
static int join_lines_locked(mq_index *idx, const uint8_t *d_region, uint64_t at, uint64_t bytes, uint64_t *joined) {
    int rc;
    *joined = 0;
    if ((rc = idx->bld.seq.ensure(bytes + 64))) return rc;
    if (!bytes) return MQ_OK;
    const uint8_t *base = d_region - at;
    const uint64_t begin = at, end = at + bytes;
    const uint64_t tiles = (end - (begin & ~15ull) + FX_TILE - 1) / FX_TILE;
    if (tiles >= (1ull << 32)) return set_err(MQ_EINVAL, "region too large");
    const uint32_t n_tiles = (uint32_t)tiles;
    if ((rc = idx->bld.join_counts.ensure(n_tiles))) return rc;
    if ((rc = idx->bld.join_off.ensure(n_tiles))) return rc;
    if (!idx->bld.join_total && (rc = idx->bld.join_total.alloc(1))) return rc;
    const uint32_t grid = fx_grid(idx, n_tiles);
    if ((rc = launch(join_count_kernel, grid, 256, 0, base, begin, end, n_tiles, idx->bld.join_counts))) return rc;
    if ((rc = launch(join_scan_kernel, 1, 1024, 0, idx->bld.join_counts, n_tiles, idx->bld.join_off, idx->bld.join_total))) return rc;
    if ((rc = launch(join_write_kernel, grid, 256, 0, base, begin, end, n_tiles, idx->bld.join_off, idx->bld.seq))) return rc;
    unsigned long long total = 0;
    HIPCHK(hipMemcpy(&total, idx->bld.join_total, 8, hipMemcpyDeviceToHost));
    *joined = total;
    return MQ_OK;
}

int64_t mq_index_add_ref_staged_lines(mq_index *idx, uint32_t ref_id, const char *name, uint64_t at, uint64_t bytes, uint64_t after_ticket, uint64_t *seq_len) {
    return guarded([&]() -> int64_t {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        int rc = use_device(idx);
        if (rc) return rc;
        const uint8_t *d_region = nullptr;
        if ((rc = idx->stage.region("mq_index_add_ref_staged_lines", at, bytes, after_ticket, &d_region))) return rc;
        std::lock_guard<std::mutex> lk(idx->mu);
        if ((rc = check_new_ref(idx, ref_id, 0))) return rc;  // before the join overwrites bld.seq (the joined length is not known yet)
        uint64_t joined = 0;
        if ((rc = join_lines_locked(idx, d_region, at, bytes, &joined))) return rc;
        if (joined >= (1ull << 32)) return set_err(MQ_EINVAL, "sequence length must be < 2^32");
        if (seq_len) *seq_len = joined;
        return add_ref_device_locked(idx, ref_id, name, idx->bld.seq, joined);
    });
}

int64_t mq_index_staged_sequence(mq_index *idx, uint64_t at, uint64_t bytes, uint64_t after_ticket, uint8_t *out, uint64_t cap) {
    return guarded([&]() -> int64_t {
        if (!idx || (!out && cap)) return set_err(MQ_EINVAL, "bad arguments");
        int rc = use_device(idx);
        if (rc) return rc;
        const uint8_t *d_region = nullptr;
        if ((rc = idx->stage.region("mq_index_staged_sequence", at, bytes, after_ticket, &d_region))) return rc;
        std::lock_guard<std::mutex> lk(idx->mu);
        if (idx->finalized) return set_err(MQ_ESTATE, "index already finalized");
        uint64_t joined = 0;
        if ((rc = join_lines_locked(idx, d_region, at, bytes, &joined))) return rc;
        if (joined > (uint64_t)INT64_MAX) return set_err(MQ_EINVAL, "region too large");
        if (!out) return (int64_t)joined;  // (cap == 0: the length alone)
        if (joined > cap) return set_err(MQ_EINVAL, "mq_index_staged_sequence: the joined sequence is longer than cap");
        if (joined) HIPCHK(hipMemcpy(out, idx->bld.seq, joined, hipMemcpyDeviceToHost));
        return (int64_t)joined;
    });
}

}  // extern "C"

// The index's table at another size (mq_index_resize; a reopened index that outgrew it): a cleared table of nslots slots, retable_kernel
// from the old one into it, and the old one freed -- once the new one holds what the index says it holds; until then the index is as it
// was.  Peak device memory: both tables.  Everything runs on the null stream, behind the clearing; the counters' read-back is the wait.
static int retable(mq_index *idx, uint64_t nslots) {
    Buf<Bucket> table;
    Buf<unsigned long long> d_acc;
    int rc;
    if ((rc = new_table(table, nslots)) || (rc = d_acc.alloc(2))) return rc;
    HIPCHK(hipMemsetAsync(d_acc, 0, 16, 0));
    const uint64_t nb1 = idx->nslots / 2 + 1;
    if ((rc = launch(retable_kernel, ahead_grid(2 * nb1), 256, 0, idx->table, nb1, table, nslots - 1, d_acc))) return rc;
    unsigned long long acc[2] = {0, 0};
    HIPCHK(hipMemcpy(acc, d_acc, 16, hipMemcpyDeviceToHost));
    if (acc[0] != idx->n_keys || acc[0] - acc[1] != idx->n_unique)
        return set_err(MQ_ESTATE, "the table holds other keys than the index records (internal error): the table keeps its size");
    idx->table = std::move(table);
    idx->nslots = nslots;
    return MQ_OK;
}

extern "C" {

// Slots of the table per inserted k-min-mer (rounded up to a power of two of slots).  The default, 8 (load <= 1/8: 17 GB for a human
// genome), is for a kernel fed from HBM: 1130 Gbases/s against 1114 / 1074 at 4 / 2.  A caller that feeds from files is bound by its
// host side at a thirtieth of that and does better with 2: a quarter of the memory per replica, of the device-to-device copy per clone,
// and of the allocation (fresh device memory can cost 30 ms per GB here) -- the native driver's default.
int mq_index_set_table_factor(mq_index *idx, uint32_t slots_per_kminmer) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        if (slots_per_kminmer < 2 || slots_per_kminmer > 64) return set_err(MQ_EINVAL, "slots per k-min-mer: 2..64");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (idx->finalized || idx->rsv.made()) return set_err(MQ_ESTATE, "mq_index_set_table_factor: before mq_index_reserve / mq_index_finalize");
        idx->table_factor = slots_per_kminmer;
        return MQ_OK;
    });
}

// DashMap::with_capacity at Index::new (src/index.rs:83 sizes the map for 39,821,990 k-min-mers before the first insert): the table
// for `expected_kminmers` inserted k-min-mers is allocated and cleared by a thread of its own, while the caller reads, uploads and
// seeds the reference -- fresh device memory costs ~30 ms per GB on this platform (tools/alloc_probe.hip: 485 ms for the 17 GB table
// of a human genome), more than every kernel of the build together.  A hint only: mq_index_finalize allocates again when the
// reference turns out to need another size.
int mq_index_reserve(mq_index *idx, uint64_t expected_kminmers) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (idx->finalized) return set_err(MQ_ESTATE, "index already finalized");
        if (idx->rsv.made()) return MQ_OK;  // one reservation per index
        idx->rsv.start(idx->device, table_slots_for(idx, expected_kminmers));
        return MQ_OK;
    });
}

int64_t mq_index_finalize(mq_index *idx) {
    return guarded([&]() -> int64_t {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (idx->finalized) return (int64_t)idx->n_unique;
        if (idx->extend_failed) return extend_failed_err(idx);
        int rc = use_device(idx);
        if (rc) return rc;
        const bool timing = env_set("MQ_BUILD_TIMING");  // diagnostic: where the wall time of finalize goes (stderr)
        auto tnow = [&]() {
            if (timing) hipDeviceSynchronize();
            return std::chrono::steady_clock::now();
        };
        auto t_0 = tnow();
        // slots per inserted k-min-mer (power-of-two rounding on top); default 8 => load <= 0.125 (17 GB for a human genome, 6 % of
        // the HBM).  ~85 % of a read's lookups miss, a miss walks to the first empty slot, and every extra step is one more dependent
        // random access of a memory system that sustains ~52 G of them per second (tools/probe_rate.py).  Measured on the CHM13-like
        // bench: factor 2: 926, 4: 1000, 8: 1034, 16: 1044, 32: 1051 Gbases/s.
        uint64_t nslots = table_slots_for(idx, idx->n_kmm_total);
        if (idx->extending) {
            // a reopened index: the table holds the earlier references' keys and only the new chunks are inserted -- table_insert does
            // not care in which order, or in how many launches, the k-min-mers of all references arrive.  It grows first when all of
            // them together ask for a larger table than it has, and never shrinks.  (A reservation made while it was open is not used.)
            (void)idx->rsv.take(0);
            if (nslots > idx->nslots) {
                if ((rc = retable(idx, nslots))) return rc;
            } else {
                nslots = idx->nslots;
            }
        } else if (Buf<Bucket> reserved = idx->rsv.take(nslots)) {  // the table mq_index_reserve allocated and cleared
            idx->table = std::move(reserved);
            idx->nslots = nslots;
            idx->table_alloc_ms = idx->rsv.ms;
        } else if ((rc = alloc_table(idx, nslots))) {  // no reservation, or the estimate was off: allocated now, at the size the reference needs
            return rc;
        }
        auto t_1 = tnow();
        Buf<unsigned long long> d_acc;
        if ((rc = d_acc.alloc(3))) return rc;
        HIPCHK(hipMemset(d_acc, 0, 24));
        // (until here a failure leaves a reopened index as it was, open, with its chunks: finalize may be called again.  From the first
        // insert launch to the end it may not: see EXTEND_FAILED)
        idx->extend_failed = idx->extending;
        for (auto &c : idx->chunks) {
            if (!c.n) continue;
            const uint32_t nb = (uint32_t)std::min<uint64_t>((c.n + 255) / 256, 1u << 20);
            if ((rc = launch(insert_kernel, nb, 256, 0, c.d, c.n, idx->table, nslots - 1, d_acc))) return rc;
        }
        auto t_2 = tnow();
        // Index::get_count (src/index.rs:90-92): keys claimed minus keys that turned dead, counted by the insertions themselves.  On top
        // of an earlier finalize's counts: a new reference that repeats an old live key claims nothing and turns one dead.
        unsigned long long acc[3] = {0, 0, 0};
        HIPCHK(hipMemcpy(acc, d_acc, 24, hipMemcpyDeviceToHost));
        d_acc.reset();
        if (!idx->extending) idx->n_keys = idx->n_unique = 0;
        idx->n_keys += acc[0];
        idx->n_unique += acc[0] - acc[1];
        auto t_3 = tnow();
        idx->chunks.clear();
        free_build_scratch(idx);
        if (timing) {
            auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
            fprintf(stderr, "mq_index_add_ref_device calls so far: %.2f ms\n", idx->t_add_ms);
            fprintf(stderr, "mq_index_finalize: table alloc + clear %.2f ms (%.1f GB), insert %.2f ms (%llu k-min-mers), read back %.2f ms, free scratch %.2f ms\n", ms(t_0, t_1),
                    table_bytes_of(nslots) / 1e9, ms(t_1, t_2), (unsigned long long)idx->n_kmm_total, ms(t_2, t_3), ms(t_3, tnow()));
        }
        if ((rc = upload_ref_lens(idx))) return rc;
        idx->finalized = true;
        idx->extending = idx->extend_failed = false;
        return (int64_t)idx->n_unique;
    });
}

// A finalized index opened again for mq_index_add_ref*: see mq_index_finalize.  The device is idle when this returns, so no launch queued
// on any context reads the table while it changes; until the next finalize the mapping entry points answer MQ_ESTATE.
int mq_index_reopen(mq_index *idx) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (!idx->finalized) return set_err(MQ_ESTATE, "mq_index_reopen: index not finalized");
        int rc = use_device(idx);
        if (rc) return rc;
        HIPCHK(hipDeviceSynchronize());
        idx->cov.drop();  // (a coverage result describes the table as it was)
        idx->finalized = false;
        idx->extending = true;
        return MQ_OK;
    });
}

int mq_index_resize(mq_index *idx, uint64_t table_slots, uint32_t slots_per_kminmer) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
        uint64_t nslots = 0;
        int rc = sized_table_slots(table_slots, slots_per_kminmer, idx->n_kmm_total, idx->n_keys, &nslots);
        if (rc) return rc;
        idx->cov.drop();  // (every accepted resize lets a coverage result go, the one that leaves the table as it is included)
        if (!nslots || nslots == idx->nslots) return MQ_OK;
        if ((rc = use_device(idx))) return rc;
        HIPCHK(hipDeviceSynchronize());  // launches queued on the contexts read the table that is about to go
        return retable(idx, nslots);
    });
}

int mq_index_get_stats(const mq_index *idx, mq_index_stats *out) {
    return guarded([&]() -> int {
        if (!idx || !out) return set_err(MQ_EINVAL, "bad arguments");
        out->n_refs = idx->refs.size();
        out->n_kminmers = idx->n_kmm_total;
        out->n_keys = idx->n_keys;
        out->n_unique = idx->n_unique;
        out->table_slots = idx->nslots;
        out->table_bytes = table_bytes_of(idx->nslots);
        out->slot_bytes = SLOT_BYTES;
        return MQ_OK;
    });
}

// The parameters an index was built with (what a loaded file says: k, l, density, use_hpc and the seeding variant decide its keys).
int mq_index_get_params(const mq_index *idx, mq_params *out) {
    return guarded([&]() -> int {
        if (!idx || !out) return set_err(MQ_EINVAL, "bad arguments");
        *out = idx->params;
        return MQ_OK;
    });
}

// The parameters that act at mapping time only (Params.c / .s in Chain::get_match src/chain.rs:147-169, .g in the gap tests
// src/chain.rs:132-142, and the feeder's case folding): a loaded index takes the command line's.  Launches queued before the call keep
// the old values.
int mq_index_set_map_params(mq_index *idx, uint32_t c, uint32_t s, uint32_t g, int fold_case) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        idx->params.c = c;
        idx->params.s = s;
        idx->params.g = g;
        idx->params.flags = (idx->params.flags & ~MQ_FLAG_FOLD_CASE) | (fold_case ? MQ_FLAG_FOLD_CASE : 0u);
        set_dev_params(idx, dev_params_from(idx->params, idx->dp.variant));
        return MQ_OK;
    });
}

int mq_index_ref_info(const mq_index *idx, uint32_t ref_id, const char **name, uint64_t *len) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        auto it = idx->refs.find(ref_id);
        if (it == idx->refs.end()) return set_err(MQ_EINVAL, "unknown ref_id");
        if (name) *name = it->second.first.c_str();
        if (len) *len = it->second.second;
        return MQ_OK;
    });
}

}  // extern "C"
