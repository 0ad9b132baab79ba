// mq_capi_index_io.hpp -- C ABI: what moves a finalized index's slots -- the on-disk index (mq_index_save / mq_index_load[_sized]), replicas
// (mq_index_clone[_sized]) and merges (mq_index_merge / mq_index_merge_file) (part of the one translation unit mq_capi.hip).  One header and
// one reference-table codec, one chunk arithmetic (IxChunks), one file-to-device slot streamer (stream_file_slots), one pack + peer copy
// (packed_slots_on), one checked scatter (SlotScatter).  Two failure conventions, one per layer: a step that parses the file returns
// nullptr or the text (the path follows it) with which the file is refused; a step that touches HIP returns an error code, set_err called.
#pragma once

// On-disk index (the reference has none and rebuilds on every run, src/closures.rs:24-94): header, parameters, reference table,
// then the OCCUPIED slots only (32 bytes each: ~1.5 GB for a human genome instead of the 17 GB table at load 1/8); mq_index_load
// scatters them into a fresh table on the device.  Little-endian, this library's layout (MQ_INDEX_MAGIC names the version).
static const char MQ_INDEX_MAGIC[8] = {'M', 'Q', 'H', 'I', 'P', 'I', 'X', '2'};
struct IxHeader {  // what follows the magic
    mq_params p;
    uint64_t w[6];
};
enum { IX_SLOT_BYTES, IX_NSLOTS, IX_N_KMM, IX_N_KEYS, IX_N_UNIQUE, IX_N_REFS };  // IxHeader::w
static_assert(sizeof(IxHeader) == sizeof(mq_params) + 6 * sizeof(uint64_t), "the header is written and read as one block");

static bool write_all(int fd, const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    while (n) {
        const ssize_t w = ::write(fd, b, n);
        if (w <= 0) return false;
        b += w;
        n -= (size_t)w;
    }
    return true;
}
static bool read_all(int fd, void *p, size_t n) {
    uint8_t *b = (uint8_t *)p;
    while (n) {
        const ssize_t r = ::read(fd, b, n);
        if (r <= 0) return false;
        b += r;
        n -= (size_t)r;
    }
    return true;
}
static bool pread_all(int fd, void *p, size_t n, off_t at) {
    uint8_t *b = (uint8_t *)p;
    while (n) {
        const ssize_t r = ::pread(fd, b, n, at);
        if (r <= 0) return false;
        b += r;
        at += r;
        n -= (size_t)r;
    }
    return true;
}

// ---- the file's parts.  A reader returns nullptr, or the text (the path follows it) with which the file is refused.
static const char *const IX_TRUNCATED = "truncated or unreadable index file: ";
static const char *const IX_BAD_SLOT = "corrupt index file (an entry names a reference the file does not have, or a malformed slot): ";
static const char *const IX_BAD_COUNTS = "corrupt index file (key counts or reference ids disagree with its header): ";
static const char *const IX_BYTES_AFTER = "corrupt index file (bytes after the last slot): ";

static bool write_header(int fd, const mq_index *idx) {
    IxHeader h;
    memcpy(&h.p, &idx->params, sizeof(h.p));  // (the bytes as the index holds them, padding included)
    h.w[IX_SLOT_BYTES] = sizeof(SavedSlot);
    h.w[IX_NSLOTS] = idx->nslots;
    h.w[IX_N_KMM] = idx->n_kmm_total;
    h.w[IX_N_KEYS] = idx->n_keys;
    h.w[IX_N_UNIQUE] = idx->n_unique;
    h.w[IX_N_REFS] = idx->refs.size();
    return write_all(fd, MQ_INDEX_MAGIC, 8) && write_all(fd, &h, sizeof(h));
}
// every refusal that comes from the header alone: before an index or a table exists
static const char *read_header(int fd, IxHeader *h) {
    char magic[8];
    const uint64_t *w = h->w;
    if (!read_all(fd, magic, 8) || memcmp(magic, MQ_INDEX_MAGIC, 8) != 0 || !read_all(fd, h, sizeof(*h)) || w[IX_SLOT_BYTES] != sizeof(SavedSlot) ||
        w[IX_NSLOTS] < 2 || (w[IX_NSLOTS] & (w[IX_NSLOTS] - 1)) != 0 || w[IX_NSLOTS] > (1ull << 40) ||
        w[IX_N_KEYS] >= w[IX_NSLOTS] /* a table without an empty slot would make a miss walk forever */ || w[IX_N_UNIQUE] > w[IX_N_KEYS] || w[IX_N_REFS] > MQ_MAX_REF_ID)
        return "not a mapquik HIP index (or another layout version): ";
    return nullptr;
}

// the reference table: per reference id u32, name length u32, length u64, name
static bool write_refs(int fd, const RefMap &refs) {
    for (auto &kv : refs) {
        const uint32_t id = kv.first, nl = (uint32_t)kv.second.first.size();
        if (!write_all(fd, &id, 4) || !write_all(fd, &nl, 4) || !write_all(fd, &kv.second.second, 8) || (nl && !write_all(fd, kv.second.first.data(), nl))) return false;
    }
    return true;
}
static const char *read_refs(int fd, uint64_t n_refs, RefMap *refs) {
    for (uint64_t i = 0; i < n_refs; ++i) {
        uint32_t id = 0, nl = 0;
        uint64_t len = 0;
        if (!read_all(fd, &id, 4) || !read_all(fd, &nl, 4) || !read_all(fd, &len, 8) || nl >= (1u << 20) || id >= MQ_MAX_REF_ID) return IX_TRUNCATED;
        std::string name(nl, '\0');
        if (nl && !read_all(fd, &name[0], nl)) return IX_TRUNCATED;
        (*refs)[id] = std::make_pair(name, len);
    }
    return nullptr;
}

// The chunks of a slot section (IxChunks, mq_ix_chunks.hpp) at the product's 64 MB per page-locked transfer buffer, for both directions
// (save: device to file; stream_file_slots: file to device).  MQ_IX_IO_CHUNK: test hook, the chunk in bytes, so that files of a few slots
// cross chunk borders.
static IxChunks ix_chunks(size_t total_bytes) { return IxChunks(total_bytes, sizeof(SavedSlot), env_int("MQ_IX_IO_CHUNK", 64 << 20)); }

// threads that are joined when their holder goes: a spawn that fails leaves none running behind the frame they work on
struct JoinedThreads {
    std::vector<std::thread> th;
    void join() {
        for (auto &t : th)
            if (t.joinable()) t.join();
    }
    ~JoinedThreads() { join(); }
};

// What one worker of stream_file_slots owns: a page-locked buffer and a device buffer of a chunk each, and a non-blocking stream.  Made by
// the worker at its first chunk; a caller that streams a file twice keeps them across the passes.  The page-locked buffer is what each
// route always had: mq_host_alloc's (huge pages, registered) for the loader's workers, hipHostMalloc's for mq_index_merge_file's one.
struct SlotLane {
    Scoped<void *, mq_host_free> huge;
    PinnedBuf<uint8_t> plain;
    Buf<uint8_t> d;
    ScopedStream st;
    uint8_t *host() const { return huge.h ? (uint8_t *)huge.h : plain.p; }
    int ensure(size_t bytes, bool huge_pages) {
        if (st) return MQ_OK;
        if (huge_pages && !(huge.h = mq_host_alloc(bytes))) return set_err(MQ_ENOMEM, "no page-locked memory for an index file's slots");
        int rc;
        if ((!huge_pages && (rc = plain.alloc(bytes))) || (rc = d.alloc(bytes))) return rc;
        HIPCHK(hipStreamCreateWithFlags(&st.h, hipStreamNonBlocking));
        return MQ_OK;
    }
};

// THE file-to-device slot streamer: the slot section of an index file (`total` bytes at slots_at), chunk by chunk -- file -> page-locked
// buffer -> device -> per_chunk(device slots, count, stream), the worker's stream waited for before its buffers are used again -- by
// n_workers threads at once, each with a SlotLane that it makes and gives back on its own thread (`kept`, if given, is the first worker's
// instead, and outlives the call).  What per_chunk launches for different chunks runs concurrently, so it meets its neighbours with
// atomics: the file read, not the copy, is what takes time.  The worker streams do not wait for the null stream, so whatever the caller
// prepared there (a cleared or regrown table, zeroed counters, an uploaded length array) is waited for first; when this returns every
// worker's stream has been waited for, so a read-back of what per_chunk counted is in order.  The file position stays.
template <class F>
static int stream_file_slots(int fd, off_t slots_at, size_t total, const char *path, int device, size_t n_workers, bool huge_pages, SlotLane *kept, F per_chunk) {
    const IxChunks ch = ix_chunks(total);
    if (!ch.n) return MQ_OK;
    HIPCHK(hipDeviceSynchronize());
    n_workers = std::min(n_workers, ch.n);
    std::atomic<size_t> next{0};
    std::mutex mu;  // the first failure, with its text (set_err's is the worker thread's own)
    int failed = MQ_OK;
    std::string failed_text;
    auto step = [&](SlotLane &L, size_t c) -> int {
        const size_t n = ch.bytes(c);
        if (!pread_all(fd, L.host(), n, slots_at + (off_t)ch.at(c))) return set_err(MQ_EINVAL, std::string(IX_TRUNCATED) + path);
        HIPCHK(hipMemcpyAsync(L.d, L.host(), n, hipMemcpyHostToDevice, L.st));
        int rc = per_chunk((const SavedSlot *)L.d.p, (uint64_t)(n / sizeof(SavedSlot)), L.st.h);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(L.st));
        return MQ_OK;
    };
    auto work = [&](SlotLane *mine) {
        SlotLane own;  // (a worker without a kept lane: made and given back on its own thread, next to its neighbours')
        SlotLane &L = mine ? *mine : own;
        int rc = hipSetDevice(device) == hipSuccess ? L.ensure(ch.buf_bytes(), huge_pages) : set_err(MQ_EHIP, "hipSetDevice failed");
        for (size_t c; !rc && (c = next.fetch_add(1)) < ch.n;) rc = step(L, c);
        if (rc) {
            std::lock_guard<std::mutex> lk(mu);
            if (!failed) failed = rc, failed_text = g_err;
        }
    };
    if (n_workers == 1) {  // on the caller's own thread, next to the memory it has been working in: a thread elsewhere reads the file slower
        work(kept);
    } else {
        JoinedThreads workers;
        for (size_t t = 0; t < n_workers; ++t) workers.th.emplace_back(work, t ? nullptr : kept);
    }
    return failed ? set_err(failed, failed_text) : MQ_OK;
}

// Checked slots scattered into idx's (fresh) table, against idx's references: unpack_slots_kernel and its flag.  begin() is on the null
// stream, so is end()'s read-back: chunks on other streams lie between a wait for the first and a wait for theirs (stream_file_slots).
struct SlotScatter {
    mq_index *idx;
    Buf<uint32_t> d_flag;
    int begin() {
        int rc = d_flag.alloc(1);
        if (rc) return rc;
        HIPCHK(hipMemset(d_flag, 0, 4));
        return MQ_OK;
    }
    int chunk(const SavedSlot *d_slots, uint64_t n, hipStream_t st) {
        return launch(unpack_slots_kernel, slot_array_grid(n), 256, st, d_slots, n, idx->table, idx->nslots - 1, max_ref_id(idx->refs), (const uint64_t *)idx->d_ref_lens.p, d_flag);
    }
    int end(uint32_t *flag) {  // *flag != 0: a slot was refused (unpack_slots_kernel's per-slot checks)
        HIPCHK(hipMemcpy(flag, d_flag, 4, hipMemcpyDeviceToHost));
        return MQ_OK;
    }
};

// mq_index_load's device side: a table of nslots slots -- the header's, or the one mq_index_load_sized asks for (no table of the header's
// size is made then) -- and the dense length array, then the file's slots scattered into the table by up to 8 workers.  The length array
// goes up BEFORE the scatter: a zero in it marks an id the file's (possibly sparse) reference table does not have, and the scatter refuses
// an entry that names one.  Leaves the file behind the last slot.
static int load_table(int fd, const IxHeader &h, uint64_t nslots, const char *path, mq_index *idx, uint32_t *flag) {
    int rc;
    *flag = 0;
    if ((rc = alloc_table(idx, nslots)) || (rc = upload_ref_lens(idx))) return rc;
    const size_t total = (size_t)h.w[IX_N_KEYS] * sizeof(SavedSlot);
    if (!total) return MQ_OK;
    const off_t slots_at = ::lseek(fd, 0, SEEK_CUR);
    if (slots_at < 0) return set_err(MQ_EINVAL, std::string(IX_TRUNCATED) + path);
    SlotScatter scatter{idx};
    if ((rc = scatter.begin())) return rc;
    if ((rc = stream_file_slots(fd, slots_at, total, path, idx->device, 8, true, nullptr, [&](const SavedSlot *s, uint64_t ns, hipStream_t st) { return scatter.chunk(s, ns, st); }))) return rc;
    if ((rc = scatter.end(flag))) return rc;
    return ::lseek(fd, slots_at + (off_t)total, SEEK_SET) >= 0 ? MQ_OK : set_err(MQ_EINVAL, std::string(IX_TRUNCATED) + path);
}

// what a finished table holds (count_kernel): acc [0] live keys, [1] keys, [2] the largest reference id + 1
static int count_table(const mq_index *idx, unsigned long long acc[3]) {
    Buf<unsigned long long> d_acc;
    const uint64_t nb1 = idx->nslots / 2 + 1;
    int rc = d_acc.alloc(3);
    if (rc) return rc;
    HIPCHK(hipMemset(d_acc, 0, 24));
    if ((rc = launch(count_kernel, bucket_walk_grid(nb1), 256, 0, idx->table, nb1, d_acc))) return rc;
    HIPCHK(hipMemcpy(acc, d_acc, 24, hipMemcpyDeviceToHost));
    return MQ_OK;
}

// mq_index_load / mq_index_load_sized.  The size arguments are refused for their form before the file is opened, and for the file's key
// count right behind the header's own checks: before an index or a table exists.  A failure of the device side reads as an unreadable file.
static mq_index *load_index(const char *path, int device, uint64_t table_slots, uint32_t slots_per_kminmer) {
    return guarded([&]() -> mq_index * {
        if (!path) {
            set_err(MQ_EINVAL, "path is NULL");
            return nullptr;
        }
        uint64_t nslots = 0;
        if (sized_table_slots(table_slots, slots_per_kminmer, 0, 0, &nslots) != MQ_OK) return nullptr;
        ScopedFd fd(::open(path, O_RDONLY));
        if (fd < 0) {
            set_err(MQ_EINVAL, std::string("cannot open: ") + path);
            return nullptr;
        }
        IxHeader h;
        const char *why = read_header(fd, &h);
        if (!why && sized_table_slots(table_slots, slots_per_kminmer, h.w[IX_N_KMM], h.w[IX_N_KEYS], &nslots) != MQ_OK) return nullptr;
        if (!nslots) nslots = h.w[IX_NSLOTS];
        IndexPtr idx;
        if (!why) {
            idx.reset(mq_index_new(&h.p, device));
            if (!idx) return nullptr;
            why = read_refs(fd, h.w[IX_N_REFS], &idx->refs);
        }
        uint32_t bad_slot = 0;
        if (!why && load_table(fd, h, nslots, path, idx.get(), &bad_slot) != MQ_OK) why = IX_TRUNCATED;
        if (!why && bad_slot) why = IX_BAD_SLOT;
        uint8_t extra = 0;
        if (!why && ::read(fd, &extra, 1) != 0) why = IX_BYTES_AFTER;
        // what the file says about its table must be what the rebuilt table holds
        unsigned long long acc[3] = {0, 0, 0};
        if (!why && count_table(idx.get(), acc) != MQ_OK) why = IX_TRUNCATED;
        if (!why && (acc[1] != h.w[IX_N_KEYS] || acc[0] != h.w[IX_N_UNIQUE] || (acc[2] != 0 && acc[2] - 1 > max_ref_id(idx->refs)))) why = IX_BAD_COUNTS;
        if (why) {
            set_err(MQ_EINVAL, std::string(why) + path);
            return nullptr;
        }
        idx->n_kmm_total = h.w[IX_N_KMM];
        idx->n_keys = h.w[IX_N_KEYS];
        idx->n_unique = h.w[IX_N_UNIQUE];
        idx->finalized = true;
        return idx.release();
    });
}

// ---- replicas and packed slots

// the occupied slots of a finalized index's table, packed on its device (which the caller has selected): n_keys of them in d_pack
static int pack_table(const mq_index *idx, const char *who, Buf<SavedSlot> &d_pack) {
    const uint64_t n_occ = idx->n_keys;
    Buf<unsigned long long> d_cur;
    if (d_pack.try_alloc(n_occ + 1) != hipSuccess || d_cur.try_alloc(1) != hipSuccess || hipMemset(d_cur, 0, 8) != hipSuccess)
        return set_err(MQ_ENOMEM, std::string(who) + ": no device memory for the packed slots");
    const uint64_t nb1 = idx->nslots / 2 + 1;
    unsigned long long packed = 0;
    if (launch(pack_slots_kernel, bucket_walk_grid(nb1), 256, 0, idx->table, nb1, d_pack, d_cur, n_occ) != MQ_OK || hipMemcpy(&packed, d_cur, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return set_err(MQ_EHIP, std::string(who) + ": packing the table failed");
    if (packed != n_occ) return set_err(MQ_ESTATE, std::string(who) + ": the table holds another number of keys than the index records (internal error)");
    return MQ_OK;
}

// THE pack, peer-copy sequence: the occupied slots of src packed on its own device (selected by the caller), then carried to `device` -- 32
// bytes per key over the link, the table itself never travels.  d_in: src->n_keys slots (and one to spare: never an empty allocation) on
// `device`, which is the selected one afterwards; the packed array on the source's device is gone by then.  copy_failed: the entry point's
// own text (MQ_EHIP) for a failed allocation or copy on `device`, or nullptr for what the HIP call says (MQ_ENOMEM when memory ran out).
static int packed_slots_on(const mq_index *src, int device, const char *who, const char *copy_failed, Buf<SavedSlot> &d_in) {
    const uint64_t n = src->n_keys;
    Buf<SavedSlot> d_pack;
    int rc = pack_table(src, who, d_pack);
    if (rc) return rc;
    auto carry = [&]() -> int {
        HIPCHK(hipSetDevice(device));
        HIPCHK(d_in.try_alloc(n + 1));
        if (n) HIPCHK(hipMemcpyPeer(d_in, device, d_pack, src->device, n * sizeof(SavedSlot)));
        return MQ_OK;
    };
    if ((rc = carry()) && copy_failed) rc = set_err(MQ_EHIP, copy_failed);
    (void)hipSetDevice(src->device);  // (a Buf goes on its own device)
    d_pack.reset();
    HIPCHK(hipSetDevice(device));
    return rc;
}

// The shell of a replica of src on `device`, for mq_index_clone and mq_index_clone_sized: their refusals, then a new index (its device is
// the selected one) with src's references and counts, no table yet.  *nslots: the replica's table, src's own size when both size
// arguments are 0.  nullptr: refused, set_err called.
static IndexPtr replica_shell(const mq_index *src, int device, uint64_t table_slots, uint32_t slots_per_kminmer, uint64_t *nslots) {
    if (!src) {
        set_err(MQ_EINVAL, "src is NULL");
        return nullptr;
    }
    if (!src->finalized) {
        set_err(MQ_ESTATE, "index not finalized");
        return nullptr;
    }
    if (sized_table_slots(table_slots, slots_per_kminmer, src->n_kmm_total, src->n_keys, nslots) != MQ_OK) return nullptr;
    if (!*nslots) *nslots = src->nslots;
    IndexPtr idx(mq_index_new(&src->params, device));
    if (!idx) return nullptr;
    idx->refs = src->refs;
    idx->n_kmm_total = src->n_kmm_total;
    idx->n_keys = src->n_keys;
    idx->n_unique = src->n_unique;
    return idx;
}

// the dense reference lengths of src on dst's device (one length per reference id up to the largest: upload_ref_lens)
static int clone_ref_lens(const mq_index *src, mq_index *dst) {
    const size_t nl = src->d_ref_lens.cap;
    int rc = use_device(dst);
    if (rc || (rc = dst->d_ref_lens.alloc(nl))) return rc;
    HIPCHK(hipMemcpyPeer(dst->d_ref_lens, dst->device, src->d_ref_lens, src->device, nl * sizeof(uint64_t)));
    return MQ_OK;
}

// ---- mq_index_merge / mq_index_merge_file: another finalized index into this one (merge_table_kernel, merge_slots_kernel).
// What both routes share: the refusals that leave dst as it was, the growth, the counters, the bookkeeping afterwards.

static std::string shortest_double(double v) {
    char b[64];
    for (int prec = 1; prec <= 17; ++prec) {
        snprintf(b, sizeof(b), "%.*g", prec, v);
        if (strtod(b, nullptr) == v) break;
    }
    return b;
}
static std::string seeding_text(const mq_params &p) {
    char b[256];
    snprintf(b, sizeof(b), "-k %u -l %u -d %s%s --seeding-variant %u%s", p.k, p.l, shortest_double(p.density).c_str(), p.use_hpc ? "" : " --nohpc",
             (p.flags & MQ_FLAG_SEED_VARIANT_MASK) >> MQ_FLAG_SEED_VARIANT_SHIFT, (p.flags & MQ_FLAG_FAST_KH) ? " --fast-kh" : "");
    return b;
}
// the parameters that decide an index's keys; c, s, g and the case folding act at mapping time and stay dst's
static int merge_check_params(const char *who, const mq_params &d, const mq_params &s, const std::string &what) {
    const uint32_t seeding = MQ_FLAG_SEED_VARIANT_MASK | MQ_FLAG_FAST_KH;
    if (d.k == s.k && d.l == s.l && d.density == s.density && (d.use_hpc != 0) == (s.use_hpc != 0) && (d.flags & seeding) == (s.flags & seeding)) return MQ_OK;
    return set_err(MQ_EINVAL, std::string(who) + ": " + what + " was built with " + seeding_text(s) + ": indexes merge under the same seeding parameters (this index: " +
                                  seeding_text(d) + ")");
}
// a moved id must stay below 2^24 and must not be an id dst has
static int merge_check_ids(const char *who, const mq_index *dst, const RefMap &src_refs, uint32_t id_base) {
    for (auto &kv : src_refs) {
        const uint64_t moved = (uint64_t)kv.first + id_base;
        if (moved >= MQ_MAX_REF_ID) return set_err(MQ_EINVAL, std::string(who) + ": reference id " + std::to_string(kv.first) + " + id_base reaches 2^24");
        if (dst->refs.count((uint32_t)moved)) return set_err(MQ_EINVAL, std::string(who) + ": reference id " + std::to_string(moved) + " (moved) is already an id of this index");
    }
    return MQ_OK;
}
static int merge_check_dst(const char *who, const mq_index *dst) {
    if (dst->extend_failed) return extend_failed_err(dst);
    if (!dst->finalized) return set_err(MQ_ESTATE, std::string(who) + ": index not finalized");
    bool busy = dst->def_ctx && (dst->def_ctx->pending || dst->def_ctx->fx_kind != FxKind::None);
    {
        std::lock_guard<std::mutex> lk(const_cast<mq_index *>(dst)->ctx_mu);
        for (const mq_ctx *c : dst->ctxs) busy = busy || c->pending || c->fx_kind != FxKind::None;
    }
    if (busy) return set_err(MQ_ESTATE, std::string(who) + ": a context of this index has a submitted batch: wait for it first");
    return MQ_OK;
}
// The table grown, if the summed k-min-mers ask for it at the index's factor (finalize's rule for a reopened index: never smaller), and
// in any case so that an empty slot remains whatever the two key sets share.  Until here a failure leaves dst as it was.
static int merge_grow(const char *who, mq_index *dst, uint64_t src_kmm, uint64_t src_keys) {
    uint64_t nslots = std::max(table_slots_for(dst, dst->n_kmm_total + src_kmm), dst->nslots);
    while (nslots <= dst->n_keys + src_keys && nslots <= MQ_MAX_TABLE_SLOTS) nslots <<= 1;
    if (nslots > MQ_MAX_TABLE_SLOTS) return set_err(MQ_EINVAL, std::string(who) + ": the merged table would pass 2^40 slots");
    return nslots > dst->nslots ? retable(dst, nslots) : MQ_OK;
}
// ... and the insert counters, zeroed (null stream)
static int merge_begin(const char *who, mq_index *dst, uint64_t src_kmm, uint64_t src_keys, Buf<unsigned long long> &d_acc) {
    int rc;
    if ((rc = merge_grow(who, dst, src_kmm, src_keys)) || (rc = d_acc.alloc(3))) return rc;
    HIPCHK(hipMemset(d_acc, 0, 24));
    return MQ_OK;
}
// from the first insert launch on the only table there is has changed: a failure leaves an index that can only be freed
static int merge_fail(mq_index *dst, int rc) {
    dst->finalized = false;
    dst->extend_failed = dst->merge_failed = true;
    return rc;
}
// the counters read back (the wait for the inserts), the index's counts, references and device length array brought up to date
static int merge_finish(const char *who, mq_index *dst, const Buf<unsigned long long> &d_acc, const RefMap &src_refs, uint32_t id_base, uint64_t src_kmm, uint64_t src_keys) {
    unsigned long long acc[3] = {0, 0, 0};
    HIPCHK(hipMemcpy(acc, d_acc, 24, hipMemcpyDeviceToHost));
    if (acc[0] > src_keys || acc[1] > acc[0] || acc[1] > acc[2] || acc[2] - acc[1] > dst->n_unique + acc[0])
        return set_err(MQ_ESTATE, std::string(who) + ": the insert counters disagree with the two indexes' counts (internal error)");
    dst->n_keys += acc[0];
    dst->n_unique = dst->n_unique + acc[0] - acc[2];
    dst->n_kmm_total += src_kmm;
    for (auto &kv : src_refs) dst->refs[kv.first + id_base] = kv.second;
    return upload_ref_lens(dst);
}

// index to index; both locked, every refusal behind us.  Same device: table to table.  Another device (or MQ_MERGE_PACKED=1, test hook
// read here): the occupied slots packed on the source's device, 32 bytes per key over the link, merge_slots_kernel here.
static int merge_index_locked(mq_index *dst, const mq_index *src, uint32_t id_base) {
    const char *who = "mq_index_merge";
    int rc;
    const bool packed = src->device != dst->device || env_int("MQ_MERGE_PACKED", 0) != 0;
    const uint64_t n = src->n_keys;
    Buf<SavedSlot> d_in;  // (on dst's device)
    if (packed) {
        if ((rc = use_device(src))) return rc;
        HIPCHK(hipDeviceSynchronize());
        if ((rc = packed_slots_on(src, dst->device, who, nullptr, d_in))) return rc;
    }
    if ((rc = use_device(dst))) return rc;
    HIPCHK(hipDeviceSynchronize());  // launches queued on the contexts read the table that is about to change
    Buf<unsigned long long> d_acc;
    if ((rc = merge_begin(who, dst, src->n_kmm_total, n, d_acc))) return rc;
    if (packed) {
        if (n) rc = launch(merge_slots_kernel, ahead_grid(n), 256, 0, (const SavedSlot *)d_in.p, n, dst->table, dst->nslots - 1, id_base, d_acc);
    } else {
        const uint64_t nb1 = src->nslots / 2 + 1;
        rc = launch(merge_table_kernel, ahead_grid(2 * nb1), 256, 0, src->table, nb1, dst->table, dst->nslots - 1, id_base, d_acc);
    }
    if (rc || (rc = merge_finish(who, dst, d_acc, src->refs, id_base, src->n_kmm_total, n))) return merge_fail(dst, rc);
    return MQ_OK;
}

// From a file: two passes of stream_file_slots over its slot section, one worker each, through the same SlotLane -- a chunk of page-locked
// and of device memory is all the file's slots ever take.  Pass 1: the loader's per-slot checks over every slot, against the FILE's
// reference table, before the first insert; pass 2: the inserts.
static int merge_file_locked(mq_index *dst, const char *path, uint32_t id_base) {
    const char *who = "mq_index_merge_file";
    auto refuse = [&](const char *why) { return set_err(MQ_EINVAL, std::string(who) + ": " + why + path); };
    ScopedFd fd(::open(path, O_RDONLY));
    if (fd < 0) return set_err(MQ_EINVAL, std::string(who) + ": cannot open: " + path);
    IxHeader h;
    const char *why = read_header(fd, &h);
    if (why) return refuse(why);
    int rc = check_params(&h.p);
    if (rc) return rc;
    if ((rc = merge_check_params(who, dst->params, h.p, path))) return rc;
    RefMap file_refs;
    if ((why = read_refs(fd, h.w[IX_N_REFS], &file_refs))) return refuse(why);
    if ((rc = merge_check_ids(who, dst, file_refs, id_base))) return rc;
    const uint64_t n = h.w[IX_N_KEYS];
    const size_t total = (size_t)n * sizeof(SavedSlot);
    const off_t slots_at = ::lseek(fd, 0, SEEK_CUR);
    struct stat sb;
    if (slots_at < 0 || ::fstat(fd, &sb) != 0 || (uint64_t)sb.st_size < (uint64_t)slots_at + total) return refuse(IX_TRUNCATED);
    if ((uint64_t)sb.st_size > (uint64_t)slots_at + total) return refuse(IX_BYTES_AFTER);
    if ((rc = use_device(dst))) return rc;
    HIPCHK(hipDeviceSynchronize());
    SlotLane lane;  // (kept across the two passes)
    Buf<uint64_t> d_flens;
    Buf<unsigned long long> d_flags, d_acc;
    unsigned long long flags[2] = {0, 0};  // [0] a slot was refused, [1] the slots that would be live
    if (total) {
        const uint32_t f_max_id = max_ref_id(file_refs);
        if ((rc = upload_ref_lens(file_refs, d_flens)) || (rc = d_flags.alloc(2))) return rc;
        HIPCHK(hipMemset(d_flags, 0, 16));
        if ((rc = stream_file_slots(fd, slots_at, total, path, dst->device, 1, false, &lane, [&](const SavedSlot *s, uint64_t ns, hipStream_t st) {
                 return launch(merge_check_slots_kernel, slot_array_grid(ns), 256, st, s, ns, f_max_id, (const uint64_t *)d_flens.p, d_flags);
             })))
            return rc;
        HIPCHK(hipMemcpy(flags, d_flags, 16, hipMemcpyDeviceToHost));
    }
    if (flags[0]) return refuse(IX_BAD_SLOT);
    if (flags[1] != h.w[IX_N_UNIQUE]) return refuse(IX_BAD_COUNTS);
    if ((rc = merge_begin(who, dst, h.w[IX_N_KMM], n, d_acc))) return rc;
    rc = stream_file_slots(fd, slots_at, total, path, dst->device, 1, false, &lane, [&](const SavedSlot *s, uint64_t ns, hipStream_t st) {
        return launch(merge_slots_kernel, ahead_grid(ns), 256, st, s, ns, dst->table, dst->nslots - 1, id_base, d_acc);
    });
    if (rc || (rc = merge_finish(who, dst, d_acc, file_refs, id_base, h.w[IX_N_KMM], n))) return merge_fail(dst, rc);
    return MQ_OK;
}

// mq_index_save's slot section: the packed slots from the device to the file through two page-locked buffers -- chunk i + 1 crosses PCIe
// while chunk i goes to the file (the streamer's direction reversed; the same IxChunks).  *wrote: false when the file refused a write.
static int save_slots(int fd, const Buf<SavedSlot> &d_pack, size_t total, bool *wrote) {
    const IxChunks ch = ix_chunks(total);
    if (!ch.n) return MQ_OK;
    PinnedBuf<uint8_t> h_buf[2];
    ScopedStream st;
    ScopedEvent ev[2];
    bool hip_ok = hipStreamCreateWithFlags(&st.h, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 2 && hip_ok; ++i) hip_ok = h_buf[i].try_alloc(ch.buf_bytes()) == hipSuccess && hipEventCreate(&ev[i].h) == hipSuccess;
    if (!hip_ok) return set_err(MQ_EHIP, "mq_index_save: transfer buffers");
    auto issue = [&](size_t c) {
        return hipMemcpyAsync(h_buf[c & 1], (const uint8_t *)d_pack.p + ch.at(c), ch.bytes(c), hipMemcpyDeviceToHost, st) == hipSuccess && hipEventRecord(ev[c & 1], st) == hipSuccess;
    };
    hip_ok = issue(0);
    for (size_t c = 0; c < ch.n && *wrote && hip_ok; ++c) {
        if (c + 1 < ch.n) hip_ok = issue(c + 1);
        hip_ok = hip_ok && hipEventSynchronize(ev[c & 1]) == hipSuccess;
        *wrote = hip_ok && write_all(fd, h_buf[c & 1], ch.bytes(c));
    }
    return hip_ok ? MQ_OK : set_err(MQ_EHIP, "mq_index_save: device-to-host copy failed");
}

extern "C" {

int mq_index_save(const mq_index *idx, const char *path) {
    return guarded([&]() -> int {
        if (!idx || !path) return set_err(MQ_EINVAL, "bad arguments");
        if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
        int rc = use_device(idx);
        if (rc) return rc;
        Buf<SavedSlot> d_pack;  // occupied slots, packed on the device
        if ((rc = pack_table(idx, "mq_index_save", d_pack))) return rc;
        ScopedFd fd(::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644));
        if (fd < 0) return set_err(MQ_EINVAL, std::string("cannot open for writing: ") + path);
        bool wrote = write_header(fd, idx) && write_refs(fd, idx->refs);
        if (wrote && (rc = save_slots(fd, d_pack, (size_t)idx->n_keys * sizeof(SavedSlot), &wrote))) return rc;
        const bool closed = fd.close();
        return wrote && closed ? MQ_OK : set_err(MQ_EINVAL, std::string("short write: ") + path);
    });
}

mq_index *mq_index_load(const char *path, int device) { return load_index(path, device, 0, 0); }

// mq_index_load into a table of the caller's size (sized_table_slots): the file's slots are scattered straight into it.
mq_index *mq_index_load_sized(const char *path, int device, uint64_t table_slots, uint32_t slots_per_kminmer) {
    return load_index(path, device, table_slots, slots_per_kminmer);
}

// A replica of a finalized index on another device: the table travels device to device (xGMI between the GPUs of a node)
// instead of being rebuilt from the reference on every GPU.
mq_index *mq_index_clone(const mq_index *src, int device) {
    return guarded([&]() -> mq_index * {
        uint64_t nslots = 0;
        IndexPtr idx = replica_shell(src, device, 0, 0, &nslots);
        if (!idx) return nullptr;
        if (alloc_table(idx.get(), nslots) != MQ_OK || hipMemcpyPeer(idx->table, device, src->table, src->device, table_bytes_of(nslots)) != hipSuccess ||
            clone_ref_lens(src, idx.get()) != MQ_OK || hipDeviceSynchronize() != hipSuccess) {
            set_err(MQ_EHIP, "mq_index_clone: device-to-device copy failed");
            return nullptr;
        }
        idx->finalized = true;
        return idx.release();
    });
}

// mq_index_clone with a table of the caller's size on the destination: the occupied slots are packed on the source device, the packed
// array (32 bytes per key) crosses the link, and the destination scatters it into a fresh table -- the table itself never travels.
mq_index *mq_index_clone_sized(const mq_index *src, int device, uint64_t table_slots, uint32_t slots_per_kminmer) {
    if (src && !table_slots && !slots_per_kminmer) return mq_index_clone(src, device);
    return guarded([&]() -> mq_index * {
        const char *who = "mq_index_clone_sized";
        uint64_t nslots = 0;
        IndexPtr idx = replica_shell(src, device, table_slots, slots_per_kminmer, &nslots);
        if (!idx) return nullptr;
        Buf<SavedSlot> d_in;
        if (use_device(src) != MQ_OK || packed_slots_on(src, device, who, "mq_index_clone_sized: device-to-device copy failed", d_in) != MQ_OK) return nullptr;
        const uint64_t n = src->n_keys;
        SlotScatter scatter{idx.get()};
        uint32_t bad_slot = 1;
        if (alloc_table(idx.get(), nslots) != MQ_OK || clone_ref_lens(src, idx.get()) != MQ_OK || scatter.begin() != MQ_OK || (n && scatter.chunk(d_in, n, 0) != MQ_OK) ||
            scatter.end(&bad_slot) != MQ_OK || hipDeviceSynchronize() != hipSuccess) {
            set_err(MQ_EHIP, std::string(who) + ": device-to-device copy failed");
            return nullptr;
        }
        if (bad_slot) {
            set_err(MQ_ESTATE, std::string(who) + ": the source table holds a slot that names no reference of the index (internal error)");
            return nullptr;
        }
        idx->finalized = true;
        return idx.release();
    });
}

// Another finalized index merged into dst, source id i becoming id_base + i: dst ends where one build of both reference sets ends (the
// header has the contract).  Both indexes are locked, in address order.
int mq_index_merge(mq_index *dst, const mq_index *src, uint32_t id_base) {
    return guarded([&]() -> int {
        if (!dst || !src) return set_err(MQ_EINVAL, "mq_index_merge: dst or src is NULL");
        if (dst == src) return set_err(MQ_EINVAL, "mq_index_merge: dst and src are the same index");
        mq_index *s = const_cast<mq_index *>(src);
        std::mutex &first = dst < s ? dst->mu : s->mu, &second = dst < s ? s->mu : dst->mu;
        std::lock_guard<std::mutex> lk1(first), lk2(second);
        int rc = merge_check_dst("mq_index_merge", dst);
        if (rc) return rc;
        dst->cov.drop();  // (a coverage result describes the table as it was)
        if (!src->finalized) return set_err(MQ_ESTATE, "mq_index_merge: src is not finalized");
        if ((rc = merge_check_params("mq_index_merge", dst->params, src->params, "src"))) return rc;
        if ((rc = merge_check_ids("mq_index_merge", dst, src->refs, id_base))) return rc;
        return merge_index_locked(dst, src, id_base);
    });
}

// The same from a file written by mq_index_save: its slots are streamed through a bounded device buffer into dst's table; the file's own
// table is never allocated.
int mq_index_merge_file(mq_index *dst, const char *path, uint32_t id_base) {
    return guarded([&]() -> int {
        if (!dst || !path) return set_err(MQ_EINVAL, "mq_index_merge_file: dst or path is NULL");
        std::lock_guard<std::mutex> lk(dst->mu);
        int rc = merge_check_dst("mq_index_merge_file", dst);
        if (rc) return rc;
        dst->cov.drop();
        return merge_file_locked(dst, path, id_base);
    });
}

}  // extern "C"
