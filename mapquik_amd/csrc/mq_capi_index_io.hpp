// mq_capi_index_io.hpp -- C ABI: the on-disk index (mq_index_save / mq_index_load), replicas (mq_index_clone), reference info (part of the one
// translation unit mq_capi.hip).
#pragma once

// On-disk index (the reference has none and rebuilds on every run, src/closures.rs:24-94): header, parameters, reference table,
// then the OCCUPIED slots only (32 bytes each: ~1.5 GB for a human genome instead of the 17 GB table at load 1/8); mq_index_load
// scatters them into a fresh table on the device.  Little-endian, this library's layout (MQ_INDEX_MAGIC names the version).
static const char MQ_INDEX_MAGIC[8] = {'M', 'Q', 'H', 'I', 'P', 'I', 'X', '2'};
constexpr size_t IX_IO_CHUNK = 64u << 20;  // bytes per page-locked transfer buffer (two of them: the copy overlaps the file I/O)
struct IxHeader {  // what follows the magic
    mq_params p;
    uint64_t w[6];
};
enum { IX_SLOT_BYTES, IX_NSLOTS, IX_N_KMM, IX_N_KEYS, IX_N_UNIQUE, IX_N_REFS };  // IxHeader::w

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

// ---- mq_index_load in steps.  Each returns nullptr, or the text (the path follows it) with which the file is refused.
static const char *const IX_TRUNCATED = "truncated or unreadable index file: ";

// every refusal that comes from the header alone: before an index or a table exists
static const char *read_header(int fd, IxHeader *h) {
    char magic[8];
    const uint64_t *w = h->w;
    if (!read_all(fd, magic, 8) || memcmp(magic, MQ_INDEX_MAGIC, 8) != 0 || !read_all(fd, &h->p, sizeof(h->p)) || !read_all(fd, h->w, sizeof(h->w)) ||
        w[IX_SLOT_BYTES] != sizeof(SavedSlot) || w[IX_NSLOTS] < 2 || (w[IX_NSLOTS] & (w[IX_NSLOTS] - 1)) != 0 || w[IX_NSLOTS] > (1ull << 40) ||
        w[IX_N_KEYS] >= w[IX_NSLOTS] /* a table without an empty slot would make a miss walk forever */ || w[IX_N_UNIQUE] > w[IX_N_KEYS] || w[IX_N_REFS] > MQ_MAX_REF_ID)
        return "not a mapquik HIP index (or another layout version): ";
    return nullptr;
}

static const char *read_refs(int fd, uint64_t n_refs, mq_index *idx) {
    for (uint64_t i = 0; i < n_refs; ++i) {
        uint32_t id = 0, nl = 0;
        uint64_t len = 0;
        if (!read_all(fd, &id, 4) || !read_all(fd, &nl, 4) || !read_all(fd, &len, 8) || nl >= (1u << 20) || id >= MQ_MAX_REF_ID) return IX_TRUNCATED;
        std::string name(nl, '\0');
        if (nl && !read_all(fd, &name[0], nl)) return IX_TRUNCATED;
        idx->refs[id] = std::make_pair(name, len);
    }
    return nullptr;
}

// threads that are joined when their holder goes: a spawn that fails leaves none running behind the frame they work on
struct JoinedThreads {
    std::vector<std::thread> th;
    void join() {
        for (auto &t : th)
            if (t.joinable()) t.join();
    }
    ~JoinedThreads() { join(); }
};

// The table and the dense length array, then the file's slots into the table: file -> page-locked buffer -> device -> scatter kernel,
// by a few threads at once (each its own buffers and stream; the kernels of different chunks insert into the same table with atomics):
// the file read, not the copy, is what takes time.  Leaves the file behind the last slot.  d_flags is the caller's, to free.
// nslots: the table's size -- the header's, or the one mq_index_load_sized asks for (no table of the header's size is made then).
static const char *scatter_slots(int fd, const IxHeader &h, uint64_t nslots, mq_index *idx, Buf<uint32_t> &d_flags) {
    // the dense length array goes up BEFORE the scatter: a reference of length 0 cannot own a k-min-mer, so a zero in it marks an
    // id the file's (possibly sparse) reference table does not have, and the scatter refuses an entry that names one
    if (alloc_table(idx, nslots) != MQ_OK || upload_ref_lens(idx) != MQ_OK) return IX_TRUNCATED;
    const size_t total = (size_t)h.w[IX_N_KEYS] * sizeof(SavedSlot);
    if (!total) return nullptr;
    const off_t slots_at = ::lseek(fd, 0, SEEK_CUR);
    if (slots_at < 0 || d_flags.try_alloc(1) != hipSuccess || hipMemset(d_flags, 0, 4) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
        return IX_TRUNCATED;  // (the synchronize: the table's memset (null stream) is done before other streams write to it)
    const uint32_t max_id = max_ref_id(idx);
    const int device = idx->device;
    const size_t n_chunks = (total + IX_IO_CHUNK - 1) / IX_IO_CHUNK;
    std::atomic<size_t> next{0};
    std::atomic<int> bad{0};
    auto work = [&]() {
        Scoped<void *, mq_host_free> hh;
        Buf<uint8_t> d;
        ScopedStream st;
        const size_t cb = std::min(total, IX_IO_CHUNK);
        bool good = hipSetDevice(device) == hipSuccess && (hh.h = mq_host_alloc(cb)) != nullptr && d.try_alloc(cb) == hipSuccess &&
                    hipStreamCreateWithFlags(&st.h, hipStreamNonBlocking) == hipSuccess;
        uint8_t *const hb = (uint8_t *)hh.h;
        while (good) {
            const size_t c = next.fetch_add(1);
            if (c >= n_chunks) break;
            const size_t o = c * IX_IO_CHUNK, n = std::min(IX_IO_CHUNK, total - o);
            size_t got = 0;
            while (got < n) {
                const ssize_t r = ::pread(fd, hb + got, n - got, slots_at + (off_t)(o + got));
                if (r <= 0) break;
                got += (size_t)r;
            }
            const uint64_t ns = n / sizeof(SavedSlot);
            good = got == n && hipMemcpyAsync(d, hb, n, hipMemcpyHostToDevice, st) == hipSuccess &&
                   launch(unpack_slots_kernel, (uint32_t)std::min<uint64_t>((ns + 255) / 256, 1u << 16), 256, st, (const SavedSlot *)d.p, ns, idx->table, nslots - 1, max_id,
                          (const uint64_t *)idx->d_ref_lens.p, d_flags) == MQ_OK &&
                   hipStreamSynchronize(st) == hipSuccess;
        }
        if (!good) bad.store(1);
    };
    {
        JoinedThreads workers;
        for (size_t t = 0; t < std::min<size_t>(8, n_chunks); ++t) workers.th.emplace_back(work);
    }
    uint32_t flags = 1;
    if (bad.load() || hipMemcpy(&flags, d_flags, 4, hipMemcpyDeviceToHost) != hipSuccess) return IX_TRUNCATED;
    if (flags) return "corrupt index file (an entry names a reference the file does not have, or a malformed slot): ";
    return ::lseek(fd, slots_at + (off_t)total, SEEK_SET) >= 0 ? nullptr : IX_TRUNCATED;
}

// what the file says about its table must be what the rebuilt table holds
static const char *verify_counts(const IxHeader &h, mq_index *idx) {
    Buf<unsigned long long> d_acc;
    unsigned long long acc[3] = {0, 0, 0};
    const uint64_t nb1 = idx->nslots / 2 + 1;
    if (d_acc.try_alloc(3) != hipSuccess || hipMemset(d_acc, 0, 24) != hipSuccess || launch(count_kernel, bucket_walk_grid(nb1), 256, 0, idx->table, nb1, d_acc) != MQ_OK ||
        hipMemcpy(acc, d_acc, 24, hipMemcpyDeviceToHost) != hipSuccess)
        return IX_TRUNCATED;
    if (acc[1] != h.w[IX_N_KEYS] || acc[0] != h.w[IX_N_UNIQUE] || (acc[2] != 0 && acc[2] - 1 > max_ref_id(idx)))
        return "corrupt index file (key counts or reference ids disagree with its header): ";
    return nullptr;
}

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

// the dense reference lengths of src on dst's device (one length per reference id up to the largest: upload_ref_lens)
static bool clone_ref_lens(const mq_index *src, mq_index *dst) {
    const size_t nl = src->d_ref_lens.cap;
    return hipSetDevice(dst->device) == hipSuccess && dst->d_ref_lens.try_alloc(nl) == hipSuccess &&
           hipMemcpyPeer(dst->d_ref_lens, dst->device, src->d_ref_lens, src->device, nl * sizeof(uint64_t)) == hipSuccess;
}

// mq_index_load / mq_index_load_sized.  The size arguments are refused for their form before the file is opened, and for the file's key
// count right behind the header's own checks: before an index or a table exists.
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
        Buf<uint32_t> d_flags;  // the scatter's error flags (declared behind idx: freed before the index, on a refusal too)
        if (!why) {
            idx.reset(mq_index_new(&h.p, device));
            if (!idx) return nullptr;
            why = read_refs(fd, h.w[IX_N_REFS], idx.get());
        }
        if (!why) why = scatter_slots(fd, h, nslots, idx.get(), d_flags);
        uint8_t extra = 0;
        if (!why && ::read(fd, &extra, 1) != 0) why = "corrupt index file (bytes after the last slot): ";
        if (!why) why = verify_counts(h, idx.get());
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
static int merge_check_ids(const char *who, const mq_index *dst, const std::map<uint32_t, std::pair<std::string, uint64_t>> &src_refs, uint32_t id_base) {
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
// from the first insert launch on the only table there is has changed: a failure leaves an index that can only be freed
static int merge_fail(mq_index *dst, int rc) {
    dst->finalized = false;
    dst->extend_failed = dst->merge_failed = true;
    return rc;
}
// the counters read back (the wait for the inserts), the index's counts, references and device length array brought up to date
static int merge_finish(const char *who, mq_index *dst, const Buf<unsigned long long> &d_acc, const std::map<uint32_t, std::pair<std::string, uint64_t>> &src_refs,
                        uint32_t id_base, uint64_t src_kmm, uint64_t src_keys) {
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
static uint32_t merge_grid(uint64_t n_slots) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n_slots + 256 * RETABLE_AHEAD - 1) / (256 * RETABLE_AHEAD), 1u << 16)); }

// index to index; both locked, every refusal behind us.  Same device: table to table.  Another device (or MQ_MERGE_PACKED=1, test hook
// read here): the occupied slots packed on the source's device, 32 bytes per key over the link, merge_slots_kernel here.
static int merge_index_locked(mq_index *dst, const mq_index *src, uint32_t id_base) {
    const char *who = "mq_index_merge";
    int rc;
    const bool packed = src->device != dst->device || env_int("MQ_MERGE_PACKED", 0) != 0;
    const uint64_t n = src->n_keys;
    Buf<SavedSlot> d_in;  // (on dst's device)
    if (packed) {
        Buf<SavedSlot> d_pack;
        if ((rc = use_device(src))) return rc;
        HIPCHK(hipDeviceSynchronize());
        if ((rc = pack_table(src, who, d_pack))) return rc;
        if ((rc = use_device(dst)) || (rc = d_in.alloc(n + 1))) return rc;
        if (n) HIPCHK(hipMemcpyPeer(d_in, dst->device, d_pack, src->device, n * sizeof(SavedSlot)));
        if ((rc = use_device(src))) return rc;
        d_pack.reset();
    }
    if ((rc = use_device(dst))) return rc;
    HIPCHK(hipDeviceSynchronize());  // launches queued on the contexts read the table that is about to change
    if ((rc = merge_grow(who, dst, src->n_kmm_total, n))) return rc;
    Buf<unsigned long long> d_acc;
    if ((rc = d_acc.alloc(3))) return rc;
    HIPCHK(hipMemset(d_acc, 0, 24));
    if (packed) {
        if (n) rc = launch(merge_slots_kernel, merge_grid(n), 256, 0, (const SavedSlot *)d_in.p, n, dst->table, dst->nslots - 1, id_base, d_acc);
    } else {
        const uint64_t nb1 = src->nslots / 2 + 1;
        rc = launch(merge_table_kernel, merge_grid(2 * nb1), 256, 0, src->table, nb1, dst->table, dst->nslots - 1, id_base, d_acc);
    }
    if (rc || (rc = merge_finish(who, dst, d_acc, src->refs, id_base, src->n_kmm_total, n))) return merge_fail(dst, rc);
    return MQ_OK;
}

// A file's slots, chunk by chunk, through one page-locked buffer and one device buffer (IX_IO_CHUNK bytes at most): f(device slots, count)
// per chunk, on the null stream, waited for before the buffers are used again.
template <class F>
static int for_file_slots(int fd, off_t slots_at, size_t total, uint8_t *hb, Buf<uint8_t> &d, const char *path, F f) {
    for (size_t o = 0; o < total; o += IX_IO_CHUNK) {
        const size_t n = std::min(IX_IO_CHUNK, total - o);
        size_t got = 0;
        while (got < n) {
            const ssize_t r = ::pread(fd, hb + got, n - got, slots_at + (off_t)(o + got));
            if (r <= 0) return set_err(MQ_EINVAL, std::string(IX_TRUNCATED) + path);
            got += (size_t)r;
        }
        HIPCHK(hipMemcpy(d, hb, n, hipMemcpyHostToDevice));
        int rc = f((const SavedSlot *)d.p, (uint64_t)(n / sizeof(SavedSlot)));
        if (rc) return rc;
        HIPCHK(hipDeviceSynchronize());
    }
    return MQ_OK;
}

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
    mq_index file_side;  // (a holder for the loader's read_refs: no device state)
    file_side.device = dst->device;
    if ((why = read_refs(fd, h.w[IX_N_REFS], &file_side))) return refuse(why);
    if ((rc = merge_check_ids(who, dst, file_side.refs, id_base))) return rc;
    const uint64_t n = h.w[IX_N_KEYS];
    const size_t total = (size_t)n * sizeof(SavedSlot);
    const off_t slots_at = ::lseek(fd, 0, SEEK_CUR);
    struct stat sb;
    if (slots_at < 0 || ::fstat(fd, &sb) != 0 || (uint64_t)sb.st_size < (uint64_t)slots_at + total) return refuse(IX_TRUNCATED);
    if ((uint64_t)sb.st_size > (uint64_t)slots_at + total) return refuse("corrupt index file (bytes after the last slot): ");
    if ((rc = use_device(dst))) return rc;
    HIPCHK(hipDeviceSynchronize());
    // pass 1: the loader's per-slot checks over every slot of the file, against the FILE's reference table, before the first insert
    PinnedBuf<uint8_t> hb;
    Buf<uint8_t> d;
    Buf<uint64_t> d_flens;
    Buf<unsigned long long> d_flags, d_acc;
    const uint32_t f_max_id = max_ref_id(&file_side);
    if (total) {
        std::vector<uint64_t> lens((size_t)f_max_id + 1, 0);
        for (auto &kv : file_side.refs) lens[kv.first] = kv.second.second;
        if ((rc = hb.alloc(std::min(total, IX_IO_CHUNK))) || (rc = d.alloc(std::min(total, IX_IO_CHUNK))) || (rc = d_flens.alloc(lens.size())) || (rc = d_flags.alloc(2))) return rc;
        HIPCHK(hipMemcpy(d_flens, lens.data(), lens.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemset(d_flags, 0, 16));
        if ((rc = for_file_slots(fd, slots_at, total, hb, d, path, [&](const SavedSlot *s, uint64_t ns) {
                 return launch(merge_check_slots_kernel, (uint32_t)std::min<uint64_t>((ns + 255) / 256, 1u << 16), 256, 0, s, ns, f_max_id, (const uint64_t *)d_flens.p, d_flags);
             })))
            return rc;
        unsigned long long flags[2] = {1, 0};
        HIPCHK(hipMemcpy(flags, d_flags, 16, hipMemcpyDeviceToHost));
        if (flags[0]) return refuse("corrupt index file (an entry names a reference the file does not have, or a malformed slot): ");
        if (flags[1] != h.w[IX_N_UNIQUE]) return refuse("corrupt index file (key counts or reference ids disagree with its header): ");
    } else if (h.w[IX_N_UNIQUE] != 0) {
        return refuse("corrupt index file (key counts or reference ids disagree with its header): ");
    }
    if ((rc = merge_grow(who, dst, h.w[IX_N_KMM], n))) return rc;
    if ((rc = d_acc.alloc(3))) return rc;
    HIPCHK(hipMemset(d_acc, 0, 24));
    // pass 2: the inserts
    if (total)
        rc = for_file_slots(fd, slots_at, total, hb, d, path, [&](const SavedSlot *s, uint64_t ns) {
            return launch(merge_slots_kernel, merge_grid(ns), 256, 0, s, ns, dst->table, dst->nslots - 1, id_base, d_acc);
        });
    if (rc || (rc = merge_finish(who, dst, d_acc, file_side.refs, id_base, h.w[IX_N_KMM], n))) return merge_fail(dst, rc);
    return MQ_OK;
}

extern "C" {

int mq_index_save(const mq_index *idx, const char *path) {
    return guarded([&]() -> int {
        if (!idx || !path) return set_err(MQ_EINVAL, "bad arguments");
        if (!idx->finalized) return set_err(MQ_ESTATE, "index not finalized");
        int rc = use_device(idx);
        if (rc) return rc;
        // occupied slots, packed on the device
        const uint64_t n_occ = idx->n_keys;
        Buf<SavedSlot> d_pack;
        PinnedBuf<uint8_t> h_buf[2];
        ScopedStream st;
        ScopedEvent ev[2];
        if ((rc = pack_table(idx, "mq_index_save", d_pack))) return rc;
        ScopedFd fd(::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644));
        if (fd < 0) return set_err(MQ_EINVAL, std::string("cannot open for writing: ") + path);
        bool ok = write_all(fd, MQ_INDEX_MAGIC, 8);
        const uint64_t hdr[6] = {sizeof(SavedSlot), idx->nslots, idx->n_kmm_total, idx->n_keys, idx->n_unique, (uint64_t)idx->refs.size()};  // (IxHeader::w)
        ok = ok && write_all(fd, &idx->params, sizeof(mq_params)) && write_all(fd, hdr, sizeof(hdr));
        for (auto &kv : idx->refs) {
            const uint32_t id = kv.first, nl = (uint32_t)kv.second.first.size();
            ok = ok && write_all(fd, &id, 4) && write_all(fd, &nl, 4) && write_all(fd, &kv.second.second, 8) && (nl == 0 || write_all(fd, kv.second.first.data(), nl));
        }
        const size_t total = (size_t)n_occ * sizeof(SavedSlot);
        if (ok && total) {
            bool hip_ok = hipStreamCreateWithFlags(&st.h, hipStreamNonBlocking) == hipSuccess;
            for (int i = 0; i < 2 && hip_ok; ++i) hip_ok = h_buf[i].try_alloc(std::min(total, IX_IO_CHUNK)) == hipSuccess && hipEventCreate(&ev[i].h) == hipSuccess;
            if (!hip_ok) return set_err(MQ_EHIP, "mq_index_save: transfer buffers");
            // chunk i+1 crosses PCIe while chunk i goes to the file
            const size_t n_chunks = (total + IX_IO_CHUNK - 1) / IX_IO_CHUNK;
            auto issue = [&](size_t c) {
                const size_t o = c * IX_IO_CHUNK, n = std::min(IX_IO_CHUNK, total - o);
                return hipMemcpyAsync(h_buf[c & 1], (const uint8_t *)d_pack.p + o, n, hipMemcpyDeviceToHost, st) == hipSuccess &&
                       hipEventRecord(ev[c & 1], st) == hipSuccess;
            };
            hip_ok = issue(0);
            for (size_t c = 0; c < n_chunks && ok && hip_ok; ++c) {
                if (c + 1 < n_chunks) hip_ok = issue(c + 1);
                hip_ok = hip_ok && hipEventSynchronize(ev[c & 1]) == hipSuccess;
                const size_t o = c * IX_IO_CHUNK, n = std::min(IX_IO_CHUNK, total - o);
                ok = hip_ok && write_all(fd, h_buf[c & 1], n);
            }
            if (!hip_ok) return set_err(MQ_EHIP, "mq_index_save: device-to-host copy failed");
        }
        const bool closed = fd.close();
        return ok && closed ? MQ_OK : set_err(MQ_EINVAL, std::string("short write: ") + path);
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
        if (!src) {
            set_err(MQ_EINVAL, "src is NULL");
            return nullptr;
        }
        if (!src->finalized) {
            set_err(MQ_ESTATE, "index not finalized");
            return nullptr;
        }
        IndexPtr idx(mq_index_new(&src->params, device));
        if (!idx) return nullptr;
        idx->refs = src->refs;
        idx->n_kmm_total = src->n_kmm_total;
        idx->n_keys = src->n_keys;
        idx->n_unique = src->n_unique;
        bool ok = alloc_table(idx.get(), src->nslots) == MQ_OK;
        if (ok) ok = hipMemcpyPeer(idx->table, device, src->table, src->device, table_bytes_of(src->nslots)) == hipSuccess;
        if (ok) ok = clone_ref_lens(src, idx.get());
        if (ok) ok = hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
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
        if (!src) {
            set_err(MQ_EINVAL, "src is NULL");
            return nullptr;
        }
        if (!src->finalized) {
            set_err(MQ_ESTATE, "index not finalized");
            return nullptr;
        }
        uint64_t nslots = 0;
        if (sized_table_slots(table_slots, slots_per_kminmer, src->n_kmm_total, src->n_keys, &nslots) != MQ_OK) return nullptr;
        Buf<SavedSlot> d_pack;
        if (use_device(src) != MQ_OK || pack_table(src, "mq_index_clone_sized", d_pack) != MQ_OK) return nullptr;
        IndexPtr idx(mq_index_new(&src->params, device));  // (selects the destination device)
        if (!idx) return nullptr;
        idx->refs = src->refs;
        idx->n_kmm_total = src->n_kmm_total;
        idx->n_keys = src->n_keys;
        idx->n_unique = src->n_unique;
        const uint64_t n = src->n_keys;
        Buf<SavedSlot> d_in;
        Buf<uint32_t> d_flags;
        uint32_t flags = 1;
        bool ok = alloc_table(idx.get(), nslots) == MQ_OK && clone_ref_lens(src, idx.get()) && d_in.try_alloc(n + 1) == hipSuccess && d_flags.try_alloc(1) == hipSuccess &&
                  hipMemset(d_flags, 0, 4) == hipSuccess;
        if (ok && n) ok = hipMemcpyPeer(d_in, device, d_pack, src->device, n * sizeof(SavedSlot)) == hipSuccess;
        if (ok && n)
            ok = launch(unpack_slots_kernel, (uint32_t)std::min<uint64_t>((n + 255) / 256, 1u << 16), 256, 0, (const SavedSlot *)d_in.p, n, idx->table, nslots - 1, max_ref_id(idx.get()),
                        (const uint64_t *)idx->d_ref_lens.p, d_flags) == MQ_OK;
        if (ok) ok = hipMemcpy(&flags, d_flags, 4, hipMemcpyDeviceToHost) == hipSuccess;
        if (ok) ok = hipDeviceSynchronize() == hipSuccess;
        if (!ok) {
            set_err(MQ_EHIP, "mq_index_clone_sized: device-to-device copy failed");
            return nullptr;
        }
        if (flags) {
            set_err(MQ_ESTATE, "mq_index_clone_sized: the source table holds a slot that names no reference of the index (internal error)");
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
        return merge_file_locked(dst, path, id_base);
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

int mq_map_reserve(mq_index *idx, uint32_t n_reads, uint64_t total_bases) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = use_device(idx);
        if (rc) return rc;
        return ctx_ensure(idx->def_ctx.get(), n_reads, total_bases, list_f16(idx));
    });
}

}  // extern "C"
