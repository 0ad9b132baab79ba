// mq_capi_sort.hpp -- mq_sort_*: the host side of mq_sort_kernels.hpp (part of the one translation unit mq_capi.hip).  The host route and
// the result pass run on the sorter's own stream; the device route runs on the caller's.  Adds only append (one atomic on the cursor per
// wave) and the ordinal is part of the key, so no add is ordered against another; mq_sort_result, mq_sort_clear and mq_sort_reserve wait
// for the whole device first, which covers every stream an add was queued on.
#pragma once

constexpr uint64_t SORT_MAX_OFFERED = 0xFFFFFFFEull;  // ordinals and `offered` stay below 2^32 - 1

static uint64_t sort_tiles(uint64_t n) { return (n + MQ_SORT_TILE - 1) / MQ_SORT_TILE; }

static void sort_drop_host(mq_sorter *s) {
    std::vector<uint32_t>().swap(s->h_order);
    std::vector<mq_sort_ref>().swap(s->h_refs);
}

// (locked, the device selected and waited for) key / ord at `capacity` records with what they held; the result pass's second set and
// counts go (the next result brings them back at the new size).  A failure leaves the sorter as it was.
static int sort_grow(mq_sorter *s, uint64_t capacity) {
    unsigned long long kept = 0;
    HIPCHK(hipMemcpy(&kept, s->acc, 8, hipMemcpyDeviceToHost));
    if (kept > s->capacity) return set_err(MQ_ESTATE, "mq_sort: the cursor passed the capacity (internal error)");
    Buf<unsigned long long> key;
    Buf<uint32_t> ord;
    int rc;
    reset_all(s->key2, s->ord2, s->counts);  // (scratch only: their room may be what the larger arrays need)
    if ((rc = key.alloc(capacity + 1)) || (rc = ord.alloc(capacity + 1))) return rc;
    if (kept) {
        HIPCHK(hipMemcpy(key, s->key, kept * 8ull, hipMemcpyDeviceToDevice));
        HIPCHK(hipMemcpy(ord, s->ord, kept * 4ull, hipMemcpyDeviceToDevice));
        HIPCHK(hipDeviceSynchronize());
    }
    s->key = std::move(key);
    s->ord = std::move(ord);
    s->capacity = capacity;
    sort_drop_host(s);
    return MQ_OK;
}

// (the index locked and its device selected) everything mq_sort_add_device must find in place
static int sort_build(mq_sorter *s, const mq_index *idx, uint64_t capacity, uint32_t min_mapq) {
    const std::vector<uint64_t> lens = dense_ref_lens(idx->refs);
    for (auto &kv : idx->refs)
        if (kv.second.second) s->ref_ids.push_back(kv.first);
    s->device = idx->device;
    s->min_mapq = min_mapq;
    s->n_ids = (uint32_t)lens.size();
    s->capacity = capacity;
    int rc;
    HIPCHK(hipStreamCreateWithFlags(&s->stream.h, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&s->e0.h));
    HIPCHK(hipEventCreate(&s->e1.h));
    if ((rc = cover_upload(s->lens, lens)) || (rc = cover_upload(s->ids, s->ref_ids)) || (rc = s->acc.alloc(SORT_ACC_WORDS)) || (rc = s->key.alloc(capacity + 1)) ||
        (rc = s->ord.alloc(capacity + 1)) || (rc = s->totals.alloc(256)) || (rc = s->hist.alloc(MQ_SORT_DIGITS * 256)) || (rc = s->ref_out.alloc(2 * s->ref_ids.size() + 1)))
        return rc;
    HIPCHK(hipMemsetAsync(s->acc, 0, SORT_ACC_WORDS * sizeof(unsigned long long), s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    return MQ_OK;
}

static int sort_admit(const char *who, const mq_sorter *s, const mq_hit *hits, uint32_t n, uint32_t first_ordinal) {
    if (n && !hits) return set_err(MQ_EINVAL, std::string(who) + ": hits is NULL");
    if ((uint64_t)first_ordinal + n > SORT_MAX_OFFERED + 1) return set_err(MQ_EINVAL, std::string(who) + ": first_ordinal + n passes 2^32 - 1 (ordinals stay below it)");
    if (s->offered + n > SORT_MAX_OFFERED) return set_err(MQ_EINVAL, std::string(who) + ": 2^32 - 1 hits or more offered to one sorter (mq_sort_clear starts over)");
    return MQ_OK;
}
// (the sorter locked, its device selected, n >= 1, offered + n <= capacity)
static int sort_launch(mq_sorter *s, const mq_hit *d_hits, uint32_t n, uint32_t first_ordinal, hipStream_t st) {
    const uint32_t grid = std::min<uint32_t>((n + 255u) / 256u, 2048u);
    int rc = launch(sort_add_kernel, grid, 256, st, d_hits, n, first_ordinal, s->min_mapq, (const uint64_t *)s->lens.p, s->n_ids, s->key.p, s->ord.p, s->capacity, s->acc.p);
    if (rc) return rc;
    s->offered += n;
    return MQ_OK;
}

// (locked, the device selected and waited for) the histograms, the passes that are needed, the references, then the host copies
static int sort_result_locked(mq_sorter *s) {
    int rc;
    unsigned long long acc[SORT_ACC_WORDS];
    HIPCHK(hipMemcpy(acc, s->acc, sizeof(acc), hipMemcpyDeviceToHost));
    const uint64_t n = acc[0], n_refs = s->ref_ids.size();
    if (n > s->capacity || n + acc[1] + acc[2] + acc[3] != s->offered) return set_err(MQ_ESTATE, "mq_sort_result: the tallies disagree with the hits offered (internal error)");
    if (n && !s->key2) {
        Buf<unsigned long long> key2;
        Buf<uint32_t> ord2, counts;
        if ((rc = key2.alloc(s->capacity + 1)) || (rc = ord2.alloc(s->capacity + 1)) || (rc = counts.alloc(256 * sort_tiles(s->capacity) + 1))) return rc;
        s->key2 = std::move(key2);
        s->ord2 = std::move(ord2);
        s->counts = std::move(counts);
    }
    uint32_t passes = 0;
    HIPCHK(hipEventRecord(s->e0, s->stream));
    if (n) {
        std::vector<unsigned long long> hist(MQ_SORT_DIGITS * 256);
        HIPCHK(hipMemsetAsync(s->hist, 0, hist.size() * sizeof(unsigned long long), s->stream));
        if ((rc = launch(sort_hist_kernel, (uint32_t)std::min<uint64_t>((n + 255) / 256, 1024), 256, s->stream, (const unsigned long long *)s->key.p, (const uint32_t *)s->ord.p, n, s->hist.p)))
            return rc;
        HIPCHK(hipMemcpyAsync(hist.data(), s->hist, hist.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        const uint32_t n_tiles = (uint32_t)sort_tiles(n);
        for (uint32_t d = 0; d < MQ_SORT_DIGITS; ++d) {
            // a digit in which all kept records agree orders nothing: a stable pass over it would be the identity
            if (std::find(hist.begin() + d * 256, hist.begin() + (d + 1) * 256, (unsigned long long)n) != hist.begin() + (d + 1) * 256) continue;
            if ((rc = launch(sort_count_kernel, n_tiles, 256, s->stream, (const unsigned long long *)s->key.p, (const uint32_t *)s->ord.p, n, d, n_tiles, s->counts.p)) ||
                (rc = launch(sort_scan_kernel, 256, 256, s->stream, s->counts.p, n_tiles, s->totals.p)) ||
                (rc = launch(sort_scatter_kernel, n_tiles, 256, s->stream, (const unsigned long long *)s->key.p, (const uint32_t *)s->ord.p, n, d, n_tiles, (const uint32_t *)s->counts.p,
                             (const uint32_t *)s->totals.p, s->key2.p, s->ord2.p)))
                return rc;
            std::swap(s->key, s->key2);  // the records are in key / ord again
            std::swap(s->ord, s->ord2);
            passes++;
        }
        if (n_refs && (rc = launch(sort_refs_kernel, (uint32_t)((n_refs + 255) / 256), 256, s->stream, (const unsigned long long *)s->key.p, n, (const uint32_t *)s->ids.p, (uint32_t)n_refs,
                                   s->ref_out.p)))
            return rc;
    }
    HIPCHK(hipEventRecord(s->e1, s->stream));
    HIPCHK(hipStreamSynchronize(s->stream));
    HIPCHK(hipEventElapsedTime(&s->result_ms, s->e0, s->e1));
    s->passes = passes;
    std::vector<uint32_t> order(n);
    std::vector<unsigned long long> ref_out(2 * n_refs, 0);
    if (n) {
        HIPCHK(hipMemcpy(order.data(), s->ord, n * 4ull, hipMemcpyDeviceToHost));
        if (n_refs) HIPCHK(hipMemcpy(ref_out.data(), s->ref_out, 16ull * n_refs, hipMemcpyDeviceToHost));
    }
    std::vector<mq_sort_ref> refs(n_refs);
    for (uint64_t c = 0; c < n_refs; ++c) {
        refs[c] = mq_sort_ref{};
        refs[c].ref_id = s->ref_ids[c];
        refs[c].first = ref_out[2 * c];
        refs[c].count = ref_out[2 * c + 1];
    }
    s->h_order = std::move(order);
    s->h_refs = std::move(refs);
    s->h_totals.offered = s->offered;
    s->h_totals.kept = n;
    s->h_totals.not_mapped = acc[1];
    s->h_totals.below_mapq = acc[2];
    s->h_totals.out_of_range = acc[3];
    return MQ_OK;
}

extern "C" {

int mq_sort_new(mq_index *idx, uint64_t capacity, uint32_t min_mapq, mq_sorter **out) {
    return guarded([&]() -> int {
        if (out) *out = nullptr;
        if (!idx || !out) return set_err(MQ_EINVAL, "mq_sort_new: bad arguments");
        if (capacity > SORT_MAX_OFFERED) return set_err(MQ_EINVAL, "mq_sort_new: capacity: at most 2^32 - 2 (a sorter takes fewer than 2^32 - 1 hits)");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (!idx->finalized) return set_err(MQ_ESTATE, "mq_sort_new: index not finalized");
        int rc = use_device(idx);
        if (rc) return rc;
        std::unique_ptr<mq_sorter> s(new mq_sorter());  // (a failure below frees what was allocated: the device is selected)
        if ((rc = sort_build(s.get(), idx, capacity, min_mapq))) return rc;
        *out = s.release();
        return MQ_OK;
    });
}

void mq_sort_free(mq_sorter *s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();  // adds queued on the callers' streams write the arrays
    }
    delete s;
}

int mq_sort_clear(mq_sorter *s) {
    return guarded([&]() -> int {
        if (!s) return set_err(MQ_EINVAL, "mq_sort_clear: s is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemsetAsync(s->acc, 0, SORT_ACC_WORDS * sizeof(unsigned long long), s->stream));
        HIPCHK(hipStreamSynchronize(s->stream));
        s->offered = 0;
        sort_drop_host(s);
        return MQ_OK;
    });
}

int mq_sort_reserve(mq_sorter *s, uint64_t capacity) {
    return guarded([&]() -> int {
        if (!s) return set_err(MQ_EINVAL, "mq_sort_reserve: s is NULL");
        if (capacity > SORT_MAX_OFFERED) return set_err(MQ_EINVAL, "mq_sort_reserve: capacity: at most 2^32 - 2");
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipDeviceSynchronize());
        sort_drop_host(s);
        return capacity <= s->capacity ? MQ_OK : sort_grow(s, capacity);  // never shrinks
    });
}

int mq_sort_add(mq_sorter *s, const mq_hit *hits, uint32_t n, uint32_t first_ordinal) {
    return guarded([&]() -> int {
        if (!s) return set_err(MQ_EINVAL, "mq_sort_add: s is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        int rc = sort_admit("mq_sort_add", s, hits, n, first_ordinal);
        if (rc || !n) return rc;
        HIPCHK(hipSetDevice(s->device));
        if (s->offered + n > s->capacity) {  // the host route grows the sorter itself, by doubling
            HIPCHK(hipDeviceSynchronize());
            if ((rc = sort_grow(s, std::min<uint64_t>(std::max<uint64_t>(2 * s->capacity, s->offered + n), SORT_MAX_OFFERED)))) return rc;
        }
        if ((rc = s->stage.ensure(n))) return rc;
        HIPCHK(hipMemcpyAsync(s->stage, hits, (size_t)n * sizeof(mq_hit), hipMemcpyHostToDevice, s->stream));
        if ((rc = sort_launch(s, s->stage, n, first_ordinal, s->stream))) return rc;
        HIPCHK(hipStreamSynchronize(s->stream));  // the staging buffer is free again, the hits are in
        return MQ_OK;
    });
}

int mq_sort_add_device(mq_sorter *s, const mq_hit *d_hits, uint32_t n, uint32_t first_ordinal, void *stream) {
    return guarded([&]() -> int {
        if (!s) return set_err(MQ_EINVAL, "mq_sort_add_device: s is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        int rc = sort_admit("mq_sort_add_device", s, d_hits, n, first_ordinal);
        if (rc || !n) return rc;
        if ((uintptr_t)d_hits & 15u) return set_err(MQ_EINVAL, "mq_sort_add_device: d_hits must be 16-byte aligned");
        if (s->offered + n > s->capacity)  // capacity counts offered hits: the host knows, before anything is queued
            return set_err(MQ_EOVERFLOW, "mq_sort_add_device: " + std::to_string(s->offered) + " + " + std::to_string(n) + " hits offered to a capacity of " + std::to_string(s->capacity) +
                                             " (mq_sort_reserve grows it)");
        HIPCHK(hipSetDevice(s->device));
        return sort_launch(s, d_hits, n, first_ordinal, (hipStream_t)stream);
    });
}

int mq_sort_result(mq_sorter *s, const uint32_t **order, uint64_t *n_kept, const mq_sort_ref **refs, uint64_t *n_refs, mq_sort_totals *totals) {
    return guarded([&]() -> int {
        if (!s) return set_err(MQ_EINVAL, "mq_sort_result: s is NULL");
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->device));
        HIPCHK(hipDeviceSynchronize());
        int rc = sort_result_locked(s);
        if (rc) {
            sort_drop_host(s);
            return rc;
        }
        if (order) *order = s->h_order.data();
        if (n_kept) *n_kept = s->h_order.size();
        if (refs) *refs = s->h_refs.data();
        if (n_refs) *n_refs = s->h_refs.size();
        if (totals) *totals = s->h_totals;
        return MQ_OK;
    });
}

}  // extern "C"
