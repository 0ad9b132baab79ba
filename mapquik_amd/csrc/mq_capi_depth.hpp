// mq_capi_depth.hpp -- mq_depth_*: the host side of mq_depth_kernels.hpp (part of the one translation unit mq_capi.hip).  The host
// route and the result pass run on the accumulator's own stream; the device route runs on the caller's.  Adds commute (every one of
// their writes is an atomic add), so no add is ordered against another; mq_depth_result and mq_depth_clear wait for the whole device
// first, which covers every stream an add was queued on.
#pragma once

// The snapshot: the existing references (len > 0) in id order with their windows, the dense base array and the tile descriptors.
struct DepthPlan {
    std::vector<mq_ref_depth> refs;
    std::vector<uint64_t> lens, base;
    std::vector<DepthTile> tiles;
    uint64_t windows = 0;
};
static DepthPlan depth_plan(const RefMap &refs, uint32_t w) {
    DepthPlan P;
    P.lens = dense_ref_lens(refs);
    P.base.assign(P.lens.size(), 0);
    for (auto &kv : refs) {
        const uint64_t len = kv.second.second;
        if (!len) continue;
        mq_ref_depth r = {};
        r.ref_id = kv.first;
        r.len = len;
        r.n_windows = (len + w - 1) / w;
        r.first_window = P.windows;
        const uint32_t c = (uint32_t)P.refs.size();
        P.refs.push_back(r);
        P.base[kv.first] = P.windows;
        for (uint64_t j = 0; j < r.n_windows; j += MQ_DEPTH_TILE_WINDOWS) {
            DepthTile t = {};
            t.first_window = P.windows + j;
            t.ref = c;
            t.n_windows = (uint32_t)std::min<uint64_t>(MQ_DEPTH_TILE_WINDOWS, r.n_windows - j);
            t.ref_tile = (uint32_t)(j / MQ_DEPTH_TILE_WINDOWS);
            P.tiles.push_back(t);
        }
        P.windows += r.n_windows;
    }
    return P;
}

// the accumulators and the totals back to zero, queued on the accumulator's stream
static int depth_zero(mq_depth *d) {
    HIPCHK(hipMemsetAsync(d->edge, 0, (d->n_windows + 1) * sizeof(unsigned long long), d->stream));
    HIPCHK(hipMemsetAsync(d->diff, 0, (d->n_windows + 1) * sizeof(int), d->stream));
    HIPCHK(hipMemsetAsync(d->starts, 0, (d->n_windows + 1) * sizeof(uint32_t), d->stream));
    HIPCHK(hipMemsetAsync(d->reads, 0, ((uint64_t)d->n_ids + 1) * sizeof(unsigned long long), d->stream));
    HIPCHK(hipMemsetAsync(d->acc, 0, DEPTH_ACC_WORDS * sizeof(unsigned long long), d->stream));
    return MQ_OK;
}

// (the index locked and its device selected) everything mq_depth_add_device must find in place
static int depth_build(mq_depth *d, const mq_index *idx, uint32_t window, uint32_t min_mapq) {
    DepthPlan P = depth_plan(idx->refs, window);
    if (P.windows > 0x7FFFFFFFull)
        return set_err(MQ_ENOMEM, "mq_depth_new: more than 2^31 - 1 windows (16 bytes of accumulators and 12 of result each): choose a larger window");
    d->device = idx->device;
    d->window = window;
    d->min_mapq = min_mapq;
    d->n_ids = (uint32_t)P.lens.size();
    d->n_tiles = (uint32_t)P.tiles.size();
    d->n_windows = P.windows;
    int rc;
    HIPCHK(hipStreamCreateWithFlags(&d->stream.h, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&d->e0.h));
    HIPCHK(hipEventCreate(&d->e1.h));
    const uint64_t nw = P.windows + 1, nt = P.tiles.size() + 1;  // (never an empty allocation)
    if ((rc = cover_upload(d->lens, P.lens)) || (rc = cover_upload(d->base, P.base)) || (rc = cover_upload(d->tiles, P.tiles)) || (rc = d->edge.alloc(nw)) ||
        (rc = d->diff.alloc(nw)) || (rc = d->starts.alloc(nw)) || (rc = d->reads.alloc((uint64_t)d->n_ids + 1)) || (rc = d->acc.alloc(DEPTH_ACC_WORDS)) ||
        (rc = d->tile_sum.alloc(nt)) || (rc = d->tile_pref.alloc(nt)) || (rc = d->tile_off.alloc(nt)) || (rc = d->ref_sums.alloc(3 * (P.refs.size() + 1))))
        return rc;
    if ((rc = depth_zero(d))) return rc;
    HIPCHK(hipStreamSynchronize(d->stream));
    d->plan = std::move(P.refs);
    return MQ_OK;
}

static int depth_admit(const char *who, const mq_depth *d, const mq_hit *hits, uint32_t n) {
    if (n && !hits) return set_err(MQ_EINVAL, std::string(who) + ": hits is NULL");
    if (d->offered + n > 0x7FFFFFFFull) return set_err(MQ_EINVAL, std::string(who) + ": more than 2^31 - 1 hits offered to one accumulator (mq_depth_clear starts over)");
    return MQ_OK;
}
// (the accumulator locked, its device selected, n >= 1)
static int depth_launch(mq_depth *d, const mq_hit *d_hits, uint32_t n, hipStream_t st) {
    const uint32_t grid = std::min<uint32_t>((n + 255u) / 256u, 2048u);
    int rc = launch(depth_add_kernel, grid, 256, st, d_hits, n, d->window, d->min_mapq, (const uint64_t *)d->lens.p, (const uint64_t *)d->base.p, d->n_ids, d->edge.p, d->diff.p,
                    d->starts.p, d->reads.p, d->acc.p);
    if (rc) return rc;
    d->offered += n;
    return MQ_OK;
}

// (locked, the device selected and waited for) the three kernels, then the host copies
static int depth_result_locked(mq_depth *d) {
    int rc;
    const uint64_t n_refs = d->plan.size();
    if (!d->window_bases) {
        Buf<unsigned long long> wb;
        Buf<uint32_t> ws;
        if ((rc = wb.alloc(d->n_windows + 1)) || (rc = ws.alloc(d->n_windows + 1))) return rc;
        d->window_bases = std::move(wb);
        d->window_starts = std::move(ws);
    }
    HIPCHK(hipMemsetAsync(d->ref_sums, 0, 3 * (n_refs + 1) * sizeof(unsigned long long), d->stream));
    HIPCHK(hipEventRecord(d->e0, d->stream));
    if (d->n_tiles) {
        const uint32_t tile_grid = (d->n_tiles + 3) / 4;  // a wave per tile, four to a workgroup
        if ((rc = launch(depth_sum_kernel, tile_grid, 256, d->stream, (const int *)d->diff.p, (const DepthTile *)d->tiles.p, d->n_tiles, d->tile_sum.p)) ||
            (rc = launch(depth_scan_kernel, 1, 1024, d->stream, (const long long *)d->tile_sum.p, (const DepthTile *)d->tiles.p, d->n_tiles, d->tile_pref.p, d->tile_off.p)) ||
            (rc = launch(depth_emit_kernel, tile_grid, 256, d->stream, (const unsigned long long *)d->edge.p, (const int *)d->diff.p, (const uint32_t *)d->starts.p,
                         (const DepthTile *)d->tiles.p, d->n_tiles, (const long long *)d->tile_off.p, d->window, d->window_bases.p, d->window_starts.p, d->ref_sums.p)))
            return rc;
    }
    HIPCHK(hipEventRecord(d->e1, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    HIPCHK(hipEventElapsedTime(&d->result_ms, d->e0, d->e1));
    std::vector<unsigned long long> reads(d->n_ids), sums(3 * n_refs);
    std::vector<uint64_t> h_bases(d->n_windows);
    std::vector<uint32_t> h_starts(d->n_windows);
    HIPCHK(hipMemcpy(reads.data(), d->reads, d->n_ids * 8ull, hipMemcpyDeviceToHost));
    if (n_refs) HIPCHK(hipMemcpy(sums.data(), d->ref_sums, 24ull * n_refs, hipMemcpyDeviceToHost));
    if (d->n_windows) {
        HIPCHK(hipMemcpy(h_bases.data(), d->window_bases, d->n_windows * 8ull, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(h_starts.data(), d->window_starts, d->n_windows * 4ull, hipMemcpyDeviceToHost));
    }
    std::vector<mq_ref_depth> refs = d->plan;
    for (uint64_t c = 0; c < n_refs; ++c) {
        mq_ref_depth &r = refs[c];
        r.reads = reads[r.ref_id];
        r.bases = sums[3 * c];
        r.zero_windows = sums[3 * c + 1];
        r.max_window_bases = sums[3 * c + 2];
    }
    d->h_refs = std::move(refs);
    d->h_bases = std::move(h_bases);
    d->h_starts = std::move(h_starts);
    return MQ_OK;
}

static void depth_drop_host(mq_depth *d) {
    std::vector<mq_ref_depth>().swap(d->h_refs);
    std::vector<uint64_t>().swap(d->h_bases);
    std::vector<uint32_t>().swap(d->h_starts);
}

extern "C" {

int mq_depth_new(mq_index *idx, uint32_t window, uint32_t min_mapq, mq_depth **out) {
    return guarded([&]() -> int {
        if (out) *out = nullptr;
        if (!idx || !out) return set_err(MQ_EINVAL, "mq_depth_new: bad arguments");
        if (window == 0 || window > MQ_DEPTH_MAX_WINDOW) return set_err(MQ_EINVAL, "mq_depth_new: window: 1 .. 2^24");
        std::lock_guard<std::mutex> lk(idx->mu);
        if (!idx->finalized) return set_err(MQ_ESTATE, "mq_depth_new: index not finalized");
        int rc = use_device(idx);
        if (rc) return rc;
        std::unique_ptr<mq_depth> d(new mq_depth());  // (a failure below frees what was allocated: the device is selected)
        if ((rc = depth_build(d.get(), idx, window, min_mapq))) return rc;
        *out = d.release();
        return MQ_OK;
    });
}

void mq_depth_free(mq_depth *d) {
    if (!d) return;
    {
        std::lock_guard<std::mutex> lk(d->mu);
        (void)hipSetDevice(d->device);
        (void)hipDeviceSynchronize();  // adds queued on the callers' streams read and write the accumulators
    }
    delete d;
}

int mq_depth_clear(mq_depth *d) {
    return guarded([&]() -> int {
        if (!d) return set_err(MQ_EINVAL, "mq_depth_clear: d is NULL");
        std::lock_guard<std::mutex> lk(d->mu);
        HIPCHK(hipSetDevice(d->device));
        HIPCHK(hipDeviceSynchronize());
        int rc = depth_zero(d);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(d->stream));
        d->offered = 0;
        depth_drop_host(d);
        return MQ_OK;
    });
}

int mq_depth_add(mq_depth *d, const mq_hit *hits, uint32_t n) {
    return guarded([&]() -> int {
        if (!d) return set_err(MQ_EINVAL, "mq_depth_add: d is NULL");
        std::lock_guard<std::mutex> lk(d->mu);
        int rc = depth_admit("mq_depth_add", d, hits, n);
        if (rc || !n) return rc;
        HIPCHK(hipSetDevice(d->device));
        if ((rc = d->stage.ensure(n))) return rc;
        HIPCHK(hipMemcpyAsync(d->stage, hits, (size_t)n * sizeof(mq_hit), hipMemcpyHostToDevice, d->stream));
        if ((rc = depth_launch(d, d->stage, n, d->stream))) return rc;
        HIPCHK(hipStreamSynchronize(d->stream));  // the staging buffer is free again, the hits are in
        return MQ_OK;
    });
}

int mq_depth_add_device(mq_depth *d, const mq_hit *d_hits, uint32_t n, void *stream) {
    return guarded([&]() -> int {
        if (!d) return set_err(MQ_EINVAL, "mq_depth_add_device: d is NULL");
        std::lock_guard<std::mutex> lk(d->mu);
        int rc = depth_admit("mq_depth_add_device", d, d_hits, n);
        if (rc || !n) return rc;
        if ((uintptr_t)d_hits & 15u) return set_err(MQ_EINVAL, "mq_depth_add_device: d_hits must be 16-byte aligned");
        HIPCHK(hipSetDevice(d->device));
        return depth_launch(d, d_hits, n, (hipStream_t)stream);
    });
}

int mq_depth_result(mq_depth *d, const mq_ref_depth **refs, uint64_t *n_refs, const uint64_t **window_bases, const uint32_t **window_starts, uint64_t *n_windows,
                    mq_depth_totals *totals) {
    return guarded([&]() -> int {
        if (!d) return set_err(MQ_EINVAL, "mq_depth_result: d is NULL");
        std::lock_guard<std::mutex> lk(d->mu);
        HIPCHK(hipSetDevice(d->device));
        HIPCHK(hipDeviceSynchronize());
        int rc = depth_result_locked(d);
        if (rc) {
            depth_drop_host(d);
            return rc;
        }
        unsigned long long acc[DEPTH_ACC_WORDS];
        HIPCHK(hipMemcpy(acc, d->acc, sizeof(acc), hipMemcpyDeviceToHost));
        if (refs) *refs = d->h_refs.data();
        if (n_refs) *n_refs = d->h_refs.size();
        if (window_bases) *window_bases = d->h_bases.data();
        if (window_starts) *window_starts = d->h_starts.data();
        if (n_windows) *n_windows = d->n_windows;
        if (totals) {
            totals->offered = d->offered;
            totals->counted = acc[0];
            totals->not_mapped = acc[1];
            totals->below_mapq = acc[2];
            totals->out_of_range = acc[3];
        }
        return MQ_OK;
    });
}

}  // extern "C"
