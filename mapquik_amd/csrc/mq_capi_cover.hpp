// mq_capi_cover.hpp -- mq_index_coverage / mq_index_coverage_release: the host side of mq_cover_kernels.hpp (part of the one translation
// unit mq_capi.hip).  Everything runs on the null stream; the read-backs are the waits.
#pragma once

// The existing references (len > 0) in id order, the bitmap's words, the dense base array and the tile descriptors.
struct CoverPlan {
    std::vector<mq_ref_coverage> refs;
    std::vector<uint64_t> base, lens_c;
    std::vector<CovTile> tiles;
    uint64_t words = 0;
};
static CoverPlan cover_plan(const RefMap &refs) {
    CoverPlan P;
    P.base.assign((size_t)max_ref_id(refs) + 1, 0);
    for (auto &kv : refs) {
        const uint64_t len = kv.second.second;
        if (!len) continue;
        mq_ref_coverage r = {};
        r.ref_id = kv.first;
        r.len = len;
        const uint32_t c = (uint32_t)P.refs.size();
        P.refs.push_back(r);
        P.lens_c.push_back(len);
        P.base[kv.first] = P.words;
        const uint64_t nw = (len + 63) / 64;
        for (uint64_t w = 0; w < nw; w += MQ_COV_TILE_WORDS) {
            CovTile t;
            t.first_word = P.words + w;
            t.ref = c;
            t.n_words = (uint32_t)std::min<uint64_t>(MQ_COV_TILE_WORDS, nw - w);
            t.ref_word = (uint32_t)w;
            t.flags = (w == 0 ? COV_FIRST : 0u) | (w + MQ_COV_TILE_WORDS >= nw ? COV_LAST : 0u);
            P.tiles.push_back(t);
        }
        P.words += nw;
    }
    return P;
}

template <class T, class V>
static int cover_upload(Buf<T> &d, const std::vector<V> &h) {
    static_assert(sizeof(T) == sizeof(V), "same element");
    int rc = d.alloc(h.size() + 1);  // (never an empty allocation)
    if (rc) return rc;
    if (!h.empty()) HIPCHK(hipMemcpy(d, h.data(), h.size() * sizeof(V), hipMemcpyHostToDevice));
    return MQ_OK;
}
template <class T>
static int cover_zeroed(Buf<T> &d, uint64_t n) {
    int rc = d.alloc(n + 1);
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(d, 0, (n + 1) * sizeof(T), 0));
    return MQ_OK;
}

// MQ_COVER_TIMING=1 (diagnostic, tools/coverage_cost.py): events around every launch, and count_kernel's pass over the same table as the
// yardstick; read with mqdiag_coverage_ms.  [0] bitmap clear [1] mark [2] count [3] scan [4] emit [5] count_kernel
static thread_local float g_cover_ms[6];
struct CoverTimer {
    bool on = env_set("MQ_COVER_TIMING");
    ScopedEvent e0, e1;
    template <class F>
    int run(int slot, F f) {
        if (!on) return f();
        if (!e0.h) {
            HIPCHK(hipEventCreate(&e0.h));
            HIPCHK(hipEventCreate(&e1.h));
        }
        HIPCHK(hipEventRecord(e0, 0));
        int rc = f();
        if (rc) return rc;
        HIPCHK(hipEventRecord(e1, 0));
        HIPCHK(hipEventSynchronize(e1));
        HIPCHK(hipEventElapsedTime(&g_cover_ms[slot], e0, e1));
        return MQ_OK;
    }
};

// locked, finalized, idle, the device selected and waited for; on any failure the caller drops the state
static int cover_locked(mq_index *idx) {
    CoverState &S = idx->cov;
    CoverPlan P = cover_plan(idx->refs);
    CoverTimer tm;
    int rc;
    const uint32_t n_ids = (uint32_t)P.base.size(), n_tiles = (uint32_t)P.tiles.size(), n_refs = (uint32_t)P.refs.size();
    if (P.tiles.size() >= (1ull << 31)) return set_err(MQ_EINVAL, "mq_index_coverage: too many tiles");
    if ((rc = S.bitmap.alloc(P.words + 2))) return rc;
    if ((rc = tm.run(0, [&]() -> int {
             HIPCHK(hipMemsetAsync(S.bitmap, 0, (P.words + 2) * 8, 0));
             return MQ_OK;
         })))
        return rc;
    if ((rc = cover_upload(S.base, P.base)) || (rc = cover_upload(S.lens_c, P.lens_c)) || (rc = cover_upload(S.tiles, P.tiles)) || (rc = cover_zeroed(S.live, n_ids)) ||
        (rc = cover_zeroed(S.acc, 1)) || (rc = cover_zeroed(S.ref_sums, 2ull * n_refs)) || (rc = cover_zeroed(S.first_interval, n_refs)) || (rc = cover_zeroed(S.tile_runs, n_tiles)) ||
        (rc = cover_zeroed(S.tile_off, n_tiles + 1ull)))
        return rc;
    const uint64_t nb1 = idx->nslots / 2 + 1;
    if ((rc = tm.run(1, [&]() {
             return launch(cover_mark_kernel, ahead_grid(2 * nb1), 256, 0, idx->table, nb1, (const uint64_t *)idx->d_ref_lens.p, (const uint64_t *)S.base.p, n_ids, S.bitmap, S.live, S.acc);
         })))
        return rc;
    const uint32_t tile_grid = (n_tiles + 3) / 4;  // a wave per tile, four to a workgroup
    if (n_tiles) {
        if ((rc = tm.run(2, [&]() { return launch(cover_count_kernel, tile_grid, 256, 0, S.bitmap, S.tiles, n_tiles, S.tile_runs, S.ref_sums); }))) return rc;
        if ((rc = tm.run(3, [&]() { return launch(cover_scan_kernel, 1, 1024, 0, S.tile_runs, S.tiles, n_tiles, S.tile_off, S.first_interval); }))) return rc;
    }
    unsigned long long n_iv = 0, oor = 0;
    HIPCHK(hipMemcpy(&n_iv, S.tile_off + n_tiles, 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&oor, S.acc, 8, hipMemcpyDeviceToHost));
    if ((rc = S.intervals.alloc(n_iv + 1))) return rc;
    if (n_iv) {
        if ((rc = tm.run(4, [&]() {
                 return launch(cover_emit_kernel, tile_grid, 256, 0, S.bitmap, S.tiles, n_tiles, S.tile_off, (const uint64_t *)S.lens_c.p, S.intervals, n_iv);
             })))
            return rc;
    }
    // host copies
    std::vector<unsigned long long> live(n_ids), sums(2ull * n_refs), first(n_refs);
    HIPCHK(hipMemcpy(live.data(), S.live, n_ids * 8ull, hipMemcpyDeviceToHost));
    if (n_refs) {
        HIPCHK(hipMemcpy(sums.data(), S.ref_sums, 16ull * n_refs, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(first.data(), S.first_interval, 8ull * n_refs, hipMemcpyDeviceToHost));
    }
    S.h_intervals.resize(n_iv);
    if (n_iv) HIPCHK(hipMemcpy(S.h_intervals.data(), S.intervals, n_iv * sizeof(mq_cov_interval), hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < n_refs; ++c) {
        mq_ref_coverage &r = P.refs[c];
        r.live_kminmers = live[r.ref_id];
        r.covered_bases = sums[2 * c];
        r.n_intervals = sums[2 * c + 1];
        r.first_interval = first[c];
    }
    S.h_refs = std::move(P.refs);
    S.out_of_range = oor;
    if (tm.on) {
        unsigned long long acc[3];
        if ((rc = tm.run(5, [&]() { return count_table(idx, acc); }))) return rc;
    }
    return MQ_OK;
}

extern "C" {

int mq_index_coverage(mq_index *idx, const mq_ref_coverage **refs, uint64_t *n_refs, const mq_cov_interval **intervals, uint64_t *n_intervals, uint64_t *out_of_range) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "mq_index_coverage: idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = merge_check_dst("mq_index_coverage", idx);  // finalized, and no context with a submitted batch
        if (rc || (rc = use_device(idx))) return rc;
        idx->cov.drop();
        HIPCHK(hipDeviceSynchronize());
        try {
            rc = cover_locked(idx);
        } catch (...) {
            idx->cov.drop();
            throw;
        }
        idx->cov.free_device();  // only the host copies stay
        if (rc) {
            idx->cov.drop();
            return rc;
        }
        const CoverState &S = idx->cov;
        if (refs) *refs = S.h_refs.data();
        if (n_refs) *n_refs = S.h_refs.size();
        if (intervals) *intervals = S.h_intervals.data();
        if (n_intervals) *n_intervals = S.h_intervals.size();
        if (out_of_range) *out_of_range = S.out_of_range;
        return MQ_OK;
    });
}

int mq_index_coverage_release(mq_index *idx) {
    return guarded([&]() -> int {
        if (!idx) return set_err(MQ_EINVAL, "mq_index_coverage_release: idx is NULL");
        std::lock_guard<std::mutex> lk(idx->mu);
        int rc = use_device(idx);
        if (rc) return rc;
        idx->cov.drop();
        return MQ_OK;
    });
}

}  // extern "C"
