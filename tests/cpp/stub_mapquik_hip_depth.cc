// stub_mapquik_hip_depth.cc -- the host-only stand-in of stub_mapquik_hip_coverage.cc plus mq_depth_*.  The accumulator is the header's
// rules spelled out on the host, a loop over the windows a hit touches: slow, obvious, and enough for the driver to write real files
// from the stub's canned hits.  MQ_STUB_DEPTH_LOG=1 (test hook) writes one line per mq_depth_new / mq_depth_add / mq_depth_result to
// stderr, so that a test can tell when and with what the driver called; MQ_STUB_DEPTH_FAIL=1 makes mq_depth_add fail with the stub's own
// text.  The sanitizer builds of the driver link this file; the stubs below it stay as they are.  Test infrastructure only.
#include "stub_mapquik_hip_coverage.cc"

struct mq_depth {
    std::mutex mu;
    uint32_t window = 0, min_mapq = 0;
    std::map<uint32_t, size_t> ref_at;  // reference id -> its record
    std::vector<mq_ref_depth> refs;
    std::vector<uint64_t> bases;
    std::vector<uint32_t> starts;
    mq_depth_totals totals = {};
    std::vector<mq_ref_depth> out_refs;  // the caller's copies
    std::vector<uint64_t> out_bases;
    std::vector<uint32_t> out_starts;
};

extern "C" {

int mq_depth_new(mq_index *idx, uint32_t window, uint32_t min_mapq, mq_depth **out) {
    if (out) *out = nullptr;
    if (!idx || !out) { g_err = "mq_depth_new: bad arguments"; return MQ_EINVAL; }
    if (window == 0 || window > (1u << 24)) { g_err = "mq_depth_new: window: 1 .. 2^24"; return MQ_EINVAL; }
    if (!idx->finalized) { g_err = "mq_depth_new: index not finalized"; return MQ_ESTATE; }
    mq_depth *d = new mq_depth();
    d->window = window;
    d->min_mapq = min_mapq;
    uint64_t windows = 0;
    for (auto &kv : idx->refs) {
        if (!kv.second.second) continue;
        mq_ref_depth r = {};
        r.ref_id = kv.first;
        r.len = kv.second.second;
        r.n_windows = (r.len + window - 1) / window;
        r.first_window = windows;
        windows += r.n_windows;
        d->ref_at[r.ref_id] = d->refs.size();
        d->refs.push_back(r);
    }
    d->bases.assign(windows, 0);
    d->starts.assign(windows, 0);
    if (getenv("MQ_STUB_DEPTH_LOG")) fprintf(stderr, "stub: mq_depth_new window %u min_mapq %u, %zu references\n", window, min_mapq, d->refs.size());
    *out = d;
    return MQ_OK;
}

void mq_depth_free(mq_depth *d) { delete d; }

int mq_depth_clear(mq_depth *d) {
    if (!d) { g_err = "mq_depth_clear: d is NULL"; return MQ_EINVAL; }
    std::lock_guard<std::mutex> lk(d->mu);
    std::fill(d->bases.begin(), d->bases.end(), 0);
    std::fill(d->starts.begin(), d->starts.end(), 0);
    for (auto &r : d->refs) r.reads = 0;
    d->totals = mq_depth_totals{};
    return MQ_OK;
}

int mq_depth_add(mq_depth *d, const mq_hit *hits, uint32_t n) {
    if (!d || (n && !hits)) { g_err = "mq_depth_add: bad arguments"; return MQ_EINVAL; }
    if (getenv("MQ_STUB_DEPTH_FAIL")) { g_err = "stub (mq_depth_add): no device memory"; return MQ_ENOMEM; }
    std::lock_guard<std::mutex> lk(d->mu);
    if (d->totals.offered + n > 0x7FFFFFFFull) { g_err = "mq_depth_add: more than 2^31 - 1 hits"; return MQ_EINVAL; }
    uint32_t mapped = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const mq_hit &h = hits[i];
        d->totals.offered++;
        if (h.status != MQ_HIT_MAPPED) { d->totals.not_mapped++; continue; }
        mapped++;
        if (h.mapq < d->min_mapq) { d->totals.below_mapq++; continue; }
        auto it = d->ref_at.find(h.ref_id);
        if (it == d->ref_at.end() || h.r_start > h.r_end || h.r_start >= d->refs[it->second].len) { d->totals.out_of_range++; continue; }
        mq_ref_depth &r = d->refs[it->second];
        d->totals.counted++;
        r.reads++;
        const uint64_t s = h.r_start, e = std::min<uint64_t>(h.r_end, r.len - 1), w = d->window;
        d->starts[r.first_window + s / w]++;
        for (uint64_t j = s / w; j <= e / w; ++j) d->bases[r.first_window + j] += std::min(e, (j + 1) * w - 1) - std::max(s, j * w) + 1;
    }
    if (getenv("MQ_STUB_DEPTH_LOG")) fprintf(stderr, "stub: mq_depth_add %u hits, %u mapped\n", n, mapped);
    return MQ_OK;
}

int mq_depth_add_device(mq_depth *, const mq_hit *, uint32_t, void *) { g_err = "stub"; return MQ_EINVAL; }

int mq_depth_result(mq_depth *d, const mq_ref_depth **refs, uint64_t *n_refs, const uint64_t **window_bases, const uint32_t **window_starts, uint64_t *n_windows,
                    mq_depth_totals *totals) {
    if (!d) { g_err = "mq_depth_result: d is NULL"; return MQ_EINVAL; }
    std::lock_guard<std::mutex> lk(d->mu);
    if (getenv("MQ_STUB_DEPTH_LOG")) fprintf(stderr, "stub: mq_depth_result %llu offered\n", (unsigned long long)d->totals.offered);
    d->out_refs = d->refs;
    d->out_bases = d->bases;
    d->out_starts = d->starts;
    for (auto &r : d->out_refs)
        for (uint64_t j = r.first_window; j < r.first_window + r.n_windows; ++j) {
            r.bases += d->bases[j];
            r.zero_windows += d->bases[j] == 0;
            r.max_window_bases = std::max(r.max_window_bases, d->bases[j]);
        }
    if (refs) *refs = d->out_refs.data();
    if (n_refs) *n_refs = d->out_refs.size();
    if (window_bases) *window_bases = d->out_bases.data();
    if (window_starts) *window_starts = d->out_starts.data();
    if (n_windows) *n_windows = d->out_bases.size();
    if (totals) *totals = d->totals;
    return MQ_OK;
}

}  // extern "C"
