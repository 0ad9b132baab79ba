// stub_mapquik_hip_sort.cc -- the host-only stand-in of stub_mapquik_hip_depth.cc plus mq_sort_*.  The sorter is the header's rules spelled
// out on the host with std::sort over (ref_id, r_start, ordinal): obvious, and enough for the driver to write real files from the stub's
// canned hits.  MQ_STUB_SORT_LOG=1 (test hook) writes one line per mq_sort_new / mq_sort_add / mq_sort_result to stderr, so that a test can
// tell when and with what the driver called; MQ_STUB_SORT_FAIL=1 makes mq_sort_add fail with the stub's own text, MQ_STUB_SORT_FAIL=result
// mq_sort_result instead.  The sanitizer builds of the driver link this file; the stubs below it stay as they are.  Test infrastructure only.
#include "stub_mapquik_hip_depth.cc"

#include <algorithm>
#include <cstring>
#include <tuple>

struct mq_sorter {
    std::mutex mu;
    uint32_t min_mapq = 0;
    uint64_t capacity = 0;
    std::vector<uint32_t> ids;                                   // the existing references, ascending
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> kept;  // ref_id, r_start, ordinal
    mq_sort_totals totals = {};
    std::vector<uint32_t> out_order;  // the caller's copies
    std::vector<mq_sort_ref> out_refs;
};

extern "C" {

int mq_sort_new(mq_index *idx, uint64_t capacity, uint32_t min_mapq, mq_sorter **out) {
    if (out) *out = nullptr;
    if (!idx || !out || capacity > 0xFFFFFFFEull) { g_err = "mq_sort_new: bad arguments"; return MQ_EINVAL; }
    if (!idx->finalized) { g_err = "mq_sort_new: index not finalized"; return MQ_ESTATE; }
    mq_sorter *s = new mq_sorter();
    s->min_mapq = min_mapq;
    s->capacity = capacity;
    for (auto &kv : idx->refs)
        if (kv.second.second) s->ids.push_back(kv.first);
    if (getenv("MQ_STUB_SORT_LOG")) fprintf(stderr, "stub: mq_sort_new capacity %llu min_mapq %u, %zu references\n", (unsigned long long)capacity, min_mapq, s->ids.size());
    *out = s;
    return MQ_OK;
}

void mq_sort_free(mq_sorter *s) { delete s; }

int mq_sort_clear(mq_sorter *s) {
    if (!s) { g_err = "mq_sort_clear: s is NULL"; return MQ_EINVAL; }
    std::lock_guard<std::mutex> lk(s->mu);
    s->kept.clear();
    s->totals = mq_sort_totals{};
    return MQ_OK;
}

int mq_sort_reserve(mq_sorter *s, uint64_t capacity) {
    if (!s || capacity > 0xFFFFFFFEull) { g_err = "mq_sort_reserve: bad arguments"; return MQ_EINVAL; }
    std::lock_guard<std::mutex> lk(s->mu);
    s->capacity = std::max(s->capacity, capacity);
    return MQ_OK;
}

int mq_sort_add(mq_sorter *s, const mq_hit *hits, uint32_t n, uint32_t first_ordinal) {
    if (!s || (n && !hits)) { g_err = "mq_sort_add: bad arguments"; return MQ_EINVAL; }
    if (getenv("MQ_STUB_SORT_FAIL") && strcmp(getenv("MQ_STUB_SORT_FAIL"), "result")) { g_err = "stub (mq_sort_add): no device memory"; return MQ_ENOMEM; }
    std::lock_guard<std::mutex> lk(s->mu);
    if ((uint64_t)first_ordinal + n > 0xFFFFFFFFull || s->totals.offered + n > 0xFFFFFFFEull) { g_err = "mq_sort_add: 2^32 - 1 ordinals or hits"; return MQ_EINVAL; }
    s->capacity = std::max<uint64_t>(s->capacity, s->totals.offered + n);
    uint32_t kept = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const mq_hit &h = hits[i];
        s->totals.offered++;
        if (h.status != MQ_HIT_MAPPED) { s->totals.not_mapped++; continue; }
        if (h.mapq < s->min_mapq) { s->totals.below_mapq++; continue; }
        if (!std::binary_search(s->ids.begin(), s->ids.end(), h.ref_id)) { s->totals.out_of_range++; continue; }
        s->totals.kept++;
        kept++;
        s->kept.emplace_back(h.ref_id, h.r_start, first_ordinal + i);
    }
    if (getenv("MQ_STUB_SORT_LOG")) fprintf(stderr, "stub: mq_sort_add %u hits from ordinal %u, %u kept\n", n, first_ordinal, kept);
    return MQ_OK;
}

int mq_sort_add_device(mq_sorter *, const mq_hit *, uint32_t, uint32_t, void *) { g_err = "stub"; return MQ_EINVAL; }

int mq_sort_result(mq_sorter *s, const uint32_t **order, uint64_t *n_kept, const mq_sort_ref **refs, uint64_t *n_refs, mq_sort_totals *totals) {
    if (!s) { g_err = "mq_sort_result: s is NULL"; return MQ_EINVAL; }
    if (getenv("MQ_STUB_SORT_FAIL") && !strcmp(getenv("MQ_STUB_SORT_FAIL"), "result")) { g_err = "stub (mq_sort_result): no device memory"; return MQ_ENOMEM; }
    std::lock_guard<std::mutex> lk(s->mu);
    if (getenv("MQ_STUB_SORT_LOG")) fprintf(stderr, "stub: mq_sort_result %llu offered\n", (unsigned long long)s->totals.offered);
    std::sort(s->kept.begin(), s->kept.end());
    s->out_order.clear();
    s->out_refs.clear();
    for (auto &k : s->kept) s->out_order.push_back(std::get<2>(k));
    size_t at = 0;
    for (uint32_t id : s->ids) {
        mq_sort_ref r = {};
        r.ref_id = id;
        r.first = at;
        while (at < s->kept.size() && std::get<0>(s->kept[at]) == id) ++at;
        r.count = at - r.first;
        s->out_refs.push_back(r);
    }
    if (order) *order = s->out_order.data();
    if (n_kept) *n_kept = s->out_order.size();
    if (refs) *refs = s->out_refs.data();
    if (n_refs) *n_refs = s->out_refs.size();
    if (totals) *totals = s->totals;
    return MQ_OK;
}

}  // extern "C"
