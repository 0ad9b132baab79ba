// stub_mapquik_hip_coverage.cc -- the host-only stand-in of stub_mapquik_hip_merge.cc plus mq_index_coverage and
// mq_index_coverage_release.  The stub has no table, so the coverage is canned, derived from the canned references: every reference
// that exists owns 10 live k-min-mers and two intervals, [0, len / 4) and [len / 2, len) (one, [0, len), below four bases), and nothing
// is out of range.  MQ_STUB_COVERAGE_LOG=1 (test hook) writes one line per call to stderr with the references the index has by then, so
// that a test can tell when the driver called; MQ_STUB_COVERAGE_FAIL=1 makes the call fail with the stub's own text.  The sanitizer
// builds of the driver link this file; the stubs below it stay as they are.  Test infrastructure only.
#include "stub_mapquik_hip_merge.cc"

namespace {
struct StubCoverage {
    std::vector<mq_ref_coverage> refs;
    std::vector<mq_cov_interval> intervals;
};
std::mutex g_cov_mu;
std::map<const mq_index *, StubCoverage> g_cov;
}  // namespace

extern "C" {

int mq_index_coverage(mq_index *idx, const mq_ref_coverage **refs, uint64_t *n_refs, const mq_cov_interval **intervals, uint64_t *n_intervals, uint64_t *out_of_range) {
    if (!idx) { g_err = "mq_index_coverage: idx is NULL"; return MQ_EINVAL; }
    if (!idx->finalized) { g_err = "mq_index_coverage: index not finalized"; return MQ_ESTATE; }
    if (getenv("MQ_STUB_COVERAGE_LOG")) fprintf(stderr, "stub: mq_index_coverage %zu references\n", idx->refs.size());
    if (getenv("MQ_STUB_COVERAGE_FAIL")) { g_err = "stub (mq_index_coverage): no device memory"; return MQ_ENOMEM; }
    std::lock_guard<std::mutex> lk(g_cov_mu);
    StubCoverage &c = g_cov[idx];
    c = StubCoverage();
    for (auto &kv : idx->refs) {
        const uint64_t len = kv.second.second;
        if (!len) continue;
        mq_ref_coverage r = {};
        r.ref_id = kv.first;
        r.len = len;
        r.live_kminmers = 10;
        r.first_interval = c.intervals.size();
        if (len < 4) {
            c.intervals.push_back(mq_cov_interval{0, (uint32_t)len});
            r.covered_bases = len;
        } else {
            c.intervals.push_back(mq_cov_interval{0, (uint32_t)(len / 4)});
            c.intervals.push_back(mq_cov_interval{(uint32_t)(len / 2), (uint32_t)len});
            r.covered_bases = len / 4 + (len - len / 2);
        }
        r.n_intervals = c.intervals.size() - r.first_interval;
        c.refs.push_back(r);
    }
    if (refs) *refs = c.refs.data();
    if (n_refs) *n_refs = c.refs.size();
    if (intervals) *intervals = c.intervals.data();
    if (n_intervals) *n_intervals = c.intervals.size();
    if (out_of_range) *out_of_range = 0;
    return MQ_OK;
}

int mq_index_coverage_release(mq_index *idx) {
    if (!idx) { g_err = "mq_index_coverage_release: idx is NULL"; return MQ_EINVAL; }
    std::lock_guard<std::mutex> lk(g_cov_mu);
    g_cov.erase(idx);
    return MQ_OK;
}

}  // extern "C"
