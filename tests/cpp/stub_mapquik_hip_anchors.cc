// stub_mapquik_hip_anchors.cc -- the host-only stand-in of stub_mapquik_hip_extend.cc plus the anchor output: mq_ctx_reserve_anchors,
// mq_ctx_anchors, mq_ctx_anchors_device and their mq_map_* forms.  The stub maps nothing, so the anchors are canned like the hits, and
// made FROM the hits of the context's last batch: a mapped read has 1 + score % 3 runs, run j at q_start + 10 j / r_start + 10 j, six long,
// the counts summing to the score (tests/test_anchors_host.py restates this from the PAF columns).  The pool behaves as the library's:
// lists are laid out in read order, a list that does not fit is dropped with first = MQ_ANCHORS_DROPPED, `needed` counts on.
// MQ_STUB_ANCHORS_CAP (test hook) replaces the capacity a caller reserves, so that a test can make the pool too small.
// The stubs below stay as they are.  Which batch was the context's last is read from their state: a FASTX piece leaves its hits in the
// context (fx_hits, or the LINES state beside it); the spans form leaves none, so mq_ctx_submit_spans is compiled under another name here
// and wrapped to remember the caller's hit array (and to clear the other two).  The sanitizer builds of the driver link this file.  Test
// infrastructure only.
#define mq_ctx_submit_spans stub_ext_submit_spans
#include "stub_mapquik_hip_extend.cc"
#undef mq_ctx_submit_spans

#include <cstdlib>

namespace {
struct AnchorState {
    bool reserved = false;
    uint32_t max_reads = 0;
    uint64_t cap = 0;
    const mq_hit *sp_out = nullptr;  // the spans form's hit array (filled by the context's worker, complete after mq_ctx_wait)
    uint32_t sp_n = 0;
    std::vector<mq_anchor_span> spans;
    std::vector<mq_anchor> pool;
};
std::mutex g_anch_mu;
std::map<mq_ctx *, AnchorState> g_anch;
AnchorState &anch_of(mq_ctx *c) {
    std::lock_guard<std::mutex> lk(g_anch_mu);
    return g_anch[c];
}
std::mutex g_def_mu;
std::map<mq_index *, mq_ctx *> g_def_ctx;  // mq_map_*: a context per index, made on first use (never freed: the driver does not use them)
mq_ctx *def_ctx_of(mq_index *i) {
    std::lock_guard<std::mutex> lk(g_def_mu);
    mq_ctx *&c = g_def_ctx[i];
    if (!c) c = mq_ctx_new(i);
    return c;
}
}  // namespace

extern "C" {

int mq_ctx_submit_spans(mq_ctx *c, const uint8_t *buf, uint64_t bytes, const uint64_t *starts, const uint32_t *lens, uint32_t n, mq_hit *out) {
    if (c->pending) { g_err = "context has a submitted batch"; return MQ_ESTATE; }
    AnchorState &s = anch_of(c);
    if (s.reserved && n > s.max_reads) { g_err = "more reads in the batch than the context's anchor reservation holds"; return MQ_EINVAL; }
    c->fx_hits.clear();
    lines_of(c).hits.clear();
    s.sp_out = out;
    s.sp_n = n;
    return stub_ext_submit_spans(c, buf, bytes, starts, lens, n, out);
}

int mq_ctx_reserve_anchors(mq_ctx *c, uint32_t max_reads, uint64_t max_anchors) {
    if (!c) { g_err = "ctx is NULL"; return MQ_EINVAL; }
    if (c->pending) { g_err = "context has a submitted batch"; return MQ_ESTATE; }
    AnchorState &s = anch_of(c);
    if (max_reads == 0 && max_anchors == 0) {
        s = AnchorState();
        return MQ_OK;
    }
    if (!max_reads || !max_anchors || max_reads >= (1u << 30) || max_anchors >= 0xFFFFFFFFull) { g_err = "max_reads / max_anchors"; return MQ_EINVAL; }
    const char *e = getenv("MQ_STUB_ANCHORS_CAP");
    s.reserved = true;
    s.max_reads = max_reads;
    s.cap = e ? strtoull(e, nullptr, 10) : max_anchors;
    return MQ_OK;
}

int mq_ctx_anchors(mq_ctx *c, const mq_anchor_span **spans, const mq_anchor **anchors, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                   uint32_t *dropped_reads) {
    if (!c || !spans || !anchors || !n_reads || !stored || !needed || !dropped_reads) { g_err = "bad arguments"; return MQ_EINVAL; }
    AnchorState &s = anch_of(c);
    if (!s.reserved) { g_err = "no anchors reserved on this context"; return MQ_ESTATE; }
    if (c->pending) {
        if (lines_of(c).pending || !s.sp_out || !c->fx_hits.empty()) { g_err = "context has a submitted piece"; return MQ_ESTATE; }
        int rc = mq_ctx_wait(c);
        if (rc) return rc;
    }
    const std::vector<mq_hit> &lh = lines_of(c).hits;
    const mq_hit *hits = !c->fx_hits.empty() ? c->fx_hits.data() : !lh.empty() ? lh.data() : s.sp_out;
    const uint32_t n = !c->fx_hits.empty() ? (uint32_t)c->fx_hits.size() : !lh.empty() ? (uint32_t)lh.size() : s.sp_n;
    s.spans.assign(n, mq_anchor_span{0, 0});
    s.pool.clear();
    uint64_t cursor = 0;
    uint32_t dropped = 0;
    for (uint32_t r = 0; r < n && hits; ++r) {
        const mq_hit &h = hits[r];
        if (h.status != MQ_HIT_MAPPED) continue;
        const uint32_t cnt = 1 + h.score % 3;
        const uint64_t at = cursor;
        cursor += cnt;
        if (at + cnt > s.cap) {
            s.spans[r] = mq_anchor_span{MQ_ANCHORS_DROPPED, cnt};
            dropped++;
            continue;
        }
        s.spans[r] = mq_anchor_span{(uint32_t)at, cnt};
        for (uint32_t j = 0; j < cnt; ++j) {
            mq_anchor a;
            a.q_start = h.q_start + 10 * j;
            a.q_end = a.q_start + 6;
            a.r_start = h.r_start + 10 * j;
            a.r_end = a.r_start + 6;
            a.count = h.score / cnt + (j == 0 ? h.score % cnt : 0);
            s.pool.resize((size_t)at + j + 1);  // (a dropped list in front leaves no hole: its entries were never claimed below the capacity)
            s.pool[(size_t)at + j] = a;
        }
    }
    *spans = s.spans.data();
    *anchors = s.pool.data();
    *n_reads = n;
    *stored = cursor < s.cap ? cursor : s.cap;
    s.pool.resize((size_t)*stored);
    *anchors = s.pool.data();
    *needed = cursor;
    *dropped_reads = dropped;
    return MQ_OK;
}

int mq_ctx_anchors_device(mq_ctx *, const mq_anchor_span **, const mq_anchor **) {
    g_err = "stub: no device arrays";
    return MQ_ESTATE;
}

int mq_map_reserve_anchors(mq_index *i, uint32_t max_reads, uint64_t max_anchors) {
    if (!i) { g_err = "idx is NULL"; return MQ_EINVAL; }
    return mq_ctx_reserve_anchors(def_ctx_of(i), max_reads, max_anchors);
}

int mq_map_anchors(mq_index *i, const mq_anchor_span **spans, const mq_anchor **anchors, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                   uint32_t *dropped_reads) {
    if (!i) { g_err = "idx is NULL"; return MQ_EINVAL; }
    return mq_ctx_anchors(def_ctx_of(i), spans, anchors, n_reads, stored, needed, dropped_reads);
}

}  // extern "C"
