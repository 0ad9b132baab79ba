// stub_mapquik_hip_chains.cc -- the host-only stand-in of stub_mapquik_hip_anchors.cc plus the chains output: mq_ctx_reserve_chains,
// mq_ctx_chains, mq_ctx_chains_device, their mq_map_* forms and mq_format_paf_chain.  The stub maps nothing, so the chains are canned like
// the hits, and made FROM the hits of the context's last batch (which the anchors layer below tracks): a mapped read has 1 + score % 3
// chains -- chain 0 is the hit itself (flags MQ_CHAIN_TOP, n_runs = 1 + score % 2), chain j > 0 lies on the same reference, other strand,
// r_start + j, score / (j + 1), one run, mapq 0, not TOP; a read without a hit has none (tests/test_chains_host.py restates this from
// the PAF columns).  The pool behaves as the library's: lists in read order, a list that does not fit is dropped with first =
// MQ_CHAINS_DROPPED, `needed` counts on.  MQ_STUB_CHAINS_CAP (test hook) replaces the capacity a caller reserves.  The sanitizer builds of
// the driver link this file.  Test infrastructure only.
#include "stub_mapquik_hip_anchors.cc"

namespace {
struct ChainState {
    bool reserved = false;
    uint32_t max_reads = 0;
    uint64_t cap = 0;
    std::vector<mq_chain_span> spans;
    std::vector<mq_chain> pool;
};
std::mutex g_chn_mu;
std::map<mq_ctx *, ChainState> g_chn;
ChainState &chn_of(mq_ctx *c) {
    std::lock_guard<std::mutex> lk(g_chn_mu);
    return g_chn[c];
}
}  // namespace

extern "C" {

int mq_ctx_reserve_chains(mq_ctx *c, uint32_t max_reads, uint64_t max_chains) {
    if (!c) { g_err = "ctx is NULL"; return MQ_EINVAL; }
    if (c->pending) { g_err = "context has a submitted batch"; return MQ_ESTATE; }
    ChainState &s = chn_of(c);
    if (max_reads == 0 && max_chains == 0) {
        s = ChainState();
        return MQ_OK;
    }
    if (!max_reads || !max_chains || max_reads >= (1u << 30) || max_chains >= 0xFFFFFFFFull) { g_err = "max_reads / max_chains"; return MQ_EINVAL; }
    const char *e = getenv("MQ_STUB_CHAINS_CAP");
    s.reserved = true;
    s.max_reads = max_reads;
    s.cap = e ? strtoull(e, nullptr, 10) : max_chains;
    return MQ_OK;
}

int mq_ctx_chains(mq_ctx *c, const mq_chain_span **spans, const mq_chain **chains, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                  uint32_t *dropped_reads) {
    if (!c || !spans || !chains || !n_reads || !stored || !needed || !dropped_reads) { g_err = "bad arguments"; return MQ_EINVAL; }
    ChainState &s = chn_of(c);
    if (!s.reserved) { g_err = "no chains reserved on this context"; return MQ_ESTATE; }
    AnchorState &a = anch_of(c);  // (the layer below remembers the spans form's hit array)
    if (c->pending) {
        if (lines_of(c).pending || !a.sp_out || !c->fx_hits.empty()) { g_err = "context has a submitted piece"; return MQ_ESTATE; }
        int rc = mq_ctx_wait(c);
        if (rc) return rc;
    }
    const std::vector<mq_hit> &lh = lines_of(c).hits;
    const mq_hit *hits = !c->fx_hits.empty() ? c->fx_hits.data() : !lh.empty() ? lh.data() : a.sp_out;
    const uint32_t n = !c->fx_hits.empty() ? (uint32_t)c->fx_hits.size() : !lh.empty() ? (uint32_t)lh.size() : a.sp_n;
    s.spans.assign(n, mq_chain_span{0, 0});
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
            s.spans[r] = mq_chain_span{MQ_CHAINS_DROPPED, cnt};
            dropped++;
            continue;
        }
        s.spans[r] = mq_chain_span{(uint32_t)at, cnt};
        for (uint32_t j = 0; j < cnt; ++j) {
            mq_chain x;
            static_assert(sizeof(mq_chain) == sizeof(mq_hit), "mq_chain has the layout of mq_hit");
            memcpy(&x, &h, sizeof(x));
            x.flags = j == 0 ? MQ_CHAIN_TOP : 0u;
            x.n_runs = j == 0 ? 1 + h.score % 2 : 1;
            if (j) {
                x.rc = h.rc ? 0u : 1u;
                x.r_start = h.r_start + j;
                x.score = h.score / (j + 1);
                x.mapq = 0;
            }
            s.pool.resize((size_t)at + j + 1);
            s.pool[(size_t)at + j] = x;
        }
    }
    *spans = s.spans.data();
    *n_reads = n;
    *stored = cursor < s.cap ? cursor : s.cap;
    s.pool.resize((size_t)*stored);
    *chains = s.pool.data();
    *needed = cursor;
    *dropped_reads = dropped;
    return MQ_OK;
}

int mq_ctx_chains_device(mq_ctx *, const mq_chain_span **, const mq_chain **) {
    g_err = "stub: no device arrays";
    return MQ_ESTATE;
}

int mq_map_reserve_chains(mq_index *i, uint32_t max_reads, uint64_t max_chains) {
    if (!i) { g_err = "idx is NULL"; return MQ_EINVAL; }
    return mq_ctx_reserve_chains(def_ctx_of(i), max_reads, max_chains);
}

int mq_map_chains(mq_index *i, const mq_chain_span **spans, const mq_chain **chains, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                  uint32_t *dropped_reads) {
    if (!i) { g_err = "idx is NULL"; return MQ_EINVAL; }
    return mq_ctx_chains(def_ctx_of(i), spans, chains, n_reads, stored, needed, dropped_reads);
}

int mq_format_paf_chain(const mq_index *i, const char *q_id, uint64_t q_len, const mq_chain *chain, char *buf, size_t cap) {
    if (!i || !q_id || !chain || !buf) { g_err = "bad arguments"; return MQ_EINVAL; }
    mq_hit h;
    memcpy(&h, chain, sizeof(h));
    h.status = MQ_HIT_MAPPED;  // any chain, TOP or not
    return mq_format_paf(i, q_id, q_len, &h, buf, cap);
}

}  // extern "C"
