// stub_mapquik_hip_reads_lines.cc -- the host-only stand-in of stub_mapquik_hip_lines.cc plus MQ_FASTX_FASTA_LINES and
// mq_ctx_wait_fasta_lines: the record rule of include/mapquik_hip.h restated on the host, byte by byte (a header start is a '>' at
// `begin` or behind a '\n'; a record's sequence is every byte behind its header line that is not '\n' and not a '\r' in front of a '\n'
// or at the piece's end), with canned hits made from the joined bytes as the other paths make them from theirs.  The sanitizer builds
// of the driver link this file.  The two stubs below it stay as they are: their mq_ctx_submit_fastx / mq_ctx_wait_fasta / mq_ctx_free are
// compiled under other names here and wrapped, and the state of a LINES piece lives beside their mq_ctx.  Test infrastructure only.
#define mq_ctx_submit_fastx stub_base_submit_fastx
#define mq_ctx_wait_fasta stub_base_wait_fasta
#define mq_ctx_free stub_base_ctx_free
#include "stub_mapquik_hip_lines.cc"
#undef mq_ctx_submit_fastx
#undef mq_ctx_wait_fasta
#undef mq_ctx_free

namespace {
struct LinesState {
    bool pending = false;
    uint32_t flags = 0;
    std::vector<uint32_t> hdr_begin, hdr_end, lens;
    std::vector<mq_hit> hits;
};
std::mutex g_lines_mu;
std::map<mq_ctx *, LinesState> g_lines;  // (a std::map: references to its values stay valid while other contexts come and go)
LinesState &lines_of(mq_ctx *c) {
    std::lock_guard<std::mutex> lk(g_lines_mu);
    return g_lines[c];
}

void scan_lines(const mq_index *idx, const uint8_t *buf, uint64_t begin, uint64_t bytes, LinesState &s) {
    s.flags = 0;
    s.hdr_begin.clear();
    s.hdr_end.clear();
    s.lens.clear();
    s.hits.clear();
    if (begin >= bytes) return;  // an empty piece is regular: no records
    const uint64_t line_cap = bytes / 16 + 4096 < (1ull << 28) ? bytes / 16 + 4096 : (1ull << 28);
    std::vector<uint8_t> seq;
    bool in_header = false, bad = buf[begin] != '>';
    auto close_record = [&]() {  // the record in front of a header start (or of the piece's end) is complete
        if (s.hdr_begin.empty()) return;
        if (seq.empty()) bad = true;  // a record without a sequence byte
        mq_hit h;
        canned(idx, seq.data(), 0, (uint32_t)seq.size(), &h);
        s.hits.push_back(h);
        s.lens.push_back((uint32_t)seq.size());
        seq.clear();
    };
    for (uint64_t p = begin; p < bytes && !bad; ++p) {
        const uint8_t b = buf[p];
        if (b == '>' && (p == begin || buf[p - 1] == '\n')) {
            close_record();
            s.hdr_begin.push_back((uint32_t)p);
            s.hdr_end.push_back((uint32_t)bytes);  // (until its '\n' is seen)
            in_header = true;
        } else if (b == '\n') {
            if (in_header) s.hdr_end.back() = (uint32_t)p;
            in_header = false;
        } else if (!in_header && !(b == '\r' && (p + 1 == bytes || buf[p + 1] == '\n'))) {
            seq.push_back(b);
        }
    }
    if (!bad) close_record();
    if (bad || s.hdr_begin.size() > line_cap / 2) {
        s.flags = MQ_FASTA_IRREGULAR;
        s.hdr_begin.clear();
        s.hdr_end.clear();
        s.lens.clear();
        s.hits.clear();
    }
}
}  // namespace

extern "C" {
int mq_ctx_submit_fastx(mq_ctx *c, const uint8_t *buf, uint64_t begin, uint64_t bytes, uint32_t format) {
    if (format != MQ_FASTX_FASTA_LINES) return stub_base_submit_fastx(c, buf, begin, bytes, format);
    if (c->pending) { g_err = "context has a submitted batch"; return MQ_ESTATE; }
    LinesState *s = &lines_of(c);
    c->pending = true;
    s->pending = true;
    c->worker = std::thread([=]() { scan_lines(c->idx, buf, begin, bytes, *s); });
    return MQ_OK;
}
int mq_ctx_wait_fasta(mq_ctx *c, uint32_t *n_reads, const uint32_t **line_ends, uint32_t *n_lines, const mq_hit **hits, uint32_t *flags) {
    if (lines_of(c).pending) { g_err = "the submitted piece is MQ_FASTX_FASTA_LINES"; return MQ_ESTATE; }
    return stub_base_wait_fasta(c, n_reads, line_ends, n_lines, hits, flags);
}
int mq_ctx_wait_fasta_lines(mq_ctx *c, uint32_t *n_reads, const uint32_t **hdr_begin, const uint32_t **hdr_end, const uint32_t **seq_lens,
                            const mq_hit **hits, uint32_t *flags) {
    LinesState &s = lines_of(c);
    if (!s.pending) { g_err = "no MQ_FASTX_FASTA_LINES piece submitted on this context"; return MQ_ESTATE; }
    if (c->worker.joinable()) c->worker.join();
    c->pending = false;
    s.pending = false;
    *flags = s.flags;
    *n_reads = (uint32_t)s.hits.size();
    *hdr_begin = s.hits.empty() ? nullptr : s.hdr_begin.data();
    *hdr_end = s.hits.empty() ? nullptr : s.hdr_end.data();
    *seq_lens = s.hits.empty() ? nullptr : s.lens.data();
    *hits = s.hits.empty() ? nullptr : s.hits.data();
    return MQ_OK;
}
void mq_ctx_free(mq_ctx *c) {
    stub_base_ctx_free(c);
    std::lock_guard<std::mutex> lk(g_lines_mu);
    g_lines.erase(c);
}
}
