// stub_mapquik_hip_lines.cc -- the host-only stand-in of stub_mapquik_hip.cc plus mq_index_add_ref_staged_lines: the join of a
// line-wrapped record's lines restated on the host, byte by byte (the rule of include/mapquik_hip.h: a byte is dropped when it is '\n',
// or when it is '\r' and the next byte of the region is '\n' or there is none).  The sanitizer builds of the driver link this file.
// Test hook: MQ_STUB_DUMP_REFS=<dir> writes every joined sequence to <dir>/<ref_id>.seq.  Test infrastructure only.
#include "stub_mapquik_hip.cc"

extern "C" int64_t mq_index_add_ref_staged_lines(mq_index *i, uint32_t id, const char *name, uint64_t at, uint64_t bytes, uint64_t after,
                                                 uint64_t *seq_len) {
    std::vector<uint8_t> seq;
    {
        std::lock_guard<std::mutex> lk(i->stage_mu);
        if (after != MQ_STAGE_ALL_ISSUED && after >= i->stage_tickets) { g_err = "unknown ticket"; return MQ_EINVAL; }
        if (!i->stage_begun || at + bytes + 1 > i->stage.size()) { g_err = "record outside the staging buffer"; return MQ_EINVAL; }
        const uint8_t *r = i->stage.data() + at;
        seq.reserve((size_t)bytes);
        for (uint64_t p = 0; p < bytes; ++p) {
            if (r[p] == '\n') continue;
            if (r[p] == '\r' && (p + 1 == bytes || r[p + 1] == '\n')) continue;
            seq.push_back(r[p]);
        }
    }
    if (i->refs.count(id)) { g_err = "duplicate ref_id"; return MQ_EINVAL; }
    if (seq.size() >= (1ull << 32)) { g_err = "sequence length must be < 2^32"; return MQ_EINVAL; }
    if (const char *dir = getenv("MQ_STUB_DUMP_REFS")) {
        const std::string path = std::string(dir) + "/" + std::to_string(id) + ".seq";
        FILE *f = fopen(path.c_str(), "wb");
        if (!f || (!seq.empty() && fwrite(seq.data(), 1, seq.size(), f) != seq.size())) {
            if (f) fclose(f);
            g_err = "cannot write " + path;
            return MQ_EINVAL;
        }
        fclose(f);
    }
    if (seq_len) *seq_len = seq.size();
    return mq_index_add_ref(i, id, name, seq.data(), seq.size());
}
