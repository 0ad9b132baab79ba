// stub_mapquik_hip_merge.cc -- the host-only stand-in of stub_mapquik_hip_chains.cc plus the two entry points that take another finished
// index in: mq_index_merge and mq_index_merge_file.  The stub has no table, so a merge is canned: a file that begins with the index
// magic brings ONE reference, named after the file, under the id the caller gave (which must be free and below 2^24), and ten
// k-min-mers; any other file is refused with the stub's own text, so that a test can tell that the driver got as far as the call, in
// which order, and with which id_base.  MQ_STUB_MERGE_LOG=1 (test hook) writes one line per call to stderr.  The sanitizer builds of the
// driver link this file; the stubs below it stay as they are.  Test infrastructure only.
#include "stub_mapquik_hip_chains.cc"

namespace {
int stub_merge_one(mq_index *dst, const std::string &name, uint32_t id_base, const char *who) {
    if (getenv("MQ_STUB_MERGE_LOG")) fprintf(stderr, "stub: %s %s id_base %u\n", who, name.c_str(), id_base);
    if (id_base >= (1u << 24)) { g_err = std::string(who) + ": a moved id reaches 2^24"; return MQ_EINVAL; }
    if (dst->refs.count(id_base)) { g_err = std::string(who) + ": a moved id is already an id of this index"; return MQ_EINVAL; }
    dst->refs[id_base] = std::make_pair(name, (uint64_t)1000);
    dst->n_kmm += 10;
    return MQ_OK;
}
}  // namespace

extern "C" {

int mq_index_merge(mq_index *dst, const mq_index *src, uint32_t id_base) {
    if (!dst || !src || dst == src) { g_err = "mq_index_merge: bad arguments"; return MQ_EINVAL; }
    if (!dst->finalized || !src->finalized) { g_err = "mq_index_merge: index not finalized"; return MQ_ESTATE; }
    return stub_merge_one(dst, "merged", id_base, "mq_index_merge");
}

int mq_index_merge_file(mq_index *dst, const char *path, uint32_t id_base) {
    if (!dst || !path) { g_err = "mq_index_merge_file: bad arguments"; return MQ_EINVAL; }
    if (!dst->finalized) { g_err = "mq_index_merge_file: index not finalized"; return MQ_ESTATE; }
    char magic[8] = {0};
    FILE *f = fopen(path, "rb");
    const bool ok = f && fread(magic, 1, 8, f) == 8 && memcmp(magic, "MQHIPIX2", 8) == 0;
    if (f) fclose(f);
    if (!ok) { g_err = std::string("stub (mq_index_merge_file): not an index: ") + path; return MQ_EINVAL; }
    const std::string p(path);
    return stub_merge_one(dst, p.substr(p.find_last_of('/') + 1), id_base, "mq_index_merge_file");
}

}  // extern "C"
