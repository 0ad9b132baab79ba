// stub_mapquik_hip_extend.cc -- the host-only stand-in of stub_mapquik_hip_reads_lines.cc plus the entry points that keep and maintain
// a finalized index: mq_index_reopen, mq_index_resize, mq_index_load_sized, mq_index_clone_sized.  The stub has no table, so a size is
// only checked for its form; mq_index_load_sized refuses like the stub's mq_index_load, under its own name, so that a test can tell which
// of the two the driver called.  The sanitizer builds of the driver link this file; the stubs below it stay as they are.  Test
// infrastructure only.
#include "stub_mapquik_hip_reads_lines.cc"

namespace {
bool size_form_ok(uint64_t table_slots, uint32_t slots_per_kminmer) {
    if (table_slots && slots_per_kminmer) return false;
    if (table_slots && (table_slots < 2 || (table_slots & (table_slots - 1)) != 0 || table_slots > (1ull << 40))) return false;
    if (slots_per_kminmer && (slots_per_kminmer < 2 || slots_per_kminmer > 64)) return false;
    return true;
}
}  // namespace

extern "C" {

int mq_index_reopen(mq_index *i) {
    if (!i || !i->finalized) { g_err = "mq_index_reopen: index not finalized"; return MQ_ESTATE; }
    i->finalized = false;
    return MQ_OK;
}
int mq_index_resize(mq_index *i, uint64_t table_slots, uint32_t slots_per_kminmer) {
    if (!i || !i->finalized) { g_err = "index not finalized"; return MQ_ESTATE; }
    if (!size_form_ok(table_slots, slots_per_kminmer)) { g_err = "table size"; return MQ_EINVAL; }
    return MQ_OK;
}
mq_index *mq_index_load_sized(const char *, int, uint64_t table_slots, uint32_t slots_per_kminmer) {
    g_err = size_form_ok(table_slots, slots_per_kminmer) ? "stub (mq_index_load_sized)" : "table size";
    return nullptr;
}
mq_index *mq_index_clone_sized(const mq_index *s, int device, uint64_t table_slots, uint32_t slots_per_kminmer) {
    if (!size_form_ok(table_slots, slots_per_kminmer)) { g_err = "table size"; return nullptr; }
    return mq_index_clone(s, device);
}

}  // extern "C"
