// chains_format_test.cc -- mq_format_paf_chain called through the C ABI by a stand-alone program (the native driver formats its chains
// through PafWriter, so nothing else calls the symbol without a GPU): two references, a handful of chains -- TOP and not, both strands,
// 64-bit columns 3 / 4, a small buffer that must report the full length, an unknown reference that must be refused.  Prints one line per
// case; tests/test_chains_host.py compares them with a Python formatter.  Linked against the host-only stub under ASan + UBSan / TSan
// (make asan tsan).  Test infrastructure only.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mapquik_hip.h"

int main() {
    mq_params p;
    mq_params_default(&p);
    mq_index *idx = mq_index_new(&p, 0);
    if (!idx) return 2;
    const std::string a(5000, 'A'), b(777, 'C');
    if (mq_index_add_ref(idx, 0, "chrA some text", (const uint8_t *)a.data(), a.size()) < 0) return 2;
    if (mq_index_add_ref(idx, 7, "chrB", (const uint8_t *)b.data(), b.size()) < 0) return 2;
    mq_index_finalize(idx);
    //                 flags          ref rc mapq q_start     q_end       r_start r_end score n_runs q_start_hi q_end_hi
    const mq_chain cs[] = {{MQ_CHAIN_TOP, 0, 0, 60, 12u, 4321u, 100u, 4409u, 37u, 3u, 0u, 0u},
                           {0u, 7, 1, 0, 0u, 700u, 5u, 705u, 2u, 1u, 0u, 0u},
                           {MQ_CHAIN_TOP, 7, 1, 60, 0xFFFFEF8Fu, 9u, 0u, 776u, 11u, 2u, 0xFFFFFFFFu, 1u},
                           {0u, 0, 0, 0, 0u, 0u, 0u, 0u, 0u, 1u, 0u, 0u}};
    const char *ids[] = {"read1", "r/2 x", "wrap", "z"};
    const uint64_t lens[] = {4500, 701, 5000000000ull, 1};
    int rc = 0;
    for (size_t i = 0; i < sizeof(cs) / sizeof(cs[0]); ++i) {
        char buf[512];
        const int w = mq_format_paf_chain(idx, ids[i], lens[i], &cs[i], buf, sizeof(buf));
        if (w < 0 || (size_t)w >= sizeof(buf) || strlen(buf) != (size_t)w) { rc = 3; continue; }
        printf("%s\n", buf);
        char small[8];  // snprintf semantics: the full length comes back, the buffer holds a cut, terminated line
        const int w2 = mq_format_paf_chain(idx, ids[i], lens[i], &cs[i], small, sizeof(small));
        if (w2 != w || strlen(small) != sizeof(small) - 1 || strncmp(small, buf, sizeof(small) - 1) != 0) rc = 4;
    }
    mq_chain bad = cs[0];
    bad.ref_id = 3;  // no such reference
    char buf[64];
    printf("unknown_ref %d\n", mq_format_paf_chain(idx, "q", 10, &bad, buf, sizeof(buf)) < 0 ? 1 : 0);
    printf("null_args %d\n", mq_format_paf_chain(idx, nullptr, 10, &bad, buf, sizeof(buf)) < 0 ? 1 : 0);
    mq_index_free(idx);
    return rc;
}
