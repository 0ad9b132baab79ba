// ix_chunks_test.cc -- IxChunks (mapquik_amd/csrc/mq_ix_chunks.hpp) against a model written out slot by slot: for sections of 0, 1, 3, 4, 6,
// 7 and 25 slots of 32 bytes and chunk wishes around three slots (95, 96, 97), below one slot (31, 1, 0, negative) and the product's 64 MB,
// the chunks tile the section exactly, in whole slots, none empty, none above the chunk size.  Host only.  (tests/test_ix_chunks_host.py)
#include <cstdio>
#include <cstdlib>

#include "../../mapquik_amd/csrc/mq_ix_chunks.hpp"

static int failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "line %d: %s (slots %zu, wish %lld)\n", __LINE__, #cond, n_slots, wish); \
            failures++;                                                              \
        }                                                                            \
    } while (0)

int main() {
    const size_t SLOT = 32;
    const size_t counts[] = {0, 1, 3, 4, 6, 7, 25};
    const long long wishes[] = {95, 96, 97, 31, 1, 0, -1, -96, 64ll << 20};
    for (size_t n_slots : counts)
        for (long long wish : wishes) {
            // the rule, restated: whole slots, rounded down, one at least
            size_t per = wish >= (long long)SLOT ? (size_t)wish / SLOT : 1;
            const size_t want_n = (n_slots + per - 1) / per;
            const IxChunks ch(n_slots * SLOT, SLOT, wish);
            CHECK(ch.chunk == per * SLOT);
            CHECK(ch.n == want_n);
            CHECK(ch.buf_bytes() == (n_slots < per ? n_slots : per) * SLOT);
            size_t covered = 0;
            for (size_t c = 0; c < ch.n; ++c) {
                CHECK(ch.at(c) == covered);
                CHECK(ch.bytes(c) > 0 && ch.bytes(c) % SLOT == 0 && ch.bytes(c) <= ch.buf_bytes());
                CHECK(c + 1 == ch.n || ch.bytes(c) == per * SLOT);
                covered += ch.bytes(c);
            }
            CHECK(covered == n_slots * SLOT);
        }
    // the cases of tests/test_gpu_index_io_chunks.py by number: 96 bytes = 3 slots
    const size_t want96[] = {0, 1, 1, 2, 2, 3, 9};
    for (size_t i = 0; i < 7; ++i) {
        const size_t n_slots = counts[i];
        const long long wish = 96;
        CHECK(IxChunks(n_slots * SLOT, SLOT, wish).n == want96[i]);
    }
    if (failures) return 1;
    printf("ix_chunks ok\n");
    return 0;
}
