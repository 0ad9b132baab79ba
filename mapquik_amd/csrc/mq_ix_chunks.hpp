// mq_ix_chunks.hpp -- THE chunk arithmetic of an index file's slot section (part of the one translation unit mq_capi.hip; plain C++, so
// that tests/cpp/ix_chunks_test.cc can hold it against a model on the host).  The section crosses PCIe in chunks of whole slots:
// chunk_bytes (the caller's wish: 64 MB, or the MQ_IX_IO_CHUNK test hook) rounded down to a multiple of slot_bytes, one slot at least.
#pragma once
#include <algorithm>
#include <cstddef>

struct IxChunks {
    size_t total, chunk, n;  // bytes of the section, bytes of a chunk, chunks
    IxChunks(size_t total_bytes, size_t slot_bytes, long long chunk_bytes) : total(total_bytes) {
        const size_t slots = chunk_bytes > 0 ? (size_t)chunk_bytes / slot_bytes : 0;
        chunk = std::max<size_t>(slots, 1) * slot_bytes;
        n = (total + chunk - 1) / chunk;
    }
    size_t at(size_t c) const { return c * chunk; }                              // where chunk c begins
    size_t bytes(size_t c) const { return std::min(chunk, total - c * chunk); }  // ... and what it holds
    size_t buf_bytes() const { return std::min(total, chunk); }                  // what a transfer buffer holds
};
