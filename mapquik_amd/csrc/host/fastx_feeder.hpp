// fastx_feeder.hpp -- the read feeder of the native driver: FASTA/FASTQ (raw, gzip, lz4) -> page-locked chunks of raw file
// bytes + per-read spans, ready for mq_ctx_submit_spans.  Replaces what the reference gets from seq_io's worker pool and
// get_reader (src/main.rs:60-75, src/closures.rs:177-187).
//
// Design: a base is copied ONCE on the host (file / inflate output -> page-locked chunk) and never touched again: the
// chunk goes to the GPU as it is (headers, line ends, quality lines), reads are (start, length) spans of it, and the
// kernels fold a-z to A-Z themselves (MQ_FLAG_FOLD_CASE).  Raw files are cut into chunks at record boundaries and read
// with pread by N threads in parallel; compressed input is inflated by one thread straight into chunks (gzip and lz4
// streams are sequential by nature) and parsed by the others; BGZF (bgzip) files are the exception: their blocks are
// independent deflate streams with their sizes in the headers, so the file is indexed once and then read like a raw file,
// every reader thread inflating the blocks of its own chunk.  Multi-line FASTA records are compacted in place.
// Uncompressed FASTQ is the exception to "raw bytes as they are": half of such a file is quality values nobody reads, so the
// file is mapped and every reader copies the header and sequence lines of its records only -- the quality lines are never
// touched (not read from the page cache, not copied, not sent over PCIe).
//
// Parts: fastx_records.hpp (Chunk, record boundaries, parse_chunk), feeder_queue.hpp (ChunkQueue: buffer pool, queues, errors, worker
// threads), feeder_input.hpp (Knobs, Input with its BGZF block index, choose_reader), and the readers over them: feeder_raw.hpp (raw /
// BGZF chunks, mapped views, lean FASTQ), feeder_gzip.hpp (inflate stream, gzip members, the parser threads).  This file is the
// Feeder the consumers see.
#pragma once
#include "feeder_gzip.hpp"
#include "feeder_input.hpp"
#include "feeder_queue.hpp"
#include "feeder_raw.hpp"

namespace mapquik {
namespace feeder {

// ---------------------------------------------------------------- the feeder: an input, a chunk queue, and the reader chosen for them
class Feeder {
  public:
    // chunk_bytes: target raw bytes per chunk; n_threads: reader/parser threads
    // alloc/release: where chunk buffers come from (page-locked memory through mq_host_alloc unless a test says otherwise)
    Feeder(const std::string &path, bool fastq, uint64_t chunk_bytes, int n_threads, int max_chunks,
           std::function<void *(size_t)> alloc = mq_host_alloc, std::function<void(void *)> release = mq_host_free,
           std::function<int(void *, size_t)> lock = mq_host_register, std::function<int(void *)> unlock = mq_host_unregister)
        : in_(path, fastq, chunk_bytes, n_threads), q_(max_chunks, alloc, release, unlock) {
        views_.lock = lock;
        if (reader(true) == Reader::GzipMembers) in_.map_file();
        q_.set_buffer_floor(std::min<uint64_t>(in_.chunk_bytes + in_.chunk_bytes / 8 + (1u << 20), in_.size + 64));
    }
    ~Feeder() { release_buffers(); }

    // The pool's page-locked buffers back to the system (ChunkQueue::release_buffers), every thread of the feeder joined first.  The
    // destructor does the same.
    void release_buffers() {
        q_.stop();
        views_.stop();
        q_.release_buffers();
    }

    // MQ_FEEDER_MAPPED_FASTA=1 only (MappedViews): map the file now and fill the mapping's page tables in the background
    void premap() {
        if (reader(true) != Reader::MappedViews || in_.map) return;
        if (in_.map_file()) views_.populate(in_, knobs_);
    }

    void start() {
        const Reader r = reader();
        if (r == Reader::MappedViews) q_.set_buffer_floor(64);  // (the pool's buffers only stand in for the views)
        auto per_thread = [this](auto fn) {
            for (int t = 0; t < in_.threads; ++t) q_.run_worker(fn);
        };
        switch (r) {
        case Reader::MappedViews: per_thread([this] { views_.reader(q_, in_); }); break;
        case Reader::LeanFastq: per_thread([this] { LeanFastqReader(q_, in_).run(); }); break;
        case Reader::RawChunks: per_thread([this] { raw_chunk_reader(q_, in_, leave_unparsed_); }); break;
        case Reader::GzipMembers:  // one thread inflates (and calls in the others for a large member), the others parse
            q_.run_worker([this] { GzipMemberReader(q_, in_, knobs_).run(); }, true);
            per_thread([this] { parse_worker(q_, in_); });
            break;
        case Reader::InflateStream:
            q_.run_worker([this] { inflate_stream_reader(q_, in_); }, true);
            per_thread([this] { parse_worker(q_, in_); });
            break;
        }
    }

    // the consumer gives up (an error elsewhere in its pipeline): next() returns nullptr from now on, workers waiting for a buffer
    // leave; chunks still held by the consumer need not be recycled
    void abort() { q_.abort(); }

    // next parsed chunk (any order; seq_no says where it belongs) or nullptr at the end of the input
    Chunk *next() {
        bool end;
        return q_.take(true, end);
    }
    // next(), without waiting: a parsed chunk if one is ready, else nullptr -- `end` says whether the input is exhausted (or the
    // consumer aborted).  For consumers that hold chunks of their own and must not sit on them while nothing new arrives.
    Chunk *poll(bool &end) { return q_.take(false, end); }
    // hand a chunk back for re-use
    void recycle(Chunk *c) { q_.recycle(c); }
    size_t chunks_total() const { return q_.chunks_total(); }
    uint64_t bytes_in() const { return in_.size; }
    // Before start(): n buffers of the pool allocated (page-locked) now, by as many threads, so that the first chunks do not wait for
    // them -- the pool's buffers do not depend on the input's bytes
    void preallocate(int n) {
        if (!mapped_views()) q_.preallocate(n, std::min<uint64_t>(in_.chunk_bytes + (1u << 20) + 2, in_.size + 2));
    }
    // Before start(): chunks of an uncompressed FASTA or FASTQ file are handed over as they were read, Chunk::unparsed set, no host thread
    // having looked at a base (the consumer submits them with mq_ctx_submit_fastx; a chunk that comes back MQ_FASTA_IRREGULAR is
    // parsed with parse_chunk after all).  Compressed input is parsed here as always.
    void leave_unparsed(bool on) { leave_unparsed_ = on; }
    bool fastq() const { return in_.fastq; }
    // chunks will be (after start(): are) views of the mapped file (see premap())
    bool mapped_views() const { return reader() == Reader::MappedViews; }
    const char *kind_name() const {
        const char *names[] = {"raw", reader() == Reader::GzipMembers ? "gzip (libdeflate, whole members)" : "gzip", "lz4", "bgzf"};
        return names[(int)in_.kind];
    }

  private:
    // the reader that will run as things stand (planned: if the file can be mapped)
    Reader reader(bool planned = false) const { return choose_reader(in_, knobs_, leave_unparsed_, planned || in_.map != nullptr); }

    const Knobs knobs_;
    Input in_;
    bool leave_unparsed_ = false;
    MappedViews views_;
    ChunkQueue q_;  // (last: its threads work over everything above)
};

}  // namespace feeder
}  // namespace mapquik
