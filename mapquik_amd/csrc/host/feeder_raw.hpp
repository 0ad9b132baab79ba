// feeder_raw.hpp -- the readers of the read feeder (fastx_feeder.hpp) that hand over a file's bytes as they are: the chunked reader of
// uncompressed and BGZF input (pread / block inflate into page-locked chunks, N threads), the mapped-view experiment, and the lean reader
// of uncompressed FASTQ (header and sequence lines only).  All three number their chunks by position (claim_raw_chunk): chunk i owns
// the records whose first byte lies in [i * CH, (i + 1) * CH) of the (logical) file.
#pragma once
#include <atomic>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "feeder_input.hpp"
#include "feeder_queue.hpp"

namespace mapquik {
namespace feeder {

// The next chunk i = [lo, hi) of the file and a buffer of `need` bytes for it; false (and no buffer) when the file is handed out.
// Buffer first, chunk number second: every numbered chunk then owns a buffer, so the consumer (which may hold later chunks while it
// waits for an earlier one) can never starve the earliest chunk of memory.
inline bool claim_raw_chunk(ChunkQueue &q, const Input &in, uint64_t need, Chunk *&c, size_t &i, uint64_t &lo, uint64_t &hi) {
    c = q.get_buffer(need);
    i = q.next_chunk_no();
    if (i >= in.n_raw_chunks) {
        q.recycle(c);
        return false;
    }
    lo = (uint64_t)i * in.chunk_bytes;
    hi = std::min<uint64_t>(lo + in.chunk_bytes, in.size);
    return true;
}

// raw or BGZF file: chunk i owns the records whose first byte lies in [i*CH, (i+1)*CH)
inline void raw_chunk_reader(ChunkQueue &q, const Input &in, bool leave_unparsed) {
    std::unique_ptr<BlockInflater> blocks;
    if (in.kind == Kind::Bgzf) blocks.reset(new BlockInflater(in.deflate));
    // bytes [off, off + n) of the (logical) file into dst
    auto fetch = [&](uint8_t *dst, uint64_t off, uint64_t n) {
        if (blocks) in.bgzf.read(off, n, dst, *blocks);
        else in.read(dst, off, n);
    };
    Chunk *c;
    size_t i;
    uint64_t lo, hi;
    while (claim_raw_chunk(q, in, std::min<uint64_t>(in.chunk_bytes + (1u << 20) + 2, in.size + 2), c, i, lo, hi)) {
        // read [lo - 1, hi + tail): one byte before to know whether lo is a line start; the tail until the owning
        // record of hi's successor is complete (grown as needed)
        uint64_t tail = std::min<uint64_t>(1u << 20, in.size - hi);
        const uint64_t from = lo ? lo - 1 : 0;
        uint64_t got = 0;  // bytes of [from, ...) already in the buffer: a longer tail only reads what is missing
        for (;;) {
            const uint64_t want = hi + tail - from;
            if (c->cap < want) {  // a record longer than the tail: a private, larger buffer (beyond the pool limit if need be)
                Chunk *big = q.get_buffer(want, true);
                if (got) memcpy(big->buf, c->buf, got);
                q.recycle(c);
                c = big;
            }
            fetch(c->buf + got, from + got, want - got);
            got = want;
            const uint64_t skip = lo ? 1 : 0;  // index of byte `lo` in the buffer
            const bool at_eof = hi + tail >= in.size;
            const uint64_t first = lo ? next_record_start(c->buf, skip, got, in.fastq, at_eof) : 0;
            uint64_t last = got;
            if (first != NEED_MORE && hi < in.size) last = next_record_start(c->buf, skip + (hi - lo), got, in.fastq, at_eof);
            if (first == NEED_MORE || last == NEED_MORE) {  // the record that straddles hi is longer than the tail
                tail = std::min<uint64_t>(std::max<uint64_t>(tail * 4, in.chunk_bytes), in.size - hi);
                continue;
            }
            if (first >= last || first >= skip + (hi - lo)) {
                c->begin = c->bytes = 0;  // no record starts in this chunk (inside a long record)
            } else {
                c->begin = first;
                c->bytes = last;
            }
            break;
        }
        c->seq_no = i;
        if (leave_unparsed && in.kind == Kind::Raw && c->bytes > c->begin) c->unparsed = true;  // the consumer finds the records (on the device), FASTA or FASTQ
        else parse_chunk(*c, in.fastq);
        q.publish(c);
    }
}

// EXPERIMENT (MQ_FEEDER_MAPPED_FASTA=1; off by default).  Raw FASTA whose records the consumer finds (leave_unparsed): the file is mapped
// and the mapping's page tables are filled in the background -- no byte of the file is read, the kernel only enters the page-cache
// pages into this process's address space.  A chunk is then a view of the mapping and its copy to the device a DMA out of the page
// cache.  Measured (profiles/r04_file_h2d.txt, profiles/r04_feeder_scaling.txt): a probe copies from a mapping with full page
// tables at 46-50 GB/s with two threads and from a fresh one at 12-17; inside the driver, mapped while the reference is indexed,
// this path reaches 26-31 Gbases/s against 34-35 for pread into page-locked chunks, which therefore stays the default.
struct MappedViews {
    std::function<int(void *, size_t)> lock;  // page-locks whole pages of the mapped file (mq_host_register; Chunk::locked_at, ChunkQueue::recycle)
    bool lock_pages = false;                   // MQ_FEEDER_PAGE_LOCK (experiment): the reader threads page-lock each chunk's pages
    uint64_t page = 4096;
    std::thread populate_thread;  // fills the mapping's page tables ahead of the readers
    std::atomic<bool> populate_stop{false};

    ~MappedViews() { stop(); }
    // the (mapped) file's page tables filled from now on, in the background
    void populate(const Input &in, const Knobs &knobs) {
        page = (uint64_t)sysconf(_SC_PAGESIZE);
        lock_pages = page > 0 && knobs.page_lock;
        populate_thread = std::thread([this, &in] {
            const uint64_t step = 64ull << 20;
            for (uint64_t o = 0; o < in.map_size && !populate_stop.load(std::memory_order_relaxed); o += step) {
                const uint64_t n = std::min<uint64_t>(step, in.map_size - o);
#ifdef MADV_POPULATE_READ
                if (madvise((void *)(in.map + o), n, MADV_POPULATE_READ) != 0) break;  // an older kernel: pages are entered as they are touched
#else
                if (madvise((void *)(in.map + o), n, 22) != 0) break;
#endif
            }
        });
    }
    void stop() {
        populate_stop = true;
        if (populate_thread.joinable()) populate_thread.join();
    }

    // chunk i = a view of the records whose first byte lies in [i*CH, (i+1)*CH) of the mapping; only the lines around the two cuts are
    // looked at
    void reader(ChunkQueue &q, const Input &in) {
        Chunk *c;
        size_t i;
        uint64_t lo, hi;
        while (claim_raw_chunk(q, in, 64, c, i, lo, hi)) {
            const uint64_t first = lo ? next_record_start(in.map, lo, in.size, false, true) : 0;
            const uint64_t last = hi < in.size ? next_record_start(in.map, hi, in.size, false, true) : in.size;
            c->seq_no = i;
            if (first >= last || first >= hi) {
                c->begin = c->bytes = 0;  // no record starts in this chunk (inside a long record)
            } else {
                if (last - first >= (1ull << 32)) throw FeederError("sequence length must be < 2^32");
                c->buf = const_cast<uint8_t *>(in.map) + first;
                c->begin = 0;
                c->bytes = last - first;
                c->unparsed = true;
                // Page-lock the chunk's whole pages [floor(first), floor(last)): the copy to the device is then a DMA out of the page cache
                // that no thread waits for.  (Experimental, off by default: profiles/r04_file_h2d.txt -- locking the pages of a fresh
                // mapping runs at 12-17 GB/s whatever the thread count.)  The ranges of consecutive chunks tile the file, so no page is
                // locked twice; the chunk's last partial page belongs to the next chunk's range, and mq_ctx_submit_fasta moves those
                // < 4 KB through a buffer of its own.  Released by recycle().
                if (lock_pages) {
                    const uint64_t a = first / page * page, b = last / page * page;
                    if (b > a && lock(const_cast<uint8_t *>(in.map) + a, (size_t)(b - a)) == 0) {
                        c->locked_at = const_cast<uint8_t *>(in.map) + a;
                        c->locked_len = b - a;
                    }
                }
            }
            q.publish(c);
        }
    }
};

// ---------------------------------------------------------------- uncompressed FASTQ, lean: half of such a file is quality values nobody
// reads, so every reader thread copies the header and sequence lines of its records only.
// Chunk i owns the records whose first byte lies in [i*CH, (i+1)*CH) of the file and reads their header and
// sequence lines -- and nothing else -- straight into its page-locked buffer: ONE pread per record of about the record's header +
// sequence length (the longest of the eight records before it and a margin; what it reads too much, the start of the '+' and
// quality lines, is overwritten by the next record), the '+' line found in that surplus.  The byte at the place where the quality
// line must end if it is as long as the sequence line (the validator's test, fastq_record_at) is the byte in FRONT of the next
// record: it comes with the next record's read (into the place of this record's own line end, which is put back) -- round 5 read
// it with a pread of its own, a second system call per record, and asked for 1.125 x the record before, which one record in six
// outgrew (a second, doubled read).  Half the file's bytes never leave the page
// cache: 1 byte per base from the file and over the link instead of 2 (a reader that maps the file pays for the page tables of
// all of it: 12-17 GB/s at any thread count, profiles/r04_file_h2d.txt; this one runs at pread's rate).
struct LeanFastqReader {
    ChunkQueue &q;
    const Input &in;
    const uint64_t end;        // of the file
    std::vector<uint8_t> win;  // scratch of the boundary searches
    uint64_t est = 32768;      // bytes to ask for per record: header + sequence line of the records before it, and a margin
    uint64_t hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // header + sequence bytes of the last eight records
    unsigned hist_at = 0;
    // the chunk being filled
    Chunk *c = nullptr;
    uint64_t w = 0;         // bytes of the chunk in use
    bool pending = false;   // the byte at p - 1 (where the record before must end) is still to be looked at: it comes with this record's read
    uint64_t E3_prev = 0;   // end of the '+' line of the record before (where the search for its real end starts when that byte is no '\n')

    LeanFastqReader(ChunkQueue &q_, const Input &in_) : q(q_), in(in_), end(in_.size) {}

    void run() {
        size_t i;
        uint64_t lo, hi;
        while (claim_raw_chunk(q, in, std::min<uint64_t>(in.chunk_bytes / 2 + (1u << 20) + 2, in.size + 2), c, i, lo, hi)) {
            // [first, last): from the first record start at or after lo to the first one at or after hi -- the same cut as the
            // chunked reader's, so that a last record the validator cannot vouch for (CR-LF file without a final newline)
            // stays with its predecessor
            uint64_t p = lo ? record_start_from(lo) : 0;
            const uint64_t last = hi < end ? record_start_from(hi) : end;
            if (p >= hi) p = last;  // no record starts in this chunk
            w = 0;
            pending = false;
            E3_prev = 0;
            while (p < last) p = take_record(p, last);
            c->begin = 0;
            c->bytes = w;
            c->seq_no = i;
            q.publish(c);
        }
    }

    // ------------------------------------------------------------ the boundary search
    // first record start at or after `from`, decided like the chunked reader's cut (next_record_start over a window that grows until
    // the validator can tell)
    uint64_t record_start_from(uint64_t from) {
        uint64_t W = 1u << 18;
        for (;;) {
            const uint64_t a = from - 1, b = std::min<uint64_t>(end, from + W);
            win.resize((size_t)(b - a));
            in.read(win.data(), a, b - a);
            const uint64_t r = next_record_start(win.data(), 1, b - a, true, b >= end);
            if (r != NEED_MORE) return a + r;
            W *= 4;
        }
    }
    uint8_t byte_at(uint64_t off) {
        uint8_t x = 0;
        in.read(&x, off, 1);
        return x;
    }
    // the line end at or after `from` (file offsets), read in small steps: only for what the surplus of a record's read did not hold
    uint64_t line_end_from(uint64_t from) {
        uint8_t tmp[4096];
        for (uint64_t o = from; o < end;) {
            const uint64_t n = std::min<uint64_t>(sizeof(tmp), end - o);
            in.read(tmp, o, n);
            const uint8_t *e = (const uint8_t *)memchr(tmp, '\n', (size_t)n);
            if (e) return o + (uint64_t)(e - tmp);
            o += n;
        }
        return end;
    }

    // ------------------------------------------------------------ the record read
    struct Lines {
        uint64_t got = 0;                         // bytes of the file at p that are in the buffer at w
        uint64_t e1 = NEED_MORE, e2 = NEED_MORE;  // indices in c->buf of the header's and the sequence's line end (or of the data's end at EOF)
    };
    // The header and sequence lines of the record at file offset p into the buffer at w: `est` bytes, more while a line end is missing.
    // The read brings the byte in front of p along when the record before still waits for its check; false: that byte is no line end,
    // the quality line of the record before is not as long as its sequence line, and p has moved behind its real end.
    bool read_lines(uint64_t &p, Lines &ln) {
        for (;;) {
            const uint64_t want = std::min<uint64_t>(ln.got ? ln.got * 2 : est, end - p);
            if (w + want + 64 > c->cap) {  // records longer than the buffer: a private, larger one
                Chunk *big = q.get_buffer(std::max<uint64_t>(w + want + 64, 2 * c->cap), true);
                if (w + ln.got) memcpy(big->buf, c->buf, w + ln.got);
                big->starts.swap(c->starts);
                big->lens.swap(c->lens);
                big->ids.swap(c->ids);
                q.recycle(c);
                c = big;
            }
            if (pending) {  // (got == 0, w >= 1: buf[w - 1] is the line end of the record before)
                in.read(c->buf + w - 1, p - 1, want + 1);
                const uint8_t chk = c->buf[w - 1];
                c->buf[w - 1] = '\n';
                pending = false;
                if (chk != '\n') {
                    const uint64_t E4r = E3_prev < end ? line_end_from(E3_prev + 1) : end;
                    p = E4r < end ? E4r + 1 : end;
                    return false;
                }
            } else {
                in.read(c->buf + w + ln.got, p + ln.got, want - ln.got);
            }
            const uint64_t from = ln.e1 == NEED_MORE ? w : ln.e1 + 1;  // (what was searched already holds no line end)
            ln.got = want;
            const bool at_eof = p + ln.got >= end;
            if (ln.e1 == NEED_MORE) {
                const uint8_t *e = (const uint8_t *)memchr(c->buf + from, '\n', (size_t)(w + ln.got - from));
                if (e) ln.e1 = (uint64_t)(e - c->buf);
                else if (at_eof) ln.e1 = ln.e2 = w + ln.got;
            }
            if (ln.e1 != NEED_MORE && ln.e2 == NEED_MORE) {
                const uint64_t s = ln.e1 + 1 < w + ln.got ? ln.e1 + 1 : w + ln.got;
                const uint8_t *e = (const uint8_t *)memchr(c->buf + s, '\n', (size_t)(w + ln.got - s));
                if (e) ln.e2 = (uint64_t)(e - c->buf);
                else if (at_eof) ln.e2 = w + ln.got;
            }
            if (ln.e2 != NEED_MORE) return true;
        }
    }

    // one record at file offset p (< last, the chunk's end) into the chunk; returns where the next one starts
    uint64_t take_record(uint64_t p, uint64_t last) {
        Lines ln;
        if (!read_lines(p, ln)) return p;
        if (c->buf[w] == '\n' || c->buf[w] == '\r') return p + 1;  // blank bytes between records (rare): step over them
        if (c->buf[w] != '@') throw FeederError("malformed FASTQ record");
        const uint64_t got = ln.got, e1 = ln.e1, e2 = ln.e2;
        const uint64_t E2 = p + (e2 - w);                            // file offset of the sequence line's end
        const uint64_t s = e1 + 1 < e2 ? e1 + 1 : e2;                // the sequence line in the buffer: [s, e2)
        const uint64_t S = p + (s - w);
        uint64_t sl = e2 - s;
        if (sl && c->buf[s + sl - 1] == '\r') --sl;
        if (sl >= (1ull << 32)) throw FeederError("sequence length must be < 2^32");
        c->ids.push_back({w + 1, (uint32_t)fasta_id(c->buf + w, e1 - w)});
        c->starts.push_back(s);
        c->lens.push_back((uint32_t)sl);
        // '+' line: its end is in the surplus of the read more often than not; then a quality line as long as the sequence
        // line (else: to the next line end, like parse_chunk)
        uint64_t E3 = end;
        if (E2 < end) {
            const uint64_t ps = e2 + 1;
            const uint8_t *e = ps < w + got ? (const uint8_t *)memchr(c->buf + ps, '\n', (size_t)(w + got - ps)) : nullptr;
            E3 = e ? p + ((uint64_t)(e - c->buf) - w) : line_end_from(p + got);
        }
        uint64_t E4 = E3 < end ? E3 + 1 + (E2 - S) : end;
        if (E4 > end) {
            E4 = E3 < end ? line_end_from(E3 + 1) : end;
        } else if (E4 < end) {
            if (E4 + 1 < last && e2 < w + got) pending = true;  // looked at with the next record's read
            else if (byte_at(E4) != '\n') E4 = line_end_from(E3 + 1);
        }
        E3_prev = E3;
        note_length(E2 - p);
        w = e2 < w + got ? e2 + 1 : e2;  // the next record overwrites what was read beyond the sequence line
        return E4 < end ? E4 + 1 : end;
    }

    // ------------------------------------------------------------ the length estimate
    // a record's header + sequence bytes noted; the next read asks for the longest of the last eight and a margin
    void note_length(uint64_t header_and_sequence) {
        hist[hist_at++ & 7u] = header_and_sequence;
        uint64_t longest = 0;
        for (uint64_t hlen : hist) longest = std::max(longest, hlen);
        est = std::max<uint64_t>(4096, longest + longest / 32 + 256);
    }
};

}  // namespace feeder
}  // namespace mapquik
