// ref_loader.hpp -- the reference FASTA of the native driver, read for ONE purpose: every record, whole, in file order, as fast
// as the host can deliver it to mq_index_add_ref (src/closures.rs:46-94 reads it through seq_io and indexes record by record).
//
// A reference has few, very long records (a human chromosome is one 50-250 MB record), which is the worst case of the chunked
// read feeder (fastx_feeder.hpp): the record that straddles a chunk is read by one thread.  Here the file is read ONCE by all
// threads in parallel (pread of 16-MB blocks into one anonymous, huge-page-backed mapping of the file's size), record starts
// are found by the same threads, multi-line records are compacted in place by a pool (one record per task) while the caller
// already indexes the first ones.  Uncompressed FASTA only: compressed or FASTQ references go through the feeder.
//
// Three parts: RefLoader (the whole file in host memory); two record trackers, LineRecords and RegionRecords, that find the
// records of a file from per-block notes and know every rule about a block border (plain classes: no threads, no file, no locks); and
// RefStreamer, one block pipeline written over a tracker type, which never holds the file: blocks of a size given to its constructor
// (16 MB by default) go to the device as they are read.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "fastx_records.hpp"

namespace mapquik {
namespace feeder {

class RefLoader {
  public:
    struct Record {
        std::string id;        // seq_io's id(): the header up to its first space
        uint64_t seq = 0;      // offset of the (compacted) sequence in the buffer
        uint64_t len = 0;
        uint64_t region_end = 0;  // first byte after the record in the file
    };

    // eager: the file is read (by n_threads threads of its own) from the constructor on, while the caller does something else -- the
    // native driver constructs the loader BEFORE its first HIP call: reading 3.1 GB takes 0.08-0.1 s, bringing the HIP runtime up 0.2 s,
    // on different threads.  wait_read() (or for_each) joins.
    RefLoader(const std::string &path, int n_threads, bool eager = false) : path_(path), n_threads_(n_threads < 1 ? 1 : n_threads) {
        fd_ = open(path.c_str(), O_RDONLY);
        if (fd_ < 0) throw std::runtime_error("Error opening compressed file: " + path);  // get_reader's message (src/main.rs:62)
        struct stat st;
        fstat(fd_, &st);
        size_ = (uint64_t)st.st_size;
        mapped_ = ((size_ + 64 + (2u << 20) - 1) / (2u << 20)) * (2u << 20);
        buf_ = (uint8_t *)mmap(nullptr, mapped_, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (buf_ == MAP_FAILED) {
            buf_ = nullptr;
            close(fd_);
            throw std::runtime_error("cannot map memory for the reference: " + path);
        }
        madvise(buf_, mapped_, MADV_HUGEPAGE);
        if (eager)
            reader_ = std::thread([this] {
                try {
                    read_all();
                } catch (const std::exception &e) { read_err_ = e.what(); }
            });
    }
    ~RefLoader() {
        if (reader_.joinable()) reader_.join();
        stop_pool();
        if (buf_) munmap(buf_, mapped_);
        if (fd_ >= 0) close(fd_);
    }
    RefLoader(const RefLoader &) = delete;
    RefLoader &operator=(const RefLoader &) = delete;

    // fn(const Record &, const uint8_t *sequence) for every record, in file order.  The sequence stays valid until the loader dies.
    // the whole file is in the buffer (eager loaders: joins the reading; others: reads now)
    void wait_read() {
        if (read_done_) return;
        if (reader_.joinable()) {
            reader_.join();
            if (!read_err_.empty()) throw std::runtime_error(read_err_);
        } else {
            read_all();
        }
        read_done_ = true;
    }
    // the buffer the file was read into (whole 2-MB pages, huge-page backed: page-locking it costs milliseconds, tools/pin_rate.hip)
    uint8_t *data() const { return buf_; }
    uint64_t mapped_bytes() const { return mapped_; }
    uint64_t file_bytes() const { return size_; }
    template <class F>
    void for_each(F fn) {
        wait_read();
        find_records();
        start_pool();
        for (size_t i = 0; i < recs_.size(); ++i) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return ready_[i] || !error_.empty(); });
                if (!error_.empty()) throw std::runtime_error(error_);
            }
            fn(recs_[i], buf_ + recs_[i].seq);
        }
    }
    size_t n_records() const { return recs_.size(); }

  private:
    static constexpr uint64_t BLOCK = 16u << 20;

    void read_all() {
        const size_t n_blocks = (size_t)((size_ + BLOCK - 1) / BLOCK);
        std::atomic<size_t> next{0};
        std::vector<std::vector<uint64_t>> found(n_blocks);  // per block: offsets of '>' at a line start ('>' at a block's first byte: checked later)
        std::string err;
        std::mutex emu;
        auto work = [&]() {
            try {
                for (;;) {
                    const size_t b = next.fetch_add(1);
                    if (b >= n_blocks) break;
                    const uint64_t lo = (uint64_t)b * BLOCK, hi = std::min<uint64_t>(lo + BLOCK, size_);
                    pread_full(fd_, buf_ + lo, hi - lo, lo, path_);
                    for (uint64_t p = lo; p < hi;) {
                        const uint8_t *q = (const uint8_t *)memchr(buf_ + p, '>', hi - p);
                        if (!q) break;
                        const uint64_t at = (uint64_t)(q - buf_);
                        if (at == lo || buf_[at - 1] == '\n') found[b].push_back(at);
                        p = at + 1;
                    }
                }
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(emu);
                if (err.empty()) err = e.what();
            }
        };
        std::vector<std::thread> th;
        for (int t = 0; t < n_threads_; ++t) th.emplace_back(work);
        for (auto &t : th) t.join();
        if (!err.empty()) throw std::runtime_error(err);
        for (size_t b = 0; b < n_blocks; ++b)
            for (uint64_t at : found[b])
                if (at == 0 || buf_[at - 1] == '\n') starts_.push_back(at);  // block-first candidates: the byte before is there now
    }

    void find_records() {
        // anything before the first record must be blank (seq_io would reject it; so does the feeder's parser)
        const uint64_t first = starts_.empty() ? size_ : starts_[0];
        for (uint64_t p = 0; p < first; ++p)
            if (buf_[p] != '\n' && buf_[p] != '\r') throw std::runtime_error("malformed FASTA record");
        recs_.resize(starts_.size());
        ready_.assign(starts_.size(), 0);
        for (size_t i = 0; i < starts_.size(); ++i) recs_[i].region_end = i + 1 < starts_.size() ? starts_[i + 1] : size_;
    }

    // header -> id; sequence lines compacted in place
    void prepare(size_t i) {
        Record &r = recs_[i];
        const uint64_t h0 = starts_[i], end = r.region_end;
        const uint8_t *e1 = (const uint8_t *)memchr(buf_ + h0, '\n', end - h0);
        const uint64_t h1 = e1 ? (uint64_t)(e1 - buf_) : end;
        const uint64_t s = h1 < end ? h1 + 1 : end;
        r.id.assign((const char *)buf_ + h0 + 1, fasta_id(buf_ + h0, h1 - h0));
        uint64_t dst = s, q = s;
        while (q < end) {
            const uint8_t *e = (const uint8_t *)memchr(buf_ + q, '\n', end - q);
            const uint64_t le = e ? (uint64_t)(e - buf_) : end;
            uint64_t n = le - q;
            if (n && buf_[q + n - 1] == '\r') --n;
            if (n && dst != q) memmove(buf_ + dst, buf_ + q, n);
            dst += n;
            q = le < end ? le + 1 : end;
        }
        if (dst - s >= (1ull << 32)) throw std::runtime_error("sequence length must be < 2^32");
        r.seq = s;
        r.len = dst - s;
    }

    void start_pool() {
        next_rec_ = 0;
        const int n = (int)std::min<size_t>((size_t)n_threads_, std::max<size_t>(recs_.size(), 1));
        for (int t = 0; t < n; ++t)
            pool_.emplace_back([this] {
                for (;;) {
                    const size_t i = next_rec_.fetch_add(1);
                    if (i >= recs_.size()) return;
                    std::string err;
                    try {
                        prepare(i);
                    } catch (const std::exception &e) { err = e.what(); }
                    {
                        std::lock_guard<std::mutex> lk(mu_);
                        if (!err.empty() && error_.empty()) error_ = err;
                        ready_[i] = 1;
                    }
                    cv_.notify_all();
                }
            });
    }
    void stop_pool() {
        next_rec_ = (size_t)-1 / 2;
        for (auto &t : pool_)
            if (t.joinable()) t.join();
        pool_.clear();
    }

    std::string path_;
    int n_threads_;
    int fd_ = -1;
    uint64_t size_ = 0, mapped_ = 0;
    uint8_t *buf_ = nullptr;
    std::thread reader_;
    std::string read_err_;
    bool read_done_ = false;
    std::vector<uint64_t> starts_;
    std::vector<Record> recs_;
    std::vector<char> ready_;
    std::atomic<size_t> next_rec_{0};
    std::vector<std::thread> pool_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::string error_;
};

// ---------------------------------------------------------------- the reference streamed: two record trackers and one block pipeline
// A record tracker turns the blocks of a file into its records without ever holding the file: scan() notes what a block says about
// lines (any thread, any order), consume() takes these notes in block order, finish() closes the file; every record goes to the sink
// as (hdr_start, hdr_end, at, len), file offsets: the header line [hdr_start, hdr_end) without its line end, and the bytes
// [at, at + len) that belong to it.  false from consume() or finish(): the file is not of the tracker's shape (`irregular`).  No
// threads, no file, no locks: every rule about a block border is here, and a test can put a border anywhere (RefStreamer's block size).
using RecordSink = std::function<void(uint64_t hdr_start, uint64_t hdr_end, uint64_t at, uint64_t len)>;

// One header line, one sequence line per record (what assemblers and this repository's tools write); [at, at + len) is the sequence line
// without its line end.  Sequences over several lines, text before the first '>', a header without its sequence line: irregular.
class LineRecords {
  public:
    struct NL {
        uint64_t pos;         // file offset of a '\n'
        uint8_t cr;           // a '\r' in front of it (inside the block)
        uint8_t next_known;   // the byte behind it lies in this block ...
        uint8_t next;         // ... and is this one: the first byte of the next line
    };
    struct Summary {
        uint64_t lo = 0, n = 0;  // the block: file offset, bytes
        std::vector<NL> nl;
        bool too_many = false;
        uint8_t first_byte = 0, last_byte = 0;
    };
    static constexpr size_t MAX_LINES_PER_BLOCK = 65536;  // single-line records of >= 512 bytes on average; beyond: the host parser's case

    explicit LineRecords(RecordSink sink) : sink_(std::move(sink)) {}

    static Summary scan(const uint8_t *chunk, uint64_t n, uint64_t lo) {
        Summary sc;
        sc.lo = lo;
        sc.n = n;
        const uint8_t *p = chunk, *end = chunk + n;
        if (n) {
            sc.first_byte = chunk[0];
            sc.last_byte = chunk[n - 1];
        }
        while (p < end) {
            const uint8_t *q = (const uint8_t *)memchr(p, '\n', (size_t)(end - p));
            if (!q) break;
            if (sc.nl.size() >= MAX_LINES_PER_BLOCK) {
                sc.too_many = true;
                return sc;
            }
            NL e;
            e.pos = lo + (uint64_t)(q - chunk);
            e.cr = (q > chunk && q[-1] == '\r') ? 1 : 0;
            e.next_known = q + 1 < end ? 1 : 0;
            e.next = q + 1 < end ? q[1] : 0;
            sc.nl.push_back(e);
            p = q + 1;
        }
        return sc;
    }

    bool consume(const Summary &s) {
        if (s.too_many) return false;  // a block full of line ends: a line-wrapped FASTA (or very many tiny records): the host parser's case
        if (cur_first < 0 && s.n) cur_first = s.first_byte;  // the line that opens this block
        for (const NL &e : s.nl) {
            const bool cr = e.pos == s.lo ? (s.lo > 0 && prev_last == '\r') : e.cr != 0;
            if (!end_line(e.pos, cr)) return false;
            cur_first = e.next_known ? (int)e.next : -1;
        }
        if (s.n) prev_last = s.last_byte;
        return true;
    }

    bool finish(uint64_t file_size) {
        if (line_start < file_size && !end_line(file_size, false)) return false;  // the file's last line has no '\n'
        return !have_header;                                                      // a header without its sequence line
    }

  private:
    // a line [line_start, nl) ends (at its '\n', or at the file's end); cr: a '\r' in front of the line end.  Lines alternate: header
    // ('>' first), sequence (anything else first, or empty).  false: the file is not of that shape.
    bool end_line(uint64_t nl, bool cr) {
        const uint64_t ls = line_start, le = (cr && nl > ls) ? nl - 1 : nl;
        const bool starts_gt = ls < nl && cur_first == '>';
        line_start = nl + 1;
        if (!have_header) {
            if (ls == le) return true;     // a blank line where a header may start (before the first record, between records, at the end): skipped, as seq_io does
            if (!starts_gt) return false;  // text before the first '>', a sequence that goes on over several lines
            have_header = true;
            hdr_start = ls;
            hdr_end = le;
            return true;
        }
        if (starts_gt) return false;  // a header without its sequence line
        have_header = false;
        if (le - ls >= (1ull << 32)) throw std::runtime_error("sequence length must be < 2^32");
        sink_(hdr_start, hdr_end, ls, le - ls);
        return true;
    }

    RecordSink sink_;
    // line bookkeeping over the whole file: the start of the current line, and for a record in the making its header line
    uint64_t line_start = 0;
    bool have_header = false;
    uint64_t hdr_start = 0, hdr_end = 0;  // [hdr_start, hdr_end): the header line without its line end
    int cur_first = -1;                   // first byte of the line being read; -1: not seen yet (it opens the next block)
    uint8_t prev_last = 0;                // the last byte of the block consumed before
};

// A record is its header line plus every line up to the next line that starts with '>' (or the file's end); [at, at + len) is that whole
// region behind the header line's '\n', line ends and all.  The block scan looks for '>' at a line start and for the line end of that
// header only -- a wrapped file has 200,000 line ends per block.  Text before the first '>' other than blank lines is irregular.
// (Blank = '\n' and '\r' only, and the first '>' must follow a '\n' or open the file: "\r>a", or a '\r' and the '>' on either side of a
// block border, is irregular too.)
class RegionRecords {
  public:
    static constexpr uint64_t NONE = ~(uint64_t)0;
    struct Hdr {
        uint64_t pos;  // file offset of a '>' at a line start (at a block's first byte: whether a line starts there is known later)
        uint64_t nl;   // file offset of the '\n' that ends that line; NONE: it lies in a later block
        uint8_t cr;    // a '\r' in front of it
    };
    // the header lines that start in the block, the block's first '\n' (it ends a header that began earlier) and the number of blank
    // bytes ('\n', '\r') the block opens with (all of the file in front of its first '>' must be)
    struct Summary {
        uint64_t lo = 0, n = 0;  // the block: file offset, bytes
        std::vector<Hdr> hdrs;
        uint64_t first_nl = NONE, lead_blank = 0;
        uint8_t first_nl_cr = 0, last_byte = 0;
    };

    explicit RegionRecords(RecordSink sink) : sink_(std::move(sink)) {}

    static Summary scan(const uint8_t *c, uint64_t n64, uint64_t lo) {
        Summary sc;
        sc.lo = lo;
        sc.n = n64;
        const size_t n = (size_t)n64;
        if (!n) return sc;
        sc.last_byte = c[n - 1];
        size_t b = 0;
        while (b < n && (c[b] == '\n' || c[b] == '\r')) ++b;
        sc.lead_blank = b;
        if (const uint8_t *q = (const uint8_t *)memchr(c, '\n', n)) {
            sc.first_nl = lo + (uint64_t)(q - c);
            sc.first_nl_cr = (q > c && q[-1] == '\r') ? 1 : 0;
        }
        for (size_t p = 0; p < n;) {
            const uint8_t *q = (const uint8_t *)memchr(c + p, '>', n - p);
            if (!q) break;
            const size_t o = (size_t)(q - c);
            if (o && c[o - 1] != '\n') {
                p = o + 1;
                continue;
            }
            const uint8_t *e = (const uint8_t *)memchr(q, '\n', n - o);
            Hdr h;
            h.pos = lo + o;
            h.nl = e ? lo + (uint64_t)(e - c) : NONE;
            h.cr = (e && e[-1] == '\r') ? 1 : 0;
            sc.hdrs.push_back(h);
            p = e ? (size_t)(e - c) + 1 : n;
        }
        return sc;
    }

    bool consume(const Summary &s) {
        const bool ok = headers_of(s);
        if (s.n) prev_last = s.last_byte;
        return ok;
    }

    bool finish(uint64_t file_size) {
        if (open) close_record(file_size);
        return true;  // (an empty or all-blank file has no record: the pipeline's business)
    }

  private:
    bool headers_of(const Summary &s) {
        const uint64_t lo = s.lo;
        if (open && cur_he == NONE && s.first_nl != NONE) {  // the header that began in an earlier block ends here
            cur_he = s.first_nl;
            cur_cr = s.first_nl == lo ? prev_last == '\r' : s.first_nl_cr != 0;
        }
        bool first = true;
        for (const Hdr &h : s.hdrs) {
            if (h.pos == lo && lo > 0 && prev_last != '\n') continue;  // a '>' that opens the block but not a line
            if (first && !seen_header && s.lead_blank < h.pos - lo) return false;  // text before the first '>'
            first = false;
            if (open) close_record(h.pos);
            open = seen_header = true;
            cur_hs = h.pos;
            cur_he = h.nl;
            cur_cr = h.cr != 0;
        }
        return !(first && !seen_header && s.lead_blank < s.n);
    }
    // (a record closed by the next header knows its header's line end: a '>' at a line start lies behind a '\n')
    void close_record(uint64_t region_end) {
        const uint64_t he = cur_he == NONE ? region_end : cur_he;  // (a file that ends inside a header line: region_end is the file's end)
        const bool cr = cur_he == NONE ? prev_last == '\r' : cur_cr;
        const uint64_t at = std::min<uint64_t>(he + 1, region_end);
        sink_(cur_hs, (cr && he > cur_hs + 1) ? he - 1 : he, at, region_end - at);
        open = false;
    }

    RecordSink sink_;
    // the record in the making -- its header line [cur_hs, cur_he) ('\n' at cur_he; NONE: not seen yet, it lies in a later block),
    // cur_cr: a '\r' in front of that line end
    bool open = false, seen_header = false;
    uint64_t cur_hs = 0, cur_he = NONE;
    bool cur_cr = false;
    uint8_t prev_last = 0;  // the last byte of the block consumed before
};

// RefStreamer -- the same file, never held in host memory: the common shape of a reference FASTA written by a tool (one header line, one
// sequence line per record) goes to the device as it is read.  Reader threads pread blocks (16 MB unless the constructor is told
// otherwise) into a small pool of page-locked chunks and note what the record tracker wants to know of each (Tracker::scan); the
// calling thread queues every block's copy into the index's staging buffer the moment it is read (mq_index_stage_piece: the PCIe link
// runs beside the reads, 3.1 GB in ~0.08 s), recycles a chunk when its copy is done, and feeds the notes to the tracker in block
// order; a third thread hands every record to the index as soon as its last block is on its way (mq_index_add_ref_staged: the build's
// kernels wait on the device for the pieces, not on the host).  The host looks at a header line only (pread of its few bytes) and
// never at a base: lower case and CR-LF are the kernels' / the spans' business.
// The tracker is LineRecords, and anything but "header line, sequence line" -- sequences over several lines, text before the first
// '>' -- ends the run as `irregular`: the caller falls back to RefLoader (a line-wrapped FASTA shows in its first block, before
// anything was indexed).  join_lines (the driver's --ref-join device): the tracker is RegionRecords, the callback gets the whole
// region of a record and its lines are joined on the device (mq_index_add_ref_staged_lines).  The pipeline is the same for both and
// knows nothing of lines.
class RefStreamer {
  public:
    struct Hooks {
        std::function<void *(size_t)> alloc;                                          // page-locked memory (mq_host_alloc)
        std::function<void(void *)> release;
        std::function<uint64_t(uint64_t at, const uint8_t *src, uint64_t n)> piece;   // mq_index_stage_piece: returns the ticket, throws on error
        std::function<bool(uint64_t ticket, bool wait)> done;                         // mq_index_stage_done
    };
    struct Result {
        bool irregular = false;  // not of the tracker's shape all through
        size_t handed = 0;       // records handed to the callback before that was noticed
        size_t records = 0;
    };
    static constexpr uint64_t BLOCK = 16u << 20;

    // block_bytes: the size of a block and of a chunk (tests put block borders where they want them)
    RefStreamer(const std::string &path, int n_threads, Hooks hooks, bool join_lines = false, uint64_t block_bytes = BLOCK)
        : path_(path), n_threads_(n_threads < 1 ? 1 : n_threads), hooks_(std::move(hooks)), join_lines_(join_lines),
          block_(block_bytes < 1 ? 1 : block_bytes) {
        fd_ = open(path.c_str(), O_RDONLY);
        if (fd_ < 0) throw std::runtime_error("Error opening compressed file: " + path);  // get_reader's message (src/main.rs:62)
        struct stat st;
        fstat(fd_, &st);
        size_ = (uint64_t)st.st_size;
    }
    ~RefStreamer() {
        for (void *c : all_chunks_) hooks_.release(c);
        if (fd_ >= 0) close(fd_);
    }
    RefStreamer(const RefStreamer &) = delete;
    RefStreamer &operator=(const RefStreamer &) = delete;
    uint64_t file_bytes() const { return size_; }

    // fn(record number, id, offset of the sequence in the file = in the staging buffer, length), in file order, from a thread of its own
    // (join_lines: offset and length of the region behind the header line, line ends and all)
    template <class F>
    Result run(F fn) {
        return join_lines_ ? run_with<RegionRecords>(fn) : run_with<LineRecords>(fn);
    }

  private:
    template <class Tracker, class F>
    Result run_with(F &fn) {
        struct Block {
            size_t block = 0;
            uint8_t *chunk = nullptr;
            uint64_t n = 0;
            typename Tracker::Summary notes;
        };
        Result res;
        const size_t n_blocks = (size_t)((size_ + block_ - 1) / block_);
        const size_t pool_size = (size_t)n_threads_ + 4;
        std::mutex mu;
        std::condition_variable cv;
        std::vector<void *> pool;           // free chunks
        size_t allocated = 0;               // chunks made so far (each reader makes its own first one: the pinning runs in parallel)
        std::deque<Block> scanned;          // blocks read and scanned, any order
        std::atomic<size_t> next_block{0};
        bool stop = false;
        std::string err;
        auto reader = [&]() {
            try {
                for (;;) {
                    const size_t b = next_block.fetch_add(1);
                    if (b >= n_blocks) return;
                    void *chunk = nullptr;
                    {
                        std::unique_lock<std::mutex> lk(mu);
                        cv.wait(lk, [&] { return stop || !pool.empty() || allocated < pool_size; });
                        if (stop) return;
                        if (!pool.empty()) {
                            chunk = pool.back();
                            pool.pop_back();
                        } else {
                            ++allocated;
                        }
                    }
                    if (!chunk) {
                        chunk = hooks_.alloc((size_t)block_);
                        if (!chunk) throw std::runtime_error("cannot allocate a page-locked block for the reference");
                        std::lock_guard<std::mutex> lk(mu);
                        all_chunks_.push_back(chunk);
                    }
                    Block sc;
                    sc.block = b;
                    sc.chunk = (uint8_t *)chunk;
                    const uint64_t lo = (uint64_t)b * block_, hi = std::min<uint64_t>(lo + block_, size_);
                    sc.n = hi - lo;
                    pread_full(fd_, sc.chunk, sc.n, lo, path_);
                    sc.notes = Tracker::scan(sc.chunk, sc.n, lo);
                    {
                        std::lock_guard<std::mutex> lk(mu);
                        scanned.push_back(std::move(sc));
                    }
                    cv.notify_all();
                }
            } catch (const std::exception &e) {
                std::lock_guard<std::mutex> lk(mu);
                if (err.empty()) err = e.what();
                stop = true;
                cv.notify_all();
            }
        };
        // the indexer: records in file order, as soon as the calling thread has queued their last block's copy
        struct Rec {
            std::string id;
            uint64_t at, len;
        };
        std::deque<Rec> to_index;
        bool no_more_records = false;
        std::thread indexer([&]() {
            size_t k = 0;
            for (;;) {
                Rec r;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return !to_index.empty() || no_more_records; });
                    if (to_index.empty()) return;
                    r = std::move(to_index.front());
                    to_index.pop_front();
                }
                try {
                    fn(k, r.id, r.at, r.len);
                    ++k;
                    std::lock_guard<std::mutex> lk(mu);
                    res.handed = k;
                } catch (const std::exception &e) {
                    std::lock_guard<std::mutex> lk(mu);
                    if (err.empty()) err = e.what();
                    stop = true;
                    to_index.clear();
                    no_more_records = true;
                    cv.notify_all();
                    return;
                }
            }
        });
        std::vector<std::thread> readers;
        for (int t = 0; t < n_threads_; ++t) readers.emplace_back(reader);

        std::deque<std::pair<uint64_t, void *>> inflight;        // (ticket, chunk) in issue order
        std::map<size_t, typename Tracker::Summary> held;        // the notes of blocks waiting for their turn in the tracker
        size_t next_in_order = 0, issued = 0;
        auto give_back = [&](void *chunk) {
            {
                std::lock_guard<std::mutex> lk(mu);
                pool.push_back(chunk);
            }
            cv.notify_all();
        };
        auto recycle = [&](bool must) {  // chunks whose copy is done go back to the pool; must: wait for the oldest one
            while (!inflight.empty()) {
                if (!hooks_.done(inflight.front().first, must)) break;
                give_back(inflight.front().second);
                inflight.pop_front();
                must = false;
            }
        };
        // a record goes to the indexer: header line [hs, he) without its line end, sequence (join_lines: region) [at, at + len)
        Tracker tracker([&](uint64_t hs, uint64_t he, uint64_t at, uint64_t len) {
            Rec r;
            r.at = at;
            r.len = len;
            // seq_io's id(): the header up to its first space -- the only bytes of the file the host reads
            std::vector<uint8_t> h((size_t)(he - hs));
            pread_full(fd_, h.data(), h.size(), hs, path_);
            if (!h.empty()) r.id.assign((const char *)h.data() + 1, (size_t)fasta_id(h.data(), h.size(), true));
            {
                std::lock_guard<std::mutex> lk(mu);
                to_index.push_back(std::move(r));
            }
            ++res.records;
            cv.notify_all();
        });
        try {
            while (issued < n_blocks && !res.irregular) {
                Block sc;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    if (scanned.empty() && !stop) {
                        lk.unlock();
                        recycle(false);
                        lk.lock();
                        // nothing scanned yet: with copies in flight wait for the oldest (a reader may be waiting for its chunk), else for a scan
                        if (scanned.empty() && !stop) {
                            if (!inflight.empty()) {
                                lk.unlock();
                                recycle(true);
                                continue;
                            }
                            cv.wait(lk, [&] { return !scanned.empty() || stop; });
                        }
                    }
                    if (stop) break;
                    if (scanned.empty()) continue;
                    sc = std::move(scanned.front());
                    scanned.pop_front();
                }
                inflight.emplace_back(hooks_.piece((uint64_t)sc.block * block_, sc.chunk, sc.n), sc.chunk);
                ++issued;
                // (the bytes are the link's now; the tracker uses what the scan noted)
                held.emplace(sc.block, std::move(sc.notes));
                for (auto it = held.find(next_in_order); it != held.end() && !res.irregular; it = held.find(next_in_order)) {
                    if (!tracker.consume(it->second)) res.irregular = true;
                    held.erase(it);
                    ++next_in_order;
                }
            }
            if (!res.irregular && !stop) {
                if (!tracker.finish(size_)) res.irregular = true;
                if (res.records == 0) res.irregular = true;  // (an empty or all-blank file: the host parser says what it is)
            }
        } catch (const std::exception &e) {
            std::lock_guard<std::mutex> lk(mu);
            if (err.empty()) err = e.what();
        }
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
            no_more_records = true;
            if (res.irregular) to_index.clear();
        }
        cv.notify_all();
        for (auto &t : readers) t.join();
        indexer.join();
        try {
            while (!inflight.empty()) recycle(true);
        } catch (const std::exception &e) {
            if (err.empty()) err = e.what();
        }
        if (!err.empty()) throw std::runtime_error(err);
        return res;
    }

    std::string path_;
    int n_threads_;
    Hooks hooks_;
    bool join_lines_ = false;
    uint64_t block_ = BLOCK;
    int fd_ = -1;
    uint64_t size_ = 0;
    std::vector<void *> all_chunks_;
};

}  // namespace feeder
}  // namespace mapquik
