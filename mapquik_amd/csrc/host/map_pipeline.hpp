// map_pipeline.hpp -- the map phase of the native driver (mapquik_main.cc): chunks of reads from the feeder go to the GPUs through the
// stream slots of the submitting threads, come back with their hits, are formatted as PAF by a small pool and written in input order
// by the calling thread (main_thread_mer, src/closures.rs:117-123).  One mutex and one condition variable guard the queue between
// submitters and formatters and the map of formatted chunks waiting for their turn.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fastx_feeder.hpp"
#include "mapquik_host.hpp"

namespace mapquik {

using Clock = std::chrono::steady_clock;
inline double secs(Clock::time_point a) { return std::chrono::duration<double>(Clock::now() - a).count(); }
inline long long us_since(Clock::time_point a) { return (long long)std::chrono::duration_cast<std::chrono::microseconds>(Clock::now() - a).count(); }

// The records of a chunk that was submitted unparsed (mq_ctx_submit_fastx): hits and line ends (or header spans, fx_format
// MQ_FASTX_FASTA_LINES) come back together and become the chunk's spans and hits.  A chunk the device hands back MQ_FASTA_IRREGULAR
// (sequences over several lines, blank lines, ...) goes the old way: parsed here, its spans submitted, waited for.  Returns whether it did.
inline bool collect_device_records(mq_ctx *ctx, feeder::Chunk &c, uint32_t fx_format) {
    const bool wrapped = fx_format == MQ_FASTX_FASTA_LINES;
    uint32_t n = 0, n_lines = 0, flags = 0;
    const uint32_t *line_ends = nullptr, *hdr_begin = nullptr, *hdr_end = nullptr, *seq_lens = nullptr;
    const mq_hit *hits = nullptr;
    if (wrapped ? mq_ctx_wait_fasta_lines(ctx, &n, &hdr_begin, &hdr_end, &seq_lens, &hits, &flags) != MQ_OK
                : mq_ctx_wait_fasta(ctx, &n, &line_ends, &n_lines, &hits, &flags) != MQ_OK)
        throw Error(std::string(wrapped ? "mq_ctx_wait_fasta_lines: " : "mq_ctx_wait_fasta: ") + last_error());
    if (flags & MQ_FASTA_IRREGULAR) {
        c.materialize();  // a view of the mapped file: the parser compacts sequence lines in place
        feeder::parse_chunk(c, fx_format == MQ_FASTX_FASTQ);
        c.hits.resize(c.starts.size());
        if (!c.starts.empty() && (mq_ctx_submit_spans(ctx, c.buf, c.bytes, c.starts.data(), c.lens.data(), (uint32_t)c.starts.size(), c.hits.data()) != MQ_OK ||
                                  mq_ctx_wait(ctx) != MQ_OK))
            throw Error(std::string("mq_ctx_submit_spans: ") + last_error());
        return true;
    }
    if (wrapped) feeder::spans_from_headers(c, hdr_begin, hdr_end, seq_lens, n);
    else feeder::spans_from_line_ends(c, line_ends, n_lines, fx_format == MQ_FASTX_FASTQ ? 4u : 2u);
    c.hits.assign(hits, hits + n);
    return false;
}

// --anchors, --chains: the spans and pool entries of the batch the slot has just finished become the chunk's (the library's host copies
// last until the slot's next submit).  A pool that was too small for the chunk ends the run, like any other pipeline failure, with what it
// needed.  read_back: mq_ctx_anchors / mq_ctx_chains, `call` its name; option, pool_noun: "--anchors", "anchor" / "--chains", "chain"
template <class Span, class Item, class ReadBack>
inline void take_pooled(ReadBack read_back, const char *call, const char *option, const char *pool_noun, mq_ctx *ctx, const feeder::Chunk &c,
                        feeder::PooledItems<Span, Item> &out) {
    out.spans.clear();
    out.pool.clear();
    if (c.hits.empty()) return;  // nothing was mapped for this chunk: the slot's last batch is somebody else's
    const Span *spans = nullptr;
    const Item *pool = nullptr;
    uint32_t n = 0, dropped = 0;
    uint64_t stored = 0, needed = 0;
    if (read_back(ctx, &spans, &pool, &n, &stored, &needed, &dropped) != MQ_OK) throw Error(std::string(call) + ": " + last_error());
    if (n != c.hits.size()) throw Error(std::string(call) + ": " + std::to_string(n) + " spans for a chunk of " + std::to_string(c.hits.size()) + " reads");
    if (dropped)
        throw Error(std::string(option) + ": the " + pool_noun + " pool of a stream slot was too small for " + std::to_string(dropped) + " reads of a chunk: " +
                    std::to_string(needed) + " entries needed, " + std::to_string(stored) + " reserved");
    out.spans.assign(spans, spans + n);
    out.pool.assign(pool, pool + stored);
}

// --chains: the lines of read i -- one per chain, in span order: the twelve PAF columns of the chain (mq_format_paf_chain's bytes), tp:A:P
// for the read's unique top chain and tp:A:S for every other, cn:i:<n_runs>, and tie:i:1 on a top chain of a tied read (tp S: no primary)
inline std::string format_chains(feeder::Chunk &c, PafWriter &pw, size_t i) {
    if (!c.chains.holds(i)) return "--chains: a read without its chains";
    const mq_chain *ch = c.chains.pool.data() + c.chains.spans[i].first;
    const uint32_t n = c.chains.spans[i].count;
    uint32_t tops = 0;
    for (uint32_t j = 0; j < n; ++j) tops += (ch[j].flags & MQ_CHAIN_TOP) ? 1u : 0u;
    char tag[64];
    for (uint32_t j = 0; j < n; ++j) {
        mq_hit h;  // field for field the chain's layout: the columns are where the PAF writer reads them
        static_assert(sizeof(mq_hit) == sizeof(mq_chain), "mq_chain has the layout of mq_hit");
        memcpy(&h, &ch[j], sizeof(h));
        pw.append(c.chains.text, (const char *)c.buf + c.ids[i].off, c.ids[i].len, c.lens[i], h);
        c.chains.text.pop_back();  // (the writer's newline)
        const bool top = (ch[j].flags & MQ_CHAIN_TOP) != 0;
        c.chains.text.append(tag, (size_t)snprintf(tag, sizeof(tag), "\ttp:A:%c\tcn:i:%u%s\n", top && tops == 1 ? 'P' : 'S', ch[j].n_runs, top && tops > 1 ? "\ttie:i:1" : ""));
    }
    return "";
}

// A mapped chunk's output: PAF lines of the mapped reads (src/mers.rs:181), and of the unmapped ones the names (want_unmapped) and the
// records as FASTA (want_fasta, for a second pass).  Returns the error text for a hit that is neither, "" else.
// want_anchors: beside a mapped read's PAF line, one line per Match run of its chain, in read order (take_pooled filled c.anchors):
// q_id, q_start, q_end, strand, r_name, r_start, r_end, count
// want_chains: one line per candidate chain of EVERY read, mapped or tied (format_chains)
inline std::string format_chunk(feeder::Chunk &c, PafWriter &pw, bool want_unmapped, bool want_fasta, bool want_anchors = false, bool want_chains = false) {
    std::string id;
    c.paf.reserve(c.lens.size() * 96);
    for (size_t i = 0; i < c.lens.size(); ++i) {
        const mq_hit &h = c.hits[i];
        if (want_chains && (h.status == MQ_HIT_MAPPED || h.status == MQ_HIT_UNMAPPED)) {
            const std::string err = format_chains(c, pw, i);
            if (!err.empty()) return err;
        }
        if (h.status == MQ_HIT_MAPPED) {
            pw.append(c.paf, (const char *)c.buf + c.ids[i].off, c.ids[i].len, c.lens[i], h);  // src/mers.rs:181
            if (want_anchors) {
                if (!c.anchors.holds(i)) return "--anchors: a mapped read without its anchors";
                const std::string &rn = pw.ref_name(h.ref_id);
                char num[128];
                std::string &txt = c.anchors.text;
                for (uint32_t j = 0; j < c.anchors.spans[i].count; ++j) {
                    const mq_anchor &a = c.anchors.pool[(size_t)c.anchors.spans[i].first + j];
                    txt.append((const char *)c.buf + c.ids[i].off, c.ids[i].len);
                    txt.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%u\t%c\t", a.q_start, a.q_end, h.rc ? '-' : '+'));
                    txt += rn;
                    txt.append(num, (size_t)snprintf(num, sizeof(num), "\t%u\t%u\t%u\n", a.r_start, a.r_end, a.count));
                }
            }
            continue;
        }
        id.assign((const char *)c.buf + c.ids[i].off, c.ids[i].len);
        if (h.status != MQ_HIT_UNMAPPED) return "find_matches: read " + id + " could not be processed";
        if (want_unmapped) { c.unmapped += id; c.unmapped.push_back('\n'); }
        if (want_fasta) {
            c.unmapped_fa.push_back('>');
            c.unmapped_fa += id;
            c.unmapped_fa.push_back('\n');
            if (!c.regions.empty()) feeder::append_joined_region(c, c.regions[i].first, c.regions[i].second, c.unmapped_fa);  // (joined on the device: no starts)
            else c.unmapped_fa.append((const char *)c.buf + c.starts[i], c.lens[i]);
            c.unmapped_fa.push_back('\n');
        }
    }
    return std::string();
}

// --sort: the pass's sorter and, per read number in input order, where the read's line lies in <prefix>.paf and how long it is (0: the
// read has no line).  The ordered writer fills it: only there is a chunk's first read number known (a chunk whose records the device
// finds says how many reads it holds when it comes back, and chunks come back in any order).
struct SortLines {
    mq_sorter *sorter = nullptr;
    std::vector<uint64_t> at;
    std::vector<uint32_t> len;
    uint64_t paf_bytes = 0;
};

class MapPipeline {
  public:
    struct Config {
        int n_format;        // PAF formatters
        uint32_t fx_format;  // MQ_FASTX_* of the chunks that come unparsed
        long fail_at;        // MQ_DRIVER_FAIL_AT (test hook): the submitter that takes this chunk number reports a failure; -1: none
        FILE *anchors = nullptr;  // --anchors: <prefix>.anchors, written the way the unmapped names are
        double density = 0;       // ... and what a slot's reservation is sized with (Ctx::reserve_anchors)
        FILE *chains = nullptr;   // --chains: <prefix>.chains, the same way
        mq_depth *depth = nullptr;  // --depth: the run's accumulator; every chunk's final hits are added where the chunk goes to the formatters
        SortLines *sort = nullptr;  // --sort: every chunk's final hits are added by the ordered writer, under the reads' numbers in input order
    };
    // slots[w]: the stream slots of submitter w (n_sub submitters per GPU, each over its GPU's index); index: where the formatters look
    // reference names up; paf, unmapped, unmapped_fa: the open output files, the last two may be null
    MapPipeline(feeder::Feeder &feed, std::vector<std::vector<Ctx>> &slots, const ReadOnlyIndex &index, FILE *paf, FILE *unmapped, FILE *unmapped_fa, const Config &cfg)
        : feed_(feed), slots_(slots), index_(index), paf_(paf), unm_(unmapped), ufa_(unmapped_fa), cfg_(cfg), submitters_left_((int)slots.size()) {}

    // Starts the submitters and the formatters, writes on the calling thread, joins.  On a failure the feeder is aborted and the first
    // error is thrown.
    void run() {
        std::vector<std::thread> submitters, formatters;
        for (size_t w = 0; w < slots_.size(); ++w) submitters.emplace_back([this, w] { submit_loop(w); });
        for (int f = 0; f < cfg_.n_format; ++f) formatters.emplace_back([this] { format_loop(); });
        write_in_order();
        // On a failure the chunks in flight are never recycled, so the feeder's workers (waiting for a buffer) and the submitters
        // (waiting for a chunk) would wait forever: the feeder is told to give up, which wakes both.
        if (failed()) feed_.abort();
        for (auto &t : submitters) t.join();
        cv_.notify_all();
        for (auto &t : formatters) t.join();
        if (!werr_.empty()) throw Error(werr_);
    }

    // MQ_DRIVER_TIMING (diagnostic, stderr): where the map phase's threads spent their time
    void report(double phase_secs) const {
        fprintf(stderr, "map phase %.3f s; summed over threads: submit %.3f s, finish (wait + spans) %.3f s, waiting for a chunk %.3f s (%d submitters), "
                        "format %.3f s (%d formatters), write + recycle %.3f s\n", phase_secs, t_submit_us_ / 1e6, t_finish_us_ / 1e6, t_fetch_us_ / 1e6, (int)slots_.size(),
                t_format_us_ / 1e6, cfg_.n_format, t_write_us_ / 1e6);
        fprintf(stderr, "unparsed chunks %llu irregular %llu\n", (unsigned long long)n_unparsed_.load(), (unsigned long long)n_irregular_.load());
    }

  private:
    using Chunk = feeder::Chunk;

    // one submitting thread: its stream slots and the chunks in flight in them
    struct Submitter {
        MapPipeline &p;
        std::vector<Ctx> &ctx;
        std::vector<Chunk *> inflight;
        std::vector<size_t> age;  // submit order of the chunk in the slot
        size_t submitted = 0;
        Submitter(MapPipeline &p_, std::vector<Ctx> &ctx_) : p(p_), ctx(ctx_), inflight(ctx_.size(), nullptr), age(ctx_.size(), 0) {}

        int free_slot() const {
            for (int sl = 0; sl < (int)inflight.size(); ++sl)
                if (!inflight[sl]) return sl;
            return -1;
        }
        // the busy slot that was submitted longest ago (-1: none is busy)
        int oldest_busy() const {
            int best = -1;
            for (int sl = 0; sl < (int)inflight.size(); ++sl)
                if (inflight[sl] && (best < 0 || age[sl] < age[best])) best = sl;
            return best;
        }
        void submit(Chunk *c, int sl) {
            const auto ts0 = Clock::now();
            // --anchors: the slots reserve for the feeder's chunk size when they are made; a chunk that is larger (one very long record) makes its slot reserve again
            if (p.cfg_.anchors && c->bytes > ctx[sl].anchors_bytes()) ctx[sl].reserve_anchors(c->bytes, p.cfg_.density);
            if (p.cfg_.chains && c->bytes > ctx[sl].chains_bytes()) ctx[sl].reserve_chains(c->bytes, p.cfg_.density);
            if (c->unparsed) {
                if (mq_ctx_submit_fastx(ctx[sl].handle(), c->buf, c->begin, c->bytes, p.cfg_.fx_format) != MQ_OK) throw Error(std::string("mq_ctx_submit_fastx: ") + last_error());
            } else if (mq_ctx_submit_spans(ctx[sl].handle(), c->buf, c->bytes, c->starts.data(), c->lens.data(), (uint32_t)c->starts.size(), c->hits.data()) != MQ_OK) {
                throw Error(std::string("mq_ctx_submit_spans: ") + last_error());
            }
            p.t_submit_us_ += us_since(ts0);
            inflight[sl] = c;
            age[sl] = submitted++;
        }
        // waits for the slot's chunk and passes it to the formatters (after a failure too: the writer counts on every chunk)
        void finish_slot(int sl) {
            if (!inflight[sl]) return;
            const auto tf0 = Clock::now();
            Chunk *c = inflight[sl];
            try {
                if (c->unparsed) {  // records found on the device
                    ++p.n_unparsed_;
                    if (collect_device_records(ctx[sl].handle(), *c, p.cfg_.fx_format)) ++p.n_irregular_;
                } else if (mq_ctx_wait(ctx[sl].handle()) != MQ_OK) {
                    throw Error(std::string("mq_ctx_wait: ") + last_error());
                }
                if (p.cfg_.anchors) take_pooled(mq_ctx_anchors, "mq_ctx_anchors", "--anchors", "anchor", ctx[sl].handle(), *c, c->anchors);
                if (p.cfg_.chains) take_pooled(mq_ctx_chains, "mq_ctx_chains", "--chains", "chain", ctx[sl].handle(), *c, c->chains);
                // --depth: behind the wait, so the host-driven redos are in; one call per chunk, from whichever GPU's slot it came
                if (p.cfg_.depth && !c->hits.empty() && mq_depth_add(p.cfg_.depth, c->hits.data(), (uint32_t)c->hits.size()) != MQ_OK)
                    throw Error(std::string("mq_depth_add: ") + last_error());
            } catch (const std::exception &e) { p.fail(e.what()); }
            c->unparsed = false;
            inflight[sl] = nullptr;
            p.to_formatters(c);
            p.t_finish_us_ += us_since(tf0);
        }
    };

    void fail(const std::string &m) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (werr_.empty()) werr_ = m;
        }
        cv_.notify_all();
    }
    bool failed() {
        std::lock_guard<std::mutex> lk(mu_);
        return !werr_.empty();
    }
    void to_formatters(Chunk *c) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            to_format_.push_back(c);
        }
        cv_.notify_all();
    }

    void submit_loop(size_t worker) {
        Submitter s(*this, slots_[worker]);
        try {
            for (;;) {
                if (failed()) break;  // somebody failed: stop pulling chunks
                // Never wait for a new chunk while holding submitted ones: the writer may be waiting for exactly one of
                // them while every other buffer of the pool sits behind the writer (formatted, out of turn) -- then no
                // new chunk can ever be parsed.  With nothing ready, the oldest submitted chunk is passed on first.
                bool end = false;
                Chunk *c = feed_.poll(end);
                if (!c) {
                    if (end) break;
                    const int busy = s.oldest_busy();
                    if (busy >= 0) {
                        s.finish_slot(busy);
                        continue;
                    }
                    const auto tq0 = Clock::now();
                    c = feed_.next();
                    t_fetch_us_ += us_since(tq0);
                    if (!c) break;
                }
                if (cfg_.fail_at >= 0 && (long)c->seq_no == cfg_.fail_at) throw Error("injected failure (MQ_DRIVER_FAIL_AT)");
                // the slot to use: a free one, else the one submitted longest ago
                int sl = s.free_slot();
                if (sl < 0) {
                    sl = s.oldest_busy();
                    s.finish_slot(sl);
                }
                if (!c->unparsed) {
                    c->hits.resize(c->starts.size());
                    if (c->starts.empty()) {  // nothing to map in this chunk (the middle of a very long record)
                        to_formatters(c);
                        continue;
                    }
                }
                s.submit(c, sl);
            }
            for (int q = s.oldest_busy(); q >= 0; q = s.oldest_busy()) s.finish_slot(q);
        } catch (const std::exception &e) { fail(e.what()); }
        {
            std::lock_guard<std::mutex> lk(mu_);
            submitters_left_--;
        }
        cv_.notify_all();
    }

    void format_loop() {
        PafWriter pw(index_);
        for (;;) {
            Chunk *c = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return !to_format_.empty() || submitters_left_ == 0; });
                if (to_format_.empty()) return;
                c = to_format_.front();
                to_format_.pop_front();
                formatting_++;
            }
            const auto tm0 = Clock::now();
            try {
                const std::string err = format_chunk(*c, pw, unm_ != nullptr, ufa_ != nullptr, cfg_.anchors != nullptr, cfg_.chains != nullptr);
                if (!err.empty()) fail(err);
            } catch (const std::exception &e) { fail(e.what()); }
            t_format_us_ += us_since(tm0);
            {
                std::lock_guard<std::mutex> lk(mu_);
                done_[c->seq_no] = c;
                formatting_--;
            }
            cv_.notify_all();
        }
    }

    // the calling thread: chunks in input order (main_thread_mer, src/closures.rs:117-123), until everything is written or somebody failed
    void write_in_order() {
        for (size_t next_out = 0;; ++next_out) {
            Chunk *c = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] {
                    return done_.count(next_out) != 0 || !werr_.empty() || (submitters_left_ == 0 && to_format_.empty() && formatting_ == 0);
                });
                auto it = done_.find(next_out);
                if (it == done_.end()) return;
                c = it->second;
                done_.erase(it);
            }
            const auto tw0 = Clock::now();
            if (cfg_.sort && !sort_chunk(*c)) return;
            if (!c->paf.empty()) fwrite(c->paf.data(), 1, c->paf.size(), paf_);
            if (unm_ && !c->unmapped.empty()) fwrite(c->unmapped.data(), 1, c->unmapped.size(), unm_);
            if (ufa_ && !c->unmapped_fa.empty()) fwrite(c->unmapped_fa.data(), 1, c->unmapped_fa.size(), ufa_);
            if (cfg_.anchors && !c->anchors.text.empty()) fwrite(c->anchors.text.data(), 1, c->anchors.text.size(), cfg_.anchors);
            if (cfg_.chains && !c->chains.text.empty()) fwrite(c->chains.text.data(), 1, c->chains.text.size(), cfg_.chains);
            feed_.recycle(c);
            t_write_us_ += us_since(tw0);
        }
    }

    // --sort: one mq_sort_add per chunk, first_ordinal = the number of the chunk's first read in input order (the hits are final: the chunk
    // is behind its wait), and the chunk's lines -- one per mapped read, in read order -- entered into the line table.  false: it failed.
    bool sort_chunk(const Chunk &c) {
        SortLines &S = *cfg_.sort;
        const uint64_t first = S.len.size();
        if (!c.hits.empty() && (first > 0xFFFFFFFFull || mq_sort_add(S.sorter, c.hits.data(), (uint32_t)c.hits.size(), (uint32_t)first) != MQ_OK)) {
            fail(first > 0xFFFFFFFFull ? std::string("--sort: more than 2^32 reads") : std::string("mq_sort_add: ") + last_error());
            return false;
        }
        size_t pos = 0;
        for (const mq_hit &h : c.hits) {
            size_t n = 0;
            if (h.status == MQ_HIT_MAPPED && pos < c.paf.size()) {
                const void *e = memchr(c.paf.data() + pos, '\n', c.paf.size() - pos);
                n = e ? (size_t)((const char *)e - (c.paf.data() + pos)) + 1 : 0;
            }
            S.at.push_back(S.paf_bytes + pos);
            S.len.push_back((uint32_t)n);
            pos += n;
        }
        S.paf_bytes += c.paf.size();
        return true;
    }

    feeder::Feeder &feed_;
    std::vector<std::vector<Ctx>> &slots_;
    const ReadOnlyIndex &index_;
    FILE *paf_, *unm_, *ufa_;
    const Config cfg_;

    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Chunk *> to_format_;     // mapped, waiting for a formatter
    std::map<size_t, Chunk *> done_;    // formatted, waiting for their turn in the output
    int submitters_left_;
    int formatting_ = 0;                // chunks a formatter is working on right now
    std::string werr_;                  // the first error
    std::atomic<long long> t_submit_us_{0}, t_finish_us_{0}, t_fetch_us_{0}, t_format_us_{0}, t_write_us_{0};
    std::atomic<unsigned long long> n_unparsed_{0}, n_irregular_{0};  // chunks submitted unparsed / handed back by the device for the host's parser
};

}  // namespace mapquik
