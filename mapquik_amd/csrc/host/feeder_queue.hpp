// feeder_queue.hpp -- the core of the read feeder (fastx_feeder.hpp): the pool of chunk buffers, the queue of parsed chunks the consumer
// takes from, the queue of filled chunks that wait for a parser thread, the error / abort state and the worker threads with their
// accounting.  Knows nothing about files: the readers (feeder_raw.hpp, feeder_gzip.hpp) work over it.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "fastx_records.hpp"

namespace mapquik {
namespace feeder {

class ChunkQueue {
  public:
    // alloc / release: where chunk buffers come from; unlock: releases the pages a mapped-view chunk had locked (Chunk::locked_at)
    ChunkQueue(int max_chunks, std::function<void *(size_t)> alloc, std::function<void(void *)> release, std::function<int(void *)> unlock)
        : max_chunks_(max_chunks), alloc_(alloc), release_(release), unlock_(unlock) {}
    ~ChunkQueue() { release_buffers(); }

    // capacity a new buffer of the pool gets at least (what a reader asks for beyond it is granted as asked)
    void set_buffer_floor(uint64_t cap) { floor_cap_ = cap; }

    // ------------------------------------------------------------ the consumer's side
    // the next parsed chunk (any order; seq_no says where it belongs), or nullptr: nothing ready (wait == false), the input exhausted or
    // the consumer aborted (`end` set in both cases).  Throws the first worker's error.
    Chunk *take(bool wait, bool &end) {
        std::unique_lock<std::mutex> lk(mu_);
        if (wait) cv_.wait(lk, [&] { return aborted_ || !ready_.empty() || finished_locked() || !error_.empty(); });
        end = aborted_;
        if (aborted_) return nullptr;
        if (!error_.empty()) throw FeederError(error_);
        if (ready_.empty()) {
            end = finished_locked();
            return nullptr;
        }
        Chunk *c = ready_.front();
        ready_.pop_front();
        return c;
    }
    // hand a chunk back for re-use
    void recycle(Chunk *c) {
        if (c->locked_len) {  // a view of the mapped file whose pages were locked for the copy to the device
            unlock_(c->locked_at);
            c->locked_at = nullptr;
            c->locked_len = 0;
        }
        c->clear();
        update([&] { free_.push_back(c); });
    }
    // the consumer gives up: take() returns nullptr from now on, workers waiting for a buffer leave
    void abort() { update([&] { aborted_ = stopping_ = true; }); }
    // n buffers of `need` bytes allocated now, by as many threads
    void preallocate(int n, uint64_t need) {
        std::vector<std::thread> th;
        std::vector<Chunk *> got((size_t)std::max(0, std::min(n, max_chunks_)), nullptr);
        for (size_t i = 0; i < got.size(); ++i)
            th.emplace_back([&, i] {
                try { got[i] = get_buffer(need, true); } catch (const std::exception &) {}
            });
        for (auto &t : th) t.join();
        for (Chunk *c : got)
            if (c) recycle(c);
    }
    // workers told to leave and joined
    void stop() {
        update([&] { stopping_ = true; });
        for (auto &t : threads_)
            if (t.joinable()) t.join();
        threads_.clear();
    }
    // The pool's page-locked buffers back to the system, by as many threads as there are buffers (un-pinning and unmapping 33 MB takes
    // ~3 ms and the driver has a dozen): for a consumer that is done with every chunk and wants its teardown short.
    void release_buffers() {
        stop();
        std::vector<std::thread> th;
        for (auto &c : all_) {
            void *b = c->own ? c->own : c->buf;
            c->own = c->buf = nullptr;
            if (b) th.emplace_back([this, b] { release_(b); });
        }
        for (auto &t : th) t.join();
        all_.clear();
        free_.clear();
        ready_.clear();
        to_parse_.clear();
    }
    size_t chunks_total() const { return produced_.load(); }

    // ------------------------------------------------------------ the workers' side
    // One worker thread around fn: whatever fn throws becomes the feeder's error (the first one wins), and the worker is counted out
    // either way.  feeds_parsers: this worker is the one that fills to_parse_; the parser threads leave once it is gone.
    template <class F>
    void run_worker(F fn, bool feeds_parsers = false) {
        threads_.emplace_back([this, fn, feeds_parsers] {
            std::string err;
            try { fn(); } catch (const std::exception &e) { err = e.what(); }
            update([&] {
                if (!err.empty() && error_.empty()) error_ = err;
                if (feeds_parsers) feed_done_ = true;
                done_workers_++;
            });
        });
    }
    // a free buffer of at least `need` bytes; waits for one unless the pool may grow (force: beyond its limit)
    Chunk *get_buffer(uint64_t need, bool force = false) {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            for (auto it = free_.begin(); it != free_.end(); ++it)
                if ((*it)->cap >= need) {
                    Chunk *c = *it;
                    free_.erase(it);
                    return c;
                }
            if (force || (int)all_.size() < max_chunks_ || free_.size() == all_.size()) {  // grow the pool (or replace a too-small buffer when nothing is in flight)
                lk.unlock();
                std::unique_ptr<Chunk> c(new Chunk());
                const uint64_t cap = std::max<uint64_t>(need, floor_cap_);
                c->buf = (uint8_t *)alloc_(cap);
                if (!c->buf) throw FeederError("cannot allocate a chunk buffer");
                c->own = c->buf;
                c->cap = cap;
                lk.lock();
                all_.push_back(std::move(c));
                return all_.back().get();
            }
            if (stopping_) throw FeederError("stopped");
            cv_.wait(lk);
        }
    }
    // chunk numbers for the readers that number their chunks by position in the file (claim_raw_chunk)
    size_t next_chunk_no() { return next_no_.fetch_add(1); }
    // a parsed chunk to the consumer
    void publish(Chunk *c) {
        update([&] {
            ready_.push_back(c);
            produced_++;
        });
    }
    // a filled chunk to the parser threads
    void queue_for_parse(Chunk *c) { update([&] { to_parse_.push_back(c); }); }
    // the next chunk to parse; nullptr once the worker that feeds the parsers is gone and the queue is empty (or the feeder stops)
    Chunk *take_for_parse() {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return !to_parse_.empty() || feed_done_ || stopping_; });
        if (to_parse_.empty()) return nullptr;
        Chunk *c = to_parse_.front();
        to_parse_.pop_front();
        return c;
    }

  private:
    // a change of the shared state, under the lock; everybody who waits looks again
    template <class F>
    void update(F change) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            change();
        }
        cv_.notify_all();
    }
    bool finished_locked() const { return done_workers_ == (int)threads_.size(); }

    int max_chunks_;
    std::function<void *(size_t)> alloc_;
    std::function<void(void *)> release_;
    std::function<int(void *)> unlock_;
    uint64_t floor_cap_ = 64;
    std::atomic<size_t> next_no_{0}, produced_{0};
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<std::unique_ptr<Chunk>> all_;
    std::deque<Chunk *> free_, ready_, to_parse_;
    std::vector<std::thread> threads_;
    int done_workers_ = 0;
    bool feed_done_ = false, stopping_ = false, aborted_ = false;
    std::string error_;
};

}  // namespace feeder
}  // namespace mapquik
