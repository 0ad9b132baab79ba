// mapquik (HIP backend) -- command-line driver with the reference's surface: src/main.rs:77-272 (flags, defaults, log
// lines) and src/closures.rs:22-212 (index the reference, map the reads, write <prefix>.paf in input order).
// The hot path runs on the GPU through mapquik_host.hpp / the C ABI.  Reads come through fastx_feeder.hpp (parallel chunk
// reader for raw files, one inflate thread + parser threads for .gz / .lz4), go to the GPU as raw FASTX bytes + spans
// (mq_ctx_submit_spans, three stream slots per GPU so that copy-in, kernels and copy-out of consecutive chunks overlap),
// and the PAF is formatted by a small thread pool and written in input order (map_pipeline.hpp).  The reference FASTA comes through the same
// feeder (its records go to mq_index_add_ref straight from the page-locked chunks).
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include "fastx_feeder.hpp"
#include "map_pipeline.hpp"
#include "mapquik_host.hpp"
#include "ref_loader.hpp"

using namespace mapquik;

// every environment variable the driver listens to, read once (the feeder's own: feeder::Knobs)
struct DriverKnobs {
    // diagnostic, stderr: where the wall time of a whole job goes -- seconds since main() started at every step of the reference phase,
    // the map phase and the teardown (on a 0.1-s map phase the fixed costs around it are most of the job) -- and where the map phase's
    // threads spend their time
    bool timing = set("MQ_DRIVER_TIMING");
    bool ref_host = set("MQ_DRIVER_REF_HOST");        // diagnostic: earlier rounds' path (reference records copied from pageable memory one by one)
    bool ref_preload = set("MQ_DRIVER_REF_PRELOAD");  // experiment: the reference read into host memory whole, before the first HIP call
    bool no_reserve = set("MQ_DRIVER_NO_RESERVE");    // the index's table is not allocated ahead of the first insert
    bool late_slots = set("MQ_DRIVER_LATE_SLOTS");    // diagnostic: no stream slot or chunk buffer is set up beside the reference phase
    bool prefetch = set("MQ_DRIVER_PREFETCH") && !set("MQ_DRIVER_NO_PREFETCH");  // the read feeder starts while the reference is still being indexed
    bool host_parse = set("MQ_DRIVER_HOST_PARSE");    // every chunk of reads is parsed by the reader threads
    bool fastq_device = getenv("MQ_DRIVER_FASTQ") && strcmp(getenv("MQ_DRIVER_FASTQ"), "device") == 0;  // FASTQ records found on the device
    long fail_at = set("MQ_DRIVER_FAIL_AT") ? atol(getenv("MQ_DRIVER_FAIL_AT")) : -1;  // test hook: the worker that takes this chunk number reports a failure
    bool fast_exit = set("MQ_DRIVER_FAST_EXIT");      // experiment: the last pass leaves without unwinding
    bool fake_multi = set("MQ_FAKE_MULTI");           // test hook: several workers on one device

    static bool set(const char *name) { return getenv(name) != nullptr; }
};
static const DriverKnobs g_knobs;

static const Clock::time_point g_t_main = Clock::now();
static void tl(const char *what) {
    if (g_knobs.timing) fprintf(stderr, "[+%.3f s] %s\n", secs(g_t_main), what);
}

// `{:?}` of a std::time::Duration
static std::string rust_duration(double seconds) {
    unsigned long long ns = (unsigned long long)(seconds * 1e9 + 0.5);
    const char *unit[4] = {"s", "ms", "\xC2\xB5s", "ns"};
    const unsigned long long div[4] = {1000000000ull, 1000000ull, 1000ull, 1ull};
    for (int u = 0; u < 4; ++u) {
        if (ns >= div[u] || u == 3) {
            unsigned long long whole = ns / div[u], frac = ns % div[u];
            char buf[64];
            if (frac == 0 || div[u] == 1) {
                snprintf(buf, sizeof(buf), "%llu%s", whole, unit[u]);
                return buf;
            }
            int digits = u == 0 ? 9 : u == 1 ? 6 : 3;
            char fr[16];
            snprintf(fr, sizeof(fr), "%0*llu", digits, frac);
            std::string f(fr);
            while (!f.empty() && f.back() == '0') f.pop_back();
            snprintf(buf, sizeof(buf), "%llu.%s%s", whole, f.c_str(), unit[u]);
            return buf;
        }
    }
    return "0ns";
}

// `{}` of an f64 for the values that occur here
static std::string rust_float(double x) {
    char buf[64];
    if (x == (double)(long long)x && std::abs(x) < 1e15) {
        snprintf(buf, sizeof(buf), "%lld", (long long)x);
        return buf;
    }
    for (int prec = 1; prec < 18; ++prec) {
        snprintf(buf, sizeof(buf), "%.*g", prec, x);
        if (strtod(buf, nullptr) == x) break;
    }
    return buf;
}

static bool contains(const std::string &s, const char *t) { return s.find(t) != std::string::npos; }
static bool ends_with(const std::string &s, const char *t) {
    const size_t n = strlen(t);
    return s.size() >= n && s.compare(s.size() - n, n, t) == 0;
}
// src/main.rs:196,202
static bool is_fasta_name(const std::string &n) {
    return contains(n, ".fasta.") || ends_with(n, ".fna") || contains(n, ".fna.") || contains(n, ".fa.") || ends_with(n, ".fa") ||
           ends_with(n, ".fasta");
}

struct Opt {
    std::string reads, reference, prefix;
    bool has_prefix = false, debug = false, low_memory = false, nosimd = false, nohpc = false, parallelfastx = false, unmapped = false, anchors = false, chains = false, coverage = false, depth = false, sort = false;
    long depth_window = 1000, depth_min_mapq = 60, sort_min_mapq = 0;
    long k = -1, l = -1, c = -1, s = -1, g = -1, threads = -1, b = -1, q = -1;
    double density = -1;
    int device = 0;
    int gpus = 1;
    int seeding_variant = 0;  // MQ_SEEDVAR_* bits (include/mapquik_hip.h)
    bool fast_kh = false;     // MQ_FLAG_FAST_KH
    bool ref_join_device = false;  // --ref-join device: a line-wrapped reference is streamed too, its lines joined on the device
    bool reads_join_device = false;  // --reads-join device: a line-wrapped reads FASTA goes to the device unparsed too, its records found and joined there
    bool last_pass = true;  // no second pass follows this one
    int table_factor = 2;  // table slots per inserted k-min-mer: this driver is bound by its host side (mq_index_set_table_factor)
    bool table_factor_given = false;  // --table-factor on the command line: only then is a loaded index's table given another size
    std::string add_reference;  // --add-reference (with --index): a FASTA whose records are added to the loaded index; `reference` holds it too, so it takes the routes of --reference
    std::vector<std::string> merge_index;  // --merge-index, repeatable: saved indexes merged, in this order, into the finalized index of this run (mq_index_merge_file)
    std::string save_index, load_index;  // --save-index / --index: the on-disk index (the reference has none and re-indexes on every run)
    std::string second;  // "k2,l2,d2"
    long k2 = 0, l2 = 0;
    double d2 = 0;
    unsigned long long batch_bases = 0;  // raw input bytes per chunk (page-locked buffers this size); 0 = 32 MB, and 64 MB for a reads file of 2 GB or
                                         // more read by at most four threads (28.5 -> 30.8 Gbases/s on the 4.6-GB FASTA of the bench on one box, no
                                         // change on another; with eight or more readers the rate does not move and the job's wall time grows by
                                         // 0.06-0.13 s: twice the page-locked memory to set up; tools/chunk_probe.py, profiles/NOTES.md)
};

static void usage() {
    puts("mapquik 0.1.0 (HIP backend)\nOriginal implementation of mapquik, a fast HiFi read mapper.\n\n"
         "USAGE:\n    mapquik [FLAGS] [OPTIONS] [reads]\n\nFLAGS:\n        --debug\n        --low-memory\n        --nohpc\n        --nosimd\n"
         "        --parallelfastx\n        --unmapped      (extension) also write <prefix>.unmapped.out\n        --anchors       (extension) also write <prefix>.anchors: the Match runs of every mapped read's winning chain\n        --chains        (extension) also write <prefix>.chains: every candidate chain of every read, ties included\n        --coverage      (extension) also write <prefix>.coverage.bed (the reference bases the index's live k-min-mers span) and <prefix>.coverage.tsv (per reference: live k-min-mers, covered bases), once the index is complete\n        --depth         (extension) also write <prefix>.depth.bed (per window of every reference: bases of the mapped reads that landed there, reads that start there, mean depth) and <prefix>.depth.tsv (per reference: reads, bases, mean depth, empty windows, the deepest window's mean)\n        --sort          (extension) also write <prefix>.sorted.paf (the lines of <prefix>.paf in the order of reference id, column 8, input order; sorted on the device) and <prefix>.sorted.tsv (per reference: lines, first line, byte offset of its first line in the sorted file)\n\nOPTIONS:\n"
         "    -b <b>\n    -c, --chain <chain>\n    -d, --density <density>\n    -g, --gap-diff <gap-diff>\n    -k <k>\n    -l <l>\n"
         "    -p, --prefix <prefix>\n    -q <q>\n        --reference <reference>\n    -s, --seed <seed>\n        --threads <threads>\n"
         "        --depth-window <n> (extension, with --depth) bases per window, 1 .. 2^24 (default 1000)\n        --depth-min-mapq <q> (extension, with --depth) count the reads with mapq >= q (default 60; 0: every mapped read)\n        --sort-min-mapq <q> (extension, with --sort) keep the lines with mapq >= q (default 0: every PAF line)\n        --device <n>    (extension) first HIP device ordinal\n        --gpus <n>      (extension) shard read batches over n GPUs, index replicated\n        --batch-bases <n> (extension) raw input bytes per chunk\n        --table-factor <n> (extension) index table slots per k-min-mer (default 2 here: a file-fed run is host-bound; the library's default for HBM-resident batches is 8)\n        --ref-join <device|host> (extension) where the lines of a line-wrapped reference FASTA are joined: host (default: such a file is read into host memory) or device (streamed like a single-line file, never in host memory)\n        --reads-join <device|host> (extension) where the lines of a line-wrapped reads FASTA are joined: host (default: such a chunk is parsed and compacted by a host thread) or device (the chunk goes to the GPU as it lies in the file; headers found and lines joined there)\n        --save-index <file> (extension) write the finalized index (occupied slots only) for later runs\n        --index <file>  (extension) map against a saved index instead of indexing --reference (same -k -l -d --nohpc as it was built with); with --table-factor its table gets that size on load\n        --add-reference <fasta> (extension, with --index) add the file's records to the loaded index (ids continue behind its largest), then map; --save-index writes the extended index\n        --merge-index <file> (extension, repeatable) merge this saved index (same seeding parameters) into the one --index / --reference / --add-reference produced, ids continuing behind its largest, in command-line order; --save-index writes the merged index\n        --seeding-variant <v> (extension) reading of the k-min-mer iterator's unpinned decisions, bits 1 2 4 8 16 32 (include/mapquik_hip.h); 0 = frozen\n        --fast-kh       (extension) cheap k-min-mer tuple hash instead of SipHash-1-3: same PAF (the hash acts through equality only), fewer instructions\n        --second-pass <k2,l2,d2> (extension) map the unmapped reads again with these parameters: <prefix>-k2-l2-d2.{fa,paf,unmapped.out}\n\nARGS:\n    <reads>");
}

// the last two lines of a run (src/main.rs:270-271)
static void print_totals(Clock::time_point start) {
    printf("Total execution time: %s\n", rust_duration(secs(start)).c_str());  // src/main.rs:270
    struct rusage ru;
    getrusage(RUSAGE_SELF, &ru);
    const float gb = (float)((double)ru.ru_maxrss * 1024.0) / 1024.0f / 1024.0f / 1024.0f;
    char fb[64];
    for (int prec = 1; prec < 12; ++prec) {
        snprintf(fb, sizeof(fb), "%.*g", prec, (double)gb);
        if ((float)strtod(fb, nullptr) == gb) break;
    }
    printf("Maximum RSS: %sGB\n", strchr(fb, '.') || strchr(fb, 'e') ? fb : (std::string(fb) + ".0").c_str());  // src/main.rs:271
}

// ---------------------------------------------------------------- the reference phase: one function per route (build_or_load_index decides which)
// what the routes share
struct RefPhase {
    const Opt &o;
    const Params &P;
    std::unique_ptr<Index> &index;  // the index being built (build_or_load_index replaces it when the streamer gives a file back late)
    int n_parse;                    // host threads
    const std::function<void()> &start_feed;  // starts the read feeder (once)
    bool prefetch;                  // MQ_DRIVER_PREFETCH: the read feeder starts while the reference is still being indexed
    size_t &first_id;               // id of the file's first record (0; --add-reference: behind the loaded index's largest id)
};

// --index: the finalized table from a file written by --save-index (occupied slots only; validated against its header on load)
static std::unique_ptr<ReadOnlyIndex> load_index_file(const Opt &o, const Params &P, int device, bool announce = true) {
    std::unique_ptr<ReadOnlyIndex> loaded(new ReadOnlyIndex(ReadOnlyIndex::load(o.load_index, device, 0, o.table_factor_given ? (uint32_t)o.table_factor : 0u)));
    mq_params fp;
    if (mq_index_get_params(loaded->handle(), &fp) != MQ_OK) throw Error("mq_index_get_params: " + last_error());
    const mq_params want = P.to_abi();
    if (fp.k != want.k || fp.l != want.l || fp.density != want.density || fp.use_hpc != want.use_hpc ||
        (fp.flags & (MQ_FLAG_SEED_VARIANT_MASK | MQ_FLAG_FAST_KH)) != (want.flags & (MQ_FLAG_SEED_VARIANT_MASK | MQ_FLAG_FAST_KH))) {
        char msg[640];
        snprintf(msg, sizeof(msg), "%s was built with -k %u -l %u -d %s%s --seeding-variant %u%s: run with the same seeding parameters (this run: -k %u -l %u -d %s%s --seeding-variant %u%s)",
                 o.load_index.c_str(), fp.k, fp.l, rust_float(fp.density).c_str(), fp.use_hpc ? "" : " --nohpc", (fp.flags & MQ_FLAG_SEED_VARIANT_MASK) >> MQ_FLAG_SEED_VARIANT_SHIFT,
                 (fp.flags & MQ_FLAG_FAST_KH) ? " --fast-kh" : "",
                 want.k, want.l, rust_float(want.density).c_str(), want.use_hpc ? "" : " --nohpc", (want.flags & MQ_FLAG_SEED_VARIANT_MASK) >> MQ_FLAG_SEED_VARIANT_SHIFT,
                 (want.flags & MQ_FLAG_FAST_KH) ? " --fast-kh" : "");
        throw Error(msg);
    }
    // the chaining thresholds and the case folding are this run's (they act at mapping time only)
    if (mq_index_set_map_params(loaded->handle(), want.c, want.s, want.g, (want.flags & MQ_FLAG_FOLD_CASE) ? 1 : 0) != MQ_OK) throw Error("mq_index_set_map_params: " + last_error());
    mq_index_stats st;
    mq_index_get_stats(loaded->handle(), &st);
    if (announce) printf("Loaded index %s: %llu references, %llu k-min-mers.\n", o.load_index.c_str(), (unsigned long long)st.n_refs, (unsigned long long)st.n_kminmers);
    tl("index file loaded");
    return loaded;
}

// an uncompressed FASTA of one sequence line per record (what assemblers and this repository's tools write): streamed to the
// device block by block as it is read, records indexed while the blocks behind them are still on the link (RefStreamer);
// the host reads the header lines only.  Any other shape (Result::irregular): nothing is printed, the caller sends the file elsewhere.
static feeder::RefStreamer::Result stream_reference(const RefPhase &rp) {
    feeder::RefStreamer::Hooks hooks;
    hooks.alloc = [](size_t n) { return mq_host_alloc(n); };
    hooks.release = [](void *q) { mq_host_free(q); };
    mq_index *h = rp.index->handle();
    hooks.piece = [h](uint64_t at, const uint8_t *src, uint64_t n) {
        uint64_t t = 0;
        if (mq_index_stage_piece(h, at, src, n, &t) != MQ_OK) throw Error("mq_index_stage_piece: " + last_error());
        return t;
    };
    hooks.done = [h](uint64_t t, bool wait) {
        const int r = mq_index_stage_done(h, t, wait ? 1 : 0);
        if (r < 0) throw Error("mq_index_stage_done: " + last_error());
        return r == 1;
    };
    const bool join_dev = rp.o.ref_join_device;  // a record = its header line + everything up to the next '>' at a line start
    feeder::RefStreamer rs(rp.o.reference, rp.n_parse, hooks, join_dev);
    std::vector<std::string> lines;  // printed once the file's shape is known to be regular (else the loader below prints its own)
    const feeder::RefStreamer::Result res = rs.run([&](size_t k, const std::string &id, uint64_t at, uint64_t len) {
        const auto tr0 = Clock::now();
        const uint32_t rid = (uint32_t)(rp.first_id + k);
        const int64_t cnt = join_dev ? mq_index_add_ref_staged_lines(h, rid, id.c_str(), at, len, MQ_STAGE_ALL_ISSUED, nullptr)
                                     : mq_index_add_ref_staged(h, rid, id.c_str(), at, len, MQ_STAGE_ALL_ISSUED);  // index_mers, src/closures.rs:46-51
        if (cnt < 0) throw Error("ref_extract: " + last_error());
        if (g_knobs.timing && join_dev) fprintf(stderr, "[+%.3f s] reference record %zu: %llu bytes handed over, ref_extract returned after %.3f ms\n", secs(g_t_main), k, (unsigned long long)len, secs(tr0) * 1e3);
        lines.push_back("Indexed reference " + id + ": " + std::to_string(cnt) + " k-min-mers.");  // src/closures.rs:58
    });
    if (!res.irregular) {
        for (const std::string &ln : lines) puts(ln.c_str());
        tl(join_dev ? "reference streamed: every record handed to ref_extract (lines joined on the device)" : "reference streamed: every record handed to ref_extract");
    }
    return res;
}

// an uncompressed FASTA: the whole file read once by all threads (since before the HIP runtime came up), multi-line records
// compacted in place by a pool, records handed over whole and in order (ref_loader.hpp).  The buffer is page-locked in one
// call (huge pages: milliseconds), every record's bytes are queued for the device the moment the record is ready
// (mq_index_stage_piece: the link runs at its full rate, 3.1 GB in 0.06 s) and a second thread indexes record after record
// behind its piece (mq_index_add_ref_staged) -- copied record by record from pageable memory this was 0.24 s.
// ref_host (MQ_DRIVER_REF_HOST): records copied from pageable memory one by one, as in earlier rounds.  stage_begin: the index is a new
// one (the streamer's went away with its staging buffer) and gets a staging buffer here.
static void load_reference_whole(const RefPhase &rp, feeder::RefLoader &rl, bool ref_host, bool stage_begin) {
    rl.wait_read();
    tl("reference file in host memory");
    mq_index *h = rp.index->handle();
    struct stat rst;
    bool staged = !ref_host && stat(rp.o.reference.c_str(), &rst) == 0 && (uint64_t)rst.st_size == rl.file_bytes();
    if (staged && stage_begin) {
        if (mq_index_stage_begin(h, rl.file_bytes()) != MQ_OK) staged = false;
    }
    bool locked = false;
    if (staged) {
        locked = mq_host_register(rl.data(), (size_t)rl.mapped_bytes()) == MQ_OK;  // (not locked: the copies still work, at the pageable rate)
        tl(locked ? "reference buffer page-locked" : "reference buffer could not be page-locked: pageable copies");
    }
    struct Job {
        size_t idx;
        std::string id;
        uint64_t at, len, ticket;
    };
    std::mutex jmu;
    std::condition_variable jcv;
    std::deque<Job> jobs;
    bool jobs_done = false;
    std::string jerr;
    std::vector<std::string> lines;
    std::thread indexer;
    if (staged)
        indexer = std::thread([&]() {
            for (;;) {
                Job j;
                {
                    std::unique_lock<std::mutex> lk(jmu);
                    jcv.wait(lk, [&] { return !jobs.empty() || jobs_done; });
                    if (jobs.empty()) return;
                    j = std::move(jobs.front());
                    jobs.pop_front();
                }
                const int64_t cnt = mq_index_add_ref_staged(h, (uint32_t)j.idx, j.id.c_str(), j.at, j.len, j.ticket);  // index_mers, src/closures.rs:46-51
                if (cnt < 0) {
                    std::lock_guard<std::mutex> lk(jmu);
                    if (jerr.empty()) jerr = "ref_extract: " + last_error();
                    return;
                }
                printf("Indexed reference %s: %lld k-min-mers.\n", j.id.c_str(), (long long)cnt);  // src/closures.rs:58
            }
        });
    size_t ref_idx = rp.first_id;
    std::string ferr;
    uint64_t last_ticket = 0;
    bool any_ticket = false;
    try {
        rl.for_each([&](const feeder::RefLoader::Record &r, const uint8_t *seq) {
            if (ref_idx == rp.first_id) tl("first reference record ready");
            if (rp.prefetch) rp.start_feed();  // the whole file has been read by now: the host threads are free
            if (staged) {
                uint64_t t = 0;
                if (mq_index_stage_piece(h, r.seq, seq, r.len, &t) != MQ_OK) throw Error("mq_index_stage_piece: " + last_error());
                last_ticket = t;
                any_ticket = true;
                {
                    std::lock_guard<std::mutex> lk(jmu);
                    if (!jerr.empty()) throw Error(jerr);
                    jobs.push_back(Job{ref_idx, r.id, r.seq, r.len, t});
                }
                jcv.notify_all();
            } else {
                const size_t cnt = mers::ref_extract(ref_idx, r.id, seq, r.len, rp.P, *rp.index);
                printf("Indexed reference %s: %zu k-min-mers.\n", r.id.c_str(), cnt);  // src/closures.rs:58
            }
            ++ref_idx;
        });
    } catch (const std::exception &e) { ferr = e.what(); }
    {
        std::lock_guard<std::mutex> lk(jmu);
        jobs_done = true;
        if (!ferr.empty()) jobs.clear();
    }
    jcv.notify_all();
    if (indexer.joinable()) indexer.join();
    // the copies read the buffer until the last piece is done (a record too short to be seeded is "indexed" without waiting for its piece)
    if (any_ticket) mq_index_stage_done(h, last_ticket, 1);
    if (locked) mq_host_unregister(rl.data());
    if (!ferr.empty()) throw Error(ferr);
    if (!jerr.empty()) throw Error(jerr);
    tl("every reference record indexed");
    // (the buffer goes back to the system at the end of the run, beside the rest of the teardown: handing 3 GB back takes 0.14 s
    // here and stalls whoever maps or allocates memory meanwhile -- index finalisation, stream-slot set-up)
}

// compressed (or FASTQ) reference: through the chunked feeder, pageable chunk buffers (every reference byte is copied to
// the device exactly once)
static void feed_reference_chunked(const RefPhase &rp, bool ref_fasta) {
    using feeder::Chunk;
    if (rp.prefetch) rp.start_feed();
    feeder::Feeder rfeed(rp.o.reference, !ref_fasta, 1ull << 28, rp.n_parse, rp.n_parse + 4, [](size_t n) { return malloc(n); },
                         [](void *q) { free(q); }, [](void *, size_t) { return 0; }, [](void *) { return 0; });
    rfeed.start();
    std::map<size_t, Chunk *> held;
    size_t next = 0, ref_idx = rp.first_id;
    std::string name;
    auto flush = [&]() {
        for (auto it = held.find(next); it != held.end(); it = held.find(next)) {
            Chunk *c = it->second;
            for (size_t i = 0; i < c->starts.size(); ++i) {
                name.assign((const char *)c->buf + c->ids[i].off, c->ids[i].len);
                const size_t cnt = mers::ref_extract(ref_idx, name, c->buf + c->starts[i], c->lens[i], rp.P, *rp.index);
                printf("Indexed reference %s: %zu k-min-mers.\n", name.c_str(), cnt);  // src/closures.rs:58
                ++ref_idx;
            }
            held.erase(it);
            rfeed.recycle(c);
            ++next;
        }
    };
    while (Chunk *c = rfeed.next()) {
        held[c->seq_no] = c;
        flush();
    }
    flush();
}

// ---------------------------------------------------------------- one pass: what run_pass is made of, in the order it runs

// A thread that is joined when it goes out of scope: an exception on the way finds it joined before what it works on goes away.
struct JoiningThread {
    std::thread t;
    JoiningThread() = default;
    explicit JoiningThread(std::function<void()> f) : t(std::move(f)) {}
    JoiningThread(JoiningThread &&) = default;
    JoiningThread &operator=(JoiningThread &&) = default;
    ~JoiningThread() { join(); }
    void join() {
        if (t.joinable()) t.join();
    }
};

// every task on a thread of its own, all joined, then the first error (in task order) rethrown
static void run_all(const std::vector<std::function<void()>> &tasks) {
    std::vector<std::exception_ptr> errs(tasks.size());
    std::vector<std::thread> th;
    for (size_t i = 0; i < tasks.size(); ++i)
        th.emplace_back([&, i]() {
            try {
                tasks[i]();
            } catch (...) { errs[i] = std::current_exception(); }
        });
    for (auto &t : th) t.join();
    for (auto &e : errs)
        if (e) std::rethrow_exception(e);
}

// The files of one pass: <prefix>.paf, created first (src/closures.rs:32; it stays behind, empty, when the reference phase fails),
// <prefix>.unmapped.out, and the unmapped reads as FASTA for a second pass (seqtk subseq in the reference's script).  The one place
// that closes them.
struct OutputFiles {
    const std::string paf_path;
    FILE *paf, *unm = nullptr, *ufa = nullptr, *anc = nullptr, *chn = nullptr;
    OutputFiles(const std::string &prefix, bool unmapped, const std::string &second_fa, bool anchors = false, bool chains = false) : paf_path(prefix + ".paf"), paf(fopen(paf_path.c_str(), "w")) {
        if (!paf) return;
        if (anchors) anc = fopen((prefix + ".anchors").c_str(), "w");
        if (chains) chn = fopen((prefix + ".chains").c_str(), "w");
        if (unmapped) unm = fopen((prefix + ".unmapped.out").c_str(), "w");
        if (!second_fa.empty()) ufa = fopen(second_fa.c_str(), "w");
    }
    OutputFiles(const OutputFiles &) = delete;
    ~OutputFiles() { close(); }
    void close() {
        for (FILE **f : {&paf, &unm, &ufa, &anc, &chn}) {
            if (*f) fclose(*f);
            *f = nullptr;
        }
    }
    // the map phase failed: never leave a partial PAF behind a failure
    void discard_paf() {
        close();
        remove(paf_path.c_str());
    }
};

// --gpus N: the index is replicated (every GPU indexes the same reference), read batches are dealt round-robin,
// PAF lines are written in batch order = input order.  No collective: reads are independent.
struct Devices {
    int first, visible;
    bool fake;  // MQ_FAKE_MULTI (test hook): several workers on one device
    bool enough_for(int gpus) const { return fake || first + gpus <= visible || visible <= 0; }
    int of(int g) const { return fake && visible > 0 ? (first + g) % visible : first + g; }
};

static const int N_SLOTS = 3;  // stream slots per submitting thread: copy-in, kernels and copy-out of consecutive chunks overlap

// How the reference and the reads of this pass travel: decided from the arguments, the file names and the environment alone.
struct Routes {
    int n_parse;   // host threads
    int n_format;  // PAF formatters (the reader threads of a mapped FASTA file have next to nothing to do)
    unsigned long long batch_bases;
    // An uncompressed reference FASTA goes to the device through a small pool of page-locked blocks as it is read (RefStreamer);
    // a file that is not one sequence line per record is read into host memory whole, its records joined there (RefLoader).
    // MQ_DRIVER_REF_PRELOAD=1 (experiment): the whole-file read starts before the first HIP call -- bringing the HIP runtime up
    // takes 0.15-0.3 s of one thread, reading 3.1 GB 0.08-0.1 s of the others -- and the records go to the device from that buffer,
    // page-locked in one call.  Measured slower than streaming on the bench's job (profiles/r05_driver_medians.txt): 3 GB of host
    // memory cost 0.14 s to hand back on this platform (pages are cleared when freed: tools/thp_probe.c, 45 ms per GB), whoever does it.
    bool ref_fasta, ref_plain, ref_preload;
    bool preload_now;  // a RefLoader starts reading the reference before the first HIP call
    bool stream_ref;   // RefStreamer
    // An uncompressed FASTA file goes to the GPU as it lies in the file: the reader threads only copy file bytes into page-locked
    // chunks (pread, cut at record starts), the records are found on the device (mq_ctx_submit_fasta) and the host reads a header
    // only to print it.  MQ_DRIVER_HOST_PARSE=1: every chunk is parsed by the reader threads as in earlier rounds (same PAF; tests compare).
    // FASTQ: the lean reader by default -- header and sequence lines only, one pread per record, qualities never read: 1 byte per base
    // from the file and on the link: 12 / 20 / 31 / 35 Gbases/s at 2 / 4 / 8 / 16 reader threads against 9 / 17 / 22 / 21 with the
    // records found on the device, where the whole file (2 bytes per base) is read and crosses the link
    // (profiles/r05_fastq_readers.txt).  MQ_DRIVER_FASTQ=device selects that path (mq_ctx_submit_fastx).
    bool on_device;
    // --reads-join device: FASTA chunks as MQ_FASTX_FASTA_LINES -- sequences over several lines (60, 70, 80 columns) are joined on the
    // device instead of coming back irregular for a host thread to compact
    uint32_t fx_format;
};

static Routes describe_routes(const Opt &o, const std::string &reads_path, bool reads_fasta, bool ref_fasta, size_t threads) {
    Routes rt;
    rt.n_parse = (int)std::max<size_t>(1, threads);
    rt.n_format = std::max(2, std::min(8, rt.n_parse));
    rt.batch_bases = o.batch_bases;
    if (rt.batch_bases == 0) {
        struct stat sb;
        rt.batch_bases = (rt.n_parse <= 4 && stat(reads_path.c_str(), &sb) == 0 && (unsigned long long)sb.st_size >= (2ull << 30)) ? (1ull << 26) : (1ull << 25);
    }
    rt.ref_fasta = ref_fasta;
    rt.ref_plain = ref_fasta && !ends_with(o.reference, ".gz") && !ends_with(o.reference, ".lz4");
    rt.ref_preload = g_knobs.ref_preload && !o.low_memory;
    const bool indexes = o.load_index.empty() || !o.add_reference.empty();  // reference records are indexed in this run
    rt.preload_now = rt.ref_plain && indexes && (rt.ref_preload || g_knobs.ref_host);
    rt.stream_ref = rt.ref_plain && indexes && !rt.ref_preload && !g_knobs.ref_host;
    rt.on_device = !g_knobs.host_parse && (reads_fasta || g_knobs.fastq_device);
    rt.fx_format = !reads_fasta ? MQ_FASTX_FASTQ : o.reads_join_device ? MQ_FASTX_FASTA_LINES : MQ_FASTX_FASTA;
    return rt;
}

// The stream slots of the map phase, [submitting thread][slot] (device staging, minimizer lists, Match scratch: a few hundred MB of
// device memory per submitting thread).  run_pass declares them after the indexes, so that on every path they go first.
struct StreamSlots {
    std::vector<std::vector<Ctx>> of;
    const uint64_t chunk_bytes;  // what a slot has room for from the start
    const bool anchors;          // --anchors: every slot reserves spans and an anchor pool for chunk_bytes (Ctx::reserve_anchors states the bound)
    const double density;
    const bool chains;           // --chains: the same for spans and a chain pool (Ctx::reserve_chains)
    StreamSlots(size_t n_submitters, uint64_t batch_bases, uint64_t bytes_in, bool anchors_ = false, double density_ = 0, bool chains_ = false)
        : of(n_submitters), chunk_bytes(std::min<uint64_t>(batch_bases + batch_bases / 8 + (1u << 20), bytes_in + 64)), anchors(anchors_), density(density_), chains(chains_) {
        for (auto &v : of) v.reserve((size_t)N_SLOTS);
    }
    bool complete(size_t w) const { return of[w].size() == (size_t)N_SLOTS; }
    // the slots submitter w still lacks, over index h
    void fill(size_t w, mq_index *h) {
        while (!complete(w)) {
            of[w].emplace_back(h);
            of[w].back().reserve((uint32_t)std::min<uint64_t>(chunk_bytes / 16000 + 512, 1u << 24), chunk_bytes);  // (sized for long reads; a chunk of short reads makes its slot grow once)
            if (anchors) of[w].back().reserve_anchors(chunk_bytes, density);
            if (chains) of[w].back().reserve_chains(chunk_bytes, density);
        }
    }
    void drop() {
        for (auto &v : of) v.clear();
    }
};

// The stream slots and the feeder's first page-locked chunk buffers depend on neither the reference nor the reads: the first GPU's
// are set up by a thread of its own BESIDE the reference phase (0.03-0.04 s of a 0.1-s phase when they came after it).
class EarlySetup {
  public:
    // n_buffers: chunk buffers to preallocate, 0 for none (MQ_DRIVER_PREFETCH: the feeder, started early, allocates its own)
    EarlySetup(StreamSlots &slots, feeder::Feeder &feed, int n_sub, int n_buffers) : slots_(slots), feed_(feed), n_sub_(n_sub), n_buffers_(n_buffers) {}
    void start(mq_index *h) {
        if (g_knobs.late_slots) return;  // (diagnostic: everything after the reference phase, as in earlier rounds)
        thread_ = JoiningThread([this, h]() {
            try {
                for (int w = 0; w < n_sub_; ++w) slots_.fill((size_t)w, h);
                if (n_buffers_ > 0) {
                    feed_.preallocate(n_buffers_);
                    pool_ready_ = true;
                }
            } catch (const std::exception &e) { err_ = e.what(); }
        });
    }
    void join() { thread_.join(); }
    // after join():
    const std::string &error() const { return err_; }
    bool pool_ready() const { return pool_ready_; }

  private:
    StreamSlots &slots_;
    feeder::Feeder &feed_;
    const int n_sub_, n_buffers_;
    std::string err_;
    bool pool_ready_ = false;
    JoiningThread thread_;  // (last: joined before the rest goes away)
};

static std::unique_ptr<Index> new_index(const Opt &o, const Params &P, int device) {
    std::unique_ptr<Index> index(new Index(P, device));
    index->table_factor((uint32_t)o.table_factor);
    return index;
}

// --add-reference: the loaded index opened again (mq_index_reopen); the table grows, if it has to, by this run's factor.  *first_id: the
// smallest id behind every id the file has (a file of this driver's has 0 .. n_refs - 1; any other is searched id by id).
static std::unique_ptr<Index> reopen_index_file(const Opt &o, const Params &P, int device, size_t *first_id, bool announce) {
    std::unique_ptr<ReadOnlyIndex> loaded = load_index_file(o, P, device, announce);
    mq_index_stats st;
    mq_index_get_stats(loaded->handle(), &st);
    size_t next = 0;
    for (uint64_t seen = 0; seen < st.n_refs; ++next)
        if (mq_index_ref_info(loaded->handle(), (uint32_t)next, nullptr, nullptr) == MQ_OK) ++seen;
    *first_id = next;
    std::unique_ptr<Index> index(new Index(std::move(*loaded).reopen(P)));
    index->table_factor((uint32_t)o.table_factor);
    return index;
}

static void reserve_table(const Opt &o, const Params &P, bool ref_plain, Index &index) {
    if (!ref_plain || g_knobs.no_reserve || !o.add_reference.empty()) return;  // (a reopened index keeps its table)
    // Index::new sizes its map before the first insert (src/index.rs:83: with_capacity(39,821,990), CHM13 at the defaults); here the
    // expected count follows from the reference's size: canonical selection keeps 1 - (1 - d)^2 of the l-mers, homopolymer
    // compression about three quarters of the bases.  The table is allocated in the background while the reference is read and seeded.
    struct stat rst;
    if (stat(o.reference.c_str(), &rst) == 0 && rst.st_size > 0) {
        const double d = std::min(1.0, std::max(0.0, P.density));
        index.with_capacity((uint64_t)((double)rst.st_size * (1.0 - (1.0 - d) * (1.0 - d)) * (P.use_hpc ? 0.75 : 1.0)) + 1);
    }
}

// --index: the table from a file, into `loaded`.  Else index_mers (src/closures.rs:46-51) per reference record, in file order, on the
// first GPU, into rp.index, by the route the file takes; the kernels fold soft-masked lower case.  Device allocations queue behind
// each other, hence this order: the reference's staging buffer, the table (in the background), the stream slots (EarlySetup).
static void build_or_load_index(const RefPhase &rp, const Routes &rt, int device, std::unique_ptr<feeder::RefLoader> &preload,
                                std::unique_ptr<ReadOnlyIndex> &loaded, StreamSlots &slots, EarlySetup &early) {
    const Opt &o = rp.o;
    if (!o.load_index.empty() && o.add_reference.empty()) {
        loaded = load_index_file(o, rp.P, device);
        return;
    }
    // --add-reference: the loaded index, reopened, takes the place of a new one; the file's records follow by the route of --reference.
    // (again: the rare file the streamer gives back after records were indexed -- those cannot be taken out of a table, so the index
    // file is read once more, without its log line)
    auto open_index = [&](bool again) { return o.add_reference.empty() ? new_index(o, rp.P, device) : reopen_index_file(o, rp.P, device, &rp.first_id, !again); };
    rp.index = open_index(false);
    tl("Index::new returned (HIP runtime up, device chosen)");
    if (rt.stream_ref || (preload && !g_knobs.ref_host)) {
        // the device's staging buffer of the reference FIRST: device allocations queue behind each other, and this one (the file's
        // size) must not wait behind the table's, which is larger and not needed before the last record is indexed
        struct stat rst;
        if (stat(o.reference.c_str(), &rst) != 0) throw Error("Error opening compressed file: " + o.reference);  // get_reader's message (src/main.rs:62)
        if (mq_index_stage_begin(rp.index->handle(), (uint64_t)rst.st_size) != MQ_OK) throw Error("mq_index_stage_begin: " + last_error());
        tl("staging buffer for the reference allocated");
    }
    reserve_table(o, rp.P, rt.ref_plain, *rp.index);
    early.start(rp.index->handle());
    feeder::RefStreamer::Result streamed;  // the streamer's, where it ran
    bool index_replaced = false;           // ... and gave the file back after records had been indexed: that index was replaced by a new one
    if (rt.stream_ref) {
        streamed = stream_reference(rp);
        if (streamed.irregular) {
            // not one sequence line per record (a line-wrapped FASTA shows in its first block, before anything was indexed): an index
            // that took records already is dropped, and the file goes through the loader below
            if (streamed.handed > 0) {  // (an index that has seen nothing stays: its table is being allocated in the background already)
                early.join();  // the slots set up so far belong to the index that goes away
                slots.drop();
                rp.index.reset();
                rp.index = open_index(true);
                index_replaced = true;
                reserve_table(o, rp.P, rt.ref_plain, *rp.index);
            }
            tl("reference is not one line per record: host loader");
        }
    }
    if (!rt.stream_ref || streamed.irregular) {
        if (rt.ref_plain && !(o.low_memory && rt.stream_ref)) {  // (--low-memory: a file the streamer gave back goes through the chunked reader, record by record)
            if (!preload) preload.reset(new feeder::RefLoader(o.reference, rt.n_parse, false));  // (the streamer above sent the file here)
            load_reference_whole(rp, *preload, g_knobs.ref_host, index_replaced);
        } else {
            feed_reference_chunked(rp, rt.ref_fasta);
        }
    }
}

// The index built on the first GPU is finalized, saved where --save-index asks for it, and the finalized table is copied device to
// device to the other GPUs (mq_index_clone).
// --coverage: <prefix>.coverage.bed and <prefix>.coverage.tsv of the finished index (ReadOnlyIndex::coverage), and one log line
static void write_coverage(const std::string &prefix, ReadOnlyIndex &index) {
    const ReadOnlyIndex::Coverage c = index.coverage();
    const std::pair<std::string, std::string> files[2] = {{prefix + ".coverage.bed", c.bed()}, {prefix + ".coverage.tsv", c.tsv()}};
    for (const auto &f : files) {
        FILE *fp = fopen(f.first.c_str(), "w");
        const bool ok = fp && fwrite(f.second.data(), 1, f.second.size(), fp) == f.second.size();
        if ((fp && fclose(fp) != 0) || !ok) throw Error("Couldn't write " + f.first);
    }
    printf("Coverage: %llu of %llu bases in %llu intervals (%llu entries out of range)\n", (unsigned long long)c.covered(), (unsigned long long)c.total(),
           (unsigned long long)c.n_intervals, (unsigned long long)c.out_of_range);
    mq_index_coverage_release(index.handle());
}

static void finalise_save_clone(const Opt &o, const Devices &dev, std::unique_ptr<Index> &building, std::vector<std::unique_ptr<ReadOnlyIndex>> &ro, const std::string &prefix,
                                OutputFiles &out) {
    if (building) {
        ro[0].reset(new ReadOnlyIndex(std::move(*building).into_read_only()));
        tl("into_read_only returned (table allocated, k-min-mers inserted)");
        building.reset();
    }
    // --merge-index: before the index is saved and before the replicas are made
    for (const std::string &path : o.merge_index) {
        const ReadOnlyIndex::Merged m = ro[0]->merge_file(path);
        printf("Merged index %s: %llu references, %llu k-min-mers.\n", path.c_str(), (unsigned long long)m.refs, (unsigned long long)m.kminmers);
        tl("index file merged");
    }
    if (!o.save_index.empty()) {
        const auto ts = Clock::now();
        ro[0]->save(o.save_index);
        printf("Saved index to %s in %s.\n", o.save_index.c_str(), rust_duration(secs(ts)).c_str());
    }
    // --coverage: the index phase is complete; once, on the primary index, before the replicas are made
    if (o.coverage) {
        try {
            write_coverage(prefix, *ro[0]);
        } catch (...) {
            out.discard_paf();  // (a failure here ends the run like one of the map phase: no PAF)
            throw;
        }
        tl("coverage written");
    }
    std::vector<std::function<void()>> clones;
    for (int g = 1; g < o.gpus; ++g) clones.push_back([&, g]() { ro[g].reset(new ReadOnlyIndex(ro[0]->clone_to(dev.of(g)))); });
    run_all(clones);
}

// The stream slots of the other GPUs (the first GPU's were set up beside the reference phase), whatever of the first GPU's is still
// missing, and the first page-locked chunk buffers (n_buffers of them; 0: the feeder allocates its own).
static void finish_slots_and_pool(EarlySetup &early, StreamSlots &slots, const std::vector<std::unique_ptr<ReadOnlyIndex>> &ro, feeder::Feeder &feed, int n_buffers) {
    early.join();
    if (!early.error().empty()) throw Error(early.error());
    const size_t n_sub = slots.of.size() / ro.size();
    std::vector<std::function<void()>> tasks;
    for (size_t w = 0; w < slots.of.size(); ++w)
        if (!slots.complete(w)) tasks.push_back([&, w]() { slots.fill(w, ro[w / n_sub]->handle()); });
    if (n_buffers > 0 && !early.pool_ready()) tasks.push_back([&]() { feed.preallocate(n_buffers); });
    run_all(tasks);
}

// teardown, side by side: the stream slots and then the indexes (contexts go before their index) on one thread, the feeder's
// page-locked pool on this one -- 0.08 s one after the other on a 0.6-s job
static void teardown(const Opt &o, StreamSlots &slots, std::vector<std::unique_ptr<ReadOnlyIndex>> &ro, std::unique_ptr<feeder::RefLoader> &preload, feeder::Feeder &feed) {
    if (o.last_pass && g_knobs.fast_exit) {
        // EXPERIMENT: the run's output is complete and closed -- leave without unwinding (stream slots, the table, the page-locked
        // pool: the operating system takes a process's device and host memory back in one go when it ends)
        print_totals(g_t_main);
        fflush(stdout);
        fflush(stderr);
        _exit(0);
    }
    JoiningThread dev_side([&]() {
        slots.drop();
        ro.clear();
    });
    JoiningThread ref_reaper;
    if (preload) ref_reaper = JoiningThread([pl = preload.release()]() { delete pl; });
    feed.release_buffers();
    dev_side.join();
    ref_reaper.join();
}

// --depth: the run's one accumulator (ReadOnlyIndex::Depth).  It is made on the first pass's primary index once the index phase is
// complete; every chunk of every GPU's slots, and of the second pass, is added to it where the chunk goes to the formatters; the last
// pass writes <prefix>.depth.bed and <prefix>.depth.tsv under the FIRST pass's prefix and prints the log line.
static std::unique_ptr<ReadOnlyIndex::Depth> g_depth;
static std::string g_depth_prefix;
static void write_depth() {
    g_depth->fetch();
    const std::pair<std::string, std::string> files[2] = {{g_depth_prefix + ".depth.bed", g_depth->bed()}, {g_depth_prefix + ".depth.tsv", g_depth->tsv()}};
    for (const auto &f : files) {
        FILE *fp = fopen(f.first.c_str(), "w");
        const bool ok = fp && fwrite(f.second.data(), 1, f.second.size(), fp) == f.second.size();
        if ((fp && fclose(fp) != 0) || !ok) throw Error("Couldn't write " + f.first);
    }
    puts(g_depth->log_line().c_str());
}

// --sort: <prefix>.sorted.paf gathered from the <prefix>.paf this pass has just closed (mapped, its lines written one by one: neither
// file is held in memory), <prefix>.sorted.tsv, and the log line.  A failure leaves none of the three files behind, as a failure of the
// map phase leaves no PAF.
static void write_sorted(ReadOnlyIndex::Sorter &sorter, const SortLines &lines, const std::string &prefix) {
    const std::string paf_path = prefix + ".paf", sorted_path = prefix + ".sorted.paf", tsv_path = prefix + ".sorted.tsv";
    void *map = MAP_FAILED;
    const size_t size = (size_t)lines.paf_bytes;
    try {
        sorter.fetch();
        if (size) {
            const int fd = open(paf_path.c_str(), O_RDONLY);
            struct stat sb;
            if (fd >= 0 && fstat(fd, &sb) == 0 && (size_t)sb.st_size == size) map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (fd >= 0) close(fd);
            if (map == MAP_FAILED) throw Error("Couldn't read " + paf_path);
        }
        std::vector<uint64_t> offsets;
        FILE *fp = fopen(sorted_path.c_str(), "w");
        const bool ok = fp && sorter.gather((const char *)map, size, lines.at, lines.len, fp, offsets);
        if ((fp && fclose(fp) != 0) || !ok) throw Error("Couldn't write " + sorted_path);
        const std::string tsv = sorter.tsv(offsets);
        fp = fopen(tsv_path.c_str(), "w");
        const bool wrote = fp && fwrite(tsv.data(), 1, tsv.size(), fp) == tsv.size();
        if ((fp && fclose(fp) != 0) || !wrote) throw Error("Couldn't write " + tsv_path);
    } catch (...) {
        if (map != MAP_FAILED) munmap(map, size);
        for (const std::string *f : {&paf_path, &sorted_path, &tsv_path}) remove(f->c_str());
        throw;
    }
    if (map != MAP_FAILED) munmap(map, size);
    puts(sorter.log_line().c_str());
}

// One run of the reference's flow (src/closures.rs:22-212): index the reference, map the reads, write <prefix>.paf in input
// order.  second_fa != "": the reads left unmapped also go to that FASTA file (for the second pass).
static int run_pass(const Opt &o, const Params &P, const std::string &reads_path, bool reads_fasta, bool ref_fasta, const std::string &prefix,
                    size_t threads, const std::string &second_fa) {
    OutputFiles out(prefix, o.unmapped || !o.second.empty(), second_fa, o.anchors, o.chains);
    if (o.chains && out.paf && !out.chn) { fprintf(stderr, "Couldn't create %s.chains\n", prefix.c_str()); return 101; }
    if (o.anchors && out.paf && !out.anc) { fprintf(stderr, "Couldn't create %s.anchors\n", prefix.c_str()); return 101; }
    if (!out.paf) { fprintf(stderr, "Couldn't create %s.paf\n", prefix.c_str()); return 101; }

    const Routes rt = describe_routes(o, reads_path, reads_fasta, ref_fasta, threads);
    std::unique_ptr<feeder::RefLoader> preload;
    if (rt.preload_now) preload.reset(new feeder::RefLoader(o.reference, rt.n_parse, !g_knobs.ref_host));  // (HERE: before the first HIP call)
    const Devices dev{o.device, mq_device_count(), g_knobs.fake_multi};
    tl("HIP runtime up (first HIP call returned)");
    if (!dev.enough_for(o.gpus)) {
        fprintf(stderr, "mapquik: --gpus %d from device %d needs %d devices, %d visible\n", o.gpus, o.device, o.device + o.gpus, dev.visible);
        return 101;
    }

    // The read feeder (constructed here, started below): parsing reads does not depend on the index.
    feeder::Feeder feed(reads_path, !reads_fasta, rt.batch_bases, rt.n_parse, rt.n_parse + o.gpus * (N_SLOTS + 1) + rt.n_format + 2);
    feed.leave_unparsed(rt.on_device);  // (acts on uncompressed input only, FASTA or FASTQ)
    feed.premap();  // MQ_FEEDER_MAPPED_FASTA=1 only (experiment): the file is mapped, not read, while the reference is indexed
    // The read feeder starts when the index is ready.  MQ_DRIVER_PREFETCH=1 starts it while the reference is still being indexed
    // (it then allocates its page-locked chunk buffers and parses the first chunks early): that was the default while pinning
    // the pool was the read phase's start-up cost; with the huge-page pool it makes the map phase 15 % shorter and the index
    // phase twice as long (the pool's hipHostRegister calls and the index calls share the driver) -- 1.47 s against 1.0 s for
    // the whole job on the bench's input.
    bool feed_started = false;
    const std::function<void()> start_feed = [&]() {
        if (!feed_started) {
            feed.start();
            feed_started = true;
        }
    };

    auto t0 = Clock::now();
    // Declared in this order, so that on every path out of here the early thread is joined first, then the stream slots go, then
    // the indexes they work on.
    std::unique_ptr<Index> building;
    std::vector<std::unique_ptr<ReadOnlyIndex>> ro((size_t)o.gpus);
    // Submitting threads per GPU.  Chunks that are views of the mapped file are copied to the device from pageable memory: that
    // copy occupies the thread that asks for it, hence two (experimental path, MQ_FEEDER_MAPPED_FASTA=1; see Feeder::premap).
    const int n_sub = feed.mapped_views() ? 2 : 1;
    StreamSlots slots((size_t)(o.gpus * n_sub), rt.batch_bases, feed.bytes_in(), o.anchors, P.density, o.chains);
    const int n_buffers = g_knobs.prefetch ? 0 : rt.n_parse + N_SLOTS;  // chunk buffers page-locked ahead of the feeder's start
    EarlySetup early(slots, feed, n_sub, n_buffers);
    size_t first_ref_id = 0;
    build_or_load_index(RefPhase{o, P, building, rt.n_parse, start_feed, g_knobs.prefetch, first_ref_id}, rt, dev.of(0), preload, ro[0], slots, early);
    tl("every reference record handed to ref_extract");
    finalise_save_clone(o, dev, building, ro, prefix, out);
    finish_slots_and_pool(early, slots, ro, feed, n_buffers);
    tl("replicas cloned, stream slots and first chunk buffers set up");
    printf("Indexed %llu unique k-min-mers in %s.\n", (unsigned long long)ro[0]->unique_count(), rust_duration(secs(t0)).c_str());

    if (o.depth && !g_depth) {  // (the second pass finds the first pass's)
        try {
            g_depth.reset(new ReadOnlyIndex::Depth(*ro[0], (uint32_t)o.depth_window, (uint32_t)o.depth_min_mapq));
            g_depth_prefix = prefix;
        } catch (...) {
            out.discard_paf();
            throw;
        }
    }
    std::unique_ptr<ReadOnlyIndex::Sorter> sorter;  // --sort: one per pass, on the pass's primary index (it goes before the index does)
    SortLines sort_lines;
    if (o.sort) {
        try {
            sorter.reset(new ReadOnlyIndex::Sorter(*ro[0], (uint32_t)o.sort_min_mapq));
            sort_lines.sorter = sorter->handle();
        } catch (...) {
            out.discard_paf();
            throw;
        }
    }

    t0 = Clock::now();
    if (P.use_pfx && !ends_with(reads_path, ".gz") && !ends_with(reads_path, ".lz4")) puts("Warning: using experimental rust-parallelfastx (exciting!)");
    start_feed();
    MapPipeline pipeline(feed, slots.of, *ro[0], out.paf, out.unm, out.ufa, MapPipeline::Config{rt.n_format, rt.fx_format, g_knobs.fail_at, out.anc, P.density, out.chn, g_depth ? g_depth->handle() : nullptr, sorter ? &sort_lines : nullptr});
    try {
        pipeline.run();
    } catch (...) {
        out.discard_paf();
        throw;
    }
    out.close();
    if (g_depth) {
        if (o.last_pass) {
            write_depth();
            g_depth.reset();
        } else {
            g_depth->detach();  // this pass's index goes; the accumulator and the names stay for the second pass
        }
    }
    if (sorter) {
        write_sorted(*sorter, sort_lines, prefix);
        sorter.reset();
    }
    if (g_knobs.timing) pipeline.report(secs(t0));
    printf("Mapped query sequences in %s.\n", rust_duration(secs(t0)).c_str());  // src/closures.rs:211
    tl("PAF written");
    teardown(o, slots, ro, preload, feed);
    tl("stream slots, indexes and the page-locked pool released");
    return 0;
}

int main(int argc, char **argv) {
    const auto start = Clock::now();
    Opt o;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        auto val = [&]() -> const char * {
            if (i + 1 >= argc) { fprintf(stderr, "error: %s needs a value\n", a.c_str()); exit(2); }
            return argv[++i];
        };
        if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (a == "--debug") o.debug = true;
        else if (a == "--low-memory") o.low_memory = true;
        else if (a == "--nosimd") o.nosimd = true;
        else if (a == "--nohpc") o.nohpc = true;
        else if (a == "--parallelfastx") o.parallelfastx = true;
        else if (a == "--unmapped") o.unmapped = true;
        else if (a == "--coverage") o.coverage = true;
        else if (a == "--depth") o.depth = true;
        else if (a == "--depth-window") {
            o.depth_window = atol(val());
            if (o.depth_window < 1 || o.depth_window > (1l << 24)) { fprintf(stderr, "error: --depth-window wants 1..16777216\n"); return 2; }
        }
        else if (a == "--depth-min-mapq") {
            o.depth_min_mapq = atol(val());
            if (o.depth_min_mapq < 0 || o.depth_min_mapq > 0xFFFFFFFFl) { fprintf(stderr, "error: --depth-min-mapq wants a 32-bit value\n"); return 2; }
        }
        else if (a == "--sort") o.sort = true;
        else if (a == "--sort-min-mapq") {
            o.sort_min_mapq = atol(val());
            if (o.sort_min_mapq < 0 || o.sort_min_mapq > 0xFFFFFFFFl) { fprintf(stderr, "error: --sort-min-mapq wants a 32-bit value\n"); return 2; }
        }
        else if (a == "--anchors") o.anchors = true;
        else if (a == "--chains") o.chains = true;
        else if (a == "-p" || a == "--prefix") { o.prefix = val(); o.has_prefix = true; }
        else if (a == "-k") o.k = atol(val());
        else if (a == "-l") o.l = atol(val());
        else if (a == "-d" || a == "--density") o.density = atof(val());
        else if (a == "-c" || a == "--chain") o.c = atol(val());
        else if (a == "-s" || a == "--seed") o.s = atol(val());
        else if (a == "-g" || a == "--gap-diff") o.g = atol(val());
        else if (a == "--reference") o.reference = val();
        else if (a == "--threads") o.threads = atol(val());
        else if (a == "-b") o.b = atol(val());
        else if (a == "-q") o.q = atol(val());
        else if (a == "--device") o.device = atoi(val());
        else if (a == "--gpus") o.gpus = std::max(1, atoi(val()));
        else if (a == "--batch-bases") o.batch_bases = strtoull(val(), nullptr, 10);
        else if (a == "--table-factor") {
            o.table_factor_given = true;
            o.table_factor = atoi(val());
            if (o.table_factor < 2 || o.table_factor > 64) { fprintf(stderr, "error: --table-factor wants 2..64\n"); return 2; }
        }
        else if (a == "--ref-join") {
            const std::string v = val();
            if (v != "device" && v != "host") { fprintf(stderr, "error: --ref-join wants device or host\n"); return 2; }
            o.ref_join_device = v == "device";
        }
        else if (a == "--reads-join") {
            const std::string v = val();
            if (v != "device" && v != "host") { fprintf(stderr, "error: --reads-join wants device or host\n"); return 2; }
            o.reads_join_device = v == "device";
        }
        else if (a == "--save-index") o.save_index = val();
        else if (a == "--index") o.load_index = val();
        else if (a == "--add-reference") o.add_reference = val();
        else if (a == "--merge-index") o.merge_index.push_back(val());
        else if (a == "--seeding-variant") {
            o.seeding_variant = atoi(val());
            if (o.seeding_variant < 0 || o.seeding_variant > 63) { fprintf(stderr, "error: --seeding-variant wants 0..63 (bits 1 2 4 8 16 32)\n"); return 2; }
        }
        else if (a == "--fast-kh") o.fast_kh = true;
        else if (a == "--second-pass") {
            o.second = val();
            char *e1 = nullptr, *e2 = nullptr;
            o.k2 = strtol(o.second.c_str(), &e1, 10);
            o.l2 = (e1 && *e1 == ',') ? strtol(e1 + 1, &e2, 10) : 0;
            o.d2 = (e2 && *e2 == ',') ? atof(e2 + 1) : -1;
            if (o.k2 < 1 || o.l2 < 1 || !(o.d2 > 0)) { fprintf(stderr, "error: --second-pass wants k2,l2,d2\n"); return 2; }
        }
        else if (!a.empty() && a[0] == '-') { fprintf(stderr, "error: Found argument '%s' which wasn't expected\n", a.c_str()); return 2; }
        else o.reads = a;
    }
    if (!o.add_reference.empty() && (o.load_index.empty() || !o.reference.empty())) {
        fprintf(stderr, "error: --add-reference adds to the index given with --index (and excludes --reference)\n");
        return 2;
    }
    if (!o.merge_index.empty() && o.load_index.empty() && o.reference.empty() && o.add_reference.empty()) {
        fprintf(stderr, "error: --merge-index merges into the index given with --index or built from --reference\n");
        return 2;
    }
    if (!o.add_reference.empty()) o.reference = o.add_reference;  // from here on the file is this run's reference file: same routes, same log lines
    if (o.reads.empty()) { fprintf(stderr, "Please specify an input file.\n"); return 101; }          // panic!, src/main.rs:191
    if (o.reference.empty() && o.load_index.empty()) { fprintf(stderr, "Please specify a reference file.\n"); return 101; }   // src/main.rs:192
    if (!o.load_index.empty() && ((!o.save_index.empty() && o.add_reference.empty() && o.merge_index.empty()) || !o.second.empty())) {
        fprintf(stderr, "error: --index cannot be combined with --save-index (unless --add-reference extends it) or --second-pass (a second pass builds its own index)\n");
        return 2;
    }

    Params P;
    size_t threads = 8;
    const bool reads_fasta = is_fasta_name(o.reads), ref_fasta = is_fasta_name(o.reference);
    if (reads_fasta) printf("Input file: %s\nFormat: FASTA\n", o.reads.c_str());
    if (ref_fasta && (o.load_index.empty() || !o.add_reference.empty())) printf("Reference file: %s\nFormat: FASTA\n", o.reference.c_str());
    if (o.k >= 0) P.k = (size_t)o.k; else printf("Warning: Using default k value (%zu).\n", P.k);
    if (o.l >= 0) P.l = (size_t)o.l; else printf("Warning: Using default l value (%zu).\n", P.l);
    if (o.b >= 0) P.b = (size_t)o.b; else printf("Warning: Using default buffer size (%zuX).\n", P.b);
    if (o.q >= 0) P.q = (size_t)o.q; else printf("Warning: Using default queue length (%zu).\n", P.q);
    if (o.density >= 0) P.density = o.density; else printf("Warning: Using default density value (%s%%).\n", rust_float(P.density * 100.0).c_str());
    if (o.threads >= 0) threads = (size_t)o.threads; else printf("Warning: Using default number of threads (8).\n");
    if (o.c >= 0) P.c = (size_t)o.c; else printf("Warning: Using default minimum chain length (%zu).\n", P.c);
    if (o.s >= 0) P.s = (size_t)o.s; else printf("Warning: Using default minimum number of matching seeds (%zu).\n", P.s);
    if (o.g >= 0) P.g = (size_t)o.g; else printf("Warning: Using default maximum seed gap difference (%zu).\n", P.g);
    std::string prefix = "mapquik-k" + std::to_string(P.k) + "-d" + rust_float(P.density) + "-l" + std::to_string(P.l);
    if (o.has_prefix) prefix = o.prefix; else printf("Warning: Using default output prefix (%s).\n", prefix.c_str());
    P.debug = o.debug;
    P.use_hpc = !o.nohpc;
    P.use_simd = !o.nosimd;
    P.use_pfx = o.parallelfastx;
    P.fold_case = true;  // raw FASTX bytes go to the GPU: the kernels do the reference's to_ascii_uppercase
    P.seeding_variant = (unsigned)o.seeding_variant;
    if (o.seeding_variant) printf("Seeding variant %d (reading of rust-seq2kminmers other than the frozen one; include/mapquik_hip.h).\n", o.seeding_variant);
    P.fast_kh = o.fast_kh;
    if (o.fast_kh) puts("Fast k-min-mer tuple hash (MQ_FLAG_FAST_KH): same PAF, KminmerHash.hash is not the reference's value.");
    if (P.use_hpc) puts(P.use_simd ? "Using HPC ntHash, with SIMD" : "Using HPC ntHash, scalar");
    else puts(P.use_simd ? "Using regular ntHash (not HPC), with SIMD" : "Using regular ntHash (not HPC), scalar");

    const std::string second_prefix = prefix + "-" + std::to_string(o.k2) + "-" + std::to_string(o.l2) + "-" + rust_float(o.d2);
    try {
        tl("arguments parsed");
        o.last_pass = o.second.empty();
        int rc = run_pass(o, P, o.reads, reads_fasta, ref_fasta, prefix, threads, o.second.empty() ? std::string() : second_prefix + ".fa");
        tl("run_pass returned (index, feeder and its page-locked pool released)");
        if (rc) return rc;
        if (!o.second.empty()) {
            // the second pass of experiments/chm13/run_chm13_mapquik_unmapped.sh:8-24: the reads the first pass left unmapped,
            // mapped again with (k2, l2, d2) against a second index of the same reference
            P.k = (size_t)o.k2;
            P.l = (size_t)o.l2;
            P.density = o.d2;
            printf("Second pass: %s with k=%zu l=%zu density=%s\n", (second_prefix + ".fa").c_str(), P.k, P.l, rust_float(P.density).c_str());
            o.last_pass = true;
            rc = run_pass(o, P, second_prefix + ".fa", true, ref_fasta, second_prefix, threads, std::string());
            if (rc) return rc;
        }
    } catch (const std::exception &e) {  // mapquik::Error, feeder::FeederError: the reference panics (exit code 101)
        g_depth.reset();
        fflush(stdout);
        fprintf(stderr, "mapquik: %s\n", e.what());
        return 101;
    }
    tl("all passes done");
    print_totals(start);
    return 0;
}
