// mapquik_host.hpp -- C++ host-side mirror of the reference's interface for the hot path, on top of the C ABI
// (include/mapquik_hip.h).  The reference is Rust; there is no Rust toolchain in this image, so the layer a Rust
// maintainer would write over the extern "C" block is written in C++ with the same names and argument
// meaning:   Params (src/main.rs:33-47) . Index / ReadOnlyIndex (src/index.rs:73-128) . mers::ref_extract (src/mers.rs:15)
//            . mers::find_matches (src/mers.rs:77) -> std::optional<std::string> for Option<String>.
// Errors: the reference panics; this layer throws mapquik::Error (never across the C ABI).  No CPU compute path exists.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/mapquik_hip.h"

namespace mapquik {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// src/main.rs:33-47, defaults src/main.rs:174-188
struct Params {
    size_t k = 5;
    size_t l = 31;
    double density = 0.01;
    bool use_hpc = true;
    bool use_simd = true;   // a speed switch in the reference (src/main.rs:150-155); no effect here
    bool use_pfx = false;
    bool debug = false;
    bool a = false;
    bool fold_case = false;  // extension: the kernels treat a-z as A-Z (the reference upper-cases on the host, src/closures.rs:63,106)
    unsigned seeding_variant = 0;  // extension: MQ_SEEDVAR_* bits (include/mapquik_hip.h); 0 = the frozen reading of rust-seq2kminmers
    bool fast_kh = false;    // extension: MQ_FLAG_FAST_KH, the cheap tuple hash (same PAF; KminmerHash.hash is then not the reference's value)
    size_t c = 4;
    size_t s = 11;
    size_t g = 2000;
    size_t b = 1;
    size_t q = 200;
    mq_params to_abi() const {
        mq_params p;
        p.k = (uint32_t)k;
        p.l = (uint32_t)l;
        p.density = density;
        p.use_hpc = use_hpc ? 1u : 0u;
        p.c = (uint32_t)c;
        p.s = (uint32_t)s;
        p.g = (uint32_t)g;
        p.flags = (fold_case ? MQ_FLAG_FOLD_CASE : 0u) | (fast_kh ? MQ_FLAG_FAST_KH : 0u) | MQ_FLAG_SEED_VARIANT(seeding_variant);
        return p;
    }
};

inline std::string last_error() { return mq_last_error() ? mq_last_error() : ""; }

class ReadOnlyIndex;

// Index (src/index.rs:73-105) + the ref_map of src/closures.rs:30
class Index {
  public:
    explicit Index(const Params &params, int device = 0) : params_(params) {
        const mq_params p = params.to_abi();
        h_ = mq_index_new(&p, device);
        if (!h_) throw Error("Index::new: " + last_error());
    }
    Index(const Index &) = delete;
    Index &operator=(const Index &) = delete;
    Index(Index &&o) noexcept : h_(o.h_), params_(o.params_) { o.h_ = nullptr; }
    ~Index() { mq_index_free(h_); }
    mq_index *handle() const { return h_; }
    const Params &params() const { return params_; }
    // table slots per inserted k-min-mer (mq_index_set_table_factor): 8 by default, 2 for host-bound file-fed runs
    void table_factor(uint32_t slots_per_kminmer) {
        if (mq_index_set_table_factor(h_, slots_per_kminmer) != MQ_OK) throw Error("Index::table_factor: " + last_error());
    }
    // DashMap::with_capacity (src/index.rs:83): the table for about n k-min-mers is allocated and cleared while the references load
    void with_capacity(uint64_t n_kminmers) {
        if (mq_index_reserve(h_, n_kminmers) != MQ_OK) throw Error("Index::with_capacity: " + last_error());
    }
    // get_count (src/index.rs:90-92) is reported by into_read_only()
    ReadOnlyIndex into_read_only() &&;

  private:
    friend class ReadOnlyIndex;
    Index(mq_index *h, const Params &params) : h_(h), params_(params) {}  // (ReadOnlyIndex::reopen)
    mq_index *h_ = nullptr;
    Params params_;
};

// ReadOnlyIndex (src/index.rs:108-128): finalized, resident in HBM
class ReadOnlyIndex {
  public:
    ReadOnlyIndex(const ReadOnlyIndex &) = delete;
    ReadOnlyIndex(ReadOnlyIndex &&o) noexcept : h_(o.h_), unique_(o.unique_) { o.h_ = nullptr; }
    ~ReadOnlyIndex() { mq_index_free(h_); }
    mq_index *handle() const { return h_; }
    uint64_t unique_count() const { return unique_; }
    // table_slots / slots_per_kminmer (at most one of them non-zero; include/mapquik_hip.h): the table's size, whatever the file records
    static ReadOnlyIndex load(const std::string &path, int device = 0, uint64_t table_slots = 0, uint32_t slots_per_kminmer = 0) {
        mq_index *h = table_slots || slots_per_kminmer ? mq_index_load_sized(path.c_str(), device, table_slots, slots_per_kminmer) : mq_index_load(path.c_str(), device);
        if (!h) throw Error("ReadOnlyIndex::load: " + last_error());
        mq_index_stats st;
        mq_index_get_stats(h, &st);
        return ReadOnlyIndex(h, st.n_unique);
    }
    // a replica on another device (device-to-device copy of the table; with a size, of its occupied slots into a table of that size)
    ReadOnlyIndex clone_to(int device, uint64_t table_slots = 0, uint32_t slots_per_kminmer = 0) const {
        mq_index *h = table_slots || slots_per_kminmer ? mq_index_clone_sized(h_, device, table_slots, slots_per_kminmer) : mq_index_clone(h_, device);
        if (!h) throw Error("ReadOnlyIndex::clone_to: " + last_error());
        return ReadOnlyIndex(h, unique_);
    }
    // the table rebuilt on the device at another size
    void resize(uint64_t table_slots, uint32_t slots_per_kminmer = 0) {
        if (mq_index_resize(h_, table_slots, slots_per_kminmer) != MQ_OK) throw Error("ReadOnlyIndex::resize: " + last_error());
    }
    // back to an Index that takes references (mq_index_reopen): into_read_only() then inserts the new ones into the existing table
    Index reopen(const Params &params) && {
        if (mq_index_reopen(h_) != MQ_OK) throw Error("ReadOnlyIndex::reopen: " + last_error());
        mq_index *h = h_;
        h_ = nullptr;
        return Index(h, params);
    }
    void save(const std::string &path) const {
        if (mq_index_save(h_, path.c_str()) != MQ_OK) throw Error("ReadOnlyIndex::save: " + last_error());
    }
    // a saved index merged into this one (mq_index_merge_file), its reference ids behind every id this index has; returns what it brought
    struct Merged {
        uint64_t refs, kminmers;
    };
    Merged merge_file(const std::string &path) {
        mq_index_stats a, b;
        mq_index_get_stats(h_, &a);
        uint32_t next = 0;
        for (uint64_t seen = 0; seen < a.n_refs; ++next)
            if (mq_index_ref_info(h_, next, nullptr, nullptr) == MQ_OK) ++seen;
        if (mq_index_merge_file(h_, path.c_str(), next) != MQ_OK) throw Error("ReadOnlyIndex::merge_file: " + last_error());
        mq_index_get_stats(h_, &b);
        unique_ = b.n_unique;
        return Merged{b.n_refs - a.n_refs, b.n_kminmers - a.n_kminmers};
    }
    // Which bases of which reference the live k-min-mers span (mq_index_coverage): the library's host copies, valid until the next call
    // that changes this index or asks again.  bed() / tsv(): the two files of --coverage.
    struct Coverage {
        const mq_index *index = nullptr;
        const mq_ref_coverage *refs = nullptr;
        const mq_cov_interval *intervals = nullptr;
        uint64_t n_refs = 0, n_intervals = 0, out_of_range = 0;
        uint64_t covered() const {
            uint64_t s = 0;
            for (uint64_t i = 0; i < n_refs; ++i) s += refs[i].covered_bases;
            return s;
        }
        uint64_t total() const {
            uint64_t s = 0;
            for (uint64_t i = 0; i < n_refs; ++i) s += refs[i].len;
            return s;
        }
        std::string name(const mq_ref_coverage &r) const {
            const char *n = "";
            if (mq_index_ref_info(index, r.ref_id, &n, nullptr) != MQ_OK) throw Error("Coverage: " + last_error());
            return n;
        }
        std::string bed() const {  // r_name \t start \t end, one line per interval
            std::string out;
            for (uint64_t i = 0; i < n_refs; ++i) {
                const std::string n = name(refs[i]);
                for (uint64_t j = refs[i].first_interval; j < refs[i].first_interval + refs[i].n_intervals; ++j)
                    out += n + "\t" + std::to_string(intervals[j].start) + "\t" + std::to_string(intervals[j].end) + "\n";
            }
            return out;
        }
        std::string tsv() const {
            std::string out = "#ref\tlen\tlive_kminmers\tcovered\tfraction\tintervals\n";
            for (uint64_t i = 0; i < n_refs; ++i) {
                const mq_ref_coverage &r = refs[i];
                char frac[64];
                snprintf(frac, sizeof(frac), "%.6f", (double)r.covered_bases / (double)r.len);
                out += name(r) + "\t" + std::to_string(r.len) + "\t" + std::to_string(r.live_kminmers) + "\t" + std::to_string(r.covered_bases) + "\t" + frac + "\t" +
                       std::to_string(r.n_intervals) + "\n";
            }
            return out;
        }
    };
    Coverage coverage() {
        Coverage c;
        c.index = h_;
        if (mq_index_coverage(h_, &c.refs, &c.n_refs, &c.intervals, &c.n_intervals, &c.out_of_range) != MQ_OK) throw Error("ReadOnlyIndex::coverage: " + last_error());
        return c;
    }
    // Where the reads landed (mq_depth): an accumulator on this index's device with a snapshot of its reference ids and lengths, fed with
    // finished hits from any thread.  Names are resolved when it is made, so it may be read after the index has gone (the second pass of
    // the native driver adds to the first pass's accumulator).  bed() / tsv() / log_line(): the two files and the log line of --depth.
    class Depth {
      public:
        Depth(const ReadOnlyIndex &index, uint32_t window, uint32_t min_mapq) : window_(window), min_mapq_(min_mapq) {
            if (mq_depth_new(index.h_, window, min_mapq, &h_) != MQ_OK) throw Error("ReadOnlyIndex::Depth: " + last_error());
            index_ = index.h_;
        }
        Depth(const Depth &) = delete;
        Depth &operator=(const Depth &) = delete;
        ~Depth() { mq_depth_free(h_); }
        mq_depth *handle() const { return h_; }
        void add(const mq_hit *hits, uint32_t n) {
            if (mq_depth_add(h_, hits, n) != MQ_OK) throw Error("mq_depth_add: " + last_error());
        }
        // the result (the library's host copies, valid until the next fetch) with the references' names, looked up while the index lives
        void fetch() {
            if (mq_depth_result(h_, &refs_, &n_refs_, &bases_, &starts_, &n_windows_, &totals_) != MQ_OK) throw Error("mq_depth_result: " + last_error());
            if (!index_) return;
            names_.clear();
            for (uint64_t i = 0; i < n_refs_; ++i) {
                const char *n = "";
                if (mq_index_ref_info(index_, refs_[i].ref_id, &n, nullptr) != MQ_OK) throw Error("Depth: " + last_error());
                names_.push_back(n);
            }
        }
        // the index is about to go: the names are kept, later fetches do not ask it again
        void detach() {
            fetch();
            index_ = nullptr;
        }
        std::string bed() const {  // r_name \t start \t end \t bases \t starts \t mean, one line per window
            std::string out;
            char mean[64];
            for (uint64_t i = 0; i < n_refs_; ++i) {
                const mq_ref_depth &r = refs_[i];
                for (uint64_t j = 0; j < r.n_windows; ++j) {
                    const uint64_t a = j * window_, b = std::min<uint64_t>((j + 1) * window_, r.len), v = bases_[r.first_window + j];
                    snprintf(mean, sizeof(mean), "%.2f", (double)v / (double)(b - a));
                    out += names_[i] + "\t" + std::to_string(a) + "\t" + std::to_string(b) + "\t" + std::to_string(v) + "\t" + std::to_string(starts_[r.first_window + j]) + "\t" + mean + "\n";
                }
            }
            return out;
        }
        std::string tsv() const {
            std::string out = "#ref\tlen\treads\tbases\tmean\tzero_windows\tmax_window_mean\n";
            char mean[64], deepest[64];
            for (uint64_t i = 0; i < n_refs_; ++i) {
                const mq_ref_depth &r = refs_[i];
                snprintf(mean, sizeof(mean), "%.2f", (double)r.bases / (double)r.len);
                snprintf(deepest, sizeof(deepest), "%.2f", (double)r.max_window_bases / (double)std::min<uint64_t>(window_, r.len));
                out += names_[i] + "\t" + std::to_string(r.len) + "\t" + std::to_string(r.reads) + "\t" + std::to_string(r.bases) + "\t" + mean + "\t" + std::to_string(r.zero_windows) +
                       "\t" + deepest + "\n";
            }
            return out;
        }
        std::string log_line() const {
            uint64_t bases = 0, windows = 0;
            for (uint64_t i = 0; i < n_refs_; ++i) bases += refs_[i].bases, windows += refs_[i].n_windows;
            return "Depth: " + std::to_string(totals_.counted) + " of " + std::to_string(totals_.offered) + " hits counted (" + std::to_string(totals_.not_mapped) + " not mapped, " +
                   std::to_string(totals_.below_mapq) + " below mapq " + std::to_string(min_mapq_) + ", " + std::to_string(totals_.out_of_range) + " out of range): " +
                   std::to_string(bases) + " bases in " + std::to_string(windows) + " windows of " + std::to_string(window_);
        }

      private:
        mq_depth *h_ = nullptr;
        const mq_index *index_ = nullptr;
        uint32_t window_, min_mapq_;
        const mq_ref_depth *refs_ = nullptr;
        const uint64_t *bases_ = nullptr;
        const uint32_t *starts_ = nullptr;
        uint64_t n_refs_ = 0, n_windows_ = 0;
        mq_depth_totals totals_ = {};
        std::vector<std::string> names_;
    };
    // The coordinate order of a run's hits (mq_sorter): a sorter on this index's device with a snapshot of its reference ids, fed with
    // finished hits under their reads' numbers in input order.  It lives inside its index's lifetime.  fetch() / gather() / tsv() /
    // log_line(): the two files and the log line of --sort.
    class Sorter {
      public:
        Sorter(const ReadOnlyIndex &index, uint32_t min_mapq) : index_(index.h_), min_mapq_(min_mapq) {
            if (mq_sort_new(index.h_, 0, min_mapq, &h_) != MQ_OK) throw Error("ReadOnlyIndex::Sorter: " + last_error());
        }
        Sorter(const Sorter &) = delete;
        Sorter &operator=(const Sorter &) = delete;
        ~Sorter() { mq_sort_free(h_); }
        mq_sorter *handle() const { return h_; }
        void add(const mq_hit *hits, uint32_t n, uint32_t first_ordinal) {
            if (mq_sort_add(h_, hits, n, first_ordinal) != MQ_OK) throw Error("mq_sort_add: " + last_error());
        }
        // the result (the library's host copies, valid until the next fetch)
        void fetch() {
            if (mq_sort_result(h_, &order_, &n_kept_, &refs_, &n_refs_, &totals_) != MQ_OK) throw Error("mq_sort_result: " + last_error());
        }
        const uint32_t *order() const { return order_; }
        uint64_t n_kept() const { return n_kept_; }
        // <prefix>.sorted.paf: the lines of the paf_size bytes at `paf` (<prefix>.paf, mapped) written to `out` in sorted order, one line at a
        // time -- nothing of either file is held in memory; at[o], len[o]: where read number o's line lies there and how long it is (0: it
        // has none).  offsets gets where every sorted line begins, and the size behind the last.  false: a write failed.
        bool gather(const char *paf, uint64_t paf_size, const std::vector<uint64_t> &at, const std::vector<uint32_t> &len, FILE *out, std::vector<uint64_t> &offsets) const {
            offsets.assign(1, 0);
            offsets.reserve(n_kept_ + 1);
            for (uint64_t j = 0; j < n_kept_; ++j) {
                const uint32_t o = order_[j];
                if (o >= len.size() || !len[o] || at[o] + len[o] > paf_size) throw Error("--sort: read " + std::to_string(o) + " was kept but has no PAF line");
                if (fwrite(paf + at[o], 1, len[o], out) != len[o]) return false;
                offsets.push_back(offsets.back() + len[o]);
            }
            return true;
        }
        std::string tsv(const std::vector<uint64_t> &offsets) const {  // a seek table: per reference its lines and where the first begins
            std::string out = "#ref\tlen\tlines\tfirst_line\toffset\n";
            for (uint64_t i = 0; i < n_refs_; ++i) {
                const mq_sort_ref &r = refs_[i];
                const char *name = "";
                uint64_t len = 0;
                if (mq_index_ref_info(index_, r.ref_id, &name, &len) != MQ_OK) throw Error("Sorter: " + last_error());
                out += std::string(name) + "\t" + std::to_string(len) + "\t" + std::to_string(r.count) + "\t" + std::to_string(r.first) + "\t" + std::to_string(offsets.at(r.first)) + "\n";
            }
            return out;
        }
        std::string log_line() const {
            uint64_t lines = 0, with = 0;
            for (uint64_t i = 0; i < n_refs_; ++i) lines += refs_[i].count, with += refs_[i].count != 0;
            return "Sorted: " + std::to_string(totals_.kept) + " of " + std::to_string(totals_.offered) + " hits kept (" + std::to_string(totals_.not_mapped) + " not mapped, " +
                   std::to_string(totals_.below_mapq) + " below mapq " + std::to_string(min_mapq_) + ", " + std::to_string(totals_.out_of_range) + " out of range): " +
                   std::to_string(lines) + " lines on " + std::to_string(with) + " references";
        }

      private:
        mq_sorter *h_ = nullptr;
        const mq_index *index_;
        uint32_t min_mapq_;
        const uint32_t *order_ = nullptr;
        const mq_sort_ref *refs_ = nullptr;
        uint64_t n_kept_ = 0, n_refs_ = 0;
        mq_sort_totals totals_ = {};
    };

  private:
    friend class Index;
    ReadOnlyIndex(mq_index *h, uint64_t u) : h_(h), unique_(u) {}
    mq_index *h_ = nullptr;
    uint64_t unique_ = 0;
};

inline ReadOnlyIndex Index::into_read_only() && {
    const int64_t u = mq_index_finalize(h_);
    if (u < 0) throw Error("Index::into_read_only: " + last_error());
    mq_index *h = h_;
    h_ = nullptr;
    return ReadOnlyIndex(h, (uint64_t)u);
}

// A stream slot of an index (mq_ctx: device staging, minimizer lists, Match scratch of one batch in flight).  It uses its index until
// it is destroyed: contexts go before their index.
class Ctx {
  public:
    explicit Ctx(mq_index *index) : h_(mq_ctx_new(index)) {
        if (!h_) throw Error("mq_ctx_new: " + last_error());
    }
    Ctx(const Ctx &) = delete;
    Ctx &operator=(const Ctx &) = delete;
    Ctx(Ctx &&o) noexcept : h_(o.h_), anchors_bytes_(o.anchors_bytes_), chains_bytes_(o.chains_bytes_) { o.h_ = nullptr; }
    ~Ctx() { mq_ctx_free(h_); }
    mq_ctx *handle() const { return h_; }
    // room for batches of up to max_reads reads in max_bytes bytes, so that the first batches do not grow the slot
    void reserve(uint32_t max_reads, uint64_t max_bytes) {
        if (mq_ctx_reserve(h_, max_reads, max_bytes) != MQ_OK) throw Error("mq_ctx_reserve: " + last_error());
    }
    // --anchors, --chains: spans and a pool for chunks of up to max_bytes raw bytes (pool_bounds).  A chunk that needs more (reads inside
    // dense tandem arrays) reports dropped reads, and the run ends with what it needed.
    void reserve_anchors(uint64_t max_bytes, double density) {
        const PoolBounds b = pool_bounds(max_bytes, density);
        if (mq_ctx_reserve_anchors(h_, b.reads, b.entries) != MQ_OK) throw Error("mq_ctx_reserve_anchors: " + last_error());
        anchors_bytes_ = max_bytes;
    }
    uint64_t anchors_bytes() const { return anchors_bytes_; }  // the chunk size the slot's anchor reservation was made for (0: none)
    void reserve_chains(uint64_t max_bytes, double density) {
        const PoolBounds b = pool_bounds(max_bytes, density);
        if (mq_ctx_reserve_chains(h_, b.reads, b.entries) != MQ_OK) throw Error("mq_ctx_reserve_chains: " + last_error());
        chains_bytes_ = max_bytes;
    }
    uint64_t chains_bytes() const { return chains_bytes_; }

  private:
    // The bounds of both pooled outputs: a record takes at least four bytes of a file (">\nA\n"), so a chunk holds at most max_bytes / 4 + 1
    // reads; a read has no more chains than Match runs, no more runs than k-min-mers and fewer k-min-mers than minimizers, and the library
    // sizes its minimizer lists at bytes x (4 density + 1/512) entries -- the same number of pool entries here.
    struct PoolBounds {
        uint32_t reads;
        uint64_t entries;
    };
    static PoolBounds pool_bounds(uint64_t max_bytes, double density) {
        const double f = std::min(1.0, 4.0 * (density > 0 ? density : 0.0) + 1.0 / 512.0);
        return {(uint32_t)std::min<uint64_t>(max_bytes / 4 + 1, (1u << 30) - 1), std::min<uint64_t>((uint64_t)((double)max_bytes * f) + 64, 0xFFFFFFFEull - 1)};
    }
    mq_ctx *h_ = nullptr;
    uint64_t anchors_bytes_ = 0, chains_bytes_ = 0;
};

// The format! of src/mers.rs:181 for many reads: the same bytes as mq_format_paf, appended to a string, with the reference names and
// lengths looked up once per reference (a formatter thread of the native driver writes ~200,000 lines per batch; snprintf and a map
// lookup per line were 3-4 us of it).
class PafWriter {
  public:
    explicit PafWriter(const ReadOnlyIndex &index) : idx_(index.handle()) {}
    // appends "q_id\tq_len\t...\tmapq\n" for a mapped hit
    void append(std::string &out, const char *q_id, size_t q_id_len, uint64_t q_len, const mq_hit &h) {
        const Ref &r = ref(h.ref_id);
        char num[8 * 21 + 16];
        char *p = num;
        auto u = [&](uint64_t x) {
            char t[20];
            int n = 0;
            do { t[n++] = (char)('0' + x % 10); x /= 10; } while (x);
            while (n) *p++ = t[--n];
        };
        out.append(q_id, q_id_len);
        *p++ = '\t'; u(q_len);
        *p++ = '\t'; u(((uint64_t)h.q_start_hi << 32) | h.q_start);
        *p++ = '\t'; u(((uint64_t)h.q_end_hi << 32) | h.q_end);
        *p++ = '\t'; *p++ = h.rc ? '-' : '+'; *p++ = '\t';
        out.append(num, (size_t)(p - num));
        out += r.name;
        p = num;
        *p++ = '\t'; u(r.len);
        *p++ = '\t'; u(h.r_start);
        *p++ = '\t'; u(h.r_end);
        *p++ = '\t'; u(h.score);
        *p++ = '\t'; u(r.len);
        *p++ = '\t'; u(h.mapq);
        *p++ = '\n';
        out.append(num, (size_t)(p - num));
    }

    const std::string &ref_name(uint32_t id) { return ref(id).name; }

  private:
    struct Ref {
        std::string name;
        uint64_t len = 0;
        bool known = false;
    };
    const Ref &ref(uint32_t id) {
        if (id >= refs_.size()) refs_.resize((size_t)id + 1);
        Ref &r = refs_[id];
        if (!r.known) {
            const char *name = nullptr;
            uint64_t len = 0;
            if (mq_index_ref_info(idx_, id, &name, &len) != MQ_OK) throw Error("find_coords: " + last_error());
            r.name = name ? name : "";
            r.len = len;
            r.known = true;
        }
        return r;
    }
    mq_index *idx_;
    std::vector<Ref> refs_;
};

namespace mers {

// mers::ref_extract (src/mers.rs:15-38) + ref_map.insert (src/closures.rs:49).  Returns the reference's k-min-mer count.
inline size_t ref_extract(size_t ref_idx, const std::string &ref_id, const uint8_t *inp_seq_raw, size_t len, const Params &, Index &mers_index) {
    const int64_t n = mq_index_add_ref(mers_index.handle(), (uint32_t)ref_idx, ref_id.c_str(), inp_seq_raw, (uint64_t)len);
    if (n < 0) throw Error("ref_extract: " + last_error());
    return (size_t)n;
}

// Batch form of find_matches: one Option<String> per read, in input order.
inline std::vector<std::optional<std::string>> find_matches_batch(const std::vector<std::string> &q_ids, const uint8_t *bases,
                                                                  const std::vector<uint64_t> &offsets, const ReadOnlyIndex &mers_index,
                                                                  const Params &) {
    const uint32_t n = (uint32_t)q_ids.size();
    std::vector<std::optional<std::string>> out(n);
    if (!n) return out;
    std::vector<mq_hit> hits(n);
    if (mq_map_batch(mers_index.handle(), bases, offsets.data(), n, hits.data()) != MQ_OK) throw Error("find_matches: " + last_error());
    std::vector<char> buf(4096);
    for (uint32_t i = 0; i < n; ++i) {
        if (hits[i].status == MQ_HIT_MAPPED) {
            int w = mq_format_paf(mers_index.handle(), q_ids[i].c_str(), offsets[i + 1] - offsets[i], &hits[i], buf.data(), buf.size());
            if (w >= (int)buf.size()) {  // long read / contig names: the return value is the full length, format again
                buf.resize((size_t)w + 1);
                w = mq_format_paf(mers_index.handle(), q_ids[i].c_str(), offsets[i + 1] - offsets[i], &hits[i], buf.data(), buf.size());
            }
            if (w < 0) throw Error("find_coords: " + last_error());
            out[i] = std::string(buf.data(), (size_t)w);
        } else if (hits[i].status != MQ_HIT_UNMAPPED) {
            throw Error("find_matches: read " + q_ids[i] + " could not be processed");
        }
    }
    return out;
}

// mers::find_matches (src/mers.rs:77-102): the PAF line, or nothing when the reference returns None.
inline std::optional<std::string> find_matches(const std::string &q_id, size_t q_len, const uint8_t *q_str, const ReadOnlyIndex &mers_index,
                                               const Params &params) {
    return find_matches_batch({q_id}, q_str, {0, (uint64_t)q_len}, mers_index, params)[0];
}

}  // namespace mers
}  // namespace mapquik
