// feeder_input.hpp -- what the read feeder (fastx_feeder.hpp) reads and how: the environment's knobs, read once; the description of the
// input file (kind, sizes, mapping, chunking, the BGZF block index); and the one function that names the reader that will run.
#pragma once
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fastx_records.hpp"
#include "par_gzip.hpp"

namespace mapquik {
namespace feeder {

// every environment variable the feeder listens to (MQ_FEEDER_NO_LIBDEFLATE aside: Deflate reads that one itself)
struct Knobs {
    bool no_lean_fastq = getenv("MQ_FEEDER_NO_LEAN_FASTQ") != nullptr;  // uncompressed FASTQ through the chunked reader, quality lines and all
    bool mapped_fasta = num("MQ_FEEDER_MAPPED_FASTA", 0) != 0;          // experiment: chunks of raw FASTA as views of the mapped file
    bool page_lock = getenv("MQ_FEEDER_PAGE_LOCK") != nullptr;          // ... whose pages the reader threads page-lock
    bool timing = getenv("MQ_FEEDER_TIMING") != nullptr;                // the gzip member reader reports each member on stderr
    bool gz_whole_limit_set = getenv("MQ_GZ_WHOLE_LIMIT") != nullptr;   // (set: no member is inflated by all threads just because it could be)
    uint64_t gz_whole_limit = num("MQ_GZ_WHOLE_LIMIT", 4ull << 30);     // one thread: gzip files beyond this stream through zlib
    bool pargz = num("MQ_PARGZ", 1) != 0;                               // large gzip members inflated by all threads
    uint64_t pargz_min = num("MQ_PARGZ_MIN", 16u << 20);                // compressed bytes from which a member is worth many threads
    uint64_t pargz_seg = num("MQ_PARGZ_SEG", pargz::Options().seg_bytes);
    uint64_t pargz_minseg = num("MQ_PARGZ_MINSEG", pargz::Options().min_seg_bytes);

    static uint64_t num(const char *name, uint64_t dflt) {
        const char *v = getenv(name);
        return v ? strtoull(v, nullptr, 10) : dflt;
    }
};

// ---------------------------------------------------------------- BGZF (bgzip): a series of independent deflate streams with their sizes in
// the headers, so the file is indexed once and then read like a raw file -- BgzfIndex::read gives any range of the inflated ("logical") file

// One thread's inflater of BGZF blocks (raw deflate payloads): a libdeflate decompressor where the library is there, a z_stream else.
struct BlockInflater {
    explicit BlockInflater(const Deflate &dl) : dl_(dl) {
        if (dl_.ok()) {
            d_ = dl_.alloc();
            if (!d_) throw FeederError("libdeflate: no decompressor");
        } else {
            memset(&zs_, 0, sizeof(zs_));
            if (inflateInit2(&zs_, -15) != Z_OK) throw FeederError("inflateInit2 failed");  // raw deflate: BGZF payloads
        }
    }
    ~BlockInflater() {
        if (d_) dl_.free_(d_);
        else inflateEnd(&zs_);
    }
    BlockInflater(const BlockInflater &) = delete;

    // in[0, in_n) inflates to exactly out_n bytes at out
    bool inflate_block(const uint8_t *in, size_t in_n, uint8_t *out, size_t out_n) {
        if (d_) {
            size_t got = 0;
            return dl_.raw(d_, in, in_n, out, out_n, &got) == 0 && got == out_n;
        }
        if (inflateReset(&zs_) != Z_OK) throw FeederError("inflateReset failed");
        zs_.next_in = const_cast<Bytef *>(in);
        zs_.avail_in = (uInt)in_n;
        zs_.next_out = out;
        zs_.avail_out = (uInt)out_n;
        return inflate(&zs_, Z_FINISH) == Z_STREAM_END && zs_.avail_out == 0;
    }
    uint32_t crc(const uint8_t *p, size_t n) const { return dl_.crc ? dl_.crc(0, p, n) : (uint32_t)crc32(0L, p, (uInt)n); }

  private:
    const Deflate &dl_;
    void *d_ = nullptr;
    z_stream zs_;
};

struct BgzfIndex {
    const uint8_t *file = nullptr;     // the compressed file, mapped
    std::vector<uint64_t> coff, uoff;  // per block (+ end): compressed / inflated offsets
    std::vector<uint16_t> hdr;         // per block: header bytes before the deflate data
    std::string path;                  // (for error messages)

    uint64_t logical_size() const { return uoff.empty() ? 0 : uoff.back(); }

    // BGZF (bgzip): every block is a gzip member whose extra field 'BC' holds the block size; the last four bytes of a block
    // hold its inflated size.  Returns false (plain gzip) unless the WHOLE file m[0, size) parses as BGZF blocks.
    bool index(const uint8_t *m, uint64_t size, const std::string &file_path) {
        std::vector<uint64_t> co, uo;
        std::vector<uint16_t> hd;
        uint64_t p = 0, u = 0;
        while (p < size) {
            if (p + 18 > size || m[p] != 0x1f || m[p + 1] != 0x8b || m[p + 2] != 8 || !(m[p + 3] & 4)) return false;
            const uint32_t xlen = m[p + 10] | (m[p + 11] << 8);
            uint32_t bsize = 0;
            for (uint32_t q = 0; q + 4 <= xlen;) {  // subfields: SI1 SI2 SLEN(2) data
                const uint8_t *f = m + p + 12 + q;
                if (p + 12 + q + 4 > size) break;
                const uint32_t sl = f[2] | (f[3] << 8);
                if (f[0] == 'B' && f[1] == 'C' && sl == 2 && p + 12 + q + 6 <= size) bsize = (f[4] | (f[5] << 8)) + 1u;
                q += 4 + sl;
            }
            if (!bsize || bsize < 12 + xlen + 8 || p + bsize > size) return false;
            const uint8_t *t = m + p + bsize - 4;
            const uint32_t isize = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
            if (isize > 65536) return false;
            co.push_back(p);
            uo.push_back(u);
            hd.push_back((uint16_t)(12 + xlen));
            p += bsize;
            u += isize;
        }
        if (co.empty()) return false;
        co.push_back(p);
        uo.push_back(u);
        file = m;
        path = file_path;
        coff.swap(co);
        uoff.swap(uo);
        hdr.swap(hd);
        return true;
    }

    // bytes [off, off + n) of the logical file into dst: the blocks that overlap the range; a block wholly inside inflates straight into dst
    void read(uint64_t off, uint64_t n, uint8_t *dst, BlockInflater &inf) const {
        size_t b = (size_t)(std::upper_bound(uoff.begin(), uoff.end(), off) - uoff.begin()) - 1;
        uint8_t tmp[65536];
        const uint64_t end = off + n;
        for (; b + 1 < uoff.size() && uoff[b] < end; ++b) {
            const uint64_t u0 = uoff[b], u1 = uoff[b + 1];
            if (u1 == u0) continue;
            const bool whole = u0 >= off && u1 <= end;
            uint8_t *out = whole ? dst + (u0 - off) : tmp;
            const uint8_t *cin = file + coff[b] + hdr[b];
            const size_t cin_n = (size_t)(coff[b + 1] - coff[b] - hdr[b] - 8);
            if (!inf.inflate_block(cin, cin_n, out, (size_t)(u1 - u0))) throw FeederError("BGZF block corrupt: " + path);
            // the block's CRC-32 (the four bytes before ISIZE): a damaged block of the right length is an error, as for flate2
            const uint8_t *t = file + coff[b + 1] - 8;
            const uint32_t want = t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
            if (inf.crc(out, (size_t)(u1 - u0)) != want) throw FeederError("BGZF block corrupt: " + path);
            if (!whole) {
                const uint64_t a = std::max(u0, off), e = std::min(u1, end);
                memcpy(dst + (a - off), tmp + (a - u0), e - a);
            }
        }
    }
};

// ---------------------------------------------------------------- the input
enum class Kind { Raw, Gzip, Lz4, Bgzf };
enum class Reader { RawChunks, LeanFastq, MappedViews, GzipMembers, InflateStream };

struct Input {
    std::string path;
    bool fastq;
    uint64_t chunk_bytes;  // target raw bytes per chunk
    int threads;           // reader / parser threads
    Kind kind = Kind::Raw;
    int fd = -1;
    uint64_t size = 0;            // of the file the readers see: the inflated ("logical") one for BGZF, the file's own otherwise
    const uint8_t *map = nullptr;  // the file as it is on disk, mapped (BGZF, whole gzip members, mapped views)
    uint64_t map_size = 0;
    size_t n_raw_chunks = 0;  // Raw, Bgzf: chunk i = the records whose first byte lies in [i * chunk_bytes, (i + 1) * chunk_bytes)
    BgzfIndex bgzf;
    Deflate deflate;

    Input(const std::string &path_, bool fastq_, uint64_t chunk_bytes_, int threads_)
        : path(path_), fastq(fastq_), chunk_bytes(chunk_bytes_ < 64 ? 64 : chunk_bytes_), threads(threads_ < 1 ? 1 : threads_) {
        auto ends = [&](const char *t) {
            const size_t n = strlen(t);
            return path.size() >= n && path.compare(path.size() - n, n, t) == 0;
        };
        kind = ends(".gz") ? Kind::Gzip : ends(".lz4") ? Kind::Lz4 : Kind::Raw;
        fd = open(path.c_str(), O_RDONLY);
        if (fd < 0) throw FeederError("Error opening compressed file: " + path);  // get_reader's message (src/main.rs:62)
        struct stat st;
        fstat(fd, &st);
        size = (uint64_t)st.st_size;
        if (kind == Kind::Gzip && size >= 28 && map_file(MAP_PRIVATE)) {
            if (bgzf.index(map, map_size, path)) {
                kind = Kind::Bgzf;  // logical (inflated) size from here on; chunked and read like a raw file
                size = bgzf.logical_size();
            } else {
                unmap_file();
            }
        }
        if (kind == Kind::Raw || kind == Kind::Bgzf) {
            if (chunk_bytes > size + 1) chunk_bytes = size + 1;
            n_raw_chunks = (size_t)((size + chunk_bytes - 1) / chunk_bytes);
        }
    }
    ~Input() {
        unmap_file();
        if (fd >= 0) close(fd);
    }
    Input(const Input &) = delete;

    bool map_file(int flags = MAP_SHARED) {
        const void *m = mmap(nullptr, size, PROT_READ, flags, fd, 0);
        if (m == MAP_FAILED) return false;
        map = (const uint8_t *)m;
        map_size = size;
        return true;
    }
    void unmap_file() {
        if (map) munmap((void *)map, map_size);
        map = nullptr;
    }
    // exactly n bytes of the file at off into dst
    void read(void *dst, uint64_t off, uint64_t n) const { pread_full(fd, dst, n, off, path); }
    const char *stream_name() const { return kind == Kind::Gzip ? "gzip" : "lz4"; }
};

// THE place where the reader is chosen.  leave_unparsed: the consumer finds the records of uncompressed input itself (Feeder::leave_unparsed);
// have_map: the file is mapped, or can be taken to be (asked before the mapping is made: a reader that needs one gives way when mmap fails).
inline Reader choose_reader(const Input &in, const Knobs &k, bool leave_unparsed, bool have_map) {
    switch (in.kind) {
    case Kind::Bgzf: return Reader::RawChunks;  // every reader thread inflates the blocks of its own chunk
    case Kind::Lz4: return Reader::InflateStream;
    case Kind::Gzip: {
        // a plain gzip file: members inflated whole into a buffer of their own -- large ones by all threads, round by round, the
        // pages of a round given back as soon as the parsers have copied its records out (memory stays bounded whatever the
        // file's size); with a single thread a member is one libdeflate call whose whole output has to be resident, so files
        // beyond MQ_GZ_WHOLE_LIMIT then stream through zlib
        const bool par_possible = !k.gz_whole_limit_set && in.threads >= 2 && k.pargz;
        const bool whole = in.deflate.ok() && in.size > 0 && (in.size <= k.gz_whole_limit || par_possible) && have_map;
        return whole ? Reader::GzipMembers : Reader::InflateStream;
    }
    case Kind::Raw: break;
    }
    // records found by the consumer: the chunked reader hands the file's bytes over as they are -- or, as an experiment, views of the mapping
    if (leave_unparsed) return !in.fastq && in.size > 0 && k.mapped_fasta && have_map ? Reader::MappedViews : Reader::RawChunks;
    return in.fastq && in.size > 0 && !k.no_lean_fastq ? Reader::LeanFastq : Reader::RawChunks;
}

}  // namespace feeder
}  // namespace mapquik
