// feeder_gzip.hpp -- the readers of compressed streams (read feeder, fastx_feeder.hpp): one worker inflates and cuts the bytes into chunks
// at record boundaries, the parser threads parse them.  gzip and lz4 streams go through zlib / liblz4 straight into chunks; plain gzip
// with libdeflate at hand is inflated member by member (a large member by all threads, par_gzip.hpp).  (BGZF is read like a raw file:
// feeder_raw.hpp.)
#pragma once
#include <zlib.h>

#include <chrono>
#include <cstdio>
#include <memory>
#include <vector>

#include "feeder_input.hpp"
#include "feeder_queue.hpp"

namespace mapquik {
namespace feeder {

// a parser thread: chunks filled by the inflating worker -> parsed chunks
inline void parse_worker(ChunkQueue &q, const Input &in) {
    while (Chunk *c = q.take_for_parse()) {
        if (c->ext_src) {  // whole-member gzip reader: the bytes come out of the member's inflate buffer here, in parallel
            memcpy(c->buf, c->ext_src, c->bytes);
            // the whole pages of this range are not needed again (the inflater keeps its own copy of the last 32 KB): back to
            // the system, so that a member of any size costs the memory of the rounds in flight
            const uintptr_t pa = ((uintptr_t)c->ext_src + 4095u) & ~(uintptr_t)4095u, pb = ((uintptr_t)c->ext_src + c->bytes) & ~(uintptr_t)4095u;
            if (pb > pa) madvise((void *)pa, pb - pa, MADV_DONTNEED);
            c->ext_src = nullptr;
            c->ext_hold.reset();
        }
        parse_chunk(*c, in.fastq);
        q.publish(c);
    }
}

// gzip (zlib) or lz4 stream: one thread inflates into chunks cut at record boundaries
inline void inflate_stream_reader(ChunkQueue &q, const Input &in) {
    std::vector<uint8_t> src(4u << 20);
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    std::unique_ptr<Lz4> lz;
    struct ZEnd {  // inflateEnd on every way out (an exception on a corrupt or truncated stream included)
        z_stream *z = nullptr;
        ~ZEnd() { if (z) inflateEnd(z); }
    } zend;
    if (in.kind == Kind::Gzip) {
        if (inflateInit2(&zs, 15 + 32) != Z_OK) throw FeederError("inflateInit2 failed");
        zend.z = &zs;
    } else {
        lz.reset(new Lz4());
    }
    const uint64_t cap_need = in.chunk_bytes + in.chunk_bytes / 8 + (1u << 20);
    Chunk *c = q.get_buffer(cap_need);
    size_t seq = 0;
    uint64_t file_pos = 0;
    size_t in_have = 0, in_pos = 0;
    bool mid_stream = false;  // inside a gzip member / an lz4 frame: the input may not end here (flate2's UnexpectedEof)
    auto cut_and_queue = [&](bool final) {
        // keep whole records in c, carry the incomplete last one to a fresh chunk
        Chunk *nxt = nullptr;
        if (!final) {
            // the last sure record start in the second half of the buffer
            const uint64_t keep = last_sure_record_start(c->buf, c->bytes / 2, c->bytes, in.fastq);
            if (keep == NEED_MORE || keep == 0) throw FeederError("a single record does not fit a chunk: raise --batch-bases");
            nxt = q.get_buffer(cap_need);
            memcpy(nxt->buf, c->buf + keep, c->bytes - keep);
            nxt->bytes = c->bytes - keep;
            c->bytes = keep;
        }
        c->seq_no = seq++;
        q.queue_for_parse(c);
        c = nxt;
    };
    for (;;) {
        if (in_pos == in_have) {
            const ssize_t r = pread(in.fd, src.data(), src.size(), (off_t)file_pos);
            if (r < 0) throw FeederError("read error: " + in.path);
            if (r == 0) {
                if (mid_stream) throw FeederError(std::string(in.stream_name()) + " stream truncated: " + in.path);
                break;
            }
            file_pos += (uint64_t)r;
            in_have = (size_t)r;
            in_pos = 0;
        }
        while (in_pos < in_have) {
            if (c->bytes + (1u << 16) > c->cap - 64 || c->bytes >= in.chunk_bytes) cut_and_queue(false);
            size_t produced = 0, consumed = 0;
            if (in.kind == Kind::Gzip) {
                zs.next_in = src.data() + in_pos;
                zs.avail_in = (uInt)(in_have - in_pos);
                zs.next_out = c->buf + c->bytes;
                zs.avail_out = (uInt)std::min<uint64_t>(c->cap - 64 - c->bytes, 1u << 30);
                const uInt out0 = zs.avail_out;
                const int rc = inflate(&zs, Z_NO_FLUSH);
                consumed = (in_have - in_pos) - zs.avail_in;
                produced = out0 - zs.avail_out;
                if (rc == Z_STREAM_END) {
                    mid_stream = false;
                    if (zs.avail_in > 0 || file_pos < in.size) inflateReset(&zs);  // concatenated gzip members
                } else if (rc != Z_OK && rc != Z_BUF_ERROR) {
                    throw FeederError("gzip stream corrupt: " + in.path);
                } else if (consumed || produced) {
                    mid_stream = true;
                }
            } else {
                size_t dst = (size_t)(c->cap - 64 - c->bytes), n_src = in_have - in_pos;
                const size_t rc = lz->decompress(lz->ctx, c->buf + c->bytes, &dst, src.data() + in_pos, &n_src, nullptr);
                if (lz->is_error(rc)) throw FeederError("lz4 stream corrupt: " + in.path);
                consumed = n_src;
                produced = dst;
                mid_stream = rc != 0;  // LZ4F_decompress returns 0 exactly when a frame is complete
            }
            in_pos += consumed;
            c->bytes += produced;
            if (!consumed && !produced) break;
        }
    }
    cut_and_queue(true);
}

// Plain gzip, member by member: a member is inflated whole into a huge-page buffer (behind the unfinished record the previous
// member may have ended with), cut into chunk-sized ranges at record boundaries, and the ranges are handed to the parser
// threads, which copy them into page-locked chunk buffers and parse them.  A large member is inflated by all threads
// (par_gzip.hpp: block starts found by search, 16-bit symbols, windows resolved afterwards) and its ranges go to the parsers
// round by round while the next round inflates; a small one by one libdeflate call.
struct GzipMemberReader {
    ChunkQueue &q;
    const Input &in;
    const Knobs &knobs;
    const bool par_on;
    std::unique_ptr<void, void (*)(void *)> d;  // libdeflate decompressor of the one-call members
    size_t seq = 0;
    std::vector<uint8_t> carry;  // the previous member's unfinished last record
    // the member at hand
    std::shared_ptr<BigBuf> big;  // carry + the member's inflated bytes
    uint64_t a = 0;               // start of the bytes of big not yet handed to a parser
    size_t ain = 0, aout = 0;     // the member's compressed / inflated bytes

    GzipMemberReader(ChunkQueue &q_, const Input &in_, const Knobs &k)
        : q(q_), in(in_), knobs(k), par_on(k.pargz && in_.threads >= 2), d(in_.deflate.alloc(), in_.deflate.free_) {
        if (!d) throw FeederError("libdeflate: no decompressor");
    }

    void run() {
        uint64_t p = 0;
        bool prev_small = false;  // a file of many small members: do not start a round of threads for each
        while (p < in.size) {
            if (in.size - p < 18 || in.map[p] != 0x1f || in.map[p + 1] != 0x8b) throw FeederError("gzip stream truncated or corrupt: " + in.path);
            inflate_member(p, prev_small);
            prev_small = ain < knobs.pargz_min;
            const uint64_t total = carry.size() + aout;
            carry.clear();
            p += ain;
            cut_member(total, p >= in.size);
        }
        if (!carry.empty()) {  // (cannot happen: the last member's tail is cut with at_eof) -- never drop bytes silently
            Chunk *c = q.get_buffer(carry.size() + 64, true);
            memcpy(c->buf, carry.data(), carry.size());
            c->begin = 0;
            c->bytes = carry.size();
            c->seq_no = seq++;
            q.queue_for_parse(c);
        }
    }

    // bytes [from, to) of big to a parser thread
    void hand_over(uint64_t from, uint64_t to) {
        Chunk *c = q.get_buffer(to - from + 64, (to - from + 64) > in.chunk_bytes + in.chunk_bytes / 8 + (1u << 20));
        c->begin = 0;
        c->bytes = to - from;
        c->ext_src = big->p + from;
        c->ext_hold = big;
        c->seq_no = seq++;
        q.queue_for_parse(c);
    }

    // ------------------------------------------------------------ reservation and retry ladder
    // The member at file offset p inflated into a fresh `big` behind the carry: sets ain, aout (and a: the all-threads inflater's
    // rounds are cut into ranges as they complete).
    void inflate_member(uint64_t p, bool prev_small) {
        const uint64_t rest = in.size - p;
        const bool par_ok = par_on && rest >= knobs.pargz_min;
        bool par = par_ok && !prev_small;
        // address space; pages exist once written.  All threads: what deflate can expand to at most (1032 : 1), within 16 TB (but
        // 64 : 1 at least), since pages behind the parsers go back to the system; one call: 12 : 1, doubled when it was not enough.
        // A one-call attempt made only because the PREVIOUS member was small is bounded (a small member fits 16 x par_min): a
        // member that does not fit is a large one after all and goes to all threads, so that a tiny first member in front of a
        // multi-GB one does not make the large one inflate fully resident.
        auto cap_for = [&](bool all_threads) -> uint64_t {
            if (all_threads) return std::max<uint64_t>(64 * rest, std::min<uint64_t>(1100 * rest, 16ull << 40)) + carry.size();
            const uint64_t one = std::max<uint64_t>(64u << 20, 12 * rest);
            return (par_ok ? std::min<uint64_t>(one, std::max<uint64_t>(64u << 20, 16 * knobs.pargz_min)) : one) + carry.size();
        };
        uint64_t cap = cap_for(par);
        ain = aout = 0;
        a = 0;
        for (;;) {
            for (;;) {  // a refused reservation (strict overcommit accounting) is asked for again at a quarter, down to 2 x the rest of the file
                try {
                    big = std::make_shared<BigBuf>(cap + 64);
                    break;
                } catch (const FeederError &) {
                    if (cap / 4 < 2 * rest + carry.size() + (64u << 20)) throw;
                    cap /= 4;
                }
            }
            if (!carry.empty()) memcpy(big->p, carry.data(), carry.size());
            const auto tt0 = std::chrono::steady_clock::now();
            const int rc = par ? inflate_by_all_threads(p, cap) : in.deflate.gzip_ex(d.get(), in.map + p, (size_t)rest, big->p + carry.size(), (size_t)(cap - carry.size()), &ain, &aout);
            if (knobs.timing) fprintf(stderr, "gzip member (%s): rc %d, %zu -> %zu bytes in %.3f s\n", par ? "all threads" : "libdeflate", rc, ain, aout, std::chrono::duration<double>(std::chrono::steady_clock::now() - tt0).count());
            if (rc == 0) return;
            if (rc != 3 || cap > (1ull << 37)) throw FeederError("gzip stream truncated or corrupt: " + in.path);
            if (!par && par_ok) {  // not a small member after all
                par = true;
                cap = cap_for(true);
                continue;
            }
            cap *= 2;  // insufficient space: a member compressed better than expected
        }
    }
    // libdeflate's result codes: 0 done, 3 the member expands beyond cap (and nothing of it was handed over yet: it can be done again)
    int inflate_by_all_threads(uint64_t p, uint64_t cap) {
        pargz::Options o;
        o.threads = in.threads;
        o.seg_bytes = knobs.pargz_seg;
        o.min_seg_bytes = knobs.pargz_minseg;
        o.timing = knobs.timing;
        o.crc_fn = in.deflate.crc;
        try {
            pargz::MemberInflater inf(in.map + p, in.size - p, o);
            uint64_t produced = 0;
            ain = (size_t)inf.run(big->p + carry.size(), cap - carry.size(), &produced, [&](uint64_t so_far, bool finished) {
                if (!finished) cut_round(carry.size() + so_far);  // the member's tail is cut by cut_member, where it is known whether more members follow
            });
            aout = (size_t)produced;
        } catch (const pargz::Error &e) {
            const bool space = strncmp(e.what(), "space", 5) == 0;
            if (space && a == 0) return 3;
            throw FeederError(std::string(space ? "gzip member expands beyond the buffer" : e.what()) + ": " + in.path);
        }
        return 0;
    }

    // ------------------------------------------------------------ cutting of ranges
    // while the member still inflates, big[0, avail) valid: ranges that end at a record start found with bytes to spare
    void cut_round(uint64_t avail) {
        while (a + in.chunk_bytes < avail) {
            const uint64_t b = next_record_start(big->p, a + in.chunk_bytes, avail, in.fastq, false);
            if (b == NEED_MORE || b >= avail) break;
            hand_over(a, b);
            a = b;
        }
    }
    // the whole member, big[0, total): ranges [a, b), b = the first record start at or after a + chunk_bytes (the end of the data in the
    // last member); what may be an unfinished record at the end of another member becomes the carry
    void cut_member(uint64_t total, bool last_member) {
        while (a < total) {
            uint64_t b = total;
            if (a + in.chunk_bytes < total) {
                const uint64_t r = next_record_start(big->p, a + in.chunk_bytes, total, in.fastq, last_member);
                b = (r == NEED_MORE) ? total : r;
            }
            if (b >= total && !last_member) {
                // the tail may hold an unfinished record: keep everything from the last sure record start for the next member
                const uint64_t lastrec = last_sure_record_start(big->p, a, total, in.fastq);
                if (lastrec == NEED_MORE || lastrec <= a) {
                    // no further record start inside [a, total): all of it is carry (a == 0: the whole member is (part of) one record)
                    carry.assign(big->p + a, big->p + total);
                    break;
                }
                carry.assign(big->p + lastrec, big->p + total);
                b = lastrec;
            }
            hand_over(a, b);
            a = b;
        }
    }
};

}  // namespace feeder
}  // namespace mapquik
