/*
 * mapquik_hip.h -- C ABI of the MI355X (gfx950) implementation of mapquik's hot path:
 * k-min-mer seeding -> unique-k-min-mer index lookup -> Match runs -> pseudo-chain -> PAF columns.
 *
 * This is the drop-in boundary.  The reference (ekimb/mapquik, Rust) has no FFI of its own; the
 * internal seam these entry points replace is the pair called from the seq_io worker closures
 * (src/closures.rs:46-51,100-104):
 *     mers::ref_extract (ref_idx, &[u8], &Params, &Index) -> usize            src/mers.rs:15
 *     mers::find_matches(q_id, q_len, &[u8], &ref_map, &ReadOnlyIndex, &Params) -> Option<String>   src/mers.rs:77
 * in batch form (many sequences per call), with plain pointers and sizes only.
 * INTEGRATION.md shows the `extern "C"` block a Rust maintainer would add.
 *
 * Conventions
 *   - Sequences are bytes exactly as the reference's seam receives them: upper-cased ASCII
 *     (src/closures.rs:63,106).  Any byte other than A,C,G,T hashes as ntHash seed 0.
 *   - All functions return 0 (or a non-negative count) on success and a negative MQ_E* code on error;
 *     mq_last_error() returns a thread-local message.  Nothing throws across the boundary.
 *   - The caller owns every buffer it passes; the library owns device memory behind mq_index.
 *   - The compute path is HIP only.  There is no CPU fallback: without a usable GPU every compute entry
 *     point fails with MQ_ENODEVICE.
 *   - Limits (checked, MQ_EINVAL otherwise): 1 <= l <= 64, 1 <= k <= 32, sequence length < 2^32, fewer than 2^30 reads per batch.
 */
#ifndef MAPQUIK_HIP_H
#define MAPQUIK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MQ_ABI_VERSION 4

#define MQ_OK 0
#define MQ_EINVAL (-1)
#define MQ_ENODEVICE (-2)
#define MQ_EHIP (-3)
#define MQ_ENOMEM (-4)
#define MQ_ESTATE (-5)
#define MQ_EOVERFLOW (-6)

/* Params (src/main.rs:33-47); defaults src/main.rs:174-188.  I/O-only members (b, q, threads, debug) are host-side. */
typedef struct mq_params {
    uint32_t k;       /* k-min-mer length, default 5 */
    uint32_t l;       /* minimizer length, default 31 */
    double   density; /* FH density, default 0.01 */
    uint32_t use_hpc; /* 1 unless --nohpc */
    uint32_t c;       /* minimum chain length, default 4 */
    uint32_t s;       /* minimum matching seeds, default 11 */
    uint32_t g;       /* maximum gap difference, default 2000 */
    uint32_t flags;   /* MQ_FLAG_*; default 0 */
} mq_params;
/* The reference upper-cases every sequence before the seam (to_ascii_uppercase, src/closures.rs:63,106).  With this flag the
 * kernels treat a-z as A-Z themselves, so a feeder can hand over raw FASTX bytes without touching them. */
#define MQ_FLAG_FOLD_CASE 1u
/* Opt-in: a cheap k-min-mer tuple hash in place of the reference's SipHash-1-3 (Rust DefaultHasher over the tuple, src/index.rs:100-104 via
 * the crate's KminmerHash).  The PAF depends on that hash only through EQUALITY (index hit / miss / duplicate, src/index.rs:118-126,
 * src/match.rs:39-58), so the lines are the same; mq_kminmer.hash is then NOT the reference's value.  An add-rotate-xor chain on two 64-bit
 * words (one step per minimizer, six to finish; the test suite's CPU checker has the same function).  The index and the reads must be hashed
 * alike: the flag belongs to the seeding parameters (a saved index carries it).  Default off; never used for a headline number. */
#define MQ_FLAG_FAST_KH 2u
/* Seeding variants (flags bits 8..13; default 0 = the frozen reading of DESIGN.md section 2).  The k-min-mer iterator is a third-party
 * crate (rust-seq2kminmers, Cargo.toml:30, no pinned revision; call sites src/mers.rs:22-27,53) that this image cannot build, so
 * six of its decisions are switchable: tools/check_against_upstream.sh finds, on a machine with cargo, which combination reproduces
 * the crate, and the product is then run with that value (`mapquik --seeding-variant v`).  Bits, any combination:
 *    1  D3      strict `<` on the density bound (frozen: `<=`)
 *    2  D2      FH = f32: the bound is computed in single precision
 *    4  D2/D12  H = u32: 32-bit ntHash (low halves of the seeds, rotations mod 32) and a 32-bit bound -- what a 16-lane AVX-512
 *               HashMode::HpcSimd (the reference's default mode, src/mers.rs:22) may use; hashes are zero-extended into the tuple
 *    8  D5      a minimizer's position = raw index of the LAST base of its first base's homopolymer run (frozen: the run head); needs l >= 2
 *   16  D6      end = raw position of the last compressed base of the last minimizer's l-mer (frozen: pos[k-1] + l - 1)
 *   32  D8      rev = reversed tuple <= forward tuple (frozen: strict <; differs on palindromic tuples only)
 * mq_index_new rejects undefined bits and unsupported combinations with MQ_EINVAL. */
#define MQ_FLAG_SEED_VARIANT_SHIFT 8
#define MQ_FLAG_SEED_VARIANT_MASK (0x3Fu << MQ_FLAG_SEED_VARIANT_SHIFT)
#define MQ_FLAG_SEED_VARIANT(v) (((uint32_t)(v) & 0x3Fu) << MQ_FLAG_SEED_VARIANT_SHIFT)
#define MQ_SEEDVAR_STRICT_BOUND 1u
#define MQ_SEEDVAR_F32_BOUND 2u
#define MQ_SEEDVAR_HASH32 4u
#define MQ_SEEDVAR_POS_RUN_END 8u
#define MQ_SEEDVAR_END_COMPRESSED 16u
#define MQ_SEEDVAR_REV_ON_EQUAL 32u

/* One k-min-mer as the reference's KminmerHash exposes it (fields used at src/index.rs:57-58,101). 24 bytes. */
typedef struct mq_kminmer {
    uint64_t hash;
    uint32_t start;
    uint32_t end;
    uint32_t offset;
    uint32_t rev;
} mq_kminmer;

/* Result of find_matches for one read: the numeric PAF columns of src/mers.rs:181.  48 bytes.
 * status 0 => the reference returns None (no line is written, src/closures.rs:119-121).
 * Columns 3 and 4 are 64-bit (low word, high word): find_coords computes in usize and a run that the Match::check precedence
 * quirk (src/match.rs:39-43) extended onto ANOTHER, longer reference makes `r_len - r_end - 1` wrap (src/mers.rs:131-183; release
 * builds wrap silently), so the reference prints values like 18446744073709547279 there -- and so does mq_format_paf. */
#define MQ_HIT_UNMAPPED 0u
#define MQ_HIT_MAPPED 1u
#define MQ_HIT_OVERFLOW 2u /* more Match runs than the per-read scratch holds: result NOT computed (loud, never silent) */
typedef struct mq_hit {
    uint32_t status;
    uint32_t ref_id;     /* index passed to mq_index_add_ref */
    uint32_t rc;         /* 1 => '-' */
    uint32_t mapq;       /* 0 or 60 */
    uint32_t q_start;    /* column 3, low 32 bits */
    uint32_t q_end;      /* column 4 (inclusive, as the reference prints it), low 32 bits */
    uint32_t r_start;    /* column 8 */
    uint32_t r_end;      /* column 9 (inclusive) */
    uint32_t score;      /* column 10: number of matching k-min-mers */
    uint32_t n_kminmers; /* k-min-mers extracted from the read (diagnostic) */
    uint32_t q_start_hi; /* column 3, high 32 bits (0 unless the usize arithmetic of find_coords wrapped) */
    uint32_t q_end_hi;   /* column 4, high 32 bits */
} mq_hit;

/* The Match runs of a mapped read's winning pseudo-chain (opt-in: mq_ctx_reserve_anchors below) -- what Chain::filter_matches_max leaves
 * (src/chain.rs:123-129), of which the hit keeps the first and the last.  A Match of src/match.rs as the chain holds it: raw coordinates,
 * q_end / r_end as Match stores them (get_match subtracts 1), BEFORE find_coords; strand and reference are the hit's (every kept run has the
 * anchor's strand or equals it field by field). */
typedef struct mq_anchor {
    uint32_t q_start, q_end, r_start, r_end, count;
} mq_anchor; /* 20 bytes */
typedef struct mq_anchor_span {
    uint32_t first, count; /* read r's anchors: pool[first .. first + count), in read order */
} mq_anchor_span;
#define MQ_ANCHORS_DROPPED 0xFFFFFFFFu /* mq_anchor_span::first of a mapped read whose anchors found no room in the pool (count is still right) */

/* Every candidate pseudo-chain of a read (opt-in: mq_ctx_reserve_chains below): one per reference that has at least one Match run in
 * the read -- what find_matches builds and find_largest_two_chains looks through (src/mers.rs:77-129), of which the hit is the strictly
 * largest.  48 bytes, field for field the layout of mq_hit: the unique top chain of a mapped read equals the read's mq_hit in every word
 * but word 9 (n_runs here, n_kminmers there), and its flags == MQ_CHAIN_TOP == MQ_HIT_MAPPED.
 * Order: a read's chains are listed in the order of each reference's first run in the read.  The reference keeps its chains in a HashMap,
 * whose order is unspecified: this is one of its legal orders.
 * Ties: a read is mapped <=> exactly one of its chains has MQ_CHAIN_TOP (find_largest_two_chains + determine_best_match: a tie <=> the top
 * score occurs twice); a tied read has status MQ_HIT_UNMAPPED and two or more TOP chains. */
#define MQ_CHAIN_TOP 1u /* mq_chain::flags: no chain of this read scores higher */
typedef struct mq_chain {
    uint32_t flags;
    uint32_t ref_id, rc, mapq; /* mapq by get_match's own rule for THIS chain (c, s; src/chain.rs:158-161) */
    uint32_t q_start, q_end, r_start, r_end; /* after find_coords against THIS chain's reference length (low words of columns 3 and 4) */
    uint32_t score;            /* sum of the kept runs' counts */
    uint32_t n_runs;           /* len_f: runs filter_matches_max left */
    uint32_t q_start_hi, q_end_hi; /* high words of columns 3 and 4, as in mq_hit */
} mq_chain;
typedef struct mq_chain_span {
    uint32_t first, count; /* read r's chains: pool[first .. first + count) */
} mq_chain_span;
#define MQ_CHAINS_DROPPED 0xFFFFFFFFu /* mq_chain_span::first of a read whose chains found no room in the pool (count is still right) */

typedef struct mq_index mq_index; /* opaque: Index / ReadOnlyIndex (src/index.rs:73-128) + ref_map (src/closures.rs:30) */

typedef struct mq_index_stats {
    uint64_t n_refs;
    uint64_t n_kminmers;  /* total inserted, sum of mq_index_add_ref returns */
    uint64_t n_keys;      /* distinct hashes (incl. tombstones) */
    uint64_t n_unique;    /* Index::get_count(): non-tombstones (src/index.rs:90-92) */
    uint64_t table_slots; /* power of two */
    uint64_t table_bytes;
    uint64_t slot_bytes;
} mq_index_stats;

const char *mq_last_error(void);
int mq_abi_version(void);
/* number of HIP devices visible; 0 or negative => no compute possible */
int mq_device_count(void);
void mq_params_default(mq_params *p); /* src/main.rs:174-188 */

/* Index::new (src/index.rs:78-88) on HIP device `device`. */
mq_index *mq_index_new(const mq_params *params, int device);
void mq_index_free(mq_index *idx);

/* index_mers closure (src/closures.rs:46-51) = ref_extract (src/mers.rs:15-38) + ref_map.insert.
 * Returns the number of k-min-mers of this reference (the "Indexed reference {}: {} k-min-mers." count) or <0.
 * ref_id values must be distinct; seq is host memory (mq_index_add_ref) or device memory (.._device). */
int64_t mq_index_add_ref(mq_index *idx, uint32_t ref_id, const char *name, const uint8_t *seq, uint64_t len);
int64_t mq_index_add_ref_device(mq_index *idx, uint32_t ref_id, const char *name, const uint8_t *d_seq, uint64_t len);

/* The reference file handed over in pieces (the batch form of the reader loop of src/closures.rs:46-94 for a caller that never holds a
 * whole record in host memory): the file's bytes go to a device buffer of the index piece by piece, asynchronously, and a record is
 * indexed from there while the pieces behind it are still on their way.
 *   mq_index_stage_begin(idx, total_bytes)       the device buffer, total_bytes = the file's size; once per index, before the first piece
 *   mq_index_stage_piece(idx, at, src, n, &t)    queues the copy of src[0, n) to buffer offset `at` and returns; src (page-locked memory,
 *                                                mq_host_alloc, for the link's full rate) must stay untouched until
 *   mq_index_stage_done(idx, t, wait)            returns 1 (copied; src may be reused), 0 (not yet; only with wait == 0) or <0
 *   mq_index_add_ref_staged(idx, id, name, at, len, t)  = mq_index_add_ref_device on buffer[at, at + len), ordered (on the device) behind
 *                                                piece t and every piece issued before it -- the last piece that holds bytes of the
 *                                                record -- or, t = MQ_STAGE_ALL_ISSUED, behind every piece issued so far
 * Pieces may be issued from one thread while another asks for records.  The buffer is released by mq_index_finalize. */
#define MQ_STAGE_ALL_ISSUED (~(uint64_t)0)
int mq_index_stage_begin(mq_index *idx, uint64_t total_bytes);
int mq_index_stage_piece(mq_index *idx, uint64_t at, const uint8_t *src, uint64_t n, uint64_t *ticket);
int mq_index_stage_done(mq_index *idx, uint64_t ticket, int wait);
int64_t mq_index_add_ref_staged(mq_index *idx, uint32_t ref_id, const char *name, uint64_t at, uint64_t len, uint64_t after_ticket);
/* mq_index_add_ref_staged for a record whose sequence is spread over lines: buffer[at, at + bytes) is everything between the
 * header's line end and the next record's '>' (or the end of the file).  The lines are joined on the device -- the region is split at
 * every '\n', one trailing '\r' is cut from each piece (the last one, which has no '\n', included), the pieces are concatenated; every
 * other byte is kept as it is -- and the result is indexed as mq_index_add_ref_device would index it.  *seq_len (may be NULL) receives
 * the joined length: the reference's length in mq_index_ref_info and in PAF columns 7 / 11.  Returns the k-min-mer count or <0. */
int64_t mq_index_add_ref_staged_lines(mq_index *idx, uint32_t ref_id, const char *name, uint64_t at, uint64_t bytes,
                                      uint64_t after_ticket, uint64_t *seq_len);
/* Parity/debug: the joined bytes themselves, copied to host memory; returns the joined length (out may be NULL when cap == 0: the
 * length alone), MQ_EINVAL when it exceeds cap (nothing is written then). */
int64_t mq_index_staged_sequence(mq_index *idx, uint64_t at, uint64_t bytes, uint64_t after_ticket, uint8_t *out, uint64_t cap);

/* DashMap::with_capacity (src/index.rs:83 sizes its map for 39,821,990 k-min-mers at Index::new): a hint that about
 * expected_kminmers k-min-mers will be inserted.  The table is allocated and cleared in the background while the references are
 * added; mq_index_finalize adopts it when the size fits and allocates anew when it does not.  Fresh device memory costs ~30 ms per GB
 * here (0.5 s for a human genome's table): call this as early as the reference's size is known.  One reservation per index. */
int mq_index_reserve(mq_index *idx, uint64_t expected_kminmers);
/* Slots of the table per inserted k-min-mer (2..64, rounded up to a power of two of slots; default 8: load <= 1/8, the fastest lookups
 * for a kernel fed from HBM).  A caller bound by its host side (files -> PAF runs at a thirtieth of the kernel's rate) takes 2: a
 * quarter of the memory per replica and of its allocation, for 5 % of kernel speed it never sees.  Before mq_index_reserve / finalize. */
int mq_index_set_table_factor(mq_index *idx, uint32_t slots_per_kminmer);
/* get_count + into_read_only (src/closures.rs:92-94): dedup (a hash seen twice is a tombstone,
 * src/index.rs:94-104), build the HBM-resident table.  Returns the unique count or <0. */
int64_t mq_index_finalize(mq_index *idx);
int mq_index_get_stats(const mq_index *idx, mq_index_stats *out);
/* On-disk form of a finalized index (the reference has none: it re-indexes the FASTA on every run, src/closures.rs:24-94).
 * The file holds the parameters, the reference names/lengths and the slot table; mq_index_load returns a finalized index. */
int mq_index_save(const mq_index *idx, const char *path);
mq_index *mq_index_load(const char *path, int device);
/* A replica of a finalized index on HIP device `device` (device-to-device copy of the table; the multi-GPU drivers build the
 * index once and clone it instead of indexing the reference on every GPU).  Free it with mq_index_free. */
mq_index *mq_index_clone(const mq_index *src, int device);
/* A finalized index kept and maintained (the on-disk index is this library's own: the reference re-indexes on every run).
 * The table is order independent -- a slot is claimed once, and a key that arrives again only ever sets its tombstone bit -- so adding
 * references to a populated table gives the table that a build from all references at once gives, and a table can be rebuilt at any
 * other legal size from its own occupied slots.
 *   mq_index_reopen(idx)     a finalized index (built, loaded or cloned) takes mq_index_add_ref* again, by every route, with reference ids
 *                            distinct from the ones it has.  Waits for the device first.  Until the next mq_index_finalize every mapping
 *                            entry point answers MQ_ESTATE, as for any index that is not finalized.  MQ_ESTATE when idx is not finalized.
 *   mq_index_finalize(idx)   on a reopened index inserts the NEW references' k-min-mers into the existing table: no earlier reference is
 *                            seeded or inserted again.  The table grows first (on the device, table to table; peak memory: both
 *                            tables) when all k-min-mers together ask for a larger one than it has, and never shrinks; the counts are
 *                            brought up to date from the insert's own counters (a new reference may turn an old unique key dead).
 *                            Contexts made before the reopen stay valid, with their reservations and redo arenas, and map against the
 *                            new table afterwards.  The growth follows the index's table factor, and a loaded or cloned index has the
 *                            default (8) whatever size its table has: a caller that wants another calls mq_index_set_table_factor
 *                            between mq_index_reopen and mq_index_finalize.  A finalize that fails before anything was inserted (no
 *                            memory for the larger table, say) leaves the index open with its new references: it may be called
 *                            again.  One that fails later has left part of the new keys in the table, and a second insertion would
 *                            turn them dead: from then on mq_index_finalize and mq_index_add_ref* answer MQ_ESTATE and the index can
 *                            only be freed (a build from scratch retries into a new table; an extension has no second table).
 *   mq_index_resize(idx, table_slots, slots_per_kminmer)   the finalized index's table rebuilt at another size, on the device; waits for
 *                            the device first.  Contexts stay valid.  Peak memory: the old table plus the new one.
 *   mq_index_load_sized(path, device, table_slots, slots_per_kminmer)   mq_index_load with the file's slots scattered straight into a
 *                            table of the chosen size (a table of the file's own size is never allocated).  Every refusal of
 *                            mq_index_load stays; a size that does not exceed the file's key count is refused too.
 *   mq_index_clone_sized(src, device, table_slots, slots_per_kminmer)   mq_index_clone with a table of the chosen size on the destination:
 *                            the occupied slots are packed on the source device and 32 bytes per key cross the link, not the table.
 * The size arguments, the same in the three sized calls -- at most one of them non-zero:
 *   table_slots         an exact size: a power of two in [2, 2^40] and greater than n_keys (a table without an empty slot would make a
 *                       miss walk forever)
 *   slots_per_kminmer   2..64: the size a build of n_kminmers k-min-mers gets at that factor (mq_index_set_table_factor), raised if need
 *                       be to the smallest legal size
 *   both 0              as it is: mq_index_resize does nothing, the other two behave exactly like mq_index_load / mq_index_clone
 * Anything else is MQ_EINVAL, checked before anything is allocated: the index is then untouched and usable. */
int mq_index_reopen(mq_index *idx);
int mq_index_resize(mq_index *idx, uint64_t table_slots, uint32_t slots_per_kminmer);
mq_index *mq_index_load_sized(const char *path, int device, uint64_t table_slots, uint32_t slots_per_kminmer);
mq_index *mq_index_clone_sized(const mq_index *src, int device, uint64_t table_slots, uint32_t slots_per_kminmer);
/* Another finished index taken in.  Merging src into dst with source reference id i becoming id_base + i ends exactly where one
 * mq_index_new + mq_index_add_ref of all of dst's references (under their ids) and all of src's (under the moved ids) +
 * mq_index_finalize ends: the same key set; the same live set (a key live in both turns dead, a key dead in either is dead); for every
 * live key the same payload with the id moved; n_kminmers = the sum, n_keys = the distinct keys, n_unique = the live keys; the same
 * reference names and lengths.  A dead key's payload is unspecified, as everywhere.  The argument is the one of the extension above: an
 * occupied slot re-inserted as (key, first payload, once / more than once) is all another table needs.
 *   mq_index_merge(dst, src, id_base)        both finalized, dst != src.  On one device the source table is streamed straight into dst's
 *                            table; across devices the occupied slots are packed on src's device and 32 bytes per key cross the link
 *                            (as mq_index_clone_sized sends them).  src is only read.
 *   mq_index_merge_file(dst, path, id_base)  the same from a file mq_index_save wrote: its slots are streamed in bounded chunks through a
 *                            device buffer; the file's own table is never allocated.  Before the first insert one pass over the file's
 *                            slots applies mq_index_load's per-slot checks (a count of 0, a key 0 outside its slot, is_key0 > 1, an id the
 *                            file's reference table does not have) and holds the live slots against the header's n_unique.  One
 *                            corruption is out of a merge's reach: the same key in two slots of the file, which mq_index_load catches by
 *                            recounting an otherwise empty table -- such a file behaves as if the key had been inserted twice.
 * Both wait for the device first (as mq_index_reopen and mq_index_resize do) and answer MQ_ESTATE when dst or src is not finalized or
 * a context of dst has a submitted batch that was not waited for.  Refused with MQ_EINVAL, dst untouched and usable: seeding parameters
 * that differ (k, l, density, use_hpc, the seeding-variant bits, MQ_FLAG_FAST_KH; mq_last_error names both sets -- c, s, g and the case
 * folding stay dst's); a moved id that reaches 2^24 or is already an id of dst; dst == src; everything mq_index_load refuses.
 * The table grows first (mq_index_resize's route; peak memory: both tables) when the summed n_kminmers ask for a larger one at the
 * index's table factor (mq_index_finalize's rule for a reopened index), and never shrinks.  A failure up to there (no memory for the
 * larger table or the chunk buffer) leaves dst finalized and usable; one behind the first insert launch has changed the only table there
 * is, and dst answers MQ_ESTATE to everything but mq_index_free.  Afterwards dst is finalized, its contexts stay valid, and
 * mq_index_save of it is loadable. */
int mq_index_merge(mq_index *dst, const mq_index *src, uint32_t id_base);
int mq_index_merge_file(mq_index *dst, const char *path, uint32_t id_base);
/* Index coverage: which bases of which reference the live k-min-mers of a finalized index span, and how many live k-min-mers each
 * reference owns -- what extending, resizing and merging an index can silently change (a decoy that repeats a key of chr1 kills it for
 * both), and where a read cannot map.  A slot is live as everywhere else (inserted once, end != 0).  A live entry of a reference of
 * length len covers the bases [start, min(end, len - 1)], both ends inclusive: the interval the entry records, what a Match of that
 * k-min-mer alone reports as r_start / r_end (with homopolymer compression the recorded end may stop short of the l-mer's true last
 * base; the coverage reports the index, it does not repair it).  A live entry with start > end or start >= len covers nothing and is
 * counted in *out_of_range (only a crafted file holds one).  Dead entries contribute nothing; a base whose only possible entry would
 * have end == 0 is never covered.  A reference's coverage is the union of its live entries' intervals:
 *   refs       one record per reference that exists (len > 0), in id order: its live k-min-mers, its covered bases, and its intervals
 *              intervals[first_interval, first_interval + n_intervals)
 *   intervals  the maximal runs of covered bases, half-open [start, end), sorted by reference id, then by start; no interval runs
 *              from one reference into the next
 * mq_index_coverage locks the index, waits for the device (as mq_index_resize does), computes from the table as it is now and returns
 * host copies that stay valid until the next mq_index_coverage, mq_index_coverage_release, mq_index_reopen, mq_index_resize,
 * mq_index_merge* or mq_index_free on the index (each drops them).  The device memory it takes (one bit per base: 390 MB for a 3.1-Gbp
 * genome) is given back before it returns.  MQ_ESTATE: the index is not finalized, or a context of it has a submitted batch that was
 * not waited for.  MQ_ENOMEM leaves the index usable and without a result.  Any of the five outputs may be NULL. */
typedef struct mq_ref_coverage {   /* 48 bytes */
    uint32_t ref_id, reserved;
    uint64_t len, live_kminmers, covered_bases, n_intervals, first_interval;
} mq_ref_coverage;
typedef struct mq_cov_interval { uint32_t start, end; } mq_cov_interval;   /* [start, end), 8 bytes */
int mq_index_coverage(mq_index *idx, const mq_ref_coverage **refs, uint64_t *n_refs,
                      const mq_cov_interval **intervals, uint64_t *n_intervals, uint64_t *out_of_range);
int mq_index_coverage_release(mq_index *idx);
/* Mapping depth: where the reads landed, per window of every reference, accumulated on the device from finished mq_hit records (the
 * companion of the coverage: that one says "no live k-min-mer here", this one "no read landed here").  An mq_depth is bound to a
 * snapshot of the index's reference ids and lengths, taken at mq_depth_new.
 * Which hits count.  A hit is counted iff status == MQ_HIT_MAPPED and mapq >= min_mapq (min_mapq 0: every mapped read).  A hit with
 * another status (MQ_HIT_UNMAPPED, MQ_HIT_OVERFLOW) is tallied as not_mapped, a mapped one with mapq < min_mapq as below_mapq.
 * What a counted hit covers.  On a reference of length len: the bases [r_start, min(r_end, len - 1)], both ends inclusive -- columns 8
 * and 9 as the PAF prints them.  It covers nothing, and is tallied as out_of_range instead, when r_start > r_end, when r_start >= len,
 * when ref_id lies beyond the snapshot, or in a hole of a sparse id range (len == 0).  (The Match::check precedence quirk can make
 * find_coords wrap, so such hits are legal outputs of the mapper.)
 * Windows.  1 <= window <= 2^24, any integer.  Window j of a reference is [j * window, min((j + 1) * window, len)); a reference has
 * ceil(len / window) windows, and the windows of all references lie behind one another in id order: reference r's are
 * [first_window, first_window + n_windows) of the two window arrays.
 *   window_bases[j]   (u64) the sum, over the counted hits, of the number of the hit's bases inside the window
 *   window_starts[j]  (u32) the number of counted hits whose r_start lies in the window
 *   refs              one 64-byte record per reference that exists (len > 0), in id order: reads = its counted hits, bases = the sum of
 *                     its windows' window_bases, zero_windows = its windows with window_bases == 0, max_window_bases
 *   totals            offered = counted + not_mapped + below_mapq + out_of_range
 * The result is a function of the multiset of hits offered since mq_depth_new or the last mq_depth_clear: not of their order, of the
 * batches they came in, or of the route (host or device) they took.  An accumulator refuses a batch with MQ_EINVAL once `offered` would
 * pass 2^31 - 1 (the running count of a window is 32 bits wide).
 *   mq_depth_new(idx, window, min_mapq, &out)   MQ_ESTATE: idx is not finalized; MQ_EINVAL: window == 0 or > 2^24; MQ_ENOMEM (nothing is
 *                          left behind): no device memory, or more than 2^31 - 1 windows in all -- 16 bytes of accumulators per window and
 *                          12 for a result: 90 MB for a 3.1-Gbp genome at window 1000; window 1 on a human genome is MQ_ENOMEM.
 *   mq_depth_add(d, hits, n)                    hits in host memory: staged, accumulated, and in when the call returns.  n == 0 is legal.
 *   mq_depth_add_device(d, d_hits, n, stream)   hits in device memory (16-byte aligned) on the index's device, asynchronous on `stream`
 *                          (a hipStream_t, may be NULL): nothing is allocated, nothing is read by the host.  Queued behind
 *                          mq_map_batch_device on the same stream it sees that call's final hits, the redo arena's included.
 *   mq_depth_result(d, ...)                     waits for the device (every queued mq_depth_add_device included), computes from the
 *                          accumulators without changing them -- more hits may follow -- and returns host copies that stay valid until
 *                          the next mq_depth_result, mq_depth_clear or mq_depth_free on the accumulator.  Any output may be NULL.
 *   mq_depth_clear(d)                           waits for the device; everything back to zero.
 * Every call on one accumulator locks it: several threads, and several contexts' streams, may add to one accumulator.  The snapshot is
 * the accumulator's own: after mq_index_reopen / mq_index_merge* of its index, hits on the ids it does not know are out_of_range.  Free
 * every accumulator before its index, as a context; an accumulator that is only added to and read may outlive it (after mq_depth_new
 * it uses the index's device, not the index: the native driver's second pass adds to the first pass's accumulator). */
typedef struct mq_depth mq_depth;
typedef struct mq_ref_depth {   /* 64 bytes */
    uint32_t ref_id, reserved;
    uint64_t len, n_windows, first_window, reads, bases, zero_windows, max_window_bases;
} mq_ref_depth;
typedef struct mq_depth_totals {   /* 40 bytes */
    uint64_t offered, counted, not_mapped, below_mapq, out_of_range;
} mq_depth_totals;
int mq_depth_new(mq_index *idx, uint32_t window, uint32_t min_mapq, mq_depth **out);
void mq_depth_free(mq_depth *d);
int mq_depth_clear(mq_depth *d);
int mq_depth_add(mq_depth *d, const mq_hit *hits, uint32_t n);
int mq_depth_add_device(mq_depth *d, const mq_hit *d_hits, uint32_t n, void *stream);
int mq_depth_result(mq_depth *d, const mq_ref_depth **refs, uint64_t *n_refs, const uint64_t **window_bases,
                    const uint32_t **window_starts, uint64_t *n_windows, mq_depth_totals *totals);
/* Coordinate order: the permutation that puts finished mq_hit records -- the PAF lines -- in the order of (reference, r_start), by a
 * stable radix sort on the device.  An mq_sorter is an object beside the index, as mq_depth: bound to the index's device and to a
 * snapshot of its reference ids (dense lengths, len > 0 <=> the id exists), taken at mq_sort_new.
 * What is kept.  Hit i of an add call with first_ordinal = o carries the ordinal o + i (u32): the caller's name for the hit, typically
 * the read's number in input order.  It is kept iff status == MQ_HIT_MAPPED, mapq >= min_mapq, and ref_id exists in the snapshot.  Any
 * other status is tallied not_mapped; a mapped hit below min_mapq below_mapq; a mapped hit at or above min_mapq whose ref_id lies beyond
 * the snapshot or in a hole out_of_range.  r_start is not range-checked: a wrapped find_coords value sorts where its number puts it.
 * The order.  Kept records ascend by the 88-bit key (ref_id : 24 bits, r_start : 32 bits, ordinal : 32 bits).  Two records that agree
 * in all three fields come out in unspecified order: the caller gave one ordinal twice.  The result is a function of the multiset of
 * (hit, ordinal) pairs offered since mq_sort_new or the last mq_sort_clear: not of their order, their batches, the route or the stream.
 *   order   the kept records' ordinals in that order (u32 each), n_kept of them
 *   refs    one 24-byte record per reference that exists, in id order: its records are order[first, first + count)
 *   totals  offered = kept + not_mapped + below_mapq + out_of_range
 * Capacity is counted in OFFERED hits, not kept ones: the host knows every n, so no add can overflow on the device and nothing is ever
 * dropped.  Ordinals and `offered` stay below 2^32 - 1: a call that would pass this (first_ordinal + n wrapping included) is MQ_EINVAL.
 *   mq_sort_new(idx, capacity, min_mapq, &out)   MQ_ESTATE: idx is not finalized; MQ_EINVAL: capacity > 2^32 - 2; MQ_ENOMEM: nothing is left
 *                          behind.  capacity 0 is legal (the host route grows).  Device memory: 12 bytes per record of capacity (an 8-byte
 *                          key ref_id << 32 | r_start and the ordinal); the first mq_sort_result adds a second key / ordinal set, 12 bytes
 *                          more per record, and the per-tile digit counts, 1 KB per tile of 2,048 records (0.5 byte per record): 24.5 bytes
 *                          per record in all, 98 MB for 4 M reads.  Beside these: the snapshot (8 bytes per reference id up to the
 *                          largest, 4 per existing reference and 16 for its first / count), a fixed 22.5 KB block of digit histograms
 *                          and row totals, and -- the host route only -- a staging buffer of 48 bytes per hit of the largest
 *                          mq_sort_add so far (with a quarter of slack), kept until mq_sort_free.
 *   mq_sort_add(s, hits, n, first_ordinal)       hits in host memory: staged, filtered, appended, and in when the call returns.  Grows the
 *                          sorter itself when offered + n > capacity, by doubling (it is synchronous anyway).  n == 0 is legal.
 *   mq_sort_add_device(s, d_hits, n, first_ordinal, stream)   hits in device memory (16-byte aligned) on the index's device, asynchronous
 *                          on `stream` (a hipStream_t, may be NULL): nothing is allocated, nothing is read by the host.  When
 *                          offered + n > capacity it answers MQ_EOVERFLOW before anything is queued, and nothing has changed.  Queued
 *                          behind mq_map_batch_device on the same stream it sees that call's final hits, the redo arena's included.
 *   mq_sort_reserve(s, capacity)                 waits for the device, grows the sorter to `capacity` and keeps its contents; never shrinks;
 *                          MQ_ENOMEM leaves the sorter as it was (its result scratch aside, which the next result brings back).
 *   mq_sort_result(s, ...)                       waits for the device (every queued mq_sort_add_device included), sorts, and returns host
 *                          copies that stay valid until the next mq_sort_result, _clear, _reserve or _free on the sorter.  More adds
 *                          may follow, and a later result covers everything.  Any output may be NULL.
 *   mq_sort_clear(s)                             waits for the device; the sorter is empty again, its capacity stays.
 * Every call on one sorter locks it: several threads, and several contexts' streams, may add to one sorter.  The snapshot is the
 * sorter's own, as an accumulator's; free every sorter before its index. */
typedef struct mq_sorter mq_sorter;
typedef struct mq_sort_ref {      /* 24 bytes; one per existing reference, in id order */
    uint32_t ref_id, reserved;
    uint64_t first, count;        /* its records: order[first, first + count) */
} mq_sort_ref;
typedef struct mq_sort_totals {   /* 40 bytes */
    uint64_t offered, kept, not_mapped, below_mapq, out_of_range;   /* offered = the sum of the other four */
} mq_sort_totals;
int mq_sort_new(mq_index *idx, uint64_t capacity, uint32_t min_mapq, mq_sorter **out);   /* capacity 0 is legal (host route grows) */
void mq_sort_free(mq_sorter *s);
int mq_sort_clear(mq_sorter *s);
int mq_sort_reserve(mq_sorter *s, uint64_t capacity);
int mq_sort_add(mq_sorter *s, const mq_hit *hits, uint32_t n, uint32_t first_ordinal);
int mq_sort_add_device(mq_sorter *s, const mq_hit *d_hits, uint32_t n, uint32_t first_ordinal, void *stream);
int mq_sort_result(mq_sorter *s, const uint32_t **order, uint64_t *n_kept, const mq_sort_ref **refs, uint64_t *n_refs,
                   mq_sort_totals *totals);
int mq_index_ref_info(const mq_index *idx, uint32_t ref_id, const char **name, uint64_t *len);
/* The parameters an index was built with (a loaded file's k, l, density, use_hpc and seeding variant decide its keys), and the ones that
 * act at mapping time only -- Params.c / .s (Chain::get_match, src/chain.rs:147-169), .g (the gap tests, src/chain.rs:132-142) and the
 * case folding -- which a loaded index takes from its caller's command line. */
int mq_index_get_params(const mq_index *idx, mq_params *out);
int mq_index_set_map_params(mq_index *idx, uint32_t c, uint32_t s, uint32_t g, int fold_case);

/* find_matches (src/mers.rs:77-102) for n reads.  bases: concatenated reads; offsets: n+1 prefix offsets.
 * Host-buffer form: copies in, runs, copies out, synchronises.  Reads that overflow the per-wave Match scratch or whose
 * minimizer list outgrows its region are mapped again on the GPU with worst-case scratch, so no MQ_HIT_OVERFLOW is returned
 * from this entry point. */
int mq_map_batch(mq_index *idx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, mq_hit *out);
/* Device-resident form: all pointers are device memory on the index's device; asynchronous on `stream`
 * (a hipStream_t, may be NULL).  total_bases = d_offsets[n] - d_offsets[0] (the host knows it: it built the offsets); it sizes
 * the per-read minimizer lists.  No allocation happens here once the scratch has grown to the batch shape (mq_map_reserve).
 * A read with more Match runs than the scratch holds (MQ_MATCH_CAP, default 2048) or with a minimizer list denser than
 * 4*density + 1/512 per base gets status MQ_HIT_OVERFLOW here (loud, never a wrong line) -- unless a redo arena has been reserved
 * (mq_map_reserve_redo / mq_ctx_reserve_redo below): then those reads are finished on the device, on the same stream. */
int mq_map_batch_device(mq_index *idx, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, uint64_t total_bases,
                        mq_hit *d_out, void *stream);

/* THREADING CONTRACT.  The reference maps on --threads workers over one read-only index (src/closures.rs:183,187,
 * src/index.rs:108-116).  Here: every mq_index_* / mq_map_* entry point locks the index, so calls on ONE index from several
 * threads are safe and run one after another (they share the index's default context: one set of work counters, scratch and
 * staging buffers).  For launch sequences in flight TOGETHER on one finalized index, give every worker thread (or every
 * stream slot of a pipelined feeder) its own mq_ctx: a context owns a stream, work counters, Match scratch, minimizer
 * lists, staging buffers and events, and the finalized table is only read.  One context runs one launch sequence at a time
 * (calls on one context must not overlap; successive device-form calls must be ordered by their streams).
 * mq_index_add_ref / mq_index_finalize must have returned before any context maps; free every context before its index. */
typedef struct mq_ctx mq_ctx;
mq_ctx *mq_ctx_new(mq_index *idx);
void mq_ctx_free(mq_ctx *ctx);
/* mq_map_batch on this context. */
int mq_ctx_map_batch(mq_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, mq_hit *out);
/* The same in two halves, for double buffering: submit queues H2D copy, kernels and D2H copy on the context's stream and
 * returns; `out` is filled (and overflow reads redone) by mq_ctx_wait.  bases/offsets/out must stay valid until then; bases
 * in page-locked memory (mq_host_alloc) overlaps the copy with other contexts' kernels. */
int mq_ctx_submit(mq_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, mq_hit *out);
int mq_ctx_wait(mq_ctx *ctx);
/* Spans form of mq_ctx_submit for raw FASTX buffers: the whole buffer buf[0, buf_bytes) goes to the device as it is (headers,
 * line ends, quality lines and all) and read i is buf[starts[i], starts[i] + lens[i]); spans in order and disjoint.  With
 * MQ_FLAG_FOLD_CASE the host never has to touch a base.  starts/lens/buf/out must stay valid until mq_ctx_wait. */
int mq_ctx_submit_spans(mq_ctx *ctx, const uint8_t *buf, uint64_t buf_bytes, const uint64_t *starts, const uint32_t *lens, uint32_t n,
                        mq_hit *out);
/* FASTA records found on the device (the batch form of closures.rs:100-123 for a reader that does not parse): buf[begin, bytes) is a
 * piece of an uncompressed FASTA file that holds WHOLE records, begin at a record's '>'.  The bytes go to the device as they are,
 * kernels find the line ends, and read i is the second line of record i (ONE '\r' at the end of the line is cut; a last line without
 * '\n' ends at `bytes`, and a '\r' that is the piece's last byte is cut from it like one in front of a '\n').  mq_ctx_submit_fasta
 * queues copy and scan and returns; mq_ctx_wait_fasta launches the map kernels once the record count is known and returns pointers
 * into the context's page-locked memory, valid until its next submit:
 *   line_ends[0 .. n_lines)  positions of the line ends in buf, ascending; record i: header = buf[(i ? line_ends[2i-1]+1 : begin), line_ends[2i]),
 *                            sequence = buf[line_ends[2i]+1, line_ends[2i+1])   (n_lines = 2 * n_reads)
 *   hits[0 .. n_reads)       as mq_ctx_wait fills them (overflow reads redone)
 * flags & MQ_FASTA_IRREGULAR: the piece is not "header line, sequence line" all through (an odd number of lines, a header line that is
 * empty or does not start with '>', a sequence line that starts with '>': sequences over several lines, blank lines, a header without
 * its sequence line; or more line ends than the list holds, min(bytes / 16 + 4096, 2^28)): nothing was mapped, n_reads = n_lines = 0 --
 * parse it on the host and use mq_ctx_submit_spans.  An empty piece (begin == bytes) is regular: 0 records.  buf must stay
 * valid until mq_ctx_wait_fasta has returned; page-locked memory (mq_host_alloc) gives the full PCIe rate. */
#define MQ_FASTA_IRREGULAR 1u
int mq_ctx_submit_fasta(mq_ctx *ctx, const uint8_t *buf, uint64_t begin, uint64_t bytes);
/* The same for either format (the reference reads FASTQ unless the file's name says FASTA, src/main.rs:196-205; its real-data headline
 * run is an uncompressed FASTQ, experiments/table1.sh:50).  MQ_FASTX_FASTQ: buf[begin, bytes) holds whole four-line records, begin at a
 * record's '@'; read i is the second line of record i, and mq_ctx_wait_fasta reports n_lines = 4 * n_reads line ends (record i: header
 * = buf[(i ? line_ends[4i-1]+1 : begin), line_ends[4i]), sequence = buf[line_ends[4i]+1, line_ends[4i+1])).  The device checks every
 * record the way the reference's reader would have to: '@' opens it, '+' opens its third line, one quality per base (ONE '\r' at the
 * end cut from the sequence and from the quality line; both may be empty); anything else
 * (sequences or qualities over several lines, blank lines, a truncated record) comes back MQ_FASTA_IRREGULAR for the host's parser.
 * The quality bytes cross the link but no host thread reads them. */
#define MQ_FASTX_FASTA 0u
#define MQ_FASTX_FASTQ 1u
int mq_ctx_submit_fastx(mq_ctx *ctx, const uint8_t *buf, uint64_t begin, uint64_t bytes, uint32_t format);
int mq_ctx_wait_fasta(mq_ctx *ctx, uint32_t *n_reads, const uint32_t **line_ends, uint32_t *n_lines, const mq_hit **hits, uint32_t *flags);
/* MQ_FASTX_FASTA_LINES: FASTA records whose sequences may run over several lines (what seqkit writes by default: 60, 70 or 80 columns).
 * buf[begin, bytes) holds whole records, begin at a record's '>'.  A header start is a '>' at `begin` or directly behind a '\n' (a '>'
 * anywhere else is an ordinary byte); record r is header line r plus everything up to the next header start; its sequence is every byte
 * behind the header line that is not '\n' and not a '\r' whose next byte is '\n' or which is the piece's last byte.  The device finds
 * the headers and joins the lines; mq_ctx_wait_fasta_lines (and only it: mq_ctx_wait_fasta answers MQ_ESTATE and leaves the piece
 * pending, as mq_ctx_wait_fasta_lines does for a piece of another format) launches the map kernels on the joined reads and returns
 * pointers into the context's page-locked memory, valid until its next submit:
 *   hdr_begin[r], hdr_end[r]   header line r = buf[hdr_begin[r], hdr_end[r]) ('>' first; a '\r' in front of the '\n' is inside)
 *   seq_lens[r]                the joined length of read r (PAF column 2)
 *   hits[0 .. n_reads)         as mq_ctx_wait fills them (overflow reads redone, from a host copy of those reads' joined bytes alone)
 * flags & MQ_FASTA_IRREGULAR (n_reads = 0, nothing mapped, the context stays usable): the piece does not start with '>', holds more
 * records than the span arrays (bytes / 32 + 2048), or holds a record without a sequence byte.  An empty piece is regular: 0 records. */
#define MQ_FASTX_FASTA_LINES 2u
int mq_ctx_wait_fasta_lines(mq_ctx *ctx, uint32_t *n_reads, const uint32_t **hdr_begin, const uint32_t **hdr_end, const uint32_t **seq_lens,
                            const mq_hit **hits, uint32_t *flags);
/* Pre-size the context's device staging, minimizer lists and scratch for batches of up to n_reads reads / total_bytes buffer
 * bytes, so that the first submit does not pay for the allocations. */
int mq_ctx_reserve(mq_ctx *ctx, uint32_t n_reads, uint64_t total_bytes);
/* mq_map_batch_device on this context. */
int mq_ctx_map_batch_device(mq_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_offsets, uint32_t n, uint64_t total_bases,
                            mq_hit *d_out, void *stream);

/* Overflow reads of the device-resident form redone in stream, on the device (opt-in, per context; without a reservation the device form
 * reports MQ_HIT_OVERFLOW as described above).  mq_ctx_reserve_redo allocates, now, a redo arena for up to max_reads overflow reads of up
 * to max_read_len bases each.  From then on mq_ctx_map_batch_device queues, behind its launch sequence and on the caller's stream, a
 * second launch sequence over the arena (worst-case list regions and Match windows, as the host-buffer forms use for their redo): three
 * small kernels find the records with status MQ_HIT_OVERFLOW, copy those reads' bases into the arena and write the final mq_hit over each
 * of them.  No host synchronisation, no allocation, no host read of a hit: when the stream reaches the end of the call's work, every
 * overflow read that fitted the arena holds the record the host-buffer form returns for it, byte for byte.  A read that did not fit
 * (more overflow reads than max_reads -- which of them get a place is not defined -- or longer than max_read_len) keeps
 * MQ_HIT_OVERFLOW: loud as before.  The host-buffer, spans and FASTX-piece entry points redo their overflow reads as they always did.
 *   max_reads == 0                     releases the arena: the feature is off again
 *   MQ_ESTATE                          the context has a submitted batch
 *   MQ_ENOMEM                          the context keeps the arena it had (or none)
 *   MQ_EINVAL                          max_read_len == 0 with max_reads > 0; max_reads >= 2^30 or R * S (below) >= 2^47
 * Reserve, release and mq_ctx_free only when the stream of the last device-form call has been ordered behind them by the caller, as for
 * any two calls on one context (the arena itself waits for its last launch before its memory goes).
 * What the arena costs in device memory, with R = max_reads, L = max_read_len, S = L + 64 rounded up to a multiple of 64:
 *   R * S                                   the slots
 *   (R * S + 64 R + 64) * 9/8 * 12          the slots' minimizer lists at one entry per base (* 16 with seeding variant 16)
 *   G * 8 * L * 32                          Match windows of L records for the 8 waves of each of G workgroups, G = min(resident workgroups,
 *                                           (R + 3) / 4, 2^30 / (256 L)) but at least 1: at most 1 GB unless L > 2^22
 *   about (R + 16) * 5/4 * 2048 * 32        the ordinary Match windows of a launch over R reads (MQ_MATCH_CAP records each)
 *   R * 112 + 0.6 MB                        per-read words, work descriptors, the slots' hits
 * -- about 14.5 bytes per base of R * (L + 64), plus the windows: 0.5 GB for R = 256, L = 24,000; 1.3 GB for R = 256, L = 65,536.
 * mq_ctx_redo_counts reports the last device-form call of the context: how many reads were redone and how many kept MQ_HIT_OVERFLOW
 * (it waits for that call's work on the stream; (0, 0) before the first call; MQ_ESTATE without an arena).
 * mq_map_reserve_redo / mq_map_redo_counts: the same for the index's default context (mq_map_batch_device). */
int mq_ctx_reserve_redo(mq_ctx *ctx, uint32_t max_reads, uint32_t max_read_len);
int mq_ctx_redo_counts(mq_ctx *ctx, uint32_t *redone, uint32_t *left);
int mq_map_reserve_redo(mq_index *idx, uint32_t max_reads, uint32_t max_read_len);
int mq_map_redo_counts(mq_index *idx, uint32_t *redone, uint32_t *left);

/* The winning chain's Match runs ("anchors") with every mapped read (opt-in, per context; a context without a reservation runs exactly the
 * kernels it always ran).  mq_ctx_reserve_anchors allocates, now, a span per read for batches of up to max_reads reads and a pool of
 * max_anchors anchors.  From then on every map call on the context -- mq_ctx_map_batch, mq_ctx_submit / _submit_spans + mq_ctx_wait,
 * mq_ctx_submit_fasta / _fastx + both waits, mq_ctx_map_batch_device with and without a redo arena -- takes the kernel pair that also
 * writes, for read r of the batch, spans[r] and, for a mapped read, its anchors in read order at pool[first .. first + count): count is the
 * number of runs of the chain, the sum of their `count` fields is the hit's score.  An unmapped, tied or too short read has span {0, 0}.
 * A read that is redone (MQ_HIT_OVERFLOW: through the host, or in stream with a redo arena) delivers its anchors from the redo; one that
 * leaves with MQ_HIT_OVERFLOW has span {0, 0}.  The order in which the reads' lists lie in the pool is not defined.
 * Pool exhaustion is loud, never wrong: a read whose list found no room has first == MQ_ANCHORS_DROPPED and its count; `dropped_reads`
 * counts them, `needed` says what the batch asked of the pool (reserve that much and map again: there is no automatic second pass), the
 * hits are unaffected.  A batch of more than max_reads reads is refused with MQ_EINVAL before anything is queued -- except a FASTX piece,
 * whose number of records is known only at mq_ctx_wait_fasta[_lines]: that call refuses it, before the map launch, and the piece is
 * consumed (its copy and its scan have run).  A call that fails leaves mq_ctx_anchors describing the last batch that was launched.  The
 * instrumented launch of mq_map_probe_stats and mq_kminmers_batch write no anchors.
 *   (0, 0)        releases the reservation: the feature is off again
 *   MQ_ESTATE     the context has a submitted batch
 *   MQ_EINVAL     one of the two 0; max_reads >= 2^30; max_anchors >= 2^32 - 1; the index runs the split pipeline (MQ_PIPELINE=split)
 *   MQ_ENOMEM     the context keeps the reservation it had (or none)
 * Device memory: 8 max_reads + 20 max_anchors bytes (+ 4 max_reads for the redo's id map), the same again page-locked on the host.
 * mq_ctx_anchors finishes the context's last batch (mq_ctx_wait if it was only submitted; the stream of a device-form call is waited for)
 * and returns host copies: spans[0 .. n_reads), anchors[0 .. stored), stored = min(needed, max_anchors) -- valid until the next map call,
 * reserve or free on the context.  MQ_ESTATE without a reservation or with a FASTX piece in flight; n_reads = 0 before the first batch.
 * mq_ctx_anchors_device gives the device arrays themselves and waits for nothing: for mq_ctx_map_batch_device callers that stay on their
 * stream (valid until the reservation changes).
 * mq_map_reserve_anchors / mq_map_anchors: the same for the index's default context, as mq_map_reserve_redo. */
int mq_ctx_reserve_anchors(mq_ctx *ctx, uint32_t max_reads, uint64_t max_anchors);
int mq_ctx_anchors(mq_ctx *ctx, const mq_anchor_span **spans, const mq_anchor **anchors, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                   uint32_t *dropped_reads);
int mq_ctx_anchors_device(mq_ctx *ctx, const mq_anchor_span **d_spans, const mq_anchor **d_anchors);
int mq_map_reserve_anchors(mq_index *idx, uint32_t max_reads, uint64_t max_anchors);
int mq_map_anchors(mq_index *idx, const mq_anchor_span **spans, const mq_anchor **anchors, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                   uint32_t *dropped_reads);

/* Every candidate chain of every read (opt-in, per context; a context without a reservation runs exactly the kernels it always ran).
 * mq_ctx_reserve_chains allocates, now, a span per read for batches of up to max_reads reads, a pool of max_chains chains, and a staging
 * window per mapping wave beside its Match window.  From then on every map call on the context -- mq_ctx_map_batch, mq_ctx_submit /
 * _submit_spans + mq_ctx_wait, mq_ctx_submit_fasta / _fastx + both waits, mq_ctx_map_batch_device with and without a redo arena -- takes
 * the kernel pair that also writes, for read r of the batch, spans[r] and its chains at pool[first .. first + count), in the order of each
 * reference's first run in the read.  A read with no run, or shorter than l + k - 1, has span {0, 0}.  A read that is redone
 * (MQ_HIT_OVERFLOW: through the host, or in stream with a redo arena) delivers its chains from the redo; one that leaves with
 * MQ_HIT_OVERFLOW has span {0, 0}.  The order in which the reads' lists lie in the pool is not defined.
 * A context may hold an anchors reservation and a chains reservation at once: both outputs are written then.
 * Pool exhaustion is loud, never wrong: a read whose list found no room has first == MQ_CHAINS_DROPPED and its true count;
 * `dropped_reads` counts them, `needed` says what the batch asked of the pool (reserve that much and map again: there is no automatic
 * second pass), the hits are unaffected.  A batch of more than max_reads reads is refused with MQ_EINVAL before anything is queued --
 * except a FASTX piece, whose number of records is known only at mq_ctx_wait_fasta[_lines]: that call refuses it, before the map launch,
 * and the piece is consumed (its copy and its scan have run).  A call that fails leaves mq_ctx_chains describing the last batch that was
 * launched.  The instrumented launch of mq_map_probe_stats and mq_kminmers_batch write no chains.
 *   (0, 0)        releases the reservation: the feature is off again
 *   MQ_ESTATE     the context has a submitted batch
 *   MQ_EINVAL     one of the two 0; max_reads >= 2^30; max_chains >= 2^32 - 1; the index runs the split pipeline (MQ_PIPELINE=split)
 *   MQ_ENOMEM     the context keeps the reservation it had (or none)
 * Device memory: 8 max_reads + 48 max_chains bytes (+ 4 max_reads for the redo's id map), the same again page-locked on the host, and 32
 * bytes per Match record of the windows the context's launches use.
 * mq_ctx_chains finishes the context's last batch (mq_ctx_wait if it was only submitted; the stream of a device-form call is waited for)
 * and returns host copies: spans[0 .. n_reads), chains[0 .. stored), stored = min(needed, max_chains) -- valid until the next map call,
 * reserve or free on the context.  MQ_ESTATE without a reservation or with a FASTX piece in flight; n_reads = 0 before the first batch.
 * mq_ctx_chains_device gives the device arrays themselves and waits for nothing: for mq_ctx_map_batch_device callers that stay on their
 * stream (valid until the reservation changes).
 * mq_map_reserve_chains / mq_map_chains: the same for the index's default context, as mq_map_reserve_redo. */
int mq_ctx_reserve_chains(mq_ctx *ctx, uint32_t max_reads, uint64_t max_chains);
int mq_ctx_chains(mq_ctx *ctx, const mq_chain_span **spans, const mq_chain **chains, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                  uint32_t *dropped_reads);
int mq_ctx_chains_device(mq_ctx *ctx, const mq_chain_span **d_spans, const mq_chain **d_chains);
int mq_map_reserve_chains(mq_index *idx, uint32_t max_reads, uint64_t max_chains);
int mq_map_chains(mq_index *idx, const mq_chain_span **spans, const mq_chain **chains, uint32_t *n_reads, uint64_t *stored, uint64_t *needed,
                  uint32_t *dropped_reads);

/* Page-locked host memory for the buffers handed to mq_map_batch / mq_index_add_ref (a feeder that parses FASTX straight
 * into such buffers gets the full PCIe rate on the copy in; pageable buffers work too, at roughly a quarter of it). */
void *mq_host_alloc(size_t bytes);
void mq_host_free(void *p);
/* Page-lock / release a range the caller owns, whole pages (the feeder does this to slices of the mapped reads file, so that
 * mq_ctx_submit_fasta's copy is a DMA out of the page cache that no host thread waits for).  0 on success. */
int mq_host_register(void *ptr, size_t bytes);
int mq_host_unregister(void *ptr);

/* Pre-size the default context's scratch for batches of up to n_reads reads / total_bases bases, so that mq_map_batch_device
 * never allocates. */
int mq_map_reserve(mq_index *idx, uint32_t n_reads, uint64_t total_bases);

/* Parity/debug: the k-min-mers of each sequence as KminmersIterator yields them (src/mers.rs:41-54).
 * kmm_offsets (n+1, host) gives each sequence's capacity window in `out`; counts[i] receives the true count. */
int mq_kminmers_batch(mq_index *idx, const uint8_t *bases, const uint64_t *offsets, uint32_t n, const uint64_t *kmm_offsets,
                      mq_kminmer *out, uint32_t *counts);

/* Parity/debug: probe the finalized table (ReadOnlyIndex::get, src/index.rs:118-126).  found[i]=1 on a live hit;
 * entries[i] = {hash, start, end, offset, rev=rc} with ref ids in ref_ids[i]. */
int mq_index_lookup(mq_index *idx, const uint64_t *hashes, uint32_t n, uint8_t *found, mq_kminmer *entries, uint32_t *ref_ids);

/* The format! of src/mers.rs:181 (no newline).  Returns the length or <0. */
int mq_format_paf(const mq_index *idx, const char *q_id, uint64_t q_len, const mq_hit *hit, char *buf, size_t cap);

/* The twelve columns of mq_format_paf for any chain of mq_ctx_chains, TOP or not (no newline): for the unique top chain of a mapped read
 * the bytes are those of mq_format_paf on the read's hit.  Returns the length or <0. */
int mq_format_paf_chain(const mq_index *idx, const char *q_id, uint64_t q_len, const mq_chain *chain, char *buf, size_t cap);

/* Measurement and diagnostic entry points (probe statistics, stage clocks, launch timers): include/mapquik_hip_diag.h. */

#ifdef __cplusplus
}
#endif
#endif
