"""Thin host driver with mapquik's command-line surface (reference: src/main.rs:77-272, src/closures.rs:22-212).

    python -m mapquik_amd <reads.fa|fq[.gz]> --reference <ref.fa[.gz]> [-k -l -d -c -s -g -p --threads -b -q --nohpc ...]

Same flags, defaults, log lines and `<prefix>.paf` output as the reference binary; the hot path (ref_extract /
find_matches) runs on the GPU through the C ABI.  This is the SURVEY 8(f2/f3) row kept deliberately small: a
single-threaded FASTX reader that upper-cases (src/closures.rs:63,106), batches reads and writes PAF lines in input
order (src/closures.rs:117-123).  No CPU compute fallback exists.
"""
import argparse
import gzip
import os
import resource
import sys
import time

import numpy as np

from . import api


def rust_duration(seconds):
    """`{:?}` of a std::time::Duration: s / ms / µs / ns with up to 9 significant fractional digits, zeros trimmed."""
    ns = int(round(seconds * 1e9))
    for unit, div in (("s", 10**9), ("ms", 10**6), ("µs", 10**3), ("ns", 1)):
        if ns >= div or unit == "ns":
            whole, frac = divmod(ns, div)
            if frac == 0 or div == 1:
                return "%d%s" % (whole, unit)
            digits = len(str(div)) - 1
            return "%d.%s%s" % (whole, ("%0*d" % (digits, frac)).rstrip("0"), unit)


def rust_float(x):
    """`{}` of an f64 as Rust prints it for the values that occur here (1.0 -> "1", 0.01 -> "0.01")."""
    if x == int(x) and abs(x) < 1e16:
        return str(int(x))
    return repr(float(x))


def is_fasta_name(name):
    """src/main.rs:196,202"""
    return (".fasta." in name or name.endswith(".fna") or ".fna." in name or ".fa." in name or name.endswith(".fa")
            or name.endswith(".fasta"))


def open_maybe_compressed(path):
    """get_reader (src/main.rs:60-75): raw, .gz; .lz4 is not available in this host driver."""
    if path.endswith(".lz4"):
        raise SystemExit("Error opening compressed file: lz4 input is not supported by this driver")
    if path.endswith(".gz"):
        return gzip.open(path, "rb")
    return open(path, "rb")


def read_fastx(path, fasta):
    """Yields (id, upper-cased sequence bytes).  FASTA may be multi-line; FASTQ is 4-line."""
    with open_maybe_compressed(path) as fh:
        if fasta:
            name, chunks = None, []
            for line in fh:
                line = line.rstrip(b"\r\n")
                if line.startswith(b">"):
                    if name is not None:
                        yield name, b"".join(chunks).upper()
                    name, chunks = line[1:].split(b" ", 1)[0].decode(), []  # seq_io's id(): up to the first SPACE (src/closures.rs:107)
                elif name is not None:
                    chunks.append(line)
            if name is not None:
                yield name, b"".join(chunks).upper()
        else:
            while True:
                h = fh.readline()
                if not h:
                    return
                s = fh.readline().rstrip(b"\r\n")
                fh.readline()
                fh.readline()
                yield h.rstrip(b"\r\n")[1:].split(b" ", 1)[0].decode(), s.upper()


def build_parser():
    ap = argparse.ArgumentParser(prog="mapquik", description="Original implementation of mapquik, a fast HiFi read mapper. (HIP backend)")
    ap.add_argument("reads", nargs="?")
    ap.add_argument("--debug", action="store_true")
    ap.add_argument("-p", "--prefix")
    ap.add_argument("-k", type=int)
    ap.add_argument("-l", type=int)
    ap.add_argument("-d", "--density", type=float)
    ap.add_argument("-c", "--chain", type=int)
    ap.add_argument("-s", "--seed", type=int)
    ap.add_argument("-g", "--gap-diff", type=int, dest="gap_diff")
    ap.add_argument("--reference")
    ap.add_argument("--threads", type=int)
    ap.add_argument("--low-memory", action="store_true")
    ap.add_argument("--nosimd", action="store_true")
    ap.add_argument("--nohpc", action="store_true")
    ap.add_argument("--parallelfastx", action="store_true")
    ap.add_argument("-b", type=int)
    ap.add_argument("-q", type=int)
    ap.add_argument("--device", type=int, default=0, help="HIP device ordinal (extension)")
    ap.add_argument("--batch-bases", type=int, default=1 << 30, help="bases per GPU batch (extension)")
    ap.add_argument("--save-index", dest="save_index", help="write the finalized index (occupied slots only) for later runs (extension: the "
                    "reference re-indexes the FASTA on every run, src/closures.rs:24-94)")
    ap.add_argument("--index", dest="load_index", help="map against a saved index instead of indexing --reference; same -k -l -d --nohpc as it was "
                    "built with (extension)")
    ap.add_argument("--add-reference", dest="add_reference", help="with --index: add this FASTA's records to the loaded index (ids continue behind "
                    "its largest id), then map; --save-index writes the extended index.  The table grows, when it has to, by --table-factor "
                    "(default: the library's 8, whatever factor the file was saved at) (extension)")
    ap.add_argument("--merge-index", dest="merge_index", action="append", default=[], metavar="FILE",
                    help="merge this saved index into the one --index / --reference / --add-reference produced (same seeding parameters; ids continue "
                         "behind its largest id); repeatable, applied in command-line order; --save-index then writes the merged index (extension)")
    ap.add_argument("--table-factor", type=int, dest="table_factor", help="index table slots per k-min-mer, 2..64 (library default 8); with --index "
                    "the loaded table gets that size (extension)")
    ap.add_argument("--seeding-variant", type=int, default=0, dest="seeding_variant",
                    help="reading of the k-min-mer iterator's unpinned decisions, bits 1 2 4 8 16 32 (include/mapquik_hip.h); 0 = the frozen "
                         "reading (extension; tools/check_against_upstream.sh finds the value that reproduces the crate)")
    ap.add_argument("--fast-kh", action="store_true", dest="fast_kh",
                    help="cheap k-min-mer tuple hash instead of SipHash-1-3 (MQ_FLAG_FAST_KH): the same PAF -- the hash acts through equality only, "
                         "src/index.rs:118-126 -- with fewer instructions; KminmerHash.hash is then not the reference's value (extension)")
    ap.add_argument("--unmapped", action="store_true",
                    help="also write <prefix>.unmapped.out with the ids of reads that got no PAF line (extension; the reference "
                         "has this writer commented out, src/closures.rs:38-43; feeds a second pass with other parameters)")
    ap.add_argument("--anchors", action="store_true",
                    help="also write <prefix>.anchors: one line per Match run of every mapped read's winning chain, reads in input order, runs in "
                         "read order: q_id, q_start, q_end, strand, r_name, r_start, r_end, count -- raw coordinates as the chain holds them, "
                         "before find_coords (extension; the reference's -a path, src/chain.rs:173-237, walks the same list)")
    ap.add_argument("--chains", action="store_true",
                    help="also write <prefix>.chains: one line per candidate chain of every read (one per reference with a Match run in the read, ties "
                         "included), reads in input order: the twelve PAF columns of the chain, tp:A:P for the read's unique top chain and tp:A:S "
                         "for every other, cn:i:<runs kept>, and tie:i:1 on the top chains of a tied read (extension)")
    ap.add_argument("--coverage", action="store_true",
                    help="once the index is complete (behind --index / --reference / --add-reference / --merge-index), also write <prefix>.coverage.bed: "
                         "r_name, start, end of every maximal run of reference bases that the index's live k-min-mers span, and <prefix>.coverage.tsv: "
                         "per reference its length, live k-min-mers, covered bases, covered fraction and intervals (extension)")
    ap.add_argument("--depth", action="store_true",
                    help="also write <prefix>.depth.bed: r_name, start, end, bases, starts, mean per window of every reference -- how many bases of the "
                         "mapped reads (PAF columns 8 and 9, mapq >= --depth-min-mapq) landed in the window and how many of them start there -- and "
                         "<prefix>.depth.tsv: per reference its length, reads, bases, mean depth, windows without a base and the deepest window's mean "
                         "(extension; accumulated on the device from each batch's hits)")
    ap.add_argument("--depth-window", type=int, default=1000, metavar="N", help="with --depth: bases per window, 1 .. 2^24 (default 1000)")
    ap.add_argument("--depth-min-mapq", type=int, default=60, metavar="Q", help="with --depth: count the reads with mapq >= Q (default 60; 0: every mapped read)")
    ap.add_argument("--sort", action="store_true",
                    help="also write <prefix>.sorted.paf: the lines of <prefix>.paf in the order of (reference id, column 8, input order), and "
                         "<prefix>.sorted.tsv: per reference its name, length, lines, first line and the byte offset of that line in the sorted file "
                         "(extension; each batch's hits are sorted on the device, <prefix>.paf stays as it is)")
    ap.add_argument("--sort-min-mapq", type=int, default=0, metavar="Q", help="with --sort: keep the lines with mapq >= Q (default 0: every PAF line)")
    return ap


def sort_log_line(totals, refs, min_mapq):
    """the one line both drivers print for --sort"""
    return "Sorted: %d of %d hits kept (%d not mapped, %d below mapq %d, %d out of range): %d lines on %d references" % (
        totals["kept"], totals["offered"], totals["not_mapped"], totals["below_mapq"], min_mapq, totals["out_of_range"], int(refs["count"].sum()),
        int((refs["count"] > 0).sum()))


def write_sorted(index, sorter, prefix, line_at, line_len):
    """--sort: <prefix>.sorted.paf gathered from <prefix>.paf (mapped, its lines written one by one: neither file is held in memory;
    line_at / line_len: per read number, where its line lies there and how long it is, -1 / 0 without one), <prefix>.sorted.tsv, and the
    log line.  A failure leaves none of the three files behind, as a failure of the map phase leaves no PAF."""
    import mmap
    names = [prefix + ".paf", prefix + ".sorted.paf", prefix + ".sorted.tsv"]
    try:
        order, refs, totals = sorter.result()
        offsets = np.zeros(order.size + 1, dtype=np.int64)
        with open(names[0], "rb") as src, open(names[1], "wb") as f:
            paf = mmap.mmap(src.fileno(), 0, access=mmap.ACCESS_READ) if order.size else b""
            for j, o in enumerate(order.tolist()):
                if o >= len(line_at) or line_at[o] < 0 or line_at[o] + line_len[o] > len(paf):
                    raise api.MapquikError("--sort: read %d was kept but has no PAF line" % o)
                f.write(paf[line_at[o]:line_at[o] + line_len[o]])
                offsets[j + 1] = offsets[j] + line_len[o]
            if order.size:
                paf.close()
        with open(names[2], "wb") as f:
            f.write(api.format_sorted_tsv(index, refs, offsets))
    except (api.MapquikError, OSError, ValueError):
        for n in names:
            if os.path.exists(n):
                os.remove(n)
        raise
    return sort_log_line(totals, refs, sorter.min_mapq)


def depth_log_line(totals, refs, window, min_mapq):
    """the one line both drivers print for --depth"""
    return "Depth: %d of %d hits counted (%d not mapped, %d below mapq %d, %d out of range): %d bases in %d windows of %d" % (
        totals["counted"], totals["offered"], totals["not_mapped"], totals["below_mapq"], min_mapq, totals["out_of_range"], int(refs["bases"].sum()),
        int(refs["n_windows"].sum()), window)


def write_depth(index, depth, prefix):
    """--depth: the two files of the run's accumulator, and the log line"""
    refs, wb, ws, totals = depth.result()
    with open(prefix + ".depth.bed", "wb") as f:
        f.write(api.format_depth_bed(index, refs, wb, ws, depth.window))
    with open(prefix + ".depth.tsv", "wb") as f:
        f.write(api.format_depth_tsv(index, refs, depth.window))
    return depth_log_line(totals, refs, depth.window, depth.min_mapq)


def write_coverage(index, prefix):
    """--coverage: the two files of the finished index, and the log line"""
    refs, ivs, out_of_range = index.coverage()
    with open(prefix + ".coverage.bed", "wb") as f:
        f.write(api.format_coverage_bed(index, refs, ivs))
    with open(prefix + ".coverage.tsv", "wb") as f:
        f.write(api.format_coverage_tsv(index, refs))
    index.coverage_release()
    return "Coverage: %d of %d bases in %d intervals (%d entries out of range)" % (int(refs["covered_bases"].sum()), int(refs["len"].sum()), ivs.size, out_of_range)


def chain_lines(index, names, offs, spans, chains):
    """the text of <prefix>.chains for one batch"""
    out = []
    for i, (nm, sp) in enumerate(zip(names, spans)):
        mine = chains[int(sp["first"]):int(sp["first"]) + int(sp["count"])]
        tops = int((mine["flags"] & api.MQ_CHAIN_TOP != 0).sum())
        for ch in mine:
            top = bool(int(ch["flags"]) & api.MQ_CHAIN_TOP)
            out.append("%s\ttp:A:%s\tcn:i:%d%s" % (index.format_paf_chain(nm, int(offs[i + 1] - offs[i]), ch), "P" if top and tops == 1 else "S", int(ch["n_runs"]),
                                                 "\ttie:i:1" if top and tops > 1 else ""))
    return out


def anchor_lines(names, hits, spans, anchors, ref_name):
    """the text of <prefix>.anchors for one batch; ref_name: reference id -> name"""
    out = []
    for nm, h, sp in zip(names, hits, spans):
        if int(h["status"]) != api.MQ_HIT_MAPPED:
            continue
        strand, rn = "-" if int(h["rc"]) else "+", ref_name(int(h["ref_id"]))
        for a in anchors[int(sp["first"]):int(sp["first"]) + int(sp["count"])].tolist():
            out.append("%s\t%d\t%d\t%s\t%s\t%d\t%d\t%d" % (nm, a[0], a[1], strand, rn, a[2], a[3], a[4]))
    return out


def banner_lines(opt):
    """The stdout lines main() prints before run_mers (src/main.rs:196-240); returns (lines, settings)."""
    out = []
    k, l, c, s, g, b, q, density, threads = 5, 31, 4, 11, 2000, 1, 200, 0.01, 8
    reads_fasta = is_fasta_name(opt.reads)
    ref_fasta = is_fasta_name(opt.reference) if opt.reference else False
    if reads_fasta:
        out += ["Input file: %s" % opt.reads, "Format: FASTA"]
    if ref_fasta and (not getattr(opt, "load_index", None) or getattr(opt, "add_reference", None)):
        out += ["Reference file: %s" % opt.reference, "Format: FASTA"]
    if opt.k is not None: k = opt.k
    else: out.append("Warning: Using default k value (%d)." % k)
    if opt.l is not None: l = opt.l
    else: out.append("Warning: Using default l value (%d)." % l)
    if opt.b is not None: b = opt.b
    else: out.append("Warning: Using default buffer size (%dX)." % b)
    if opt.q is not None: q = opt.q
    else: out.append("Warning: Using default queue length (%d)." % q)
    if opt.density is not None: density = opt.density
    else: out.append("Warning: Using default density value (%s%%)." % rust_float(density * 100.0))
    if opt.threads is not None: threads = opt.threads
    else: out.append("Warning: Using default number of threads (8).")
    if opt.chain is not None: c = opt.chain
    else: out.append("Warning: Using default minimum chain length (%d)." % c)
    if opt.seed is not None: s = opt.seed
    else: out.append("Warning: Using default minimum number of matching seeds (%d)." % s)
    if opt.gap_diff is not None: g = opt.gap_diff
    else: out.append("Warning: Using default maximum seed gap difference (%d)." % g)
    prefix = "mapquik-k%d-d%s-l%d" % (k, rust_float(density), l)
    if opt.prefix is not None: prefix = opt.prefix
    else: out.append("Warning: Using default output prefix (%s)." % prefix)
    use_hpc, use_simd = not opt.nohpc, not opt.nosimd
    if use_hpc:
        out.append("Using HPC ntHash, with SIMD" if use_simd else "Using HPC ntHash, scalar")
    else:
        out.append("Using regular ntHash (not HPC), with SIMD" if use_simd else "Using regular ntHash (not HPC), scalar")
    return out, dict(k=k, l=l, density=density, use_hpc=use_hpc, c=c, s=s, g=g, prefix=prefix, reads_fasta=reads_fasta,
                     ref_fasta=ref_fasta)


def main(argv=None):
    start = time.time()
    ap = build_parser()
    opt = ap.parse_args(argv)
    if opt.add_reference and (not opt.load_index or opt.reference):
        ap.error("--add-reference adds to the index given with --index (and excludes --reference)")  # exit status 2
    if opt.table_factor is not None and not 2 <= opt.table_factor <= 64:
        ap.error("--table-factor wants 2..64")
    if opt.merge_index and not opt.load_index and not opt.reference:
        ap.error("--merge-index merges into the index given with --index or built from --reference")
    if opt.add_reference:
        opt.reference = opt.add_reference  # from here on the file is this run's reference file
    if not opt.reads:
        raise SystemExit("Please specify an input file.")
    if not opt.reference and not opt.load_index:
        raise SystemExit("Please specify a reference file.")
    if opt.load_index and opt.save_index and not opt.add_reference and not opt.merge_index:
        raise SystemExit("error: --index cannot be combined with --save-index (unless --add-reference extends it)")
    lines, st = banner_lines(opt)
    for ln in lines:
        print(ln)
    if opt.seeding_variant:
        print("Seeding variant %d (reading of rust-seq2kminmers other than the frozen one; include/mapquik_hip.h)." % opt.seeding_variant)
    if opt.fast_kh:
        print("Fast k-min-mer tuple hash (MQ_FLAG_FAST_KH): same PAF, KminmerHash.hash is not the reference's value.")
    params = api.Params(k=st["k"], l=st["l"], density=st["density"], use_hpc=st["use_hpc"], c=st["c"], s=st["s"], g=st["g"],
                        seeding_variant=opt.seeding_variant, fast_kh=opt.fast_kh)
    paf = open(st["prefix"] + ".paf", "w")  # src/closures.rs:32
    unm = open(st["prefix"] + ".unmapped.out", "w") if opt.unmapped else None
    anc = open(st["prefix"] + ".anchors", "w") if opt.anchors else None
    chn = open(st["prefix"] + ".chains", "w") if opt.chains else None

    t0 = time.time()
    if opt.load_index:
        index = api.Index.load(opt.load_index, device=opt.device, factor=opt.table_factor or 0)
        fp = index.get_params()
        if (fp.k, fp.l, fp.density, fp.use_hpc, fp.seeding_variant, fp.fast_kh) != (params.k, params.l, params.density, params.use_hpc, params.seeding_variant,
                                                                                     params.fast_kh):
            raise SystemExit("%s was built with -k %d -l %d -d %s%s --seeding-variant %d%s: run with the same seeding parameters"
                             % (opt.load_index, fp.k, fp.l, rust_float(fp.density), "" if fp.use_hpc else " --nohpc", fp.seeding_variant,
                                " --fast-kh" if fp.fast_kh else ""))
        index.set_map_params(params.c, params.s, params.g, bool(params.flags & api.MQ_FLAG_FOLD_CASE))
        ist = index.stats()
        print("Loaded index %s: %d references, %d k-min-mers." % (opt.load_index, ist["n_refs"], ist["n_kminmers"]))
        unique = ist["n_unique"]
    first_id = 0
    if opt.add_reference:  # the loaded index takes references again, under ids behind every id it has
        seen = 0
        while seen < ist["n_refs"]:
            try:
                index.ref_info(first_id)
                seen += 1
            except api.MapquikError:
                pass
            first_id += 1
        index.reopen()
    elif not opt.load_index:
        index = api.Index(params, device=opt.device)
    if opt.add_reference or not opt.load_index:
        if opt.table_factor is not None:
            index.set_table_factor(opt.table_factor)
        for ref_idx, (name, seq) in enumerate(read_fastx(opt.reference, st["ref_fasta"]), first_id):
            n = index.add_ref(ref_idx, name, np.frombuffer(seq, dtype=np.uint8))
            print("Indexed reference %s: %d k-min-mers." % (name, n))  # src/closures.rs:58
        unique = index.finalize()
    for path in opt.merge_index:  # in command-line order, each file's ids behind every id the index has by then
        before = index.stats()
        index.merge_file(path)
        ist = index.stats()
        print("Merged index %s: %d references, %d k-min-mers." % (path, ist["n_refs"] - before["n_refs"], ist["n_kminmers"] - before["n_kminmers"]))
        unique = ist["n_unique"]
    if opt.save_index:
        ts = time.time()
        index.save(opt.save_index)
        print("Saved index to %s in %s." % (opt.save_index, rust_duration(time.time() - ts)))
    if opt.coverage:
        try:
            print(write_coverage(index, st["prefix"]))
        except (api.MapquikError, OSError) as e:  # as a failure of the map phase ends the native driver: no PAF, exit status 101
            paf.close()
            os.remove(st["prefix"] + ".paf")
            print("--coverage: %s" % e, file=sys.stderr)
            raise SystemExit(101)
    print("Indexed %d unique k-min-mers in %s." % (unique, rust_duration(time.time() - t0)))  # src/closures.rs:92
    depth = None
    if opt.depth:  # one accumulator on the finished index; every batch's hits go to it
        try:
            depth = api.Depth(index, window=opt.depth_window, min_mapq=opt.depth_min_mapq)
        except (api.MapquikError, ValueError) as e:
            paf.close()
            os.remove(st["prefix"] + ".paf")
            print("--depth: %s" % e, file=sys.stderr)
            raise SystemExit(101)
    sorter = None
    if opt.sort:  # one sorter on the finished index; every batch's hits go to it under their reads' numbers in input order
        try:
            sorter = api.Sorter(index, min_mapq=opt.sort_min_mapq)
        except (api.MapquikError, ValueError) as e:
            paf.close()
            os.remove(st["prefix"] + ".paf")
            print("--sort: %s" % e, file=sys.stderr)
            raise SystemExit(101)
    line_at, line_len, paf_bytes = [], [], [0]  # --sort: per read number, its line in <prefix>.paf

    t0 = time.time()
    if opt.parallelfastx and not opt.reads.endswith((".gz", ".lz4")):
        print("Warning: using experimental rust-parallelfastx (exciting!)")  # src/closures.rs:192 (same reader here)

    def flush(names, seqs):
        if not names:
            return
        offs = np.zeros(len(seqs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(x) for x in seqs])
        bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
        if anc is not None:
            # the reservation of this batch.  A read has no more Match runs than k-min-mers and fewer k-min-mers than minimizers, and the
            # library's minimizer lists are sized at bytes x (4 density + 1/512) entries: the same bound here.  A batch that needs more
            # (reads inside dense tandem arrays) ends the run with what it needed.
            index.reserve_anchors(len(seqs), min(int(bases.size * (4.0 * st["density"] + 1.0 / 512.0)) + 64, (1 << 32) - 2))
        if chn is not None:  # (a read has no more chains than runs: the anchors' bound)
            index.reserve_chains(len(seqs), min(int(bases.size * (4.0 * st["density"] + 1.0 / 512.0)) + 64, (1 << 32) - 2))
        hits = index.map_batch(bases, offs)
        if depth is not None:
            depth.add(hits)
        if chn is not None:
            spans, chains, info = index.chains()
            if info["dropped_reads"]:
                raise SystemExit("--chains: the chain pool was too small for %d reads of a batch: %d entries needed, %d reserved"
                                 % (info["dropped_reads"], info["needed"], info["stored"]))
            for ln in chain_lines(index, names, offs, spans, chains):
                chn.write(ln + "\n")
        if anc is not None:
            spans, anchors, info = index.anchors()
            if info["dropped_reads"]:
                raise SystemExit("--anchors: the anchor pool was too small for %d reads of a batch: %d entries needed, %d reserved"
                                 % (info["dropped_reads"], info["needed"], info["stored"]))
            for ln in anchor_lines(names, hits, spans, anchors, lambda r: index.ref_info(r)[0]):
                anc.write(ln + "\n")
        lines = index.paf_lines(names, offs, hits)  # input order, unmapped reads write nothing (src/closures.rs:117-123)
        for ln in lines:
            paf.write(ln + "\n")
        if sorter is not None:
            sorter.add(hits, len(line_at))
            it = iter(lines)
            for h in hits:
                n = len(next(it).encode()) + 1 if int(h["status"]) == api.MQ_HIT_MAPPED else 0
                line_at.append(paf_bytes[0] if n else -1)
                line_len.append(n)
                paf_bytes[0] += n
        if unm is not None:
            for nm, h in zip(names, hits):
                if int(h["status"]) != api.MQ_HIT_MAPPED:
                    unm.write(nm + "\n")

    names, seqs, acc = [], [], 0
    for name, seq in read_fastx(opt.reads, st["reads_fasta"]):
        names.append(name)
        seqs.append(seq)
        acc += len(seq)
        if acc >= opt.batch_bases:
            flush(names, seqs)
            names, seqs, acc = [], [], 0
    flush(names, seqs)
    paf.close()
    if depth is not None:
        print(write_depth(index, depth, st["prefix"]))
        depth.close()
    if sorter is not None:
        try:
            print(write_sorted(index, sorter, st["prefix"], line_at, line_len))
        except (api.MapquikError, OSError, ValueError) as e:
            print("--sort: %s" % e, file=sys.stderr)
            raise SystemExit(101)
        sorter.close()
    if unm is not None:
        unm.close()
    if anc is not None:
        anc.close()
    if chn is not None:
        chn.close()
    print("Mapped query sequences in %s." % rust_duration(time.time() - t0))  # src/closures.rs:211
    print("Total execution time: %s" % rust_duration(time.time() - start))  # src/main.rs:270
    rss_gb = np.float32(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024) / np.float32(1024.0 ** 3)
    print("Maximum RSS: %sGB" % repr(float(rss_gb)))  # src/main.rs:271
    return 0


if __name__ == "__main__":
    sys.exit(main())
