"""ctypes binding of libmapquik_hip.so + host mirror of the reference's interface for the hot path.

Reference seam (Rust): mers::ref_extract (src/mers.rs:15), mers::find_matches (src/mers.rs:77), Index/ReadOnlyIndex
(src/index.rs:73-128), Params (src/main.rs:33-47).  Same names and argument meaning here; errors raise MapquikError
(the reference panics).  There is NO CPU fallback: if the HIP library or a GPU is missing, calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

MQ_HIT_UNMAPPED, MQ_HIT_MAPPED, MQ_HIT_OVERFLOW = 0, 1, 2
MQ_FLAG_FOLD_CASE = 1
MQ_FLAG_FAST_KH = 2
MQ_FLAG_SEED_VARIANT_SHIFT = 8
MQ_ABI_VERSION = 4  # include/mapquik_hip.h

hit_dtype = np.dtype([("status", "<u4"), ("ref_id", "<u4"), ("rc", "<u4"), ("mapq", "<u4"), ("q_start", "<u4"), ("q_end", "<u4"),
                      ("r_start", "<u4"), ("r_end", "<u4"), ("score", "<u4"), ("n_kminmers", "<u4"), ("q_start_hi", "<u4"), ("q_end_hi", "<u4")])
kminmer_dtype = np.dtype([("hash", "<u8"), ("start", "<u4"), ("end", "<u4"), ("offset", "<u4"), ("rev", "<u4")])
assert hit_dtype.itemsize == 48 and kminmer_dtype.itemsize == 24
# mq_anchor / mq_anchor_span (Context.reserve_anchors): a Match run of the winning chain; where a read's runs lie in the anchors array
anchor_dtype = np.dtype([("q_start", "<u4"), ("q_end", "<u4"), ("r_start", "<u4"), ("r_end", "<u4"), ("count", "<u4")])
anchor_span_dtype = np.dtype([("first", "<u4"), ("count", "<u4")])
MQ_ANCHORS_DROPPED = 0xFFFFFFFF
assert anchor_dtype.itemsize == 20 and anchor_span_dtype.itemsize == 8
# mq_chain / mq_chain_span (Context.reserve_chains): a candidate chain of a read, field for field the layout of a hit; where a read's chains lie
chain_dtype = np.dtype([("flags", "<u4"), ("ref_id", "<u4"), ("rc", "<u4"), ("mapq", "<u4"), ("q_start", "<u4"), ("q_end", "<u4"),
                        ("r_start", "<u4"), ("r_end", "<u4"), ("score", "<u4"), ("n_runs", "<u4"), ("q_start_hi", "<u4"), ("q_end_hi", "<u4")])
chain_span_dtype = np.dtype([("first", "<u4"), ("count", "<u4")])
MQ_CHAIN_TOP = 1
MQ_CHAINS_DROPPED = 0xFFFFFFFF
assert chain_dtype.itemsize == 48 and chain_span_dtype.itemsize == 8
# mq_ref_coverage / mq_cov_interval (Index.coverage): one record per reference; a maximal run of covered bases, half-open [start, end)
ref_coverage_dtype = np.dtype([("ref_id", "<u4"), ("reserved", "<u4"), ("len", "<u8"), ("live_kminmers", "<u8"), ("covered_bases", "<u8"),
                               ("n_intervals", "<u8"), ("first_interval", "<u8")])
cov_interval_dtype = np.dtype([("start", "<u4"), ("end", "<u4")])
assert ref_coverage_dtype.itemsize == 48 and cov_interval_dtype.itemsize == 8
# mq_ref_depth / mq_depth_totals (Depth.result): one record per reference; the accumulator's tallies
ref_depth_dtype = np.dtype([("ref_id", "<u4"), ("reserved", "<u4"), ("len", "<u8"), ("n_windows", "<u8"), ("first_window", "<u8"), ("reads", "<u8"),
                            ("bases", "<u8"), ("zero_windows", "<u8"), ("max_window_bases", "<u8")])
depth_totals_dtype = np.dtype([(n, "<u8") for n in ("offered", "counted", "not_mapped", "below_mapq", "out_of_range")])
assert ref_depth_dtype.itemsize == 64 and depth_totals_dtype.itemsize == 40
# mq_sort_ref / mq_sort_totals (Sorter.result): one record per reference; the sorter's tallies
sort_ref_dtype = np.dtype([("ref_id", "<u4"), ("reserved", "<u4"), ("first", "<u8"), ("count", "<u8")])
sort_totals_dtype = np.dtype([(n, "<u8") for n in ("offered", "kept", "not_mapped", "below_mapq", "out_of_range")])
assert sort_ref_dtype.itemsize == 24 and sort_totals_dtype.itemsize == 40


def hit_column(hits, name):
    """A PAF column of a hits array as uint64: columns 3 and 4 (q_start, q_end) are 64-bit in mq_hit (low word + *_hi)."""
    v = hits[name].astype(np.uint64)
    if name in ("q_start", "q_end"):
        v = v | (hits[name + "_hi"].astype(np.uint64) << np.uint64(32))
    return v

# every symbol include/mapquik_hip.h (the seam) and include/mapquik_hip_diag.h (measurement / diagnostics) declare
EXPORTS = ["mq_index_set_table_factor", "mq_ctx_submit_fastx", "mq_index_get_params", "mq_index_set_map_params", "mq_index_stage_begin", "mq_index_stage_piece", "mq_index_stage_done", "mq_index_add_ref_staged", "mq_index_add_ref_staged_lines", "mq_index_staged_sequence", "mq_ctx_submit_fasta", "mq_ctx_wait_fasta", "mq_ctx_wait_fasta_lines", "mq_index_reserve", "mq_host_register", "mq_host_unregister",
           "mq_last_error", "mq_abi_version", "mq_device_count", "mq_params_default", "mq_index_new", "mq_index_free",
           "mq_index_add_ref", "mq_index_add_ref_device", "mq_index_finalize", "mq_index_get_stats", "mq_index_ref_info",
           "mq_map_batch", "mq_map_batch_device", "mq_map_reserve", "mq_kminmers_batch", "mq_index_lookup", "mq_format_paf",
           "mq_last_map_ms", "mq_last_map_path_counts", "mq_last_map_order", "mq_host_alloc", "mq_host_free", "mq_index_save", "mq_index_load", "mq_index_clone", "mq_map_probe_stats",
           "mq_ctx_new", "mq_ctx_free", "mq_ctx_map_batch", "mq_ctx_submit", "mq_ctx_submit_spans", "mq_ctx_wait", "mq_ctx_reserve", "mq_ctx_map_batch_device", "mq_ctx_last_map_ms", "mq_probe_rate", "mq_last_stage_clocks", "mq_last_read_cycles", "mq_map_launch_waves", "mq_index_table_alloc_ms",
           "mq_ctx_reserve_redo", "mq_ctx_redo_counts", "mq_map_reserve_redo", "mq_map_redo_counts",
           "mq_ctx_reserve_anchors", "mq_ctx_anchors", "mq_ctx_anchors_device", "mq_map_reserve_anchors", "mq_map_anchors",
           "mq_ctx_reserve_chains", "mq_ctx_chains", "mq_ctx_chains_device", "mq_map_reserve_chains", "mq_map_chains", "mq_format_paf_chain",
           "mq_index_reopen", "mq_index_resize", "mq_index_load_sized", "mq_index_clone_sized",
           "mq_index_merge", "mq_index_merge_file", "mq_index_coverage", "mq_index_coverage_release",
           "mq_depth_new", "mq_depth_free", "mq_depth_clear", "mq_depth_add", "mq_depth_add_device", "mq_depth_result",
           "mq_sort_new", "mq_sort_free", "mq_sort_clear", "mq_sort_reserve", "mq_sort_add", "mq_sort_add_device", "mq_sort_result"]


class MapquikError(RuntimeError):
    pass


class Params(C.Structure):
    """src/main.rs:33-47; defaults src/main.rs:174-188."""
    _fields_ = [("k", C.c_uint32), ("l", C.c_uint32), ("density", C.c_double), ("use_hpc", C.c_uint32), ("c", C.c_uint32),
                ("s", C.c_uint32), ("g", C.c_uint32), ("flags", C.c_uint32)]

    def __init__(self, k=5, l=31, density=0.01, use_hpc=True, c=4, s=11, g=2000, fold_case=False, seeding_variant=0, fast_kh=False):
        """seeding_variant: MQ_SEEDVAR_* bits (include/mapquik_hip.h), 0 = the frozen reading of the third-party k-min-mer iterator.
        fast_kh: MQ_FLAG_FAST_KH, the opt-in cheap tuple hash (same PAF; mq_kminmer.hash is then not the reference's value)."""
        if not 0 <= int(seeding_variant) < 64:
            raise ValueError("seeding_variant must be 0..63")
        super().__init__(k, l, density, 1 if use_hpc else 0, c, s, g,
                         (MQ_FLAG_FOLD_CASE if fold_case else 0) | (MQ_FLAG_FAST_KH if fast_kh else 0) | (int(seeding_variant) << MQ_FLAG_SEED_VARIANT_SHIFT))

    @property
    def fast_kh(self):
        return bool(self.flags & MQ_FLAG_FAST_KH)

    @property
    def seeding_variant(self):
        return (self.flags >> MQ_FLAG_SEED_VARIANT_SHIFT) & 0x3F


class IndexStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_refs", "n_kminmers", "n_keys", "n_unique", "table_slots", "table_bytes", "slot_bytes")]


_lib = None


def load_library(path=None):
    """Load (building if stale) the HIP library.  Raises MapquikError when it cannot be built or loaded."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or os.environ.get("MQ_LIB")  # A/B benchmarking of two builds in one session
    p = path or _build.LIB
    if path is None:
        try:
            _build.build()
        except Exception as e:  # no hipcc on this box: fine if a prebuilt .so travelled with the snapshot
            if not os.path.exists(p):
                raise MapquikError("libmapquik_hip.so is missing and could not be built: %s" % e)
    try:
        L = C.CDLL(p)
    except OSError as e:
        raise MapquikError("cannot load %s: %s" % (p, e))
    vp, u64, u32 = C.c_void_p, C.c_uint64, C.c_uint32
    L.mq_last_error.restype = C.c_char_p
    L.mq_abi_version.restype = C.c_int
    L.mq_device_count.restype = C.c_int
    L.mq_params_default.argtypes = [C.POINTER(Params)]
    L.mq_index_new.restype = vp
    L.mq_index_new.argtypes = [C.POINTER(Params), C.c_int]
    L.mq_index_free.argtypes = [vp]
    L.mq_index_add_ref.restype = C.c_int64
    L.mq_index_add_ref.argtypes = [vp, u32, C.c_char_p, vp, u64]
    L.mq_index_add_ref_device.restype = C.c_int64
    L.mq_index_add_ref_device.argtypes = [vp, u32, C.c_char_p, vp, u64]
    L.mq_index_finalize.restype = C.c_int64
    L.mq_index_finalize.argtypes = [vp]
    L.mq_index_get_stats.argtypes = [vp, C.POINTER(IndexStats)]
    L.mq_index_ref_info.argtypes = [vp, u32, C.POINTER(C.c_char_p), C.POINTER(u64)]
    L.mq_map_batch.argtypes = [vp, vp, vp, u32, vp]
    L.mq_map_batch_device.argtypes = [vp, vp, vp, u32, u64, vp, vp]
    L.mq_map_reserve.argtypes = [vp, u32, u64]
    L.mq_ctx_new.restype = vp
    L.mq_ctx_new.argtypes = [vp]
    L.mq_ctx_free.argtypes = [vp]
    L.mq_ctx_map_batch.argtypes = [vp, vp, vp, u32, vp]
    L.mq_ctx_submit.argtypes = [vp, vp, vp, u32, vp]
    L.mq_ctx_submit_spans.argtypes = [vp, vp, u64, vp, vp, u32, vp]
    L.mq_ctx_wait.argtypes = [vp]
    abi = L.mq_abi_version()
    if path is None and abi != MQ_ABI_VERSION:
        raise MapquikError("%s has ABI version %d, this binding is for %d: rebuild (python __graft_entry__.py)" % (p, abi, MQ_ABI_VERSION))
    # (an older build given by MQ_LIB / path for an A/B run may lack the newer symbols: each group under the guard of its own first symbol)
    if hasattr(L, "mq_index_reserve"):
        L.mq_index_reserve.argtypes = [vp, u64]
    if hasattr(L, "mq_ctx_submit_fasta"):  # ABI 3 on
        L.mq_host_register.argtypes = [vp, C.c_size_t]
        L.mq_host_unregister.argtypes = [vp]
        L.mq_ctx_submit_fasta.argtypes = [vp, vp, u64, u64]
        L.mq_ctx_wait_fasta.argtypes = [vp, C.POINTER(u32), C.POINTER(vp), C.POINTER(u32), C.POINTER(vp), C.POINTER(u32)]
    if hasattr(L, "mq_ctx_submit_fastx"):
        L.mq_ctx_submit_fastx.argtypes = [vp, vp, u64, u64, u32]
    if hasattr(L, "mq_ctx_wait_fasta_lines"):
        L.mq_ctx_wait_fasta_lines.argtypes = [vp, C.POINTER(u32), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(u32)]
    if hasattr(L, "mq_index_stage_begin"):  # ABI 4
        L.mq_index_set_table_factor.argtypes = [vp, u32]
        L.mq_index_get_params.argtypes = [vp, C.POINTER(Params)]
        L.mq_index_set_map_params.argtypes = [vp, u32, u32, u32, C.c_int]
        L.mq_index_stage_begin.argtypes = [vp, u64]
        L.mq_index_stage_piece.argtypes = [vp, u64, vp, u64, C.POINTER(u64)]
        L.mq_index_stage_done.argtypes = [vp, u64, C.c_int]
        L.mq_index_add_ref_staged.restype = C.c_int64
        L.mq_index_add_ref_staged.argtypes = [vp, u32, C.c_char_p, u64, u64, u64]
    if hasattr(L, "mq_index_add_ref_staged_lines"):
        L.mq_index_add_ref_staged_lines.restype = C.c_int64
        L.mq_index_add_ref_staged_lines.argtypes = [vp, u32, C.c_char_p, u64, u64, u64, C.POINTER(u64)]
        L.mq_index_staged_sequence.restype = C.c_int64
        L.mq_index_staged_sequence.argtypes = [vp, u64, u64, u64, vp, u64]
    L.mq_ctx_reserve.argtypes = [vp, u32, u64]
    L.mq_ctx_map_batch_device.argtypes = [vp, vp, vp, u32, u64, vp, vp]
    L.mq_ctx_last_map_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.mq_probe_rate.argtypes = [vp, u32, u32, u32, u32, C.POINTER(C.c_float), C.POINTER(u64), C.POINTER(u64)]
    L.mq_kminmers_batch.argtypes = [vp, vp, vp, u32, vp, vp, vp]
    L.mq_index_lookup.argtypes = [vp, vp, u32, vp, vp, vp]
    L.mq_format_paf.argtypes = [vp, C.c_char_p, u64, vp, C.c_char_p, C.c_size_t]
    L.mq_last_map_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.mq_last_stage_clocks.argtypes = [vp, vp]
    if hasattr(L, "mq_last_read_cycles"):
        L.mq_last_read_cycles.argtypes = [vp, u32, vp, vp]
    L.mq_map_probe_stats.argtypes = [vp, vp, vp, u32, u64, vp, C.POINTER(u64), C.POINTER(u64)]
    if hasattr(L, "mq_map_launch_waves"):
        L.mq_map_launch_waves.argtypes = [vp, u32, C.POINTER(u32)]
        L.mq_index_table_alloc_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.mq_index_save.argtypes = [vp, C.c_char_p]
    L.mq_index_clone.restype = vp
    L.mq_index_clone.argtypes = [vp, C.c_int]
    L.mq_index_load.restype = vp
    L.mq_index_load.argtypes = [C.c_char_p, C.c_int]
    L.mq_host_alloc.restype = vp
    L.mq_host_alloc.argtypes = [C.c_size_t]
    L.mq_host_free.argtypes = [vp]
    L.mq_last_map_path_counts.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mq_last_map_order.argtypes = [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    if hasattr(L, "mq_ctx_reserve_redo"):
        L.mq_ctx_reserve_redo.argtypes = [vp, u32, u32]
        L.mq_map_reserve_redo.argtypes = [vp, u32, u32]
        L.mq_ctx_redo_counts.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
        L.mq_map_redo_counts.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    pp = C.POINTER(vp)
    for kind in ("anchors", "chains"):  # the two pooled outputs: one family of entry points each
        if hasattr(L, "mq_ctx_reserve_" + kind):
            for scope in ("ctx", "map"):
                getattr(L, "mq_%s_reserve_%s" % (scope, kind)).argtypes = [vp, u32, u64]
                getattr(L, "mq_%s_%s" % (scope, kind)).argtypes = [vp, pp, pp, C.POINTER(u32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u32)]
            getattr(L, "mq_ctx_%s_device" % kind).argtypes = [vp, pp, pp]
    if hasattr(L, "mq_format_paf_chain"):
        L.mq_format_paf_chain.argtypes = [vp, C.c_char_p, u64, vp, C.c_char_p, C.c_size_t]
    if hasattr(L, "mq_index_reopen"):
        L.mq_index_reopen.argtypes = [vp]
        L.mq_index_resize.argtypes = [vp, u64, u32]
        L.mq_index_load_sized.restype = vp
        L.mq_index_load_sized.argtypes = [C.c_char_p, C.c_int, u64, u32]
        L.mq_index_clone_sized.restype = vp
        L.mq_index_clone_sized.argtypes = [vp, C.c_int, u64, u32]
    if hasattr(L, "mq_index_merge"):
        L.mq_index_merge.argtypes = [vp, vp, u32]
        L.mq_index_merge_file.argtypes = [vp, C.c_char_p, u32]
    if hasattr(L, "mq_index_coverage"):
        L.mq_index_coverage.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), C.POINTER(u64)]
        L.mq_index_coverage_release.argtypes = [vp]
        L.mqdiag_coverage_tile_bits.restype = u64
        L.mqdiag_coverage_tile_bits.argtypes = []
        L.mqdiag_coverage_held.restype = u64
        L.mqdiag_coverage_held.argtypes = [vp]
        L.mqdiag_coverage_ms.argtypes = [C.POINTER(C.c_float)]
    if hasattr(L, "mq_depth_new"):
        L.mq_depth_new.argtypes = [vp, u32, u32, C.POINTER(vp)]
        L.mq_depth_free.restype = None
        L.mq_depth_free.argtypes = [vp]
        L.mq_depth_clear.argtypes = [vp]
        L.mq_depth_add.argtypes = [vp, vp, u32]
        L.mq_depth_add_device.argtypes = [vp, vp, u32, vp]
        L.mq_depth_result.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(vp), C.POINTER(u64), vp]
        L.mqdiag_depth_tile_windows.restype = u64
        L.mqdiag_depth_tile_windows.argtypes = []
        L.mqdiag_depth_result_ms.argtypes = [vp, C.POINTER(C.c_float)]
    if hasattr(L, "mq_sort_new"):
        L.mq_sort_new.argtypes = [vp, u64, u32, C.POINTER(vp)]
        L.mq_sort_free.restype = None
        L.mq_sort_free.argtypes = [vp]
        L.mq_sort_clear.argtypes = [vp]
        L.mq_sort_reserve.argtypes = [vp, u64]
        L.mq_sort_add.argtypes = [vp, vp, u32, u32]
        L.mq_sort_add_device.argtypes = [vp, vp, u32, u32, vp]
        L.mq_sort_result.argtypes = [vp, C.POINTER(vp), C.POINTER(u64), C.POINTER(vp), C.POINTER(u64), vp]
        L.mqdiag_sort_tile_records.restype = u64
        L.mqdiag_sort_tile_records.argtypes = []
        L.mqdiag_sort_passes.argtypes = [vp, C.POINTER(u32)]
        L.mqdiag_sort_result_ms.argtypes = [vp, C.POINTER(C.c_float)]
    if hasattr(L, "mqdiag_last_map_spec"):
        L.mqdiag_last_map_spec.argtypes = [vp, C.POINTER(C.c_uint32)]
        L.mqdiag_ctx_last_map_spec.argtypes = [vp, C.POINTER(C.c_uint32)]
    if path is None:
        _lib = L
    return L


def _err(L, what):
    return MapquikError("%s: %s" % (what, (L.mq_last_error() or b"").decode(errors="replace")))


def _pooled(L, what, handle, span_dtype, item_dtype):
    """(spans, items, info) of mq_ctx_anchors / mq_map_anchors / mq_ctx_chains / mq_map_chains (`what`): numpy copies of the library's host arrays"""
    sp, it = C.c_void_p(), C.c_void_p()
    n, dropped = C.c_uint32(), C.c_uint32()
    stored, needed = C.c_uint64(), C.c_uint64()
    if getattr(L, what)(handle, C.byref(sp), C.byref(it), C.byref(n), C.byref(stored), C.byref(needed), C.byref(dropped)) != 0:
        raise _err(L, what)
    spans = np.frombuffer(C.string_at(sp.value, n.value * span_dtype.itemsize), dtype=span_dtype).copy() if n.value else np.zeros(0, dtype=span_dtype)
    items = np.frombuffer(C.string_at(it.value, stored.value * item_dtype.itemsize), dtype=item_dtype).copy() if stored.value else np.zeros(0, dtype=item_dtype)
    return spans, items, dict(stored=stored.value, needed=needed.value, dropped_reads=dropped.value)


def _reserve_pooled(L, what, handle, max_reads, max_entries):
    if getattr(L, what)(handle, int(max_reads), int(max_entries)) != 0:
        raise _err(L, what)


def _pooled_device(L, what, handle):
    sp, it = C.c_void_p(), C.c_void_p()
    if getattr(L, what)(handle, C.byref(sp), C.byref(it)) != 0:
        raise _err(L, what)
    return sp.value, it.value


class PinnedBuffer:
    """Page-locked host bytes (mq_host_alloc) exposed as a numpy uint8 array: fill it, pass `.array` to Index.map_batch."""

    def __init__(self, nbytes):
        self._L = load_library()
        self._p = self._L.mq_host_alloc(nbytes)
        if not self._p:
            raise _err(self._L, "mq_host_alloc")
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(self._p))

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            self._L.mq_host_free(self._p)
            self._p = None

    __del__ = close


def device_count():
    return load_library().mq_device_count()


def _seq(seq):
    if isinstance(seq, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.ascontiguousarray(seq, dtype=np.uint8)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Index:
    """Index + ReadOnlyIndex (src/index.rs:73-128) + ref_map (src/closures.rs:30), resident in HBM."""

    def __init__(self, params=None, device=0, _handle=None):
        self._L = load_library()
        self.params = params or Params()
        self._h = _handle if _handle is not None else self._L.mq_index_new(C.byref(self.params), device)
        if not self._h:
            raise _err(self._L, "mq_index_new")
        self.device = device

    def save(self, path):
        """Write the finalized index to disk (parameters, reference table, slot table)."""
        if self._L.mq_index_save(self._h, os.fsencode(path)) != 0:
            raise _err(self._L, "mq_index_save")

    @classmethod
    def load(cls, path, device=0, table_slots=0, factor=0):
        """A finalized index read back from Index.save (its parameters: Index.get_params(); the mapping-time ones can be replaced with
        Index.set_map_params).  table_slots / factor (at most one of them, see Index.resize): the file's slots go straight into a table
        of that size (mq_index_load_sized) instead of one of the size the file records."""
        L = load_library()
        if table_slots or factor:
            h, what = L.mq_index_load_sized(os.fsencode(path), device, int(table_slots), int(factor)), "mq_index_load_sized"
        else:
            h, what = L.mq_index_load(os.fsencode(path), device), "mq_index_load"
        if not h:
            raise _err(L, what)
        return cls(None, device, _handle=h)

    def clone(self, device, table_slots=0, factor=0):
        """A replica of this finalized index on another device (device-to-device copy, no re-indexing).  table_slots / factor (at most
        one of them, see Index.resize): the replica's table gets that size, and only the occupied slots cross the link
        (mq_index_clone_sized)."""
        if table_slots or factor:
            h, what = self._L.mq_index_clone_sized(self._h, device, int(table_slots), int(factor)), "mq_index_clone_sized"
        else:
            h, what = self._L.mq_index_clone(self._h, device), "mq_index_clone"
        if not h:
            raise _err(self._L, what)
        return Index(self.params, device, _handle=h)

    def reopen(self):
        """A finalized index takes add_ref* again (ids distinct from the ones it has); finalize() then inserts the new references into
        the existing table.  Until then the mapping calls fail as on any index that is not finalized."""
        if self._L.mq_index_reopen(self._h) != 0:
            raise _err(self._L, "mq_index_reopen")

    def resize(self, table_slots=0, factor=0):
        """The finalized index's table rebuilt on the device at another size: table_slots exactly (a power of two above n_keys), or what
        a build of this index's k-min-mers gets at `factor` slots each (2..64).  At most one of the two; neither: nothing happens."""
        if self._L.mq_index_resize(self._h, int(table_slots), int(factor)) != 0:
            raise _err(self._L, "mq_index_resize")

    def next_ref_id(self):
        """the smallest id behind every reference id the index has (--add-reference's rule: ids continue behind the largest)"""
        n, seen, rid = self.stats()["n_refs"], 0, 0
        name, ln = C.c_char_p(), C.c_uint64()
        while seen < n:
            if self._L.mq_index_ref_info(self._h, rid, C.byref(name), C.byref(ln)) == 0:
                seen += 1
            rid += 1
        return rid

    def merge(self, other, id_base=None):
        """Another finalized index merged into this one (mq_index_merge): `other`'s reference id i becomes id_base + i (None: this index's
        largest id + 1), and this index ends where one build of both reference sets ends.  Returns the id_base used."""
        base = self.next_ref_id() if id_base is None else int(id_base)
        if self._L.mq_index_merge(self._h, other.handle, base) != 0:
            raise _err(self._L, "mq_index_merge")
        return base

    def merge_file(self, path, id_base=None):
        """Index.merge from a file written by Index.save (mq_index_merge_file): its slots are streamed into this index's table."""
        base = self.next_ref_id() if id_base is None else int(id_base)
        if self._L.mq_index_merge_file(self._h, os.fsencode(path), base) != 0:
            raise _err(self._L, "mq_index_merge_file")
        return base

    def coverage(self):
        """(refs, intervals, out_of_range) of mq_index_coverage, as numpy copies: one ref_coverage_dtype record per reference in id order
        (its live k-min-mers, covered bases, and its intervals[first_interval : first_interval + n_intervals]), the maximal runs of
        bases the live k-min-mers span as cov_interval_dtype [start, end), and the live entries that lie outside their reference."""
        rp, ip = C.c_void_p(), C.c_void_p()
        nr, ni, oor = C.c_uint64(), C.c_uint64(), C.c_uint64()
        if self._L.mq_index_coverage(self._h, C.byref(rp), C.byref(nr), C.byref(ip), C.byref(ni), C.byref(oor)) != 0:
            raise _err(self._L, "mq_index_coverage")
        refs = np.frombuffer(C.string_at(rp.value, nr.value * 48), dtype=ref_coverage_dtype).copy() if nr.value else np.zeros(0, dtype=ref_coverage_dtype)
        ivs = np.frombuffer(C.string_at(ip.value, ni.value * 8), dtype=cov_interval_dtype).copy() if ni.value else np.zeros(0, dtype=cov_interval_dtype)
        return refs, ivs, oor.value

    def coverage_release(self):
        """the library's own copies of the last coverage() result given back (they also go with the next call that changes the index)"""
        if self._L.mq_index_coverage_release(self._h) != 0:
            raise _err(self._L, "mq_index_coverage_release")

    def close(self):
        if getattr(self, "_h", None):
            self._L.mq_index_free(self._h)
            self._h = None

    __del__ = close

    @property
    def handle(self):
        return self._h

    def add_ref(self, ref_idx, name, seq):
        """index_mers closure (src/closures.rs:46-51): returns the reference's k-min-mer count."""
        s = _seq(seq)
        n = self._L.mq_index_add_ref(self._h, ref_idx, name.encode(), _p(s), s.size)
        if n < 0:
            raise _err(self._L, "mq_index_add_ref")
        return n

    def add_ref_device(self, ref_idx, name, d_ptr, length):
        n = self._L.mq_index_add_ref_device(self._h, ref_idx, name.encode(), C.c_void_p(d_ptr), length)
        if n < 0:
            raise _err(self._L, "mq_index_add_ref_device")
        return n

    def last_read_cycles(self, n):
        """(cycles, start_ticks) of the n reads of the last probe_stats launch: what each read cost its wave, when it was taken up."""
        cyc = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint64)
        if self._L.mq_last_read_cycles(self._h, n, _p(cyc), _p(st)) != 0:
            raise _err(self._L, "mq_last_read_cycles")
        return cyc, st

    def set_table_factor(self, slots_per_kminmer):
        """Table slots per inserted k-min-mer (default 8; 2 for file-fed, host-bound runs).  Before reserve_table / finalize."""
        if self._L.mq_index_set_table_factor(self._h, int(slots_per_kminmer)) != 0:
            raise _err(self._L, "mq_index_set_table_factor")

    def get_params(self):
        """The parameters the index was built with (a loaded file's own)."""
        p = Params()
        if self._L.mq_index_get_params(self._h, C.byref(p)) != 0:
            raise _err(self._L, "mq_index_get_params")
        return p

    def set_map_params(self, c, s, g, fold_case=False):
        """Params.c / .s / .g (src/chain.rs:132-169) and the case folding act at mapping time only: a loaded index takes the caller's."""
        if self._L.mq_index_set_map_params(self._h, int(c), int(s), int(g), 1 if fold_case else 0) != 0:
            raise _err(self._L, "mq_index_set_map_params")

    def stage_begin(self, total_bytes):
        """The reference file in pieces (mq_index_stage_*): a device buffer of the file's size."""
        if self._L.mq_index_stage_begin(self._h, int(total_bytes)) != 0:
            raise _err(self._L, "mq_index_stage_begin")

    def stage_piece(self, at, piece):
        """Queues the copy of `piece` (uint8 array; page-locked for the full rate) to buffer offset `at`; returns the ticket."""
        s = _seq(piece)
        t = C.c_uint64()
        if self._L.mq_index_stage_piece(self._h, int(at), _p(s), s.size, C.byref(t)) != 0:
            raise _err(self._L, "mq_index_stage_piece")
        self._staged = getattr(self, "_staged", {})
        self._staged[t.value] = s  # the source stays alive until its copy is known to be done (stage_done) or the index is finalized
        return t.value

    def stage_done(self, ticket, wait=True):
        r = self._L.mq_index_stage_done(self._h, int(ticket), 1 if wait else 0)
        if r < 0:
            raise _err(self._L, "mq_index_stage_done")
        if r:  # copies complete in order: every source up to this ticket can go
            st = getattr(self, "_staged", {})
            for t in [t for t in st if t <= int(ticket)]:
                del st[t]
        return bool(r)

    def add_ref_staged(self, ref_idx, name, at, length, after_ticket=None):
        """ref_extract of the staging buffer's [at, at + length), behind piece `after_ticket` (None: every piece issued so far)."""
        t = 0xFFFFFFFFFFFFFFFF if after_ticket is None else int(after_ticket)
        n = self._L.mq_index_add_ref_staged(self._h, ref_idx, name.encode(), int(at), int(length), t)
        if n < 0:
            raise _err(self._L, "mq_index_add_ref_staged")
        return n

    def add_ref_staged_lines(self, ref_idx, name, at, nbytes, after_ticket=None):
        """add_ref_staged for a line-wrapped record: the staging buffer's [at, at + nbytes) is everything behind the header line; its
        lines are joined on the device.  Returns (k-min-mer count, joined length)."""
        t = 0xFFFFFFFFFFFFFFFF if after_ticket is None else int(after_ticket)
        ln = C.c_uint64()
        n = self._L.mq_index_add_ref_staged_lines(self._h, ref_idx, name.encode(), int(at), int(nbytes), t, C.byref(ln))
        if n < 0:
            raise _err(self._L, "mq_index_add_ref_staged_lines")
        return n, ln.value

    def staged_sequence(self, at, nbytes, after_ticket=None):
        """Parity / debug: the joined bytes of the staging buffer's [at, at + nbytes) as a uint8 array."""
        t = 0xFFFFFFFFFFFFFFFF if after_ticket is None else int(after_ticket)
        n = self._L.mq_index_staged_sequence(self._h, int(at), int(nbytes), t, None, 0)  # (no buffer: the checks, and the length alone)
        if n < 0:
            raise _err(self._L, "mq_index_staged_sequence")
        out = np.empty(n, dtype=np.uint8)
        if n and self._L.mq_index_staged_sequence(self._h, int(at), int(nbytes), t, _p(out), n) != n:
            raise _err(self._L, "mq_index_staged_sequence")
        return out

    def reserve_table(self, expected_kminmers):
        """DashMap::with_capacity (src/index.rs:83): the table for about this many k-min-mers is allocated and cleared in the background."""
        if self._L.mq_index_reserve(self._h, int(expected_kminmers)) != 0:
            raise _err(self._L, "mq_index_reserve")

    def finalize(self):
        """get_count + into_read_only (src/closures.rs:92-94): returns the unique k-min-mer count."""
        n = self._L.mq_index_finalize(self._h)
        if n < 0:
            raise _err(self._L, "mq_index_finalize")
        self._staged = {}  # every staged piece has been indexed: the sources can go
        return n

    def stats(self):
        st = IndexStats()
        if self._L.mq_index_get_stats(self._h, C.byref(st)) != 0:
            raise _err(self._L, "mq_index_get_stats")
        return {n: getattr(st, n) for n, _ in IndexStats._fields_}

    def ref_info(self, ref_id):
        name, ln = C.c_char_p(), C.c_uint64()
        if self._L.mq_index_ref_info(self._h, ref_id, C.byref(name), C.byref(ln)) != 0:
            raise _err(self._L, "mq_index_ref_info")
        return name.value.decode(), ln.value

    def map_batch(self, bases, offsets):
        """find_matches for every read (host buffers)."""
        bases = _seq(bases)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out = np.zeros(max(n, 0), dtype=hit_dtype)
        if n > 0 and self._L.mq_map_batch(self._h, _p(bases), _p(offsets), n, _p(out)) != 0:
            raise _err(self._L, "mq_map_batch")
        return out

    def map_batch_device(self, d_bases, d_offsets, n, total_bases, d_out, stream=0):
        """find_matches for n device-resident reads; total_bases = offsets[n] - offsets[0]."""
        rc = self._L.mq_map_batch_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n, int(total_bases), C.c_void_p(d_out),
                                         C.c_void_p(stream))
        if rc != 0:
            raise _err(self._L, "mq_map_batch_device")

    def reserve(self, n_reads, total_bases):
        if self._L.mq_map_reserve(self._h, n_reads, int(total_bases)) != 0:
            raise _err(self._L, "mq_map_reserve")

    def reserve_redo(self, max_reads, max_read_len):
        """A redo arena for map_batch_device (the default context): up to max_reads overflow reads of up to max_read_len bases are finished
        on the device, in stream, instead of coming back with status MQ_HIT_OVERFLOW.  max_reads = 0 releases it."""
        if self._L.mq_map_reserve_redo(self._h, int(max_reads), int(max_read_len)) != 0:
            raise _err(self._L, "mq_map_reserve_redo")

    def redo_counts(self):
        """(reads redone, reads left with MQ_HIT_OVERFLOW) of the last map_batch_device call; waits for its stream."""
        a, b = C.c_uint32(), C.c_uint32()
        if self._L.mq_map_redo_counts(self._h, C.byref(a), C.byref(b)) != 0:
            raise _err(self._L, "mq_map_redo_counts")
        return a.value, b.value

    def reserve_anchors(self, max_reads, max_anchors):
        """Context.reserve_anchors for the default context (map_batch, map_batch_device); (0, 0) releases."""
        _reserve_pooled(self._L, "mq_map_reserve_anchors", self._h, max_reads, max_anchors)

    def anchors(self):
        """Context.anchors for the default context."""
        return _pooled(self._L, "mq_map_anchors", self._h, anchor_span_dtype, anchor_dtype)

    def reserve_chains(self, max_reads, max_chains):
        """Context.reserve_chains for the default context (map_batch, map_batch_device); (0, 0) releases."""
        _reserve_pooled(self._L, "mq_map_reserve_chains", self._h, max_reads, max_chains)

    def chains(self):
        """Context.chains for the default context."""
        return _pooled(self._L, "mq_map_chains", self._h, chain_span_dtype, chain_dtype)

    def format_paf_chain(self, q_id, q_len, chain):
        """The twelve PAF columns of any chain of chains() (mq_format_paf_chain)."""
        rec = np.zeros(1, dtype=chain_dtype)
        rec[0] = chain
        cap = 4096
        while True:
            buf = C.create_string_buffer(cap)
            w = self._L.mq_format_paf_chain(self._h, q_id.encode(), int(q_len), _p(rec), buf, cap)
            if w < 0:
                raise _err(self._L, "mq_format_paf_chain")
            if w < cap:
                return buf.value.decode()
            cap = w + 1

    def context(self):
        """A stream slot (mq_ctx): own stream, scratch and staging; contexts of one finalized index may map concurrently."""
        return Context(self)

    def last_map_ms(self):
        ms = C.c_float()
        if self._L.mq_last_map_ms(self._h, C.byref(ms)) != 0:
            raise _err(self._L, "mq_last_map_ms")
        return ms.value

    def last_stage_clocks(self):
        """Diagnostic (-DMQ_STAGE_CLOCKS builds): cycles per stage of the last launch, summed over waves (16 stages)."""
        out = (C.c_uint64 * 16)()
        if self._L.mq_last_stage_clocks(self._h, out) != 0:
            raise _err(self._L, "mq_last_stage_clocks")
        return [int(x) for x in out]

    def probe_stats(self, d_bases, d_offsets, n, total_bases, d_out):
        """(index lookups, slots visited beyond the home slot) of one instrumented launch: p-bar = 1 + extra / lookups."""
        a, b = C.c_uint64(), C.c_uint64()
        if self._L.mq_map_probe_stats(self._h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n, int(total_bases), C.c_void_p(d_out),
                                      C.byref(a), C.byref(b)) != 0:
            raise _err(self._L, "mq_map_probe_stats")
        return a.value, b.value

    def probe_rate(self, blocks, per_thread, bitmap_log2=0, table_too=1):
        """Diagnostic: (ms, lookups, extra steps) of blocks*256 threads probing per_thread random absent keys each."""
        ms, a, b = C.c_float(), C.c_uint64(), C.c_uint64()
        if self._L.mq_probe_rate(self._h, blocks, per_thread, bitmap_log2, table_too, C.byref(ms), C.byref(a), C.byref(b)) != 0:
            raise _err(self._L, "mq_probe_rate")
        return ms.value, a.value, b.value

    def last_map_path_counts(self):
        """(reads through the fast seeding path, reads through the general path) of the last launch."""
        a, b = C.c_uint32(), C.c_uint32()
        if self._L.mq_last_map_path_counts(self._h, C.byref(a), C.byref(b)) != 0:
            raise _err(self._L, "mq_last_map_path_counts")
        return a.value, b.value

    def last_map_spec(self):
        """Which compiled-for-its-parameters kernel pair the last launch ran (include/mapquik_hip_diag.h); 0: the run-time pair."""
        a = C.c_uint32()
        if self._L.mqdiag_last_map_spec(self._h, C.byref(a)) != 0:
            raise _err(self._L, "mqdiag_last_map_spec")
        return a.value

    def table_alloc_ms(self):
        """What allocating + clearing this index's table took (on mq_index_reserve's thread or inside finalize), in ms."""
        ms = C.c_float()
        if self._L.mq_index_table_alloc_ms(self._h, C.byref(ms)) != 0:
            raise _err(self._L, "mq_index_table_alloc_ms")
        return ms.value

    def launch_waves(self, n_reads):
        """Persistent waves map_kernel employs for a launch of n_reads reads (wave w owns work items w and n_waves + w)."""
        a = C.c_uint32()
        if self._L.mq_map_launch_waves(self._h, int(n_reads), C.byref(a)) != 0:
            raise _err(self._L, "mq_map_launch_waves")
        return a.value

    def last_map_order(self):
        """(reads the ordering pass of the last launch took for short-period tandem arrays, reads it put first)."""
        a, b = C.c_uint32(), C.c_uint32()
        if self._L.mq_last_map_order(self._h, C.byref(a), C.byref(b)) != 0:
            raise _err(self._L, "mq_last_map_order")
        return a.value, b.value

    def kminmers_batch(self, bases, offsets, caps=None):
        """KminmersIterator output per sequence (src/mers.rs:41-54): list of structured arrays."""
        bases = _seq(bases)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        if caps is None:  # one k-min-mer per base is an upper bound
            caps = (offsets[1:] - offsets[:-1]).astype(np.uint64)
        koff = np.zeros(n + 1, dtype=np.uint64)
        koff[1:] = np.cumsum(np.asarray(caps, dtype=np.uint64))
        out = np.zeros(int(koff[-1]), dtype=kminmer_dtype)
        counts = np.zeros(n, dtype=np.uint32)
        if n > 0 and self._L.mq_kminmers_batch(self._h, _p(bases), _p(offsets), n, _p(koff), _p(out), _p(counts)) != 0:
            raise _err(self._L, "mq_kminmers_batch")
        res = []
        for i in range(n):
            c = int(counts[i])
            if c > int(koff[i + 1] - koff[i]):
                raise MapquikError("k-min-mer window too small for sequence %d: %d > %d" % (i, c, int(koff[i + 1] - koff[i])))
            res.append(out[int(koff[i]):int(koff[i]) + c].copy())
        return res

    def lookup(self, hashes):
        """ReadOnlyIndex::get (src/index.rs:118-126) for many hashes."""
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        n = h.size
        found = np.zeros(n, dtype=np.uint8)
        ent = np.zeros(n, dtype=kminmer_dtype)
        ids = np.zeros(n, dtype=np.uint32)
        if n > 0 and self._L.mq_index_lookup(self._h, _p(h), n, _p(found), _p(ent), _p(ids)) != 0:
            raise _err(self._L, "mq_index_lookup")
        return found, ent, ids

    def format_paf(self, q_id, q_len, hit):
        rec = np.zeros(1, dtype=hit_dtype)
        rec[0] = hit
        cap = 4096
        while True:
            buf = C.create_string_buffer(cap)
            w = self._L.mq_format_paf(self._h, q_id.encode(), int(q_len), _p(rec), buf, cap)
            if w < 0:
                raise _err(self._L, "mq_format_paf")
            if w < cap:  # the return value is the full line length (snprintf): never hand back a cut line
                return buf.value.decode()
            cap = w + 1

    def paf_lines(self, names, offsets, hits):
        """PAF text in input order; unmapped reads produce no line (src/closures.rs:117-123)."""
        out = []
        for i, name in enumerate(names):
            st = int(hits[i]["status"])
            if st == MQ_HIT_OVERFLOW:
                raise MapquikError("read %s: Match-run scratch overflow (raise MQ_MATCH_CAP)" % name)
            if st == MQ_HIT_MAPPED:
                out.append(self.format_paf(name, int(offsets[i + 1] - offsets[i]), hits[i]))
        return out


class Context:
    """mq_ctx: one stream slot of a finalized index (the reference's per-thread worker, src/closures.rs:183,187)."""

    def __init__(self, index):
        self._L = index._L
        self._index = index  # keeps the index alive
        self._h = self._L.mq_ctx_new(index.handle)
        if not self._h:
            raise _err(self._L, "mq_ctx_new")
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            self._L.mq_ctx_free(self._h)
            self._h = None

    __del__ = close

    def map_batch(self, bases, offsets):
        bases = _seq(bases)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out = np.zeros(max(n, 0), dtype=hit_dtype)
        if n > 0 and self._L.mq_ctx_map_batch(self._h, _p(bases), _p(offsets), n, _p(out)) != 0:
            raise _err(self._L, "mq_ctx_map_batch")
        return out

    def submit(self, bases, offsets):
        """Queue a batch on the context's stream; wait() returns its hits."""
        bases = _seq(bases)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out = np.zeros(max(n, 0), dtype=hit_dtype)
        if n > 0 and self._L.mq_ctx_submit(self._h, _p(bases), _p(offsets), n, _p(out)) != 0:
            raise _err(self._L, "mq_ctx_submit")
        self._keep = (bases, offsets, out)

    def submit_spans(self, buf, starts, lens):
        """Queue reads given as spans of a raw buffer (FASTX bytes as they are): read i = buf[starts[i] : starts[i] + lens[i]]."""
        buf = _seq(buf)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        n = starts.size
        out = np.zeros(max(n, 0), dtype=hit_dtype)
        if n > 0 and self._L.mq_ctx_submit_spans(self._h, _p(buf), buf.size, _p(starts), _p(lens), n, _p(out)) != 0:
            raise _err(self._L, "mq_ctx_submit_spans")
        self._keep = (buf, starts, out, lens)

    def submit_fasta(self, buf, begin=0, fastq=False, lines=False):
        """Queue a piece of an uncompressed FASTA (or, fastq=True, four-line FASTQ) file that holds whole records (buf[begin:]): the
        records are found on the device.  lines=True (MQ_FASTX_FASTA_LINES): FASTA records whose sequences may run over several lines,
        joined on the device; such a piece is finished with wait_fasta_lines()."""
        if fastq and lines:
            raise ValueError("fastq and lines exclude each other: only FASTA records are joined on the device")
        buf = _seq(buf)
        if fastq or lines:
            if self._L.mq_ctx_submit_fastx(self._h, _p(buf), int(begin), buf.size, 1 if fastq else 2) != 0:
                raise _err(self._L, "mq_ctx_submit_fastx")
        elif self._L.mq_ctx_submit_fasta(self._h, _p(buf), int(begin), buf.size) != 0:
            raise _err(self._L, "mq_ctx_submit_fasta")
        self._keep = (buf,)

    def wait_fasta(self):
        """(hits, line_ends, flags) of the piece submitted with submit_fasta; flags & 1 (MQ_FASTA_IRREGULAR): not two lines per record, nothing mapped."""
        n, nl, fl = C.c_uint32(), C.c_uint32(), C.c_uint32()
        le, hp = C.c_void_p(), C.c_void_p()
        if self._L.mq_ctx_wait_fasta(self._h, C.byref(n), C.byref(le), C.byref(nl), C.byref(hp), C.byref(fl)) != 0:
            raise _err(self._L, "mq_ctx_wait_fasta")
        self._keep = None
        if fl.value & 1 or n.value == 0:
            return np.zeros(0, dtype=hit_dtype), np.zeros(0, dtype=np.uint32), fl.value
        hits = np.frombuffer(C.string_at(hp.value, n.value * hit_dtype.itemsize), dtype=hit_dtype).copy()
        lines = np.frombuffer(C.string_at(le.value, nl.value * 4), dtype=np.uint32).copy()
        return hits, lines, fl.value

    def wait_fasta_lines(self):
        """(hits, hdr_begin, hdr_end, seq_lens, flags) of the piece submitted with submit_fasta(lines=True): header r is
        buf[hdr_begin[r]:hdr_end[r]], seq_lens[r] the joined length of read r.  flags & 1 (MQ_FASTA_IRREGULAR) or no record: empty arrays."""
        n, fl = C.c_uint32(), C.c_uint32()
        hb, he, sl, hp = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self._L.mq_ctx_wait_fasta_lines(self._h, C.byref(n), C.byref(hb), C.byref(he), C.byref(sl), C.byref(hp), C.byref(fl)) != 0:
            raise _err(self._L, "mq_ctx_wait_fasta_lines")  # (MQ_ESTATE: the piece in flight, if any, is still pending)
        self._keep = None
        if fl.value & 1 or n.value == 0:
            e = np.zeros(0, dtype=np.uint32)
            return np.zeros(0, dtype=hit_dtype), e, e.copy(), e.copy(), fl.value
        hits = np.frombuffer(C.string_at(hp.value, n.value * hit_dtype.itemsize), dtype=hit_dtype).copy()
        u = [np.frombuffer(C.string_at(q.value, n.value * 4), dtype=np.uint32).copy() for q in (hb, he, sl)]
        return hits, u[0], u[1], u[2], fl.value

    def wait(self):
        if self._L.mq_ctx_wait(self._h) != 0:
            raise _err(self._L, "mq_ctx_wait")
        out = self._keep[2] if self._keep else np.zeros(0, dtype=hit_dtype)
        self._keep = None
        return out

    def map_batch_device(self, d_bases, d_offsets, n, total_bases, d_out, stream=0):
        if self._L.mq_ctx_map_batch_device(self._h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n, int(total_bases), C.c_void_p(d_out),
                                           C.c_void_p(stream)) != 0:
            raise _err(self._L, "mq_ctx_map_batch_device")

    def reserve_redo(self, max_reads, max_read_len):
        """Index.reserve_redo for this context's map_batch_device."""
        if self._L.mq_ctx_reserve_redo(self._h, int(max_reads), int(max_read_len)) != 0:
            raise _err(self._L, "mq_ctx_reserve_redo")

    def redo_counts(self):
        a, b = C.c_uint32(), C.c_uint32()
        if self._L.mq_ctx_redo_counts(self._h, C.byref(a), C.byref(b)) != 0:
            raise _err(self._L, "mq_ctx_redo_counts")
        return a.value, b.value

    def reserve_anchors(self, max_reads, max_anchors):
        """From now on every batch of up to max_reads reads mapped on this context also delivers the Match runs of each mapped read's winning
        chain, from a pool of max_anchors entries (include/mapquik_hip.h: mq_ctx_reserve_anchors).  (0, 0) releases."""
        _reserve_pooled(self._L, "mq_ctx_reserve_anchors", self._h, max_reads, max_anchors)

    def anchors(self):
        """(spans, anchors, info) of the context's last batch, which it finishes: read r's runs are anchors[spans[r]["first"]:][:spans[r]["count"]]
        in read order (first == MQ_ANCHORS_DROPPED: the pool was too small for them); info = dict(stored, needed, dropped_reads)."""
        return _pooled(self._L, "mq_ctx_anchors", self._h, anchor_span_dtype, anchor_dtype)

    def reserve_chains(self, max_reads, max_chains):
        """From now on every batch of up to max_reads reads mapped on this context also delivers every candidate chain of every read -- one per
        reference with a Match run in the read, ties included -- from a pool of max_chains entries (include/mapquik_hip.h:
        mq_ctx_reserve_chains).  (0, 0) releases."""
        _reserve_pooled(self._L, "mq_ctx_reserve_chains", self._h, max_reads, max_chains)

    def chains(self):
        """(spans, chains, info) of the context's last batch, which it finishes: read r's chains are chains[spans[r]["first"]:][:spans[r]["count"]]
        in the order of each reference's first run in the read (first == MQ_CHAINS_DROPPED: the pool was too small for them); info =
        dict(stored, needed, dropped_reads).  A read is mapped exactly when one of its chains has flags == MQ_CHAIN_TOP."""
        return _pooled(self._L, "mq_ctx_chains", self._h, chain_span_dtype, chain_dtype)

    def chains_device(self):
        """(device pointer of the spans, device pointer of the chains): the arrays a map_batch_device call on this context writes."""
        return _pooled_device(self._L, "mq_ctx_chains_device", self._h)

    def anchors_device(self):
        """(device pointer of the spans, device pointer of the anchors): the arrays a map_batch_device call on this context writes."""
        return _pooled_device(self._L, "mq_ctx_anchors_device", self._h)

    def last_map_ms(self):
        ms = C.c_float()
        if self._L.mq_ctx_last_map_ms(self._h, C.byref(ms)) != 0:
            raise _err(self._L, "mq_ctx_last_map_ms")
        return ms.value

    def last_map_spec(self):
        a = C.c_uint32()
        if self._L.mqdiag_ctx_last_map_spec(self._h, C.byref(a)) != 0:
            raise _err(self._L, "mqdiag_ctx_last_map_spec")
        return a.value


class Depth:
    """A depth accumulator (mq_depth) on a finalized index: per window of `window` bases of every reference, how many bases of the hits
    offered so far landed there, counting the mapped hits with mapq >= min_mapq (the rules: include/mapquik_hip.h).  It keeps its own
    snapshot of the index's reference ids and lengths; close it before its index."""

    def __init__(self, index, window=1000, min_mapq=60):
        self._L = index._L
        self.window, self.min_mapq = int(window), int(min_mapq)
        if not 0 <= self.window < 1 << 32 or not 0 <= self.min_mapq < 1 << 32:
            raise ValueError("window and min_mapq are 32-bit")
        h = C.c_void_p()
        if self._L.mq_depth_new(index._h, self.window, self.min_mapq, C.byref(h)) != 0:
            raise _err(self._L, "mq_depth_new")
        self._h = h.value

    def add(self, hits):
        """the structured array map_batch returns (host memory); the hits are in when the call returns"""
        hits = np.ascontiguousarray(hits, dtype=hit_dtype)
        if self._L.mq_depth_add(self._h, _p(hits), hits.size) != 0:
            raise _err(self._L, "mq_depth_add")

    def add_device(self, d_hits, n, stream=0):
        """n hits in device memory, asynchronous on `stream`: behind map_batch_device on the same stream it sees that call's final hits"""
        if self._L.mq_depth_add_device(self._h, C.c_void_p(d_hits), int(n), C.c_void_p(stream)) != 0:
            raise _err(self._L, "mq_depth_add_device")

    def result(self):
        """(refs, window_bases, window_starts, totals) as numpy copies: one ref_depth_dtype record per reference in id order (its windows are
        [first_window, first_window + n_windows) of the two window arrays), u64 bases and u32 hit starts per window, and the tallies as a
        dict.  Waits for the device; the accumulator goes on accumulating."""
        rp, bp, sp = C.c_void_p(), C.c_void_p(), C.c_void_p()
        nr, nw = C.c_uint64(), C.c_uint64()
        tot = np.zeros(1, dtype=depth_totals_dtype)
        if self._L.mq_depth_result(self._h, C.byref(rp), C.byref(nr), C.byref(bp), C.byref(sp), C.byref(nw), _p(tot)) != 0:
            raise _err(self._L, "mq_depth_result")
        refs = np.frombuffer(C.string_at(rp.value, nr.value * 64), dtype=ref_depth_dtype).copy() if nr.value else np.zeros(0, dtype=ref_depth_dtype)
        wb = np.frombuffer(C.string_at(bp.value, nw.value * 8), dtype="<u8").copy() if nw.value else np.zeros(0, dtype="<u8")
        ws = np.frombuffer(C.string_at(sp.value, nw.value * 4), dtype="<u4").copy() if nw.value else np.zeros(0, dtype="<u4")
        return refs, wb, ws, {n: int(tot[0][n]) for n in depth_totals_dtype.names}

    def clear(self):
        if self._L.mq_depth_clear(self._h) != 0:
            raise _err(self._L, "mq_depth_clear")

    def close(self):
        if getattr(self, "_h", None):
            self._L.mq_depth_free(self._h)
            self._h = None

    __del__ = close


class Sorter:
    """A coordinate sorter (mq_sorter) on a finalized index: the permutation that orders the hits offered so far by (ref_id, r_start,
    ordinal), keeping the mapped hits with mapq >= min_mapq on references of its snapshot (the rules: include/mapquik_hip.h).  `capacity`
    counts offered hits: add() grows the sorter, add_device() never does.  Close it before its index."""

    def __init__(self, index, capacity=0, min_mapq=0):
        self._L = index._L
        self.min_mapq = int(min_mapq)
        if not 0 <= self.min_mapq < 1 << 32 or not 0 <= int(capacity) < 1 << 64:
            raise ValueError("min_mapq is 32-bit, capacity 64-bit")
        h = C.c_void_p()
        if self._L.mq_sort_new(index._h, int(capacity), self.min_mapq, C.byref(h)) != 0:
            raise _err(self._L, "mq_sort_new")
        self._h = h.value

    def add(self, hits, first_ordinal):
        """the structured array map_batch returns (host memory); hit i carries the ordinal first_ordinal + i; in when the call returns"""
        hits = np.ascontiguousarray(hits, dtype=hit_dtype)
        if self._L.mq_sort_add(self._h, _p(hits), hits.size, int(first_ordinal)) != 0:
            raise _err(self._L, "mq_sort_add")

    def add_device(self, d_hits, n, first_ordinal, stream=0):
        """n hits in device memory, asynchronous on `stream`: behind map_batch_device on the same stream it sees that call's final hits"""
        if self._L.mq_sort_add_device(self._h, C.c_void_p(d_hits), int(n), int(first_ordinal), C.c_void_p(stream)) != 0:
            raise _err(self._L, "mq_sort_add_device")

    def reserve(self, capacity):
        if self._L.mq_sort_reserve(self._h, int(capacity)) != 0:
            raise _err(self._L, "mq_sort_reserve")

    def result(self):
        """(order, refs, totals) as numpy copies: the kept hits' ordinals in sorted order (u32), one sort_ref_dtype record per reference in
        id order (its hits are order[first : first + count]) and the tallies as a dict.  Waits for the device; more adds may follow."""
        op, rp = C.c_void_p(), C.c_void_p()
        nk, nr = C.c_uint64(), C.c_uint64()
        tot = np.zeros(1, dtype=sort_totals_dtype)
        if self._L.mq_sort_result(self._h, C.byref(op), C.byref(nk), C.byref(rp), C.byref(nr), _p(tot)) != 0:
            raise _err(self._L, "mq_sort_result")
        order = np.frombuffer(C.string_at(op.value, nk.value * 4), dtype="<u4").copy() if nk.value else np.zeros(0, dtype="<u4")
        refs = np.frombuffer(C.string_at(rp.value, nr.value * 24), dtype=sort_ref_dtype).copy() if nr.value else np.zeros(0, dtype=sort_ref_dtype)
        return order, refs, {n: int(tot[0][n]) for n in sort_totals_dtype.names}

    def passes(self):
        """how many of the key's 11 digits the last result() sorted"""
        v = C.c_uint32()
        if self._L.mqdiag_sort_passes(self._h, C.byref(v)) != 0:
            raise _err(self._L, "mqdiag_sort_passes")
        return v.value

    def result_ms(self):
        v = C.c_float()
        if self._L.mqdiag_sort_result_ms(self._h, C.byref(v)) != 0:
            raise _err(self._L, "mqdiag_sort_result_ms")
        return v.value

    def clear(self):
        if self._L.mq_sort_clear(self._h) != 0:
            raise _err(self._L, "mq_sort_clear")

    def close(self):
        if getattr(self, "_h", None):
            self._L.mq_sort_free(self._h)
            self._h = None

    __del__ = close


def format_sorted_tsv(index, refs, line_offsets):
    """<prefix>.sorted.tsv of --sort: a header line, then per reference of Sorter.result() its name, length, lines, first line (0-based)
    and the byte offset of that line in <prefix>.sorted.paf -- a seek table.  line_offsets[j]: where sorted line j begins (n_kept + 1
    entries, the last one the file's size)."""
    out = [b"#ref\tlen\tlines\tfirst_line\toffset\n"]
    for r in refs:
        name, ln = index.ref_info(int(r["ref_id"]))
        out.append(b"%s\t%d\t%d\t%d\t%d\n" % (name.encode(), ln, int(r["count"]), int(r["first"]), int(line_offsets[int(r["first"])])))
    return b"".join(out)


def format_depth_bed(index, refs, window_bases, window_starts, window):
    """<prefix>.depth.bed of --depth: `r_name\tstart\tend\tbases\tstarts\tmean\n` per window of Depth.result(), references in id order; mean is
    bases / (end - start) as %.2f"""
    out = []
    w = int(window)
    for r in refs:
        name = index.ref_info(int(r["ref_id"]))[0].encode()
        first, ln = int(r["first_window"]), int(r["len"])
        for j in range(int(r["n_windows"])):
            a, b = j * w, min((j + 1) * w, ln)
            bases = int(window_bases[first + j])
            out.append(b"%s\t%d\t%d\t%d\t%d\t%.2f\n" % (name, a, b, bases, int(window_starts[first + j]), bases / (b - a)))
    return b"".join(out)


def format_depth_tsv(index, refs, window):
    """<prefix>.depth.tsv of --depth: a header line, then one line per reference; mean is bases / len, max_window_mean the largest
    window_bases over a window's width, min(window, len), both as %.2f"""
    out = [b"#ref\tlen\treads\tbases\tmean\tzero_windows\tmax_window_mean\n"]
    for r in refs:
        name = index.ref_info(int(r["ref_id"]))[0].encode()
        ln = int(r["len"])
        out.append(b"%s\t%d\t%d\t%d\t%.2f\t%d\t%.2f\n" % (name, ln, int(r["reads"]), int(r["bases"]), int(r["bases"]) / ln, int(r["zero_windows"]),
                                                        int(r["max_window_bases"]) / min(int(window), ln)))
    return b"".join(out)


def format_coverage_bed(index, refs, intervals):
    """<prefix>.coverage.bed of --coverage: `r_name\tstart\tend\n` per interval of Index.coverage(), references in id order"""
    out = []
    for r in refs:
        name = index.ref_info(int(r["ref_id"]))[0].encode()
        a = int(r["first_interval"])
        for iv in intervals[a:a + int(r["n_intervals"])]:
            out.append(b"%s\t%d\t%d\n" % (name, int(iv["start"]), int(iv["end"])))
    return b"".join(out)


def format_coverage_tsv(index, refs):
    """<prefix>.coverage.tsv of --coverage: a header line, then one line per reference; the fraction is covered / len as %.6f"""
    out = [b"#ref\tlen\tlive_kminmers\tcovered\tfraction\tintervals\n"]
    for r in refs:
        name = index.ref_info(int(r["ref_id"]))[0].encode()
        out.append(b"%s\t%d\t%d\t%d\t%.6f\t%d\n" % (name, int(r["len"]), int(r["live_kminmers"]), int(r["covered_bases"]),
                                                    int(r["covered_bases"]) / int(r["len"]), int(r["n_intervals"])))
    return b"".join(out)


def ref_extract(ref_idx, inp_seq_raw, params, mers_index, name=None):
    """mers::ref_extract (src/mers.rs:15-38) + ref_map.insert (src/closures.rs:49)."""
    assert params is mers_index.params or bytes(params) == bytes(mers_index.params)
    return mers_index.add_ref(ref_idx, name if name is not None else str(ref_idx), inp_seq_raw)


def find_matches(q_id, q_len, q_str, ref_map, mers_index, params):
    """mers::find_matches (src/mers.rs:77-102): the PAF line or None.  ref_map is carried by the index."""
    s = _seq(q_str)
    assert q_len == s.size
    hits = mers_index.map_batch(s, np.array([0, s.size], dtype=np.uint64))
    lines = mers_index.paf_lines([q_id], [0, s.size], hits)
    return lines[0] if lines else None
