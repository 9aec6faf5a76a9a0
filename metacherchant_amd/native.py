"""ctypes binding of libmcgpu.so (include/mcgpu.h).  Thin: argument marshalling and error
translation only.  There is no CPU fallback: if the HIP library is missing or no MI355X is
present, the calls raise."""
import ctypes as C
import os

import numpy as np

from . import build as _build

KEY_PACKED, KEY_POLY, KEY_FNV1A = 0, 1, 2
FLAG_SOLID_LIST = 1  # mc_config.flags: this context is a shard whose solid k-mers will be exported
MC_ENOSEED = -6


class McError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmcgpu error %d: %s" % (code, msg))
        self.code = code


class _Config(C.Structure):
    _fields_ = [("k", C.c_int32), ("key_mode", C.c_int32), ("device", C.c_int32), ("flags", C.c_int32),
                ("capacity_hint", C.c_uint64)]


class _BfsResult(C.Structure):
    _fields_ = [("n", C.c_uint64), ("hi", C.POINTER(C.c_uint64)), ("lo", C.POINTER(C.c_uint64)),
                ("dist", C.POINTER(C.c_int32)), ("cov", C.POINTER(C.c_int16)), ("last", C.POINTER(C.c_uint8)),
                ("levels", C.c_uint64), ("lookups", C.c_uint64), ("rounds", C.c_uint64), ("device_ms", C.c_double)]


class _BfsJob(C.Structure):
    _fields_ = [("seed_hi", C.POINTER(C.c_uint64)), ("seed_lo", C.POINTER(C.c_uint64)), ("n_seeds", C.c_uint64),
                ("dir", C.c_int32)]


class _ResultOwner:
    """Keeps one mc_bfs_result alive for the numpy views of its arrays; frees it with the last of them."""

    def __init__(self, lib, res):
        self._lib = lib
        self._res = _BfsResult()
        C.memmove(C.byref(self._res), C.byref(res), C.sizeof(_BfsResult))

    def __del__(self):
        try:
            self._lib.mc_bfs_result_free(C.byref(self._res))
        except Exception:  # (interpreter shutdown)
            pass


class Stats(C.Structure):
    _fields_ = [("windows", C.c_uint64), ("count_launches", C.c_uint64), ("count_ms", C.c_double),
                ("count_total_ms", C.c_double), ("table_slots", C.c_uint64), ("table_bytes", C.c_uint64),
                ("grows", C.c_uint64), ("p1_ms", C.c_double), ("p2_ms", C.c_double), ("p3_ms", C.c_double),
                ("spill_keys", C.c_uint64), ("solid_kmers", C.c_uint64), ("solid_sweeps", C.c_uint64),
                ("solid_list_builds", C.c_uint64), ("long_runs", C.c_uint64), ("dup_keys", C.c_uint64),
                ("dup_checks", C.c_uint64), ("dup_ms", C.c_double), ("dup_unchecked", C.c_uint64), ("left_bins", C.c_uint64),
                ("binned_runs", C.c_uint64)]


class ReadCov(C.Structure):
    """mc_read_cov: one read's coverage in the table (include/mcgpu.h mc_classify_reads)"""
    _fields_ = [("sum", C.c_int32), ("covered", C.c_int32), ("last", C.c_int16), ("found", C.c_uint8), ("pad", C.c_uint8)]


class _WalkOrder(C.Structure):
    """mc_walk_order_result"""
    _fields_ = [("n_components", C.c_uint64), ("n_kmers", C.c_uint64), ("reached", C.POINTER(C.c_uint64)), ("order", C.POINTER(C.c_uint32)),
                ("twice", C.POINTER(C.c_uint8)), ("levels", C.c_uint64), ("queue_entries", C.c_uint64), ("wide_levels", C.c_uint64),
                ("device_ms", C.c_double)]


class _Components(C.Structure):
    """mc_components_result"""
    _fields_ = [("n_components", C.c_uint64), ("n_kmers", C.c_uint64), ("comp_offsets", C.POINTER(C.c_uint64)),
                ("seed_seq", C.POINTER(C.c_uint64)), ("seed_pos", C.POINTER(C.c_uint64)), ("hi", C.POINTER(C.c_uint64)),
                ("lo", C.POINTER(C.c_uint64)), ("cov", C.POINTER(C.c_int16)), ("device_ms", C.c_double)]


class _Unitigs(C.Structure):
    """mc_unitigs_result"""
    _fields_ = [("n_nodes", C.c_uint64), ("deg", C.POINTER(C.c_uint8)), ("nbr", C.POINTER(C.c_uint32)), ("n_unitigs", C.c_uint64),
                ("first", C.POINTER(C.c_uint32)), ("last_rc", C.POINTER(C.c_uint32)), ("base_offsets", C.POINTER(C.c_uint64)),
                ("bases", C.POINTER(C.c_uint64)), ("n_irregular", C.c_uint64), ("irregular", C.POINTER(C.c_uint32)), ("device_ms", C.c_double)]


class _EnvJoin(C.Structure):
    """mc_env_join_result"""
    _fields_ = [("n", C.c_uint64), ("n_graphs", C.c_uint32), ("member", C.POINTER(C.c_uint64)), ("is_gene", C.POINTER(C.c_uint8)),
                ("kc", C.POINTER(C.c_int64)), ("diff", C.POINTER(C.c_uint32)), ("diff_alt", C.POINTER(C.c_uint32)), ("uni", C.POINTER(C.c_uint32)),
                ("device_ms", C.c_double)]


class _WholeReads(C.Structure):
    """mc_whole_reads"""
    _fields_ = [("declined", C.c_int), ("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("d_words", C.c_void_p), ("d_offsets", C.c_void_p),
                ("d_bad_pos", C.c_void_p), ("d_codes", C.c_void_p), ("d_phred", C.c_void_p), ("device_ms", C.c_double)]


class _RenderSide(C.Structure):
    """mc_render_side"""
    _fields_ = [("words", C.c_void_p), ("phred", C.c_void_p), ("offsets", C.c_void_p), ("stream", C.c_void_p)]


class _RenderResult(C.Structure):
    """mc_render_result"""
    _fields_ = [("start", C.c_uint64 * 16), ("bytes", C.c_uint64 * 16), ("records", C.c_uint64 * 16), ("error", C.c_int32),
                ("error_side", C.c_uint32), ("error_read", C.c_uint64), ("error_value", C.c_uint32), ("device_ms", C.c_double)]


WHOLE_FASTA, WHOLE_FASTQ = 0, 1  # mc_tokenize_whole format
WHOLE_CODES, WHOLE_PHRED = 1, 2  # mc_tokenize_whole flags
READ_COV_DTYPE = np.dtype([("sum", np.int32), ("covered", np.int32), ("last", np.int16), ("found", np.uint8), ("pad", np.uint8)])
CLASSIFY_CORRECTION = 1  # mc_classify_reads flags: findReadWithCorrection
LAST_COPY_WEAK_FP = 1  # mc_reads_last_copy flags (tests only): a 4-bit first fingerprint, so distinct reads share one
CLASS_NOT_FOUND, CLASS_HALF_FOUND, CLASS_FOUND = 0, 1, 2  # mc_triple_classes
SEQ_COV_MAX_TABLES = 4  # mc_seq_coverage
PRESENCE_MAX_TABLES = 4  # mc_kmer_presence
RENDER_MAX_STREAMS, RENDER_SKIP, RENDER_UNNUMBERED = 16, 0xFF, 2**64 - 1  # mc_render_fastq
RENDER_EMPTY, RENDER_QUALITY, RENDER_STREAM = 1, 2, 3  # mc_render_result.error
WALK_ORDER_WIDE_ONLY, WALK_ORDER_NARROW_8 = 1, 2  # mc_walk_order flags (tests only): every level grid-wide; W = 8
READS_IN_SET_WEAK_FILTER = 1  # mc_reads_in_set flags (tests only): no bit filter, every window is looked up in the set's table


# every symbol include/mcgpu.h declares; tests check that the library exports all of them
EXPORTS = [
    "mc_abi_version", "mc_create", "mc_destroy", "mc_clear", "mc_set_coverage_hint", "mc_set_read_pointers", "mc_share_read_store", "mc_last_error", "mc_set_stream", "mc_add_reads_packed",
    "mc_add_reads_packed_dev", "mc_add_reads_file", "mc_finalize_counts", "mc_get", "mc_get_dev", "mc_kmer_keys", "mc_bfs", "mc_bfs_batch",
    "mc_bfs_result_free", "mc_export", "mc_export_dev", "mc_add_pairs_dev", "mc_solid_from_pairs_dev", "mc_save_kmers", "mc_load_kmers", "mc_key_owner", "mc_extract_keys_dev",
    "mc_group_create", "mc_group_destroy", "mc_group_last_error", "mc_group_set_coverage_hint", "mc_group_add_reads_packed", "mc_group_add_reads_file",
    "mc_group_finalize_counts", "mc_group_bfs_batch", "mc_group_get_stats", "mc_add_keys_dev", "mc_superkmer_capacity", "mc_extract_superkmers_dev", "mc_add_superkmers_dev",
    "mc_superkmer_fine_buckets", "mc_extract_superkmers_binned_dev", "mc_add_superkmers_binned_dev",
    "mc_read_store_seek", "mc_read_store_tell", "mc_read_store_import_dev", "mc_get_stats", "mc_reset_stats", "mc_trim", "mc_synth_reads_dev", "mc_synth_genome",
    "mc_shard_export", "mc_shard_attach", "mc_shard_detach", "mc_classify_reads", "mc_classify_reads_dev",
    "mc_reads_last_copy", "mc_reads_last_copy_dev", "mc_triple_classes", "mc_triple_classes_dev", "mc_seq_coverage", "mc_seq_coverage_dev",
    "mc_kmer_presence", "mc_kmer_presence_dev", "mc_reads_in_set", "mc_reads_in_set_dev",
    "mc_components", "mc_components_dev", "mc_components_free", "mc_unitigs", "mc_unitigs_dev", "mc_unitigs_free",
    "mc_env_join", "mc_env_join_dev", "mc_env_join_free", "mc_trim_paths", "mc_trim_paths_dev",
    "mc_walk_order", "mc_walk_order_dev", "mc_walk_order_free",
    "mc_kmers_encode_dev", "mc_kmers_decode_dev", "mc_save_kmers_gpu", "mc_load_kmers_gpu",
    "mc_tokenize_whole", "mc_tokenize_whole_dev", "mc_whole_text_bytes", "mc_whole_reads_to_host", "mc_whole_reads_free", "mc_reads_append_dev",
    "mc_render_fastq", "mc_render_fastq_dev", "mc_render_fastq_bound",
]

_LIB = None


def lib_path():
    """The product library; MC_LIB=<path> selects a tuning build instead (metacherchant_amd/build.py build_lib(variant=...))."""
    return os.environ.get("MC_LIB") or _build.LIB


def load():
    """Loads libmcgpu.so (does not touch the GPU).  Raises if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError("libmcgpu.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(needs hipcc); there is no CPU fallback")
    # PyTorch-ROCm ships its own HIP runtime; it must be the first one initialised in a process that
    # uses both (the other order leaves torch with "No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp, u64, i64, i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_int
    u64p, i64p, i16p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int16)
    L.mc_abi_version.restype = i32
    L.mc_create.argtypes = [C.POINTER(_Config), C.POINTER(vp)]
    L.mc_destroy.argtypes = [vp]
    L.mc_destroy.restype = None
    L.mc_last_error.argtypes = [vp]
    L.mc_last_error.restype = C.c_char_p
    L.mc_set_stream.argtypes = [vp, vp]
    L.mc_clear.argtypes = [vp]
    L.mc_set_coverage_hint.argtypes = [vp, i32]
    L.mc_set_read_pointers.argtypes = [vp, i32]
    L.mc_share_read_store.argtypes = [vp, vp]
    L.mc_add_reads_packed.argtypes = [vp, u64p, u64p, u64]
    L.mc_add_reads_packed_dev.argtypes = [vp, vp, vp, u64, u64]
    L.mc_add_reads_file.argtypes = [vp, C.c_char_p, u64p]
    L.mc_finalize_counts.argtypes = [vp, u64p]
    L.mc_save_kmers.argtypes = [vp, C.c_char_p, C.c_char_p, i32, u64p, u64p]
    L.mc_load_kmers.argtypes = [vp, C.c_char_p, i32, u64p, u64p]
    if hasattr(L, "mc_kmers_encode_dev"):  # (MC_LIB may name a library built before the .kmers.bin unit)
        L.mc_kmers_encode_dev.argtypes = [vp, i32, vp, u64, vp, u64p, u64p]
        L.mc_kmers_decode_dev.argtypes = [vp, vp, u64, i32, vp, vp, u64p]
        L.mc_save_kmers_gpu.argtypes = [vp, C.c_char_p, C.c_char_p, i32, u64p, u64p]
        L.mc_load_kmers_gpu.argtypes = [vp, C.c_char_p, i32, u64p, u64p]
    L.mc_get.argtypes = [vp, i64p, u64, i16p]
    L.mc_get_dev.argtypes = [vp, vp, u64, vp]
    L.mc_kmer_keys.argtypes = [vp, u64p, u64p, u64, i64p]
    L.mc_bfs.argtypes = [vp, u64p, u64p, u64, i32, i32, i64, i64, C.POINTER(_BfsResult)]
    L.mc_bfs_batch.argtypes = [vp, C.POINTER(_BfsJob), C.c_uint32, i32, i64, i64, C.POINTER(_BfsResult)]
    L.mc_bfs_result_free.argtypes = [C.POINTER(_BfsResult)]
    L.mc_bfs_result_free.restype = None
    L.mc_export.argtypes = [vp, i32, i64p, i16p, u64, u64p]
    L.mc_export_dev.argtypes = [vp, i32, vp, vp, vp, u64, u64p]
    L.mc_add_pairs_dev.argtypes = [vp, vp, vp, vp, u64]
    L.mc_solid_from_pairs_dev.argtypes = [vp, vp, vp, vp, u64, i32, u64p]
    L.mc_key_owner.argtypes = [i64, C.c_uint32]
    L.mc_key_owner.restype = C.c_uint32
    L.mc_extract_keys_dev.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, vp, vp, u64, u64p]
    L.mc_add_keys_dev.argtypes = [vp, vp, vp, u64]
    L.mc_superkmer_capacity.argtypes = [vp, u64, u64]
    L.mc_superkmer_capacity.restype = u64
    L.mc_extract_superkmers_dev.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, vp, vp, u64, u64p]
    L.mc_add_superkmers_dev.argtypes = [vp, vp, vp, u64]
    L.mc_read_store_seek.argtypes = [vp, u64, u64]
    L.mc_read_store_tell.argtypes = [vp]
    L.mc_read_store_tell.restype = u64
    L.mc_read_store_import_dev.argtypes = [vp, vp, u64, u64]
    L.mc_superkmer_fine_buckets.argtypes = [vp, C.c_uint32]
    L.mc_superkmer_fine_buckets.restype = C.c_uint32
    L.mc_extract_superkmers_binned_dev.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, C.c_uint32, vp, vp, u64, vp, u64p, u64p]
    L.mc_add_superkmers_binned_dev.argtypes = [vp, vp, vp, u64, u64, C.c_uint32, C.c_uint32, u64p, vp]
    L.mc_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.mc_reset_stats.argtypes = [vp]
    L.mc_trim.argtypes = [vp]
    L.mc_synth_reads_dev.argtypes = [vp, u64, u64, u64, u64, u64, u64, C.c_uint32, C.c_uint32, vp, vp]
    L.mc_synth_genome.argtypes = [u64, u64, u64, C.POINTER(C.c_uint8)]
    if hasattr(L, "mc_classify_reads"):  # (a tuning build of an older revision, MC_LIB)
        L.mc_classify_reads.argtypes = [vp, u64p, u64p, u64, C.POINTER(C.c_int32), i32, C.c_double, i32, C.POINTER(ReadCov)]
        L.mc_classify_reads_dev.argtypes = [vp, vp, vp, u64, vp, i32, C.c_double, i32, vp]
    if hasattr(L, "mc_reads_last_copy"):
        u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
        L.mc_reads_last_copy.argtypes = [vp, u64p, u64p, u64, i32, u32p]
        L.mc_reads_last_copy_dev.argtypes = [vp, vp, vp, u64, i32, vp]
        L.mc_triple_classes.argtypes = [vp, C.POINTER(ReadCov), C.POINTER(ReadCov), u64p, u64p, u64, i32, u8p, u8p, u32p, u32p, u8p, u8p]
        L.mc_triple_classes_dev.argtypes = [vp] + [vp] * 4 + [u64, i32] + [vp] * 6
    if hasattr(L, "mc_seq_coverage"):
        L.mc_seq_coverage.argtypes = [C.POINTER(vp), C.c_uint32, u64p, u64p, u64, vp]
        L.mc_seq_coverage_dev.argtypes = [C.POINTER(vp), C.c_uint32, vp, vp, u64, vp]
    if hasattr(L, "mc_kmer_presence"):
        L.mc_kmer_presence.argtypes = [C.POINTER(vp), C.c_uint32, u64p, u64p, u64, C.POINTER(C.c_uint8)]
        L.mc_kmer_presence_dev.argtypes = [C.POINTER(vp), C.c_uint32, vp, vp, u64, vp]
    if hasattr(L, "mc_reads_in_set"):
        L.mc_reads_in_set.argtypes = [vp, u64p, u64p, u64, u64p, u64p, u64, i32, i32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
        L.mc_reads_in_set_dev.argtypes = [vp, vp, vp, u64, vp, vp, u64, i32, i32, vp, vp]
    if hasattr(L, "mc_components"):
        L.mc_components.argtypes = [vp, u64p, u64p, u64, C.POINTER(_Components)]
        L.mc_components_dev.argtypes = [vp, vp, vp, u64, C.POINTER(_Components)]
        L.mc_components_free.argtypes = [C.POINTER(_Components)]
        L.mc_components_free.restype = None
    if hasattr(L, "mc_unitigs"):
        L.mc_unitigs.argtypes = [vp, u64p, u64p, C.POINTER(C.c_uint8), u64, C.POINTER(_Unitigs)]
        L.mc_unitigs_dev.argtypes = [vp, vp, vp, vp, u64, C.POINTER(_Unitigs)]
        L.mc_unitigs_free.argtypes = [C.POINTER(_Unitigs)]
        L.mc_unitigs_free.restype = None
    if hasattr(L, "mc_env_join"):
        i32p = C.POINTER(C.c_int32)
        L.mc_env_join.argtypes = [vp, u64p, u64p, u64, u64p, u64p, i32p, u64p, C.c_uint32, u64p, u64, C.POINTER(_EnvJoin)]
        L.mc_env_join_dev.argtypes = [vp, vp, vp, u64, vp, vp, vp, vp, C.c_uint32, vp, u64, C.POINTER(_EnvJoin)]
        L.mc_env_join_free.argtypes = [C.POINTER(_EnvJoin)]
        L.mc_env_join_free.restype = None
    if hasattr(L, "mc_trim_paths"):
        L.mc_trim_paths.argtypes = [vp, u64p, u64p, C.POINTER(C.c_uint8), u64, i32, C.POINTER(C.c_uint8), C.POINTER(C.c_double)]
        L.mc_trim_paths_dev.argtypes = [vp, vp, vp, vp, u64, i32, vp, C.POINTER(C.c_double)]
    if hasattr(L, "mc_walk_order"):
        L.mc_walk_order.argtypes = [vp, u64p, u64p, u64p, u64, C.c_uint32, C.POINTER(_WalkOrder)]
        L.mc_walk_order_dev.argtypes = [vp, vp, vp, vp, u64, C.c_uint32, C.POINTER(_WalkOrder)]
        L.mc_walk_order_free.argtypes = [C.POINTER(_WalkOrder)]
        L.mc_walk_order_free.restype = None
    if hasattr(L, "mc_tokenize_whole"):
        wr = C.POINTER(_WholeReads)
        L.mc_tokenize_whole.argtypes = [vp, C.c_char_p, u64, i32, i32, C.c_uint32, wr]
        L.mc_tokenize_whole_dev.argtypes = [vp, vp, u64, i32, i32, i32, C.c_uint32, wr]
        L.mc_whole_text_bytes.argtypes = [u64]
        L.mc_whole_text_bytes.restype = u64
        L.mc_whole_reads_to_host.argtypes = [vp, wr, vp, vp, vp, vp, vp]
        L.mc_whole_reads_free.argtypes = [vp, wr]
        L.mc_whole_reads_free.restype = None
        L.mc_reads_append_dev.argtypes = [vp, vp, vp, u64, vp, u64, vp]
    if hasattr(L, "mc_render_fastq"):
        rs, rr = C.POINTER(_RenderSide), C.POINTER(_RenderResult)
        L.mc_render_fastq_dev.argtypes = [vp, rs, C.c_uint32, u64, C.c_uint32, u64p, vp, u64, rr]
        L.mc_render_fastq.argtypes = [vp, rs, C.c_uint32, u64, C.c_uint32, u64p, vp, u64, rr]
        L.mc_render_fastq_bound.argtypes = [u64, u64]
        L.mc_render_fastq_bound.restype = u64
    if hasattr(L, "mc_shard_export"):  # (a tuning build of an older revision, MC_LIB: scripts/gpu_variants.sh)
        L.mc_shard_export.argtypes = [vp, C.c_char_p]
        L.mc_shard_attach.argtypes = [vp, C.c_char_p, C.c_uint32, C.c_uint32, i32]
        L.mc_shard_detach.argtypes = [vp]
    _LIB = L
    return L


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _dptr(x):
    """device pointer of a torch tensor (or a raw int).  The library works on its own HIP stream, so whatever
    torch still has queued for the tensor (the fill of a torch.zeros, a copy, a collective's result) must be
    done before the pointer is handed over: the tensor's current stream is synchronised here."""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if getattr(x, "is_cuda", False):
        import torch
        torch.cuda.current_stream(x.device).synchronize()
    return C.c_void_p(x.data_ptr())


class Context:
    """One k-mer table on one GPU = the BigLong2ShortHashMap of one tool run."""

    def __init__(self, k, key_mode=KEY_PACKED, device=0, capacity_hint=0, flags=0):
        self._L = load()
        self.k, self.key_mode, self.device = k, key_mode, device
        cfg = _Config(k, key_mode, device, flags, capacity_hint)
        h = C.c_void_p()
        rc = self._L.mc_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise McError(rc, (self._L.mc_last_error(None) or b"").decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.mc_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != 0:
            raise McError(rc, (self._L.mc_last_error(self._h) or b"").decode())

    def clear(self):
        self._chk(self._L.mc_clear(self._h))

    def set_coverage_hint(self, min_cov):
        """mc_set_coverage_hint: counting keeps #(count >= min_cov) current, BFS set-up skips a table sweep."""
        self._chk(self._L.mc_set_coverage_hint(self._h, int(min_cov)))

    PTRS_NONE, PTRS_OWN_STORE, PTRS_STORE_ELSEWHERE, PTRS_ON_EVERY_RECORD = 0, 1, 2, 0x10

    def set_read_pointers(self, mode):
        """mc_set_read_pointers: False / 0 no pointers, True / 1 this context's own read store, 2 a store kept by another context
        (read_store_tell / read_store_import_dev); | PTRS_ON_EVERY_RECORD: every record it is handed carries a pointer."""
        self._chk(self._L.mc_set_read_pointers(self._h, int(mode)))

    def read_store_seek(self, at_bases, reserve_bases=0):
        self._chk(self._L.mc_read_store_seek(self._h, int(at_bases), int(reserve_bases)))

    def read_store_tell(self):
        return int(self._L.mc_read_store_tell(self._h))

    def read_store_import_dev(self, d_words, n_words, at_bases):
        self._chk(self._L.mc_read_store_import_dev(self._h, _dptr(d_words), int(n_words), int(at_bases)))

    def share_read_store(self, other):
        """mc_share_read_store: this (BFS-only) context reads its look-ahead from `other`'s read store."""
        self._chk(self._L.mc_share_read_store(self._h, other._h if other is not None else None))

    def set_stream(self, stream_ptr):
        self._chk(self._L.mc_set_stream(self._h, C.c_void_p(stream_ptr) if stream_ptr else None))

    # ---- counting
    def add_reads_packed(self, words, offsets):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = len(offsets) - 1
        if n_reads > 0 and len(words) < (int(offsets[-1]) + 31) // 32 + 1:
            raise ValueError("words[] must hold ceil(n_bases/32) + 1 entries")
        self._chk(self._L.mc_add_reads_packed(self._h, _p(words, C.c_uint64), _p(offsets, C.c_uint64), n_reads))

    def add_reads_packed_dev(self, d_words, d_offsets, n_reads, n_bases):
        self._chk(self._L.mc_add_reads_packed_dev(self._h, _dptr(d_words), _dptr(d_offsets), n_reads, n_bases))

    def add_keys_dev(self, d_keys, n, d_hints=None):
        self._chk(self._L.mc_add_keys_dev(self._h, _dptr(d_keys), _dptr(d_hints), n))

    def add_pairs_dev(self, d_keys, d_counts, n, d_hints=None):
        self._chk(self._L.mc_add_pairs_dev(self._h, _dptr(d_keys), _dptr(d_counts), _dptr(d_hints), n))

    def solid_from_pairs_dev(self, d_keys, d_counts, n, min_cov, d_hints=None):
        """BFS-only context from the gathered (key, count, hint) pairs with count >= min_cov; returns how many."""
        m = C.c_uint64(0)
        self._chk(self._L.mc_solid_from_pairs_dev(self._h, _dptr(d_keys), _dptr(d_counts), _dptr(d_hints), n, min_cov, C.byref(m)))
        return int(m.value)

    def finalize(self):
        n = C.c_uint64(0)
        self._chk(self._L.mc_finalize_counts(self._h, C.byref(n)))
        return int(n.value)

    # ---- lookups
    def get(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        out = np.zeros(len(keys), dtype=np.int16)
        self._chk(self._L.mc_get(self._h, _p(keys, C.c_int64), len(keys), _p(out, C.c_int16)))
        return out

    def get_dev(self, d_keys, n, d_out):
        self._chk(self._L.mc_get_dev(self._h, _dptr(d_keys), n, _dptr(d_out)))

    def kmer_keys(self, hi, lo):
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        hi = np.ascontiguousarray(hi, dtype=np.uint64) if hi is not None else None
        out = np.zeros(len(lo), dtype=np.int64)
        self._chk(self._L.mc_kmer_keys(self._h, _p(hi, C.c_uint64) if hi is not None else None,
                                       _p(lo, C.c_uint64), len(lo), _p(out, C.c_int64)))
        return out

    # ---- reads-classifier
    @staticmethod
    def _words(codes_or_words, offsets, packed):
        """the packed words (with their pad word) of base codes 0..3 (uint8) or of words already packed (uint64)"""
        a = np.asarray(codes_or_words)
        if packed is None:
            packed = a.dtype == np.uint64
        if packed:
            words = np.ascontiguousarray(a, dtype=np.uint64)
        else:
            codes = np.ascontiguousarray(a, dtype=np.uint8)
            words = np.zeros((len(codes) + 31) // 32 + 1, dtype=np.uint64)
            if len(codes):
                pad = (-len(codes)) % 32
                c = np.concatenate([codes & 3, np.zeros(pad, dtype=np.uint8)]).reshape(-1, 32).astype(np.uint64)
                words[:len(c)] = np.bitwise_or.reduce(c << (np.uint64(62) - np.uint64(2) * np.arange(32, dtype=np.uint64)), axis=1)
        if len(offsets) > 1 and len(words) < (int(offsets[-1]) + 31) // 32 + 1:
            raise ValueError("words[] must hold ceil(n_bases/32) + 1 entries")
        return words

    def classify_reads(self, codes_or_words, offsets, bad_pos=None, found=90, z=1.0, correction=False, packed=None):
        """Per-read coverage of a read set in this table (mc_classify_reads): returns numpy arrays sum, covered, last, found.
        codes_or_words: base codes 0..3 (uint8, one a base; N already turned into 0) or the packed words with their pad word
        (uint64; packed=None tells them apart by dtype); offsets: n_reads + 1 base offsets.  bad_pos: per read the only position
        with phred < 10, -1 for none, -2 for several (None: none anywhere).  found: the breadth threshold in percent; z: 1 or 1.96."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        words = self._words(codes_or_words, offsets, packed)
        bp = None if bad_pos is None else np.ascontiguousarray(bad_pos, dtype=np.int32)
        if bp is not None and len(bp) != n:
            raise ValueError("bad_pos needs one entry a read")
        out = np.zeros(max(n, 0), dtype=READ_COV_DTYPE)
        self._chk(self._L.mc_classify_reads(self._h, _p(words, C.c_uint64), _p(offsets, C.c_uint64), max(n, 0),
                                            _p(bp, C.c_int32) if bp is not None else None, int(found), float(z),
                                            CLASSIFY_CORRECTION if correction else 0, out.ctypes.data_as(C.POINTER(ReadCov))))
        return out["sum"].copy(), out["covered"].copy(), out["last"].copy(), out["found"].astype(bool)

    def classify_reads_dev(self, d_words, d_offsets, n_reads, d_out, d_bad_pos=None, found=90, z=1.0, correction=False):
        """mc_classify_reads_dev: d_out holds 12 bytes a read (mc_read_cov)"""
        self._chk(self._L.mc_classify_reads_dev(self._h, _dptr(d_words), _dptr(d_offsets), int(n_reads), _dptr(d_bad_pos), int(found),
                                                float(z), CLASSIFY_CORRECTION if correction else 0, _dptr(d_out)))

    # ---- triple-reads-classifier
    def reads_last_copy(self, codes_or_words, offsets, weak=False, packed=None):
        """mc_reads_last_copy: for every read, the greatest index of a read with the same bases (uint32 array).  Reads as in
        classify_reads.  weak: the tests' 4-bit first fingerprint (the result is the same)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = max(len(offsets) - 1, 0)
        words = self._words(codes_or_words, offsets, packed)
        out = np.zeros(n, dtype=np.uint32)
        self._chk(self._L.mc_reads_last_copy(self._h, _p(words, C.c_uint64), _p(offsets, C.c_uint64), n, LAST_COPY_WEAK_FP if weak else 0,
                                             _p(out, C.c_uint32)))
        return out

    def reads_last_copy_dev(self, d_words, d_offsets, n_reads, d_last, weak=False):
        """mc_reads_last_copy_dev: d_last holds 4 bytes a read"""
        self._chk(self._L.mc_reads_last_copy_dev(self._h, _dptr(d_words), _dptr(d_offsets), int(n_reads), LAST_COPY_WEAK_FP if weak else 0,
                                                 _dptr(d_last)))

    @staticmethod
    def _covs(cov):
        """mc_read_cov records from a READ_COV_DTYPE array or from classify_reads' (sum, covered, last, found)"""
        if isinstance(cov, np.ndarray) and cov.dtype == READ_COV_DTYPE:
            return np.ascontiguousarray(cov)
        s, c, last, f = cov
        out = np.zeros(len(s), dtype=READ_COV_DTYPE)
        out["sum"], out["covered"], out["last"], out["found"] = s, c, last, np.asarray(f).astype(np.uint8)
        return out

    def triple_classes(self, cov1, cov2, offsets1, offsets2, half=40, prev=None, last=None):
        """mc_triple_classes at this context's k: the classes (uint8 arrays, CLASS_*) of both mates of every pair.  cov1 / cov2: what
        classify_reads returned for each side (or READ_COV_DTYPE arrays); offsets1 / offsets2: each side's n_pairs + 1 offsets.  Pass 2:
        prev = (pass-1 classes of side 1, of side 2), last = (reads_last_copy of side 1, of side 2)."""
        c1, c2 = self._covs(cov1), self._covs(cov2)
        o1, o2 = (np.ascontiguousarray(o, dtype=np.uint64) for o in (offsets1, offsets2))
        n = len(c1)
        if len(c2) != n or len(o1) != n + 1 or len(o2) != n + 1:
            raise ValueError("both sides need one record a pair and n_pairs + 1 offsets")
        p1 = p2 = l1 = l2 = None
        if prev is not None:
            p1, p2 = (np.ascontiguousarray(p, dtype=np.uint8) for p in prev)
            l1, l2 = (np.ascontiguousarray(x, dtype=np.uint32) for x in last)
            if not all(len(x) == n for x in (p1, p2, l1, l2)):
                raise ValueError("pass 2 needs one class and one last copy a read")
        k1, k2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        cp = lambda a: a.ctypes.data_as(C.POINTER(ReadCov))  # noqa: E731
        opt = lambda a, t: _p(a, t) if a is not None else None  # noqa: E731
        self._chk(self._L.mc_triple_classes(self._h, cp(c1), cp(c2), _p(o1, C.c_uint64), _p(o2, C.c_uint64), n, int(half),
                                            opt(p1, C.c_uint8), opt(p2, C.c_uint8), opt(l1, C.c_uint32), opt(l2, C.c_uint32),
                                            _p(k1, C.c_uint8), _p(k2, C.c_uint8)))
        return k1, k2

    def triple_classes_dev(self, d_cov1, d_cov2, d_offsets1, d_offsets2, n_pairs, d_class1, d_class2, half=40, d_prev1=None, d_prev2=None,
                           d_last1=None, d_last2=None):
        """mc_triple_classes_dev: d_cov* hold 12 bytes a read (mc_read_cov), d_class* one byte"""
        self._chk(self._L.mc_triple_classes_dev(self._h, _dptr(d_cov1), _dptr(d_cov2), _dptr(d_offsets1), _dptr(d_offsets2), int(n_pairs),
                                                int(half), _dptr(d_prev1), _dptr(d_prev2), _dptr(d_last1), _dptr(d_last2), _dptr(d_class1),
                                                _dptr(d_class2)))

    # ---- BFS
    def bfs_batch(self, jobs, min_cov, max_kmers=-1, max_radius=-1):
        """jobs: list of (seed_hi or None, seed_lo, direction).  All passes run in one launch, one
        workgroup each.  Returns a list with, per job, None when no seed k-mer reaches min_cov (the
        reference's 'fail'), else a dict of numpy arrays in distanceToKmer insertion order."""
        n = len(jobs)
        arr_jobs = (_BfsJob * n)()
        keep = []
        for i, (hi, lo, d) in enumerate(jobs):
            lo = np.ascontiguousarray(lo, dtype=np.uint64)
            hi = np.ascontiguousarray(hi if hi is not None else np.zeros(len(lo)), dtype=np.uint64)
            keep.append((hi, lo))
            arr_jobs[i] = _BfsJob(_p(hi, C.c_uint64), _p(lo, C.c_uint64), len(lo), d)
        res = (_BfsResult * n)()
        self._chk(self._L.mc_bfs_batch(self._h, arr_jobs, n, min_cov, max_kmers, max_radius, res))
        out = []
        for i in range(n):
            r = res[i]
            m = int(r.n)
            if m == 0:
                out.append(None)
                continue

            # the arrays are views of the library's (page-locked) result memory, which goes back to the library when the
            # last of them is collected: no second copy of 10^5 vertices per pass
            owner = _ResultOwner(self._L, r)

            def arr(ptr, ctype, dt):
                buf = (ctype * m).from_address(C.addressof(ptr.contents))
                buf._owner = owner  # (the numpy array keeps `buf` alive as its base)
                return np.frombuffer(buf, dtype=dt)

            out.append(dict(hi=arr(r.hi, C.c_uint64, np.uint64), lo=arr(r.lo, C.c_uint64, np.uint64), dist=arr(r.dist, C.c_int32, np.int32),
                            cov=arr(r.cov, C.c_int16, np.int16), last=arr(r.last, C.c_uint8, np.uint8), levels=int(r.levels),
                            lookups=int(r.lookups), rounds=int(r.rounds), device_ms=float(r.device_ms)))
        return out

    def bfs(self, seed_hi, seed_lo, direction, min_cov, max_kmers=-1, max_radius=-1):
        """One runBfs pass; None when no seed k-mer reaches min_cov."""
        return self.bfs_batch([(seed_hi, seed_lo, direction)], min_cov, max_kmers, max_radius)[0]

    # ---- export
    def export(self, min_cov=0):
        n = C.c_uint64(0)
        self._chk(self._L.mc_export(self._h, min_cov, None, None, 0, C.byref(n)))
        cap = int(n.value)
        keys = np.zeros(cap, dtype=np.int64)
        cnt = np.zeros(cap, dtype=np.int16)
        if cap:
            self._chk(self._L.mc_export(self._h, min_cov, _p(keys, C.c_int64), _p(cnt, C.c_int16), cap, C.byref(n)))
        o = np.argsort(keys, kind="stable")
        return keys[o], cnt[o]

    def export_count(self, min_cov=0):
        n = C.c_uint64(0)
        self._chk(self._L.mc_export_dev(self._h, min_cov, None, None, None, 0, C.byref(n)))
        return int(n.value)

    def export_dev(self, min_cov, d_keys, d_counts, cap, d_hints=None):
        n = C.c_uint64(0)
        self._chk(self._L.mc_export_dev(self._h, min_cov, _dptr(d_keys), _dptr(d_counts), _dptr(d_hints), cap, C.byref(n)))
        return int(n.value)

    # ---- multi-GPU building blocks
    def extract_keys_dev(self, d_words, d_offsets, n_reads, n_bases, n_owners, d_keys, cap, d_hints=None):
        off = np.zeros(n_owners + 1, dtype=np.uint64)
        self._chk(self._L.mc_extract_keys_dev(self._h, _dptr(d_words), _dptr(d_offsets), n_reads, n_bases, n_owners,
                                              _dptr(d_keys), _dptr(d_hints), cap, _p(off, C.c_uint64)))
        return off

    def add_reads_file(self, path):
        """One --reads file (FASTA / FASTQ, optionally .gz) with the reference's reader policies; returns the reads added."""
        n = C.c_uint64(0)
        self._chk(self._L.mc_add_reads_file(self._h, os.fsencode(path), C.byref(n)))
        return int(n.value)

    def save_kmers(self, bin_path, stat_path=None, threshold=0):
        """<name>.kmers.bin (+ <name>.stat.txt): returns (keys in the table, records written)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.mc_save_kmers(self._h, os.fsencode(bin_path), os.fsencode(stat_path) if stat_path else None,
                                        threshold, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def load_kmers(self, path, freq_threshold=0):
        """Adds the records of a .kmers.bin file; returns (records read, records added)."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.mc_load_kmers(self._h, os.fsencode(path), freq_threshold, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def save_kmers_gpu(self, bin_path, stat_path=None, threshold=0):
        """save_kmers with the records encoded on the device and streamed to the file in chunks; the same files but for the
        records' order (ascending table slots), the same return value."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.mc_save_kmers_gpu(self._h, os.fsencode(bin_path), os.fsencode(stat_path) if stat_path else None,
                                            threshold, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def load_kmers_gpu(self, path, freq_threshold=0):
        """load_kmers with the records decoded on the device, chunk i + 1 read while chunk i is added; the same return value."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.mc_load_kmers_gpu(self._h, os.fsencode(path), freq_threshold, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def kmers_encode_dev(self, threshold, d_bytes, cap_bytes, d_hist=None):
        """mc_kmers_encode_dev: the .kmers.bin records of the table (10 bytes each, ascending table slots) into d_bytes (uint8, 16-byte
        aligned, cap_bytes long; None: count only), the frequency histogram of all keys into d_hist (32768 x int64; may be None).
        Returns (keys in the table, records written) as save_kmers does; McError when 10 * records > cap_bytes."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.mc_kmers_encode_dev(self._h, int(threshold), _dptr(d_bytes), int(cap_bytes), _dptr(d_hist), C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def kmers_decode_dev(self, d_bytes, n_records, freq_threshold, d_keys, d_counts):
        """mc_kmers_decode_dev: of the n_records records at d_bytes (16-byte aligned) those with count > freq_threshold into d_keys
        (int64) / d_counts (int16), n_records entries each, in any order; returns how many.  The table is not touched."""
        n = C.c_uint64(0)
        self._chk(self._L.mc_kmers_decode_dev(self._h, _dptr(d_bytes), int(n_records), int(freq_threshold), _dptr(d_keys), _dptr(d_counts), C.byref(n)))
        return int(n.value)

    def superkmer_capacity(self, n_windows, n_reads):
        """Records to make room for when a batch of reads is split with extract_superkmers_dev; 0 when this
        context counts window by window (hash keys, k < 23): use extract_keys_dev then."""
        return int(self._L.mc_superkmer_capacity(self._h, int(n_windows), int(n_reads)))

    def extract_superkmers_dev(self, d_words, d_offsets, n_reads, n_bases, n_owners, d_recs, d_bins, cap):
        """d_recs: int64 tensor of shape (cap, 2); d_bins: int32 tensor of cap entries.  Returns the owner offsets."""
        off = np.zeros(n_owners + 1, dtype=np.uint64)
        self._chk(self._L.mc_extract_superkmers_dev(self._h, _dptr(d_words), _dptr(d_offsets), n_reads, n_bases, n_owners,
                                                    _dptr(d_recs), _dptr(d_bins), cap, _p(off, C.c_uint64)))
        return off

    def add_superkmers_dev(self, d_recs, d_bins, n):
        self._chk(self._L.mc_add_superkmers_dev(self._h, _dptr(d_recs), _dptr(d_bins), n))

    # ---- the binned form of the exchange (include/mcgpu.h mc_extract_superkmers_binned_dev): the sender does the owner's first level
    def superkmer_fine_buckets(self, n_owners):
        """fine buckets to extract with for n_owners owners laid out like this context; 0: use the flat form"""
        return int(self._L.mc_superkmer_fine_buckets(self._h, int(n_owners)))

    def extract_superkmers_binned_dev(self, d_words, d_offsets, n_reads, n_bases, n_owners, n_fine, d_recs, d_bins, cap, d_fine_counts):
        """as extract_superkmers_dev; d_fine_counts: int32 tensor of n_owners x n_fine entries (written).  Returns (owner offsets,
        windows of every owner's records)."""
        off = np.zeros(n_owners + 1, dtype=np.uint64)
        win = np.zeros(n_owners, dtype=np.uint64)
        self._chk(self._L.mc_extract_superkmers_binned_dev(self._h, _dptr(d_words), _dptr(d_offsets), n_reads, n_bases, n_owners, n_fine,
                                                           _dptr(d_recs), _dptr(d_bins), cap, _dptr(d_fine_counts), _p(off, C.c_uint64), _p(win, C.c_uint64)))
        return off, win

    def add_superkmers_binned_dev(self, d_recs, d_bins, n, n_windows, n_fine, part_offsets, d_part_counts):
        """part_offsets: n_parts + 1 record offsets (host); d_part_counts: int32 tensor of n_parts x n_fine entries"""
        po = np.ascontiguousarray(part_offsets, dtype=np.uint64)
        self._chk(self._L.mc_add_superkmers_binned_dev(self._h, _dptr(d_recs), _dptr(d_bins), n, int(n_windows), n_fine, len(po) - 1,
                                                       _p(po, C.c_uint64), _dptr(d_part_counts)))

    # ---- the walk over several ranks' tables in place (include/mcgpu.h mc_shard_*)
    SHARD_HANDLE_BYTES = 128

    def shard_export(self):
        """this context's table as 128 opaque bytes for the walking rank (after finalize; keep the table as it is meanwhile)"""
        buf = C.create_string_buffer(self.SHARD_HANDLE_BYTES)
        self._chk(self._L.mc_shard_export(self._h, buf))
        return buf.raw

    def shard_attach(self, handles, self_index, by_minimizer):
        """handles[i] = rank i's shard_export() (this context's own at self_index): bfs / bfs_batch then walk all the tables"""
        blob = b"".join(handles)
        assert len(blob) == self.SHARD_HANDLE_BYTES * len(handles)
        self._chk(self._L.mc_shard_attach(self._h, blob, len(handles), self_index, 1 if by_minimizer else 0))

    def shard_detach(self):
        self._chk(self._L.mc_shard_detach(self._h))

    # ---- measurement / synthetic data
    def stats(self):
        s = Stats()
        self._chk(self._L.mc_get_stats(self._h, C.byref(s)))
        return s

    def reset_stats(self):
        self._chk(self._L.mc_reset_stats(self._h))

    def trim(self):
        """mc_trim: the counting pipeline's scratch and the pools' idle blocks go back to the driver."""
        self._chk(self._L.mc_trim(self._h))

    def unitigs(self, hi, lo, cls):
        """mc_unitigs: see the module's unitigs()"""
        return unitigs(self, hi, lo, cls)

    def unitigs_dev(self, d_hi, d_lo, d_cls, n):
        """mc_unitigs_dev: see the module's unitigs_dev()"""
        return unitigs_dev(self, d_hi, d_lo, d_cls, n)

    def trim_paths(self, hi, lo, last, dir):
        """mc_trim_paths: see the module's trim_paths()"""
        return trim_paths(self, hi, lo, last, dir)

    def trim_paths_dev(self, d_hi, d_lo, d_last, n, dir, d_kept):
        """mc_trim_paths_dev: see the module's trim_paths_dev()"""
        return trim_paths_dev(self, d_hi, d_lo, d_last, n, dir, d_kept)

    def walk_order(self, hi, lo, comp_offsets, flags=0):
        """mc_walk_order: see the module's walk_order()"""
        return walk_order(self, hi, lo, comp_offsets, flags)

    def walk_order_dev(self, d_hi, d_lo, d_comp_offsets, n_components, flags=0):
        """mc_walk_order_dev: see the module's walk_order_dev()"""
        return walk_order_dev(self, d_hi, d_lo, d_comp_offsets, n_components, flags)

    def env_join(self, hi, lo, rec_hi, rec_lo, rec_depth, graph_offsets, gene_words=None, gene_len=0):
        """mc_env_join: see the module's env_join()"""
        return env_join(self, hi, lo, rec_hi, rec_lo, rec_depth, graph_offsets, gene_words, gene_len)

    def env_join_dev(self, d_hi, d_lo, n, d_rec_hi, d_rec_lo, d_rec_depth, d_graph_offsets, n_graphs, d_gene=None, gene_len=0):
        """mc_env_join_dev: see the module's env_join_dev()"""
        return env_join_dev(self, d_hi, d_lo, n, d_rec_hi, d_rec_lo, d_rec_depth, d_graph_offsets, n_graphs, d_gene, gene_len)

    def synth_reads_dev(self, genome_seed, n_contigs, contig_len, read_seed, first_read, n_reads, read_len,
                        err_per_10k, d_words, d_offsets):
        self._chk(self._L.mc_synth_reads_dev(self._h, genome_seed, n_contigs, contig_len, read_seed, first_read,
                                             n_reads, read_len, err_per_10k, _dptr(d_words), _dptr(d_offsets)))


def _table_handles(contexts):
    contexts = list(contexts)
    return contexts, (C.c_void_p * max(len(contexts), 1))(*[c._h for c in contexts])


def seq_coverage(contexts, codes_or_words, offsets, packed=None):
    """mc_seq_coverage: depth and breadth of every sequence's k-mers in each of the contexts' tables (1 .. SEQ_COV_MAX_TABLES contexts of
    one k, key mode and device, finalized; the same one may come several times).  Sequences as Context.classify_reads takes reads: base
    codes 0..3 (uint8, N already 0) or packed words, and n_seqs + 1 base offsets.  Returns uint64 [n_seqs, n_tables, 2]: the sum of
    the windows' coverages and the number of covered windows."""
    contexts, handles = _table_handles(contexts)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = max(len(offsets) - 1, 0)
    words = Context._words(codes_or_words, offsets, packed)
    out = np.zeros((n, len(contexts), 2), dtype=np.uint64)
    rc = load().mc_seq_coverage(handles, len(contexts), _p(words, C.c_uint64), _p(offsets, C.c_uint64), n, out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise McError(rc, (load().mc_last_error(contexts[0]._h) or b"").decode() if contexts else "")
    return out


def seq_coverage_dev(contexts, d_words, d_offsets, n_seqs, d_out):
    """mc_seq_coverage_dev: d_out holds n_seqs * n_tables * 2 uint64 (mc_seq_cov records); the call zeroes it first"""
    contexts, handles = _table_handles(contexts)
    rc = load().mc_seq_coverage_dev(handles, len(contexts), _dptr(d_words), _dptr(d_offsets), int(n_seqs), _dptr(d_out))
    if rc != 0:
        raise McError(rc, (load().mc_last_error(contexts[0]._h) or b"").decode() if contexts else "")


def kmer_presence(contexts, hi, lo):
    """mc_kmer_presence: which of the contexts' tables (1 .. PRESENCE_MAX_TABLES contexts of one k, key mode and device, finalized; the
    same one may come several times) contain each oriented packed k-mer (hi << 64 | lo, as bfs results list them; hi may be None when
    k <= 32).  Returns a uint8 array: bit t of entry i is set when contexts[t] holds k-mer i."""
    contexts, handles = _table_handles(contexts)
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hi = np.ascontiguousarray(hi, dtype=np.uint64) if hi is not None else None
    if hi is not None and len(hi) != len(lo):
        raise ValueError("hi and lo need one entry a k-mer")
    out = np.zeros(len(lo), dtype=np.uint8)
    rc = load().mc_kmer_presence(handles, len(contexts), _p(hi, C.c_uint64) if hi is not None else None, _p(lo, C.c_uint64), len(lo),
                                 _p(out, C.c_uint8))
    if rc != 0:
        raise McError(rc, (load().mc_last_error(contexts[0]._h) or b"").decode() if contexts else "")
    return out


def kmer_presence_dev(contexts, d_hi, d_lo, n, d_mask):
    """mc_kmer_presence_dev: d_hi (may be None when k <= 32) and d_lo hold n uint64 each, d_mask n bytes"""
    contexts, handles = _table_handles(contexts)
    rc = load().mc_kmer_presence_dev(handles, len(contexts), _dptr(d_hi), _dptr(d_lo), int(n), _dptr(d_mask))
    if rc != 0:
        raise McError(rc, (load().mc_last_error(contexts[0]._h) or b"").decode() if contexts else "")


def reads_in_set(context, codes_or_words, offsets, hi, lo, pct=1, weak=False, packed=None):
    """mc_reads_in_set: for every read, the number of its windows 0 .. L - k - 1 (the last window is never tested, as in the reference's
    ReadsFilter) whose k-mer, or its reverse complement, is one of the oriented packed k-mers (hi << 64 | lo; hi may be None when
    k <= 32; any orientation, duplicates allowed), and whether the read is kept: hits >= max(1, (L - k + 1) * pct // 100).  Reads as
    Context.classify_reads takes them.  Needs no table.  weak: the tests' run without the bit filter (the result is the same).
    Returns (hits uint32, keep bool)."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = max(len(offsets) - 1, 0)
    words = Context._words(codes_or_words, offsets, packed)
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hi = np.ascontiguousarray(hi, dtype=np.uint64) if hi is not None else None
    if hi is not None and len(hi) != len(lo):
        raise ValueError("hi and lo need one entry a k-mer")
    hits, keep = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    context._chk(load().mc_reads_in_set(context._h, _p(words, C.c_uint64), _p(offsets, C.c_uint64), n, _p(hi, C.c_uint64) if hi is not None else None,
                                        _p(lo, C.c_uint64), len(lo), int(pct), READS_IN_SET_WEAK_FILTER if weak else 0, _p(hits, C.c_uint32),
                                        _p(keep, C.c_uint8)))
    return hits, keep.astype(bool)


def reads_in_set_dev(context, d_words, d_offsets, n_reads, d_hi, d_lo, n_set, d_hits, d_keep, pct=1, weak=False):
    """mc_reads_in_set_dev: d_hi (may be None when k <= 32) and d_lo hold n_set uint64 each, d_hits 4 bytes a read, d_keep one"""
    context._chk(load().mc_reads_in_set_dev(context._h, _dptr(d_words), _dptr(d_offsets), int(n_reads), _dptr(d_hi), _dptr(d_lo), int(n_set), int(pct),
                                            READS_IN_SET_WEAK_FILTER if weak else 0, _dptr(d_hits), _dptr(d_keep)))


def _components_result(r):
    """the library's arrays as numpy arrays of our own, and the library's freed"""
    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
    try:
        nc, nk = int(r.n_components), int(r.n_kmers)
        return {"n_components": nc, "n_kmers": nk, "comp_offsets": arr(r.comp_offsets, nc + 1, np.uint64), "seed_seq": arr(r.seed_seq, nc, np.uint64),
                "seed_pos": arr(r.seed_pos, nc, np.uint64), "hi": arr(r.hi, nk, np.uint64), "lo": arr(r.lo, nk, np.uint64),
                "cov": arr(r.cov, nk, np.int16), "device_ms": float(r.device_ms)}
    finally:
        load().mc_components_free(C.byref(r))


def components(context, codes_or_words, offsets, packed=None):
    """mc_components: the connected components of the table's k-mers (get > 0) that the sequences' windows hold, two keys joined when
    their k-mers are allNeighbors of each other; components numbered by their first window in scan order (the fmt-visualizer's
    comp<N>).  Sequences as Context.classify_reads takes reads.  Returns a dict of numpy arrays: comp_offsets (n_components + 1),
    seed_seq, seed_pos (a component), hi, lo, cov (a member; member comp_offsets[c] is component c's seed window as the read has
    it), and n_components, n_kmers, device_ms."""
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = max(len(offsets) - 1, 0)
    words = Context._words(codes_or_words, offsets, packed)
    r = _Components()
    context._chk(load().mc_components(context._h, _p(words, C.c_uint64), _p(offsets, C.c_uint64), n, C.byref(r)))
    return _components_result(r)


def components_dev(context, d_words, d_offsets, n_seqs):
    """mc_components_dev: the sequences are in device memory; the result comes back as components' does"""
    r = _Components()
    context._chk(load().mc_components_dev(context._h, _dptr(d_words), _dptr(d_offsets), int(n_seqs), C.byref(r)))
    return _components_result(r)


def _unitigs_result(r):
    """the library's arrays as numpy arrays of our own, and the library's freed"""
    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
    try:
        nn, nu, ni = int(r.n_nodes), int(r.n_unitigs), int(r.n_irregular)
        deg = arr(r.deg, nn, np.uint8)
        off = arr(r.base_offsets, nu + 1, np.uint64)
        return {"n_nodes": nn, "deg": deg, "nbr": arr(r.nbr, int(deg.sum(dtype=np.uint64)), np.uint32), "n_unitigs": nu,
                "first": arr(r.first, nu, np.uint32), "last_rc": arr(r.last_rc, nu, np.uint32), "base_offsets": off,
                "bases": arr(r.bases, int(off[nu]) // 32, np.uint64), "n_irregular": ni, "irregular": arr(r.irregular, ni, np.uint32),
                "device_ms": float(r.device_ms)}
    finally:
        load().mc_unitigs_free(C.byref(r))


def unitigs(context, hi, lo, cls):
    """mc_unitigs: what the reference's unitig compaction (initializeStructures + doMerge) leaves of the oriented packed k-mers
    (hi << 64 | lo in the subgraph's iteration order; hi may be None when k <= 32) with merge classes cls (uint8).  Entry e makes
    nodes 2e and 2e + 1 (its reverse complement).  Returns a dict of numpy arrays: deg (a node) and nbr (the neighbours lists one after
    another), first, last_rc and base_offsets (n_unitigs + 1, in bases) of the unitigs with their packed bases, irregular (the entries
    of chains whose result depends on the loop's scan order, left to the caller), and n_nodes, n_unitigs, n_irregular, device_ms.
    Needs no table."""
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hi = np.ascontiguousarray(hi, dtype=np.uint64) if hi is not None else None
    cls = np.ascontiguousarray(cls, dtype=np.uint8)
    if (hi is not None and len(hi) != len(lo)) or len(cls) != len(lo):
        raise ValueError("hi, lo and cls need one entry a k-mer")
    r = _Unitigs()
    context._chk(load().mc_unitigs(context._h, _p(hi, C.c_uint64) if hi is not None else None, _p(lo, C.c_uint64), _p(cls, C.c_uint8), len(lo),
                                   C.byref(r)))
    return _unitigs_result(r)


def unitigs_dev(context, d_hi, d_lo, d_cls, n):
    """mc_unitigs_dev: d_hi (may be None when k <= 32) and d_lo hold n uint64 each, d_cls n bytes; the result comes back as unitigs' does"""
    r = _Unitigs()
    context._chk(load().mc_unitigs_dev(context._h, _dptr(d_hi), _dptr(d_lo), _dptr(d_cls), int(n), C.byref(r)))
    return _unitigs_result(r)


def trim_paths(context, hi, lo, last, dir):
    """mc_trim_paths: which entries of one BFS pass runTrimPaths keeps.  hi, lo: the pass's distinct oriented packed k-mers (hi << 64 | lo;
    hi may be None when k <= 32), last: uint8, whether the entry is in lastKmers, dir: the pass's (-1, 0, +1).  Returns np.uint8[n]:
    1 where the entry reaches a `last` entry through neighbours on the side of dir (both sides for 0) inside the set.  Needs no table."""
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hi = np.ascontiguousarray(hi, dtype=np.uint64) if hi is not None else None
    last = np.ascontiguousarray(last, dtype=np.uint8)
    if (hi is not None and len(hi) != len(lo)) or len(last) != len(lo):
        raise ValueError("hi, lo and last need one entry a k-mer")
    kept = np.zeros(len(lo), dtype=np.uint8)
    context._chk(load().mc_trim_paths(context._h, _p(hi, C.c_uint64) if hi is not None else None, _p(lo, C.c_uint64), _p(last, C.c_uint8), len(lo),
                                      int(dir), _p(kept, C.c_uint8), None))
    return kept


def trim_paths_dev(context, d_hi, d_lo, d_last, n, dir, d_kept):
    """mc_trim_paths_dev: d_hi (may be None when k <= 32) and d_lo hold n uint64 each, d_last and d_kept n bytes; d_kept is written.
    Returns the device time in ms"""
    ms = C.c_double(0)
    context._chk(load().mc_trim_paths_dev(context._h, _dptr(d_hi), _dptr(d_lo), _dptr(d_last), int(n), int(dir), _dptr(d_kept), C.byref(ms)))
    return float(ms.value)


def _walk_order_result(r):
    """the library's arrays as numpy arrays of our own, and the library's freed"""
    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
    try:
        nc, nk = int(r.n_components), int(r.n_kmers)
        return {"n_components": nc, "n_kmers": nk, "reached": arr(r.reached, nc, np.uint64), "order": arr(r.order, nk, np.uint32),
                "twice": arr(r.twice, nk, np.uint8), "levels": int(r.levels), "queue_entries": int(r.queue_entries),
                "wide_levels": int(r.wide_levels), "device_ms": float(r.device_ms)}
    finally:
        load().mc_walk_order_free(C.byref(r))


def walk_order(context, hi, lo, comp_offsets, flags=0):
    """mc_walk_order: for every component of a components() result (its hi, lo and comp_offsets as they are; hi may be None when k <= 32;
    member comp_offsets[c] is component c's seed), the order in which KmerEnvCalculator.runBfs pops its members for the first time and
    which of them it pops again.  Returns a dict: reached (a component: the members the walk pops), order (a member: the first
    reached[c] places of a slice hold member numbers relative to the slice in first-pop order, the seed first), twice (a member: 1 when
    its put value ends as 0), levels, queue_entries, wide_levels (summed over the components), n_components, n_kmers, device_ms.
    flags: WALK_ORDER_* (tests only; the result does not depend on them).  Needs no table."""
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hi = np.ascontiguousarray(hi, dtype=np.uint64) if hi is not None else None
    comp_offsets = np.ascontiguousarray(comp_offsets, dtype=np.uint64)
    n_comp = max(len(comp_offsets) - 1, 0)
    if hi is not None and len(hi) != len(lo):
        raise ValueError("hi and lo need one entry a k-mer")
    if n_comp and int(comp_offsets[n_comp]) < (1 << 30) and int(comp_offsets.max()) > len(lo):
        raise ValueError("comp_offsets runs past the k-mers")
    r = _WalkOrder()
    context._chk(load().mc_walk_order(context._h, _p(hi, C.c_uint64) if hi is not None else None, _p(lo, C.c_uint64), _p(comp_offsets, C.c_uint64),
                                      n_comp, int(flags), C.byref(r)))
    return _walk_order_result(r)


def walk_order_dev(context, d_hi, d_lo, d_comp_offsets, n_components, flags=0):
    """mc_walk_order_dev: d_hi (may be None when k <= 32) and d_lo hold a uint64 a k-mer, d_comp_offsets n_components + 1; the result
    comes back as walk_order's does"""
    r = _WalkOrder()
    context._chk(load().mc_walk_order_dev(context._h, _dptr(d_hi), _dptr(d_lo), _dptr(d_comp_offsets), int(n_components), int(flags), C.byref(r)))
    return _walk_order_result(r)


def _env_join_result(r):
    """the library's arrays as numpy arrays of our own, and the library's freed"""
    def arr(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt)
    try:
        n, g = int(r.n), int(r.n_graphs)
        return {"n": n, "n_graphs": g, "member": arr(r.member, n, np.uint64), "is_gene": arr(r.is_gene, n, np.uint8), "kc": arr(r.kc, n, np.int64),
                "diff": arr(r.diff, g * g, np.uint32).reshape(g, g), "diff_alt": arr(r.diff_alt, g * g, np.uint32).reshape(g, g),
                "uni": arr(r.uni, g * g, np.uint32).reshape(g, g), "device_ms": float(r.device_ms)}
    finally:
        load().mc_env_join_free(C.byref(r))


def env_join(context, hi, lo, rec_hi, rec_lo, rec_depth, graph_offsets, gene_words=None, gene_len=0):
    """mc_env_join: the join of several graph files on their k-mers.  Entries: oriented packed k-mers (hi << 64 | lo; hi may be None
    when k <= 32), entry e standing for its k-mer and the reverse complement.  Records: the files' lines one graph after another
    (rec_hi may be None when k <= 32), rec_depth (int32) their depths, graph_offsets (n_graphs + 1) where each graph's records start.
    gene_words: gene_len bases packed as reads are (None for no gene).  Returns a dict of numpy arrays: member (uint64, bit g: graph g
    holds the entry in either orientation), is_gene, kc (int64: the depths of the records that spell the entry as given), the
    n_graphs x n_graphs uint32 matrices diff, diff_alt and uni (printProbability's sums modulo 2^32), and n, n_graphs, device_ms.
    Needs no table."""
    lo = np.ascontiguousarray(lo, dtype=np.uint64)
    hi = np.ascontiguousarray(hi, dtype=np.uint64) if hi is not None else None
    rec_lo = np.ascontiguousarray(rec_lo, dtype=np.uint64)
    rec_hi = np.ascontiguousarray(rec_hi, dtype=np.uint64) if rec_hi is not None else None
    rec_depth = np.ascontiguousarray(rec_depth, dtype=np.int32)
    graph_offsets = np.ascontiguousarray(graph_offsets, dtype=np.uint64)
    if (hi is not None and len(hi) != len(lo)) or (rec_hi is not None and len(rec_hi) != len(rec_lo)) or len(rec_depth) != len(rec_lo):
        raise ValueError("hi and lo need one entry a k-mer; rec_hi, rec_lo and rec_depth one a record")
    if len(graph_offsets) < 1 or (len(graph_offsets) <= 65 and int(graph_offsets[-1]) != len(rec_lo)):
        raise ValueError("graph_offsets needs n_graphs + 1 entries, the last the number of records")
    gene = np.ascontiguousarray(gene_words, dtype=np.uint64) if gene_words is not None else None
    if gene_len and (gene is None or len(gene) * 32 < gene_len):
        raise ValueError("gene_words holds fewer than gene_len bases")
    r = _EnvJoin()
    q = lambda a: _p(a, C.c_uint64) if a is not None else None
    context._chk(load().mc_env_join(context._h, q(hi), q(lo), len(lo), q(rec_hi), q(rec_lo), _p(rec_depth, C.c_int32), q(graph_offsets),
                                    len(graph_offsets) - 1, q(gene), int(gene_len), C.byref(r)))
    return _env_join_result(r)


def env_join_dev(context, d_hi, d_lo, n, d_rec_hi, d_rec_lo, d_rec_depth, d_graph_offsets, n_graphs, d_gene=None, gene_len=0):
    """mc_env_join_dev: device pointers (d_hi and d_rec_hi may be None when k <= 32, d_gene when gene_len is 0); d_graph_offsets holds
    n_graphs + 1 uint64.  The result comes back as env_join's does"""
    r = _EnvJoin()
    context._chk(load().mc_env_join_dev(context._h, _dptr(d_hi), _dptr(d_lo), int(n), _dptr(d_rec_hi), _dptr(d_rec_lo), _dptr(d_rec_depth),
                                        _dptr(d_graph_offsets), int(n_graphs), _dptr(d_gene), int(gene_len), C.byref(r)))
    return _env_join_result(r)


class WholeReadsDev:
    """A result of mc_tokenize_whole in device memory: n_reads, n_bases, device_ms and the device pointers (ints) d_words, d_offsets,
    d_bad_pos, d_codes, d_phred (0 when not asked for), ready for the *_dev calls.  free() -- or leaving a `with` block -- gives the
    memory back; to_host() returns numpy copies."""

    def __init__(self, context, res):
        self._context, self._res = context, res
        self.n_reads, self.n_bases, self.device_ms = int(res.n_reads), int(res.n_bases), float(res.device_ms)

    d_words = property(lambda self: self._res.d_words or 0)
    d_offsets = property(lambda self: self._res.d_offsets or 0)
    d_bad_pos = property(lambda self: self._res.d_bad_pos or 0)
    d_codes = property(lambda self: self._res.d_codes or 0)
    d_phred = property(lambda self: self._res.d_phred or 0)

    def to_host(self):
        """dict of numpy arrays: words (with the pad word), offsets, bad_pos, and codes / phred (None when not asked for)"""
        nr, nb = self.n_reads, self.n_bases
        out = {"words": np.zeros((nb + 31) // 32 + 1, dtype=np.uint64), "offsets": np.zeros(nr + 1, dtype=np.uint64),
               "bad_pos": np.zeros(nr, dtype=np.int32), "codes": np.zeros(nb, dtype=np.uint8) if self._res.d_codes else None,
               "phred": np.zeros(nb, dtype=np.uint8) if self._res.d_phred else None}
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
        self._context._chk(load().mc_whole_reads_to_host(self._context._h, C.byref(self._res), ptr(out["words"]), ptr(out["offsets"]),
                                                         ptr(out["bad_pos"]), ptr(out["codes"]), ptr(out["phred"])))
        return out

    def free(self):
        if self._res is not None and getattr(self._context, "_h", None):
            load().mc_whole_reads_free(self._context._h, C.byref(self._res))
        self._res = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:  # (interpreter shutdown)
            pass


def reads_append_dev(context, d_words, d_offsets, n_reads, d_dst_words, dst_bases, d_dst_offsets):
    """mc_reads_append_dev: n_reads reads of a device view (d_offsets: n_reads + 1 base positions in d_words, the first need not be 0) go
    behind the dst_bases bases of d_dst_words; d_dst_offsets (the destination's entry of the first new read) gets n_reads + 1 entries"""
    context._chk(load().mc_reads_append_dev(context._h, _dptr(d_words), _dptr(d_offsets), int(n_reads), _dptr(d_dst_words), int(dst_bases),
                                            _dptr(d_dst_offsets)))


def tokenize_whole_dev(context, text, fastq, phred_offset=33, codes=True, phred=True):
    """mc_tokenize_whole: the whole reads of FASTQ (fastq=True; phred_offset 33 or 64) or FASTA text (bytes: a whole number of
    records) with DnaQReader's policy, left in device memory.  Returns a WholeReadsDev, or None when the device declined the text (the
    host reader defines what such a text gives).  Any context will do: its table plays no part."""
    text = bytes(text)
    r = _WholeReads()
    context._chk(load().mc_tokenize_whole(context._h, text, len(text), WHOLE_FASTQ if fastq else WHOLE_FASTA, int(phred_offset),
                                          (WHOLE_CODES if codes else 0) | (WHOLE_PHRED if phred else 0), C.byref(r)))
    return None if r.declined else WholeReadsDev(context, r)


def tokenize_whole(context, text, fastq, phred_offset=33, codes=True, phred=True):
    """tokenize_whole_dev, copied back: a dict of numpy arrays words, offsets, bad_pos, codes, phred (the last two None when not asked
    for) and n_reads, n_bases, device_ms; or None when the device declined the text."""
    d = tokenize_whole_dev(context, text, fastq, phred_offset, codes, phred)
    if d is None:
        return None
    with d:
        out = d.to_host()
        out.update(n_reads=d.n_reads, n_bases=d.n_bases, device_ms=d.device_ms)
        return out


def render_fastq_bound(n_bases, n_items):
    """mc_render_fastq_bound: a capacity that always suffices for n_items records of n_bases bases in all"""
    return int(load().mc_render_fastq_bound(int(n_bases), int(n_items)))


def _render_result(r, n_streams):
    return {"start": [int(r.start[t]) for t in range(n_streams)], "bytes": [int(r.bytes[t]) for t in range(n_streams)],
            "records": [int(r.records[t]) for t in range(n_streams)], "error": int(r.error), "error_side": int(r.error_side),
            "error_read": int(r.error_read), "error_value": int(r.error_value), "device_ms": float(r.device_ms)}


def render_fastq_dev(context, sides, n_reads, n_streams, first_number, d_text, capacity):
    """mc_render_fastq_dev: the FASTQ records of n_reads reads a side as text in d_text (uint8, 16-byte aligned, `capacity` bytes).  sides:
    one or two tuples (d_words, d_phred, d_offsets, d_stream) of device tensors or pointers -- packed bases, a phred a base, n_reads + 1
    base positions, a stream byte a read (RENDER_SKIP for none); first_number: per stream the number of its first record, or
    RENDER_UNNUMBERED.  Returns a dict: start, bytes, records per stream, error (0, RENDER_EMPTY, RENDER_QUALITY), error_side,
    error_read, error_value, device_ms.  McError when `capacity` is too small (-5) or an argument is bad; then .result holds that dict."""
    arr = (_RenderSide * max(len(sides), 2))()
    for i, s in enumerate(sides):
        arr[i] = _RenderSide(*[_dptr(x) for x in s])
    first = np.ascontiguousarray(first_number, dtype=np.uint64)
    r = _RenderResult()
    rc = load().mc_render_fastq_dev(context._h, arr, len(sides), int(n_reads), int(n_streams), _p(first, C.c_uint64), _dptr(d_text),
                                    int(capacity), C.byref(r))
    return _render_checked(context, rc, r, n_streams)


def _render_checked(context, rc, r, n_streams):
    res = _render_result(r, min(max(int(n_streams), 0), RENDER_MAX_STREAMS))
    try:
        context._chk(rc)
    except McError as e:
        e.result = res
        raise
    return res


def render_fastq(context, sides, n_reads, n_streams, first_number, capacity=None, fill=0):
    """mc_render_fastq: render_fastq_dev on numpy arrays (words uint64, phred uint8, offsets uint64, stream uint8 per side).  Returns
    (text, result): text a uint8 array of `capacity` bytes (default: render_fastq_bound of the input), filled with `fill` where the call
    writes nothing, stream t at result["start"][t] : + result["bytes"][t]."""
    keep = [[np.ascontiguousarray(a, dtype=t) for a, t in zip(s, (np.uint64, np.uint8, np.uint64, np.uint8))] for s in sides]
    arr = (_RenderSide * max(len(keep), 2))()
    for i, s in enumerate(keep):
        arr[i] = _RenderSide(*[a.ctypes.data_as(C.c_void_p) for a in s])
    if capacity is None:
        capacity = render_fastq_bound(sum(int(s[2][n_reads]) - int(s[2][0]) for s in keep), n_reads * len(keep))
    text = np.full(max(int(capacity), 1), fill, dtype=np.uint8)
    first = np.ascontiguousarray(first_number, dtype=np.uint64)
    r = _RenderResult()
    rc = load().mc_render_fastq(context._h, arr, len(keep), int(n_reads), int(n_streams), _p(first, C.c_uint64), text.ctypes.data_as(C.c_void_p),
                                int(capacity), C.byref(r))
    return text[:int(capacity)], _render_checked(context, rc, r, n_streams)


def key_owner(key, n_owners):
    return int(load().mc_key_owner(int(key), n_owners))


def synth_genome(genome_seed, start, n):
    out = np.zeros(n, dtype=np.uint8)
    load().mc_synth_genome(genome_seed, start, n, _p(out, C.c_uint8))
    return out
