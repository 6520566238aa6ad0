"""ctypes binding of libfxgpu.so (include/fxgpu.h) -- the only way pyfastx_amd
reaches the GPU.  There is no CPU fallback: if the library is missing, or no
gfx950 device is usable, the calls raise."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("FX_LIBFXGPU") or os.path.join(_HERE, "csrc", "libfxgpu.so")   # the override is for kernel experiments (tools/)
_LIB = None

FX_HOST, FX_DEVICE = 0, 1
FX_UPPER, FX_REVERSE, FX_COMPLEMENT, FX_RAW = 1, 2, 4, 8
FX_SEARCH_DEGENERATE, FX_SEARCH_UPPER, FX_SEARCH_PLUS, FX_SEARCH_MINUS = 1, 2, 4, 8
FX_EDIT_ALL, FX_EDIT_BEST = 0, 1
FX_KMER_CANONICAL = 1
FX_MZ_CANONICAL, FX_MZ_LEX = 1, 2
FX_SK_CANONICAL, FX_SK_POOLED = 1, 2
FX_DUP_REVCOMP = 1
FX_OK, FX_ENOENT, FX_EFORMAT, FX_EIO, FX_EDEVICE, FX_ENOMEM, FX_ERANGE, FX_EINVAL, FX_ESTATE = \
    0, -1, -2, -3, -4, -5, -6, -7, -8


class FxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class FastaSummary(C.Structure):
    _fields_ = [("n_seq", C.c_int64), ("seq_len", C.c_int64), ("n_lines", C.c_int64), ("n_bytes", C.c_int64)]


class FastqSummary(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("size", C.c_int64), ("n_lines", C.c_int64), ("n_bytes", C.c_int64),
                ("first_id", C.c_int64)]


class LenStats(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("n_seq", "sum_len", "longest_id", "longest_len", "shortest_id", "shortest_len",
                                         "count_ge", "med_lo", "med_hi", "nx_len", "nx_count")]


class ShardSummary(C.Structure):
    _fields_ = [(k, C.c_int64) for k in (
        "base", "n_bytes", "is_last", "n_nl", "first_nl", "second_nl", "last_nl", "first_nl_prev",
        "first_byte", "last_byte", "n_hdr", "first_hdr", "last_hdr", "lead_nl", "lead_ws",
        "lead_v1", "lead_c1", "lead_v2", "lead_c2", "tail_e", "tail_first_end", "tail_nl_after", "tail_bad",
        "tail_elen", "tail_dlen", "tail_name_len", "lead_prev_nl", "second_last_nl")]


vp, cs, i32, i64, u8, u64, f64, P = C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_uint8, C.c_uint64, C.c_double, C.POINTER
pvp, pi32, pi64, pf64 = P(vp), P(i32), P(i64), P(f64)

# Every entry of include/fxgpu.h: name -> (return type, argument types).  The one place a new entry is declared: lib() sets
# these on the loaded library, SYMBOLS is its keys, and tests/test_cabi.py holds every line against the header's prototype.
PROTOTYPES = {
    "fx_last_error": (cs, []),
    "fx_version": (cs, []),
    "fx_device_count": (i32, []),
    "fx_open_file": (i32, [cs, i32, pvp]),
    "fx_open_laps": (i32, [pf64, pf64]),
    "fx_build_laps": (i32, [pf64]),
    "fx_open_file_indexed": (i32, [cs, i32, i64, vp, vp, vp, vp, vp, i64, pvp]),
    "fx_gz_checkpoints": (i32, [vp, i64, vp, vp, vp, vp, vp, pi64, pi64]),
    "fx_stream_size": (i32, [cs, pi64, pi32]),
    "fx_open_file_range": (i32, [cs, i64, i64, i64, i32, pvp]),
    "fx_open_host": (i32, [vp, i64, i32, pvp]),
    "fx_open_device": (i32, [vp, i64, i32, pvp]),
    "fx_set_shard": (i32, [vp, i64, i32, i32]),
    "fx_close": (i32, [vp]),
    "fx_release_scratch": (i32, []),
    "fx_pinned_alloc": (vp, [i64]),
    "fx_pinned_free": (None, [vp]),
    "fx_pinned_holds": (i32, [vp, i64]),
    "fx_pinned_trim": (i32, []),
    "fx_size": (i64, [vp]),
    "fx_device_memory": (i32, [i32, pi64, pi64]),
    "fx_is_gzip": (i32, [vp]),
    "fx_device_ptr": (vp, [vp]),
    "fx_read_bytes": (i32, [vp, i64, i64, vp]),
    "fx_first_byte": (i32, [vp, pi32]),
    "fx_fasta_build": (i32, [vp, i32, P(FastaSummary)]),
    "fx_fasta_build_begin": (i32, [vp, i32]),
    "fx_fasta_build_end": (i32, [vp, P(FastaSummary)]),
    "fx_fasta_table": (i32, [vp, i32] + [vp] * 9),
    "fx_fasta_set_table": (i32, [vp, i64] + [vp] * 6),
    "fx_fasta_line_regular": (i32, [vp, i32, vp]),
    "fx_fasta_len_stats": (i32, [vp, i64, f64, P(LenStats)]),
    "fx_fasta_comp": (i32, [vp, i32, vp]),
    "fx_fasta_comp_shard": (i32, [vp, i32, vp, i64, vp]),
    "fx_fasta_comp_sparse": (i32, [vp, i32, i64, vp, vp, vp, pi64, vp]),
    "fx_fastq_build": (i32, [vp, P(FastqSummary)]),
    "fx_fastq_build_comp": (i32, [vp, P(FastqSummary)]),
    "fx_fastq_comp_info": (i32, [vp, pi64, pi64, pi32]),
    "fx_set_halo": (i32, [vp, i64]),
    "fx_fastq_scan": (i32, [vp, pi64, pi64]),
    "fx_fastq_build_ctx": (i32, [vp, i64, i64, P(FastqSummary)]),
    "fx_fastq_table": (i32, [vp, i32] + [vp] * 6),
    "fx_fastq_comp": (i32, [vp, vp, vp]),
    "fx_fetch_ranges": (i32, [vp, i32, i64, vp, vp, vp, i32, vp, vp, vp, vp]),
    "fx_fetch_slices": (i32, [vp, i32, i64, vp, vp, vp, vp, i32, vp, vp, vp, vp]),
    "fx_fetch_one": (i32, [vp, i64, i64, i64, i64, i32, vp, pi64]),
    "fx_fasta_fetch": (i32, [vp, i32, i64, vp, vp, vp, i32, vp, vp, vp, vp]),
    "fx_fasta_fetch_alloc": (i32, [vp, i64, vp, vp, vp, i32, vp, pvp, pvp, pi64]),
    "fx_fasta_search": (i32, [vp, vp, vp, i32, i32, vp, i64, i64, pvp, pvp, pvp, pi64, vp]),
    "fx_fasta_search_approx": (i32, [vp, vp, vp, i32, i32, i32, u64, vp, i64, i64, pvp, pvp, pvp, pvp, pi64, vp]),
    "fx_fasta_search_edit": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, i64, i64, pvp, pvp, pvp, pvp, pvp, pi64, pi64, vp]),
    "fx_fasta_pwm_scan": (i32, [vp, vp, i32, i32, i32, vp, i64, i64, pvp, pvp, pvp, pvp, pi64, vp]),
    "fx_fasta_pwm_best": (i32, [vp, vp, i32, i32, vp, i64, vp, vp]),
    "fx_fasta_minimizers": (i32, [vp, i32, i32, i32, vp, i64, i64, pvp, pvp, pvp, pvp, pi64, vp]),
    "fx_fasta_rank_build": (i32, [vp]),
    "fx_fasta_rank_free": (i32, [vp]),
    "fx_fasta_region_counts": (i32, [vp, i32, i64, vp, vp, vp, vp, pi64]),
    "fx_fasta_window_counts": (i32, [vp, vp, i64, i64, i64, i32, i64] + [pvp] * 4 + [pi64]),
    "fx_fasta_class_runs": (i32, [vp, vp, i64, vp, i64, i64] + [pvp] * 3 + [pi64] * 2),
    "fx_fasta_low_complexity": (i32, [vp, i32, i32, i64, vp, i64, i64] + [pvp] * 3 + [pi64] * 2),
    "fx_fastq_complexity": (i32, [vp, vp, i64, vp, vp] + [pvp] * 4 + [pi64] * 2),
    "fx_fasta_tandem_repeats": (i32, [vp, vp, i32, i64, vp, i64, i64] + [pvp] * 5 + [pi64] * 2),
    "fx_fasta_orfs": (i32, [vp, u64, u64, i32, i32, i64, vp, i64, i64] + [pvp] * 5 + [pi64] * 2),
    "fx_fasta_translate_alloc": (i32, [vp, i64, vp, vp, vp, vp, vp, u8, pvp, pvp, pi64]),
    "fx_fetch_phases": (i32, [pf64, i32]),
    "fx_fastq_fetch": (i32, [vp, i32, i64, vp, i32, i32, vp, vp, vp, vp]),
    "fx_fastq_fetch_alloc": (i32, [vp, i64, vp, i32, i32, i32, pvp, pvp, pvp, pvp, pi64]),
    "fx_fastq_read_stats": (i32, [vp, vp, i64, i32, i32] + [pvp] * 7 + [pi64, pi64]),
    "fx_fastq_cycle_hist": (i32, [vp, i32, pvp, pvp, pvp]),
    "fx_fastq_select": (i32, [vp, i32, i32, i64, i64, i64, i64, i64, i64, i64, pvp, pi64]),
    "fx_fastq_trim": (i32, [vp, vp, i64, i32, i64, i64, vp, i32, i32, i64, i64, i32, i32, i64, i64, i32, pvp, pvp, pi64, pi64]),
    "fx_fastq_format_alloc": (i32, [vp, vp, i64, vp, vp, i64, pvp, pvp, pi64, pi64, pi64]),
    "fx_fasta_format_alloc": (i32, [vp, i64, vp, vp, vp, i32, vp, i64, vp, vp, i64, vp, vp, vp, i32, i32, i64, pvp, pvp, pi64, pi64, pi64]),
    "fx_fasta_format_tile": (i32, []),
    "fx_fastq_demux": (i32, [vp, vp, i64, i32, vp, vp, vp, vp, vp, i32, i32, i32] + [pvp] * 6 + [pi64, pi64]),
    "fx_fastq_pair_overlap": (i32, [vp, vp, vp, i64, i32, i32, i64, i64, pvp, pvp, pvp, pvp, pvp, pi64, pi64]),
    "fx_fastq_pair_merge_alloc": (i32, [vp, vp, vp, i64, vp, i64, pvp, pvp, pi64, pi64, pi64]),
    "fx_bgzf_compress": (i32, [vp, i64, i32, i32, pvp, pi64, pvp, pi64]),
    "fx_fastq_format_bgzf_alloc": (i32, [vp, vp, i64, vp, vp, i64, i32, pvp, pvp, pvp, pi64, pi64, pi64, pi64, pi64]),
    "fx_fasta_format_bgzf_alloc": (i32, [vp, i64, vp, vp, vp, i32, vp, i64, vp, vp, i64, vp, vp, vp, i32, i32, i64, i32, pvp, pvp, pvp, pi64, pi64, pi64,
                                         pi64, pi64]),
    "fx_fastq_pair_merge_bgzf_alloc": (i32, [vp, vp, vp, i64, vp, i64, i32, pvp, pvp, pvp, pi64, pi64, pi64, pi64, pi64]),
    "fx_deflate_code_lengths": (i32, [vp, i32, i32, vp, vp]),
    "fx_fasta_kmers": (i32, [vp, i32, i32, vp, i64, i32, pvp, pi64, pi64]),
    "fx_fastq_kmers": (i32, [vp, i32, i32, vp, i64, vp, vp, pvp, pi64]),
    "fx_fasta_kmer_table": (i32, [vp, i32, i32, vp, i64, i64, i64] + [pvp] * 2 + [pi64] * 4),
    "fx_fastq_kmer_table": (i32, [vp, i32, i32, vp, i64, vp, vp, i64, i64] + [pvp] * 2 + [pi64] * 4),
    "fx_kmer_set_create": (i32, [vp, i32, i32, vp, i64, pvp]),
    "fx_kmer_set_free": (i32, [vp]),
    "fx_kmer_set_contains": (i32, [vp, vp, i64, vp]),
    "fx_fastq_kmer_hits": (i32, [vp, vp, vp, i64, vp, vp, pvp, pvp, pi64, pi64]),
    "fx_fastq_kmer_screen": (i32, [vp, vp, vp, i64, vp, vp, i64, i64, i64, i32, pvp, pi64, pi64]),
    "fx_fasta_kmer_hits": (i32, [vp, vp, vp, i64, pvp, pvp, pi64, pi64]),
    "fx_fasta_sketch": (i32, [vp, i32, i32, vp, i64, u64, i64, i32, pvp, pi32]),
    "fx_fastq_sketch": (i32, [vp, i32, i32, vp, i64, vp, vp, u64, i64, i32, pvp, pi32, pi64]),
    "fx_sketch_info": (i32, [vp, pi32, pi32, P(u64), pi64, pi64, pi64]),
    "fx_sketch_read": (i32, [vp, pvp, pvp]),
    "fx_sketch_from_host": (i32, [i32, i32, i32, u64, i64, i64, vp, vp, pvp]),
    "fx_sketch_compare": (i32, [vp, vp, vp, i64, vp, i64, i64, u64, i64, pvp, pvp]),
    "fx_sketch_free": (i32, [vp]),
    "fx_fastq_dup_first": (i32, [vp, vp, i64, vp, vp, i32, i32, pvp, pi64, pi64, pi64, pi64]),
    "fx_fastq_dedup": (i32, [vp, vp, i64, vp, vp, i32, i32, i64, i64, pvp, pvp, pi64, pi64, pi64, pi64]),
    "fx_names_build": (i32, [vp, i32]),
    "fx_names_lookup": (i32, [vp, i32, i64, vp, vp, vp]),
    "fx_names_sort": (i32, [vp, i32, i32, vp, pi64]),
    "fx_names_pack": (i32, [vp, i32, vp, i64, vp, pi64]),
    "fx_revcomp": (i32, [i32, i32, vp, i64, i32]),
    "fx_shard_summary_get": (i32, [vp, P(ShardSummary)]),
    "fx_fasta_set_row": (i32, [vp, i64, i64, i64, i64, i64, i32, i32, i32, i32]),
    "fx_shard_route": (i32, [i64, vp, vp, vp, i64, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp] + [vp] * 8),
    "fx_shard_summary_dev": (i32, [vp, vp]),
    "fx_fasta_stitch_dev": (i32, [vp, vp, i32, i32, i32]),
    "fx_stream": (vp, [vp]),
    "fx_read_fetch": (i32, [vp, i32, i64, vp, vp, vp, i32, i32, vp, vp, vp, vp]),
    "fx_gz_points": (i32, [vp, i64, vp, vp, i64, pi64, pi64]),
    "fx_fxi_bulk_rows": (i32, [cs, i32, i64, vp, vp, i32, vp]),
    "fx_fxi_bulk_index": (i32, [cs, i32, i64, vp, vp, vp]),
    "fx_fxi_bulk_index_int": (i32, [cs, i32, i64, vp, vp]),
    "fx_fxi_dev_sort": (i32, [vp, i32, pi64]),
    "fx_fxi_dev_write": (i32, [vp, i32, cs, i32, i32, pf64]),
    "fx_fxi_dev_build": (i32, [vp, i32, cs, i32, i32, pi64, pf64]),
    "fx_fxi_presize_begin": (i32, [cs, i64, i32, pvp]),
    "fx_fxi_presize_end": (i32, [vp, i32]),
    "fx_fxi_part_shape": (i32, [vp, i32, i64, pi64]),
    "fx_fxi_part_firsts": (i32, [vp, vp]),
    "fx_fxi_part_names": (i32, [vp, i32, vp, vp]),
    "fx_fxi_part_leaves": (i32, [vp, i32, cs, i64, i64, pf64]),
    "fx_fxi_join_grow": (i32, [cs, i32, i64, i64, i32, pi64]),
    "fx_fxi_join_begin": (i32, [i32, vp, vp, i64, pvp, pi64]),
    "fx_fxi_join_write": (i32, [vp, cs, i32, i32, i64, i64, vp, i64, pf64]),
    "fx_fxi_join_end": (None, [vp]),
    "fx_scratch_policy": (i32, [vp, i32, i64, i64, vp]),
    "fx_debug_fill_info": (i32, [pi32, pi64, pi64]),
    "fx_open_file_async": (i32, [cs, i32, pvp]),
    "fx_stage_wait": (i32, [vp, i64]),
    "fx_sync": (i32, [vp]),
    "fx_prof_default": (i32, [i32]),
    "fx_prof_enable": (i32, [vp, i32]),
    "fx_prof_reset": (i32, [vp]),
    "fx_prof_count": (i32, []),
    "fx_prof_name": (cs, [i32]),
    "fx_prof_read": (i32, [vp, i32, pf64, pi64]),
    "fx_comm_unique_id": (i32, [vp]),
    "fx_comm_init": (i32, [i32, i32, vp, i32, pvp]),
    "fx_comm_destroy": (i32, [vp]),
    "fx_comm_rank": (i32, [vp]),
    "fx_comm_world": (i32, [vp]),
    "fx_comm_allgather": (i32, [vp, vp, vp, i64]),
    "fx_fasta_build_sharded_begin": (i32, [vp, vp, i32]),
    "fx_fasta_build_sharded": (i32, [vp, vp, i32, vp]),
    "fx_comm_summaries": (i32, [vp, vp, vp]),
    "fx_fastq_build_sharded": (i32, [vp, vp, vp]),
    "fx_bgzf_counts": (i32, [vp, vp]),
    "fx_sort_packed_names": (i32, [i32, vp, vp, i64, vp, pi64]),
    "fx_gunzip_parallel": (i32, [vp, i64, i32, vp, i64, pi64, pi64]),
    "fx_gz_open_mode": (i32, [vp]),
    "fx_kseq_scan": (i32, [vp, vp, vp, vp, vp]),
    "fx_kseq_records": (i32, [vp, i64, i64, vp]),
    "fx_kseq_fetch": (i32, [vp, i32, i64, i64, i32, vp, vp, vp]),
    "fx_kseq_prefix_lines": (i64, [vp]),
}
SYMBOLS = list(PROTOTYPES)


def so_path():
    return _SO


def open_laps():
    """(device allocation, page cache -> HBM) seconds of this thread's last fx_open_file of a plain file."""
    a, b = C.c_double(0.0), C.c_double(0.0)
    lib().fx_open_laps(C.byref(a), C.byref(b))
    return float(a.value), float(b.value)


def build_laps():
    """The parts of this thread's last fx_fastq_build, seconds (fx_build_laps)."""
    a = (C.c_double * 8)()
    lib().fx_build_laps(a)
    return {"sample": float(a[0]), "count_pass_enqueue": float(a[1]), "count_pass_wait": float(a[2]), "table_alloc": float(a[4]), "rows": float(a[5])}


def debug_fill_info():
    """(byte, blocks, bytes) of FX_DEBUG_FILL: the byte in force or -1, and what has been filled since load."""
    b, n, t = C.c_int(0), C.c_int64(0), C.c_int64(0)
    lib().fx_debug_fill_info(C.byref(b), C.byref(n), C.byref(t))
    return int(b.value), int(n.value), int(t.value)


def fxi_presize_begin(path, nbytes, device=-1):
    """A library thread (on the CPUs next to `device`) grows the (just created) index file to nbytes with fallocate -> token for
    fxi_presize_end."""
    tok = C.c_void_p(None)
    check(lib().fx_fxi_presize_begin(os.fsencode(path), int(nbytes), int(device), C.byref(tok)))
    return tok


def fxi_join_grow(path, root_table, nleaf_table, device, extra_bytes=0):
    """Room for the table's new pages and extra_bytes behind them (best effort) -> the page number the parts' leaves begin at."""
    first = C.c_int64(0)
    check(lib().fx_fxi_join_grow(os.fsencode(path), int(root_table), int(nleaf_table), int(extra_bytes), int(device), C.byref(first)))
    return int(first.value)


class FxiJoin:
    """The writer's side of an index file that several handles fill (fx_fxi_join_*): the names of all parts, in part order,
    back to back in device memory (d_names, d_lens: pointers as integers), sorted once."""
    LAPS = ("file_grown", "index_shape", "index_kernels", "index_to_file", "host_levels_and_header", "table_interior")

    def __init__(self, device, d_names, d_lens, n):
        self._j, nd = C.c_void_p(), C.c_int64(0)
        check(lib().fx_fxi_join_begin(int(device), C.c_void_p(int(d_names or 0)), C.c_void_p(int(d_lens or 0)), int(n), C.byref(self._j), C.byref(nd)))
        self.n_dup = int(nd.value)

    def write(self, path, root_table, root_index, n_rows, first_rows, first_new_page):
        first_rows = np.ascontiguousarray(first_rows, dtype=np.int64)
        laps = (C.c_double * 6)()
        check(lib().fx_fxi_join_write(self._j, os.fsencode(path), int(root_table), int(root_index), int(n_rows), int(first_rows.size),
                                      _ptr(first_rows) if first_rows.size else None, int(first_new_page), laps))
        return dict(zip(self.LAPS, (float(x) for x in laps)))

    def close(self):
        if self._j:
            lib().fx_fxi_join_end(self._j)
            self._j = C.c_void_p()

    __del__ = close


def fxi_presize_end(token, cancel=False):
    if token is not None and token.value:
        lib().fx_fxi_presize_end(token, 1 if cancel else 0)
        token.value = None


def fxi_bulk_rows(path, rootpage, packed_names, name_off, cols):
    """Host-side bulk load of an index table (fx_fxi_bulk_rows): packed_names uint8, name_off int64[n+1],
    cols: list of int64 arrays.  packed_names = name_off = None: a table without a TEXT column (comp).
    The database file must have no open connection."""
    arrs = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    if name_off is None:
        check(lib().fx_fxi_bulk_rows(os.fsencode(path), int(rootpage), arrs[0].size if arrs else 0, None, None, len(arrs), ptrs))
        return
    names = np.ascontiguousarray(packed_names, dtype=np.uint8)
    offs = np.ascontiguousarray(name_off, dtype=np.int64)
    check(lib().fx_fxi_bulk_rows(os.fsencode(path), int(rootpage), offs.size - 1, names.ctypes.data if names.size else None,
                                 offs.ctypes.data, len(arrs), ptrs))


def fxi_bulk_index(path, rootpage, packed_names, name_off, order):
    """Host-side bulk load of the UNIQUE INDEX on the name column (fx_fxi_bulk_index): names in row order,
    order[i] = row of the i-th smallest name."""
    names = np.ascontiguousarray(packed_names, dtype=np.uint8)
    offs = np.ascontiguousarray(name_off, dtype=np.int64)
    order = np.ascontiguousarray(order, dtype=np.int64)
    if order.size != offs.size - 1:
        raise ValueError("order must have one entry per row")
    check(lib().fx_fxi_bulk_index(os.fsencode(path), int(rootpage), offs.size - 1, names.ctypes.data if names.size else None,
                                  offs.ctypes.data, order.ctypes.data if order.size else None))


def fxi_bulk_index_int(path, rootpage, key, order):
    """Host-side bulk load of a non-unique INDEX on an INTEGER column (fx_fxi_bulk_index_int)."""
    key = np.ascontiguousarray(key, dtype=np.int64)
    order = np.ascontiguousarray(order, dtype=np.int64)
    if key.size != order.size:
        raise ValueError("one key and one order entry per row")
    check(lib().fx_fxi_bulk_index_int(os.fsencode(path), int(rootpage), key.size, key.ctypes.data if key.size else None,
                                      order.ctypes.data if order.size else None))


def lib():
    """Load libfxgpu.so (after torch, if torch is importable, so both share one HIP runtime)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise ImportError(
            "pyfastx_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C pyfastx_amd/csrc`.  There is no CPU fallback." % _SO)
    if not os.environ.get("FX_NO_TORCH"):                  # FX_NO_TORCH=1: the library alone, on the system's ROCm (no torch in the process)
        try:
            import torch  # noqa: F401  (loads torch's bundled libamdhip64 first; ours then binds to the same runtime)
        except Exception:
            pass
    L = C.CDLL(_SO, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        f = getattr(L, name)
        f.restype = res
        if args:                                               # an entry of no arguments keeps ctypes' unchecked call
            f.argtypes = args
    _LIB = L
    return L


def sort_packed_names(packed, name_off, device=0):
    """fx_sort_packed_names: BINARY-collation order of names from several handles -> (order int64[n], duplicates)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    name_off = np.ascontiguousarray(name_off, dtype=np.int64)
    n = name_off.size - 1
    order = np.empty(max(n, 0), dtype=np.int64)
    nd = C.c_int64(0)
    check(lib().fx_sort_packed_names(int(device), _ptr(packed) if packed.size else None, _ptr(name_off), n, _ptr(order) if n > 0 else None, C.byref(nd)))
    return order, int(nd.value)


def gunzip_parallel(gz, threads=8):
    """fx_gunzip_parallel (host only): the inflated bytes of ONE gzip member and the number of restart points it found, or
    None when the parallel decoder declines (small input, several members, anything it is not sure of)."""
    src = np.frombuffer(gz, dtype=np.uint8)
    n, npts = C.c_int64(0), C.c_int64(0)
    cap = max(len(gz) * 8, 1 << 20)
    for _ in range(2):
        out = np.empty(cap, dtype=np.uint8)
        rc = lib().fx_gunzip_parallel(src.ctypes.data, src.size, int(threads), out.ctypes.data, cap, C.byref(n), C.byref(npts))
        if rc == 1:
            return None
        if rc == FX_ERANGE and n.value > cap:
            cap = int(n.value)
            continue
        check(rc)
        return out[:n.value].tobytes(), int(npts.value)
    raise FxError(FX_ERANGE, "output did not fit twice")


def device_memory(device=0):
    """-> (free, total) bytes of the device's HBM now."""
    f, t = C.c_int64(0), C.c_int64(0)
    check(lib().fx_device_memory(int(device), C.byref(f), C.byref(t)))
    return f.value, t.value


def stream_size(path):
    """-> (bytes of the uncompressed stream or -1, kind): kind 0 plain, 1 BGZF, 2 single-stream gzip (fx_stream_size)."""
    n, k = C.c_int64(0), C.c_int(0)
    check(lib().fx_stream_size(os.fsencode(path), C.byref(n), C.byref(k)))
    return int(n.value), int(k.value)


def shard_route(ids, starts, stops, cols, bases, ends, flags=0, flags_per_query=None):
    """fx_shard_route: a batch of (record, start, stop) over the byte-range shards [bases[r], ends[r]) -> dict in ROUTED
    order (by answering shard, then by position in the batch): order, shard_start[n_shard + 1], off, len, skip, take,
    fl, cnt.  cols: the global table as contiguous arrays boff, blen, llen, elen (int64) and reg (uint8)."""
    ids, a, b = (np.ascontiguousarray(x, dtype=np.int64) for x in (ids, starts, stops))
    n, G = ids.size, len(bases)
    bases, ends = np.ascontiguousarray(bases, dtype=np.int64), np.ascontiguousarray(ends, dtype=np.int64)
    fpq = None if flags_per_query is None else np.ascontiguousarray(flags_per_query, dtype=np.uint8)
    out = {k: np.empty(n, dtype=np.int64) for k in ("order", "off", "len", "skip", "take")}
    out["shard_start"] = np.zeros(G + 1, dtype=np.int64)
    out["fl"], out["cnt"] = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int32)
    check(lib().fx_shard_route(n, _ptr(ids), _ptr(a), _ptr(b), cols["boff"].size, _ptr(cols["boff"]), _ptr(cols["blen"]),
                               _ptr(cols["llen"]), _ptr(cols["elen"]), _ptr(cols["reg"]), G, _ptr(bases), _ptr(ends),
                               int(flags), _ptr(fpq), _ptr(out["order"]), _ptr(out["shard_start"]), _ptr(out["off"]),
                               _ptr(out["len"]), _ptr(out["skip"]), _ptr(out["take"]), _ptr(out["fl"]), _ptr(out["cnt"])))
    return out


def pinned_array(ptr, count, dtype=np.uint8):
    """A numpy array over `count` items of pinned memory that fx_pinned_alloc (or an fx_*_alloc entry) handed out; the
    block goes back to the library's pool when the last view of the array is gone (_fxobj.PinnedBuf owns it)."""
    from . import _fxobj
    L = lib()
    dt = np.dtype(dtype)
    owner = _fxobj.PinnedBuf(int(ptr), int(count) * dt.itemsize, C.cast(L.fx_pinned_free, C.c_void_p).value)
    return np.frombuffer(owner, dtype=dt, count=int(count))


def pinned_empty(count, dtype=np.uint8):
    """numpy array of `count` items in pinned host memory (fx_pinned_alloc): query arrays built in it go to the device
    without a staging copy, answers written into it arrive by DMA."""
    dt = np.dtype(dtype)
    p = lib().fx_pinned_alloc(max(int(count) * dt.itemsize, 1))
    if not p:
        raise FxError(FX_ENOMEM, lib().fx_last_error().decode())
    return pinned_array(p, count, dt)


def fetch_phases():
    """Host-side phases of this thread's last fx_*_fetch_alloc call, ms: (stage + upload, offsets, pinned blocks, launch, answers back, total)."""
    v = (C.c_double * 6)()
    check(lib().fx_fetch_phases(v, 6))
    return dict(zip(("stage_upload_ms", "offsets_wait_ms", "pinned_blocks_ms", "launch_ms", "answers_wait_ms", "call_ms"), [round(x, 3) for x in v]))


def check(rc):
    if rc != 0:
        raise FxError(rc, lib().fx_last_error().decode("utf-8", "replace"))


def _raise(rc, **attrs):
    """FxError of a failed call, with what the call reported beside its code (first_bad=...) as attributes."""
    e = FxError(rc, lib().fx_last_error().decode())
    for k, v in attrs.items():
        setattr(e, k, v)
    raise e


def _ptr(a):
    return None if a is None else a.ctypes.data


def _sel(ids):
    """A selection of records or reads as the entries take it -> (int64 array or None, count): None stays NULL (everything),
    an empty selection still hands over a valid pointer, with count 0."""
    if ids is None:
        return None, 0
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    return (ids if ids.size else np.zeros(1, dtype=np.int64)), ids.size


RAW = "raw"


def _column(p, spec, n):
    """One pinned block an entry handed out (c_void_p, at least one item) under its column spec (see _call)."""
    if not p.value:
        return None
    if spec is RAW:
        return p.value
    dt, w = spec if isinstance(spec, tuple) else (spec, 1)
    a = pinned_array(p.value, max(n * w, 1), dt)[:n * w]
    return a if w == 1 else a.reshape(n, w)


def _call(fn, head, cols=(), counters=(0,), err=None, tail=()):
    """The call path of the entries that answer in pinned memory: fn(*head, one out-pointer per column, one int64 counter per
    start value of `counters`, *tail) -> (tuple of columns, list of counter values).  numpy arrays in head and tail go over as
    their addresses; this frame holds them until fn has returned, so a caller may pass temporaries.  cols: per out-pointer a
    dtype (the array over the first n items, n = the first counter), (dtype, w) (the same as [n, w]), RAW (the address as
    the library gave it) or None (NULL goes over: not wanted); a pointer the library left NULL comes back as None.  A status
    other than 0 raises FxError with the attribute err = (name, index of the counter that feeds it)."""
    def addr(a):
        return a.ctypes.data if isinstance(a, np.ndarray) else a
    ptrs = [None if c is None else C.c_void_p() for c in cols]
    vals = [C.c_int64(v) for v in counters]
    rc = fn(*map(addr, head), *[p if p is None else C.byref(p) for p in ptrs], *map(C.byref, vals), *map(addr, tail))
    vals = [int(v.value) for v in vals]
    if rc:
        _raise(rc, **({err[0]: vals[err[1]]} if err else {}))
    return tuple(None if p is None else _column(p, c, vals[0] if vals else 0) for p, c in zip(ptrs, cols)), vals


def _ragged(dst, offs, n):
    """The block pair of an fx_*_alloc entry (addresses; offs holds n + 2 items) -> (uint8 buffer cut to offsets[n],
    int64 offsets[n + 1]), pinned."""
    o = pinned_array(offs, n + 2, np.int64)[:n + 1]
    return pinned_array(dst, max(int(o[n]), 1))[:int(o[n])], o


def _bgzf_blocks(zdst, moff, zbytes, members):
    """The block pair of a _bgzf entry (addresses) -> (uint8 stream cut to zbytes, int64 member offsets[members + 1]), pinned."""
    return pinned_array(zdst, max(zbytes, 1))[:zbytes], pinned_array(moff, members + 1, np.int64)


def bgzf_compress(data, level=2, device=0):
    """The bytes of `data` as BGZF members of 65280 bytes (fx_bgzf_compress; no EOF member) -> (uint8 stream, int64 member
    offsets[members + 1]), pinned.  A level outside 0..2 raises FxError(FX_EINVAL)."""
    a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    dst, moff, nb, nm = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0)
    check(lib().fx_bgzf_compress(a.ctypes.data if a.size else None, a.size, int(level), int(device), C.byref(dst), C.byref(nb), C.byref(moff), C.byref(nm)))
    return _bgzf_blocks(dst.value, moff.value, int(nb.value), int(nm.value))


def deflate_code_lengths(freq, limit=15):
    """The code lengths and the bit-reversed canonical codes the encoder gives these symbol counts (fx_deflate_code_lengths; host only)."""
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    lens, codes = np.zeros(f.size, dtype=np.uint8), np.zeros(f.size, dtype=np.uint16)
    check(lib().fx_deflate_code_lengths(f.ctypes.data, f.size, int(limit), lens.ctypes.data, codes.ctypes.data))
    return lens, codes


def too_many(e, noun, arg, limit):
    """The exception to raise for the FxError of a capped entry: FX_ERANGE with a true count (.n_hits / .n_rows) above the
    caller's limit becomes the ValueError that names it, anything else is `e` itself."""
    n = getattr(e, "n_hits", getattr(e, "n_rows", 0))
    if e.code == FX_ERANGE and n > limit:
        return ValueError("%d %s, more than %s=%d" % (n, noun, arg, limit))
    return e


def outside(e, what="interval", owner="read"):
    """The exception to raise for the FxError of a query entry: FX_ERANGE that names a query (.first_bad >= 0) becomes the
    ValueError that names it, anything else is `e` itself."""
    if e.code == FX_ERANGE and getattr(e, "first_bad", -1) >= 0:
        return ValueError("the %s of query %d lies outside its %s" % (what, e.first_bad, owner))
    return e


class Comm:
    """The library's own communicator (fx_comm: RCCL bound at run time) -- one per process, one process per GPU.
    The 128-byte id comes from rank 0 (Comm.unique_id()) over whatever channel the launcher offers; share_id() uses the
    torch.distributed process group when there is one."""

    def __init__(self, rank, world, uid, device=0):
        h = C.c_void_p()
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(uid))
        check(lib().fx_comm_init(int(rank), int(world), buf, int(device), C.byref(h)))
        self._c, self.rank, self.world, self.device = h, int(rank), int(world), int(device)

    @staticmethod
    def unique_id():
        buf = (C.c_ubyte * 128)()
        check(lib().fx_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def from_process_group(cls, device):
        """rank / world of torch.distributed's default group; the id travels over it (one broadcast at setup)."""
        import torch.distributed as dist
        # Every collective below is entered by EVERY rank whatever happens on one of them (a rank that failed early and went on
        # to the next collective while the others still sat in this one hung the job): rank 0 always broadcasts something --
        # the id, or None when it could not make one -- and ncclCommInitRank, itself collective, is only reached when an id exists.
        uid = None
        if dist.get_rank() == 0:
            try:
                uid = cls.unique_id()
            except Exception:                                   # noqa: BLE001  (no RCCL to bind)
                uid = None
        box = [uid]
        dist.broadcast_object_list(box, src=0)
        if box[0] is None:
            raise FxError(FX_EDEVICE, "rank 0 could not create a communicator id (RCCL not bound)")
        return cls(dist.get_rank(), dist.get_world_size(), box[0], device)

    def allgather(self, arr):
        """A small host array of every rank to every rank -> [world, ...] (fx_comm_allgather)."""
        a = np.ascontiguousarray(arr)
        out = np.empty((self.world,) + a.shape, dtype=a.dtype)
        check(lib().fx_comm_allgather(self._c, a.ctypes.data, out.ctypes.data, a.nbytes))
        return out

    def summaries(self, blob):
        from .shard import Summary, NWORDS
        out = np.zeros((self.world, NWORDS), dtype=np.int64)
        check(lib().fx_comm_summaries(self._c, blob._h, out.ctypes.data))
        return [Summary.from_array(r) for r in out]

    def close(self):
        if self._c:
            lib().fx_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SketchObj:
    """Owning wrapper of an fx_sketch: the sorted key lists of its sets in device memory, independent of the blob that made it
    (pyfastx_amd/sketch.py builds the public object on it)."""

    def __init__(self, ptr):
        self._s = ptr
        k, fl, mk, sz, ns, nk = C.c_int(0), C.c_int(0), C.c_uint64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().fx_sketch_info(self._s, C.byref(k), C.byref(fl), C.byref(mk), C.byref(sz), C.byref(ns), C.byref(nk)))
        self.k, self.flags, self.max_key, self.size, self.n_sets, self.n_keys = k.value, fl.value, mk.value, sz.value, ns.value, nk.value

    @classmethod
    def from_host(cls, device, k, flags, max_key, size, off, keys):
        """fx_sketch_from_host: off int64[n_sets + 1], keys uint64[off[-1]]; what the device checks refuse raises FxError(FX_EINVAL)."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        s = C.c_void_p()
        check(lib().fx_sketch_from_host(int(device), int(k), int(flags), int(max_key), int(size), off.size - 1, _ptr(off), _ptr(keys) if keys.size else None,
                                        C.byref(s)))
        return cls(s)

    def _live(self):
        if self._s is None:
            raise FxError(FX_ESTATE, "the sketch has been freed")
        return self._s

    def read(self):
        """(off int64[n_sets + 1], keys uint64[n_keys]) in pinned memory (fx_sketch_read)."""
        po, pk = C.c_void_p(), C.c_void_p()
        check(lib().fx_sketch_read(self._live(), C.byref(po), C.byref(pk)))
        return pinned_array(po.value, self.n_sets + 1, np.int64), pinned_array(pk.value, max(self.n_keys, 1), np.uint64)[:self.n_keys]

    def compare(self, other, ia=None, ib=None, limit=0, max_key=0, max_pairs=10**8):
        """(shared, total), int64[n_a, n_b] in pinned memory (fx_sketch_compare); ia / ib: the sets that take part, None: all."""
        (ia, na), (ib, nb) = _sel(ia), _sel(ib)
        na, nb = (self.n_sets if ia is None else na), (other.n_sets if ib is None else nb)
        ps, pt = C.c_void_p(), C.c_void_p()
        check(lib().fx_sketch_compare(self._live(), other._live(), _ptr(ia), na, _ptr(ib), nb, int(limit), int(max_key), int(max_pairs),
                                      C.byref(ps), C.byref(pt)))
        sh, tot = (_column(p, np.int64, na * nb) for p in (ps, pt))
        return sh.reshape(na, nb), tot.reshape(na, nb)

    def close(self):
        if self._s:
            lib().fx_sketch_free(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


KSEQ_REC = np.dtype([("hdr_off", "<i8"), ("hdr_line", "<i8"), ("seq_len", "<i8"), ("seq_cum", "<i8"),
                     ("hdr_len", "<u4"), ("s_n", "<u4"), ("q_n", "<u4"), ("flags", "<u4")])


class KmerSet:
    """Owning wrapper of an fx_kmer_set: a hash set of k-mer codes in device memory, created through a blob of its device and
    independent of it afterwards."""

    def __init__(self, blob, k, canonical, codes):
        codes = np.ascontiguousarray(codes, dtype=np.int64)
        s = C.c_void_p()
        check(lib().fx_kmer_set_create(blob._h, int(k), FX_KMER_CANONICAL if canonical else 0, _ptr(codes) if codes.size else None, codes.size, C.byref(s)))
        self._s, self.k, self.canonical, self.n = s, int(k), bool(canonical), int(codes.size)

    def contains(self, codes):
        """uint8 array: 1 where the code is in the set as given (fx_kmer_set_contains)."""
        codes = np.ascontiguousarray(codes, dtype=np.int64)
        out = np.zeros(codes.size, dtype=np.uint8)
        if self._s is None:
            raise FxError(FX_ESTATE, "the k-mer set has been freed")
        if codes.size:
            check(lib().fx_kmer_set_contains(self._s, _ptr(codes), codes.size, _ptr(out)))
        return out.reshape(codes.shape)

    def close(self):
        if self._s:
            lib().fx_kmer_set_free(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Blob:
    """Owning wrapper of an fx_handle: one staged stream resident in HBM."""

    def __init__(self, handle):
        self.on_close = []
        self._h = handle

    # -- constructors -------------------------------------------------------
    @classmethod
    def from_file(cls, path, device=0, gzindex=None):
        """gzindex: the restart points of a single-stream gzip file (fxi.read_gzindex) -> the segments between them are
        inflated in parallel (fx_open_file_indexed)."""
        h = C.c_void_p()
        if gzindex and len(gzindex["cmp"]) and gzindex["windows"] is not None:
            a = [np.ascontiguousarray(gzindex[k], dtype=np.int64) for k in ("cmp", "uncmp")]
            b = [np.ascontiguousarray(gzindex[k], dtype=np.uint8) for k in ("bits", "has")]
            w = np.ascontiguousarray(gzindex["windows"], dtype=np.uint8)
            check(lib().fx_open_file_indexed(os.fsencode(path), device, a[0].size, _ptr(a[0]), _ptr(a[1]), _ptr(b[0]), _ptr(b[1]),
                                             _ptr(w) if w.size else None, int(gzindex["uncompressed_size"]), C.byref(h)))
        else:
            check(lib().fx_open_file(os.fsencode(path), device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_file_range(cls, path, off, length, halo=0, device=0):
        """One byte-range shard of a file: bytes [off, off + length + halo) of the uncompressed stream (fx_open_file_range);
        the shard context (base, previous byte, is_last, halo) comes from the file."""
        h = C.c_void_p()
        check(lib().fx_open_file_range(os.fsencode(path), int(off), int(length), int(halo), device, C.byref(h)))
        b = cls(h)
        b.base = int(off)
        return b

    @classmethod
    def from_bytes(cls, data, device=0):
        a = np.frombuffer(data, dtype=np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, dtype=np.uint8)
        h = C.c_void_p()
        check(lib().fx_open_host(a.ctypes.data if a.size else None, a.size, device, C.byref(h)))
        return cls(h)

    @classmethod
    def from_file_async(cls, path, device=0):
        """A plain file staged in the background (fx_open_file_async): work on prefixes through views until stage_wait(-1)."""
        h = C.c_void_p()
        check(lib().fx_open_file_async(os.fsencode(path), device, C.byref(h)))
        return cls(h)

    def stage_wait(self, upto=-1):
        check(lib().fx_stage_wait(self._h, int(upto)))

    @classmethod
    def from_device(cls, dptr, nbytes, device=0, keepalive=None):
        h = C.c_void_p()
        check(lib().fx_open_device(C.c_void_p(dptr), nbytes, device, C.byref(h)))
        b = cls(h)
        b._keep = keepalive
        return b

    def close(self):
        if self._h:
            for f in self.__dict__.get("on_close", ()):          # owners that cached the raw handle (the C getters of api.Fasta / Fastq) let go of it first
                try:
                    f()
                except Exception:                                # noqa: BLE001
                    pass
            lib().fx_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- basics -------------------------------------------------------------
    @property
    def size(self):
        return lib().fx_size(self._h)

    @property
    def is_gzip(self):
        return bool(lib().fx_is_gzip(self._h))

    @property
    def device_ptr(self):
        return lib().fx_device_ptr(self._h)

    def set_shard(self, base, prev_byte, is_last):
        check(lib().fx_set_shard(self._h, base, prev_byte, int(is_last)))

    def read_bytes(self, off, n):
        out = np.empty(max(int(n), 0), dtype=np.uint8)
        if n > 0:
            check(lib().fx_read_bytes(self._h, int(off), int(n), out.ctypes.data))
        return out.tobytes()

    def first_byte(self):
        v = C.c_int(-1)
        check(lib().fx_first_byte(self._h, C.byref(v)))
        return v.value

    def gz_points(self, spacing=1048576):
        """-> (cmp_off int64[], uncmp_off int64[], compressed_size) restart points for the gzindex table."""
        n, cs = C.c_int64(0), C.c_int64(0)
        check(lib().fx_gz_points(self._h, spacing, None, None, 0, C.byref(n), C.byref(cs)))
        a = np.zeros(n.value, dtype=np.int64)
        b = np.zeros(n.value, dtype=np.int64)
        if n.value:
            check(lib().fx_gz_points(self._h, spacing, a.ctypes.data, b.ctypes.data, n.value, C.byref(n), C.byref(cs)))
        return a, b, cs.value

    @property
    def gz_open_mode(self):
        """0 plain, 1 BGZF on the device, 2 one gzip stream serially, 3 one stream on all host cores, 4 from restart points."""
        return int(lib().fx_gz_open_mode(self._h))

    # -- Fastx: the kseq walk -------------------------------------------------
    def kseq_scan(self):
        """kseq_read over the whole stream (fx_kseq_scan) -> (records, lines, sequence bytes, end code -1 / -2)."""
        nr, nl, sb, code = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
        check(lib().fx_kseq_scan(self._h, C.byref(nr), C.byref(nl), C.byref(sb), C.byref(code)))
        return int(nr.value), int(nl.value), int(sb.value), int(code.value)

    def kseq_prefix_lines(self):
        """Lines of the last kseq_scan that the parallel passes took (the walk did the rest)."""
        return int(lib().fx_kseq_prefix_lines(self._h))

    def kseq_records(self, first, count):
        """Records [first, first + count) of the walk as a structured array (fx_kseq_rec)."""
        out = np.zeros(int(count), dtype=KSEQ_REC)
        if count:
            check(lib().fx_kseq_records(self._h, int(first), int(count), _ptr(out)))
        return out

    def kseq_fetch(self, first, count, nbytes, upper=False, want_qual=True):
        """The sequence (and quality) strings of records [first, first + count), one behind the other: nbytes =
        seq_cum + seq_len of the last minus seq_cum of the first."""
        seq = np.empty(max(int(nbytes), 1), dtype=np.uint8)
        qual = np.empty(max(int(nbytes), 1), dtype=np.uint8) if want_qual else None
        got = C.c_int64(0)
        check(lib().fx_kseq_fetch(self._h, FX_HOST, int(first), int(count), FX_UPPER if upper else 0, _ptr(seq), _ptr(qual), C.byref(got)))
        if got.value != int(nbytes):
            raise RuntimeError("fx_kseq_fetch: %d bytes, expected %d" % (got.value, int(nbytes)))
        return seq[:int(nbytes)], (qual[:int(nbytes)] if want_qual else None)

    def bgzf_counts(self):
        """(members, members handed over to the serial decoder, reason of the first) of the open that made this blob."""
        a = (C.c_int64 * 3)()
        check(lib().fx_bgzf_counts(self._h, a))
        return int(a[0]), int(a[1]), int(a[2])

    def gz_checkpoints(self):
        """Restart points captured while a single gzip stream was inflated (fx_gz_checkpoints) -> dict cmp, uncmp (int64),
        bits, has (uint8), windows (uint8 [n_with_data * 32768])."""
        n, nw = C.c_int64(0), C.c_int64(0)
        check(lib().fx_gz_checkpoints(self._h, 0, None, None, None, None, None, C.byref(n), C.byref(nw)))
        out = {"cmp": np.zeros(n.value, dtype=np.int64), "uncmp": np.zeros(n.value, dtype=np.int64),
               "bits": np.zeros(n.value, dtype=np.uint8), "has": np.zeros(n.value, dtype=np.uint8),
               "windows": np.zeros(nw.value * 32768, dtype=np.uint8)}
        if n.value:
            check(lib().fx_gz_checkpoints(self._h, n.value, _ptr(out["cmp"]), _ptr(out["uncmp"]), _ptr(out["bits"]), _ptr(out["has"]),
                                          _ptr(out["windows"]) if nw.value else None, C.byref(n), C.byref(nw)))
        return out

    def sync(self):
        check(lib().fx_sync(self._h))

    def prof_enable(self, on=1):
        """0 off, 1 every kernel, 2 only the dominant scan kernel (k_span_scan / k_scan)."""
        check(lib().fx_prof_enable(self._h, int(on)))

    def prof_reset(self):
        check(lib().fx_prof_reset(self._h))

    def prof_read(self):
        """-> {kernel name: (total ms, launches)} for kernels that ran."""
        out = {}
        for i in range(lib().fx_prof_count()):
            ms, cnt = C.c_double(0), C.c_int64(0)
            check(lib().fx_prof_read(self._h, i, C.byref(ms), C.byref(cnt)))
            if cnt.value:
                out[lib().fx_prof_name(i).decode()] = (ms.value, cnt.value)
        return out

    # device-array variants (pointers are raw device addresses, e.g. tensor.data_ptr())
    def fasta_fetch_dev(self, n, seq_id, start, stop, dst, dst_off, flags=0, flags_per_query=0, out_len=0):
        check(lib().fx_fasta_fetch(self._h, FX_DEVICE, n, seq_id, start, stop, int(flags),
                                   flags_per_query or None, dst, dst_off, out_len or None))

    def fasta_table_dev(self, **ptrs):
        order = ("hoff", "boff", "blen", "slen", "llen", "elen", "norm", "dlen", "name_len")
        check(lib().fx_fasta_table(self._h, FX_DEVICE, *[ptrs.get(k) or None for k in order]))

    def fasta_comp_dev(self, ptr):
        check(lib().fx_fasta_comp(self._h, FX_DEVICE, ptr))

    def shard_summary(self):
        from .shard import Summary, FIELDS
        s = ShardSummary()
        check(lib().fx_shard_summary_get(self._h, C.byref(s)))
        return Summary((k, int(getattr(s, k))) for k in FIELDS)

    def shard_summary_dev(self, d_out):
        """Enqueue the 28-word boundary summary into a device buffer (no host round trip)."""
        check(lib().fx_shard_summary_dev(self._h, d_out))

    def fasta_stitch_dev(self, d_all, world, rank, full_name=False):
        """Enqueue the completion of this shard's last record from the gathered summaries (device)."""
        check(lib().fx_fasta_stitch_dev(self._h, d_all, int(world), int(rank), int(bool(full_name))))

    @property
    def stream(self):
        return lib().fx_stream(self._h)

    def fasta_set_row(self, k, boff, blen, slen, llen, elen, norm, dlen, name_len, reg=0):
        check(lib().fx_fasta_set_row(self._h, int(k), int(boff), int(blen), int(slen), int(llen), int(elen),
                                     (int(norm) & 1) | (int(bool(reg)) << 1), int(dlen), int(name_len)))

    # -- FASTA --------------------------------------------------------------
    def fasta_set_table(self, boff, blen, slen, llen, elen, norm):
        """Install the record table of an existing .fxi (no scan); fasta_fetch by id works afterwards."""
        a = [np.ascontiguousarray(x, dtype=np.int64) for x in (boff, blen, slen, llen)]
        b = [np.ascontiguousarray(x, dtype=np.int32) for x in (elen, norm)]
        check(lib().fx_fasta_set_table(self._h, a[0].size, *[_ptr(x) for x in a + b]))
        self._table_ready = True
        self._n_fasta = int(a[0].size)
        self._hdr_cols = False                              # (the .fxi rows say nothing of where the header lines lie)

    def fasta_build_begin(self, full_name=False, comp=False):
        """Enqueue the build and return (no host synchronisation); see fasta_build_end.  comp: the composition counters
        ride on the scan (one read of the stream for index + composition; fasta_comp* then only attribute them)."""
        self._hdr_cols = True
        self._table_ready = True
        self._n_fasta = None
        check(lib().fx_fasta_build_begin(self._h, int(bool(full_name)) | (2 if comp else 0)))

    def fasta_build_sharded_begin(self, comm, full_name=False, comp=False):
        """fx_fasta_build_sharded_begin: scan + tables + summary + ncclAllGather + stitch, enqueued on the handle's stream."""
        self._hdr_cols = True
        self._table_ready = True
        self._n_fasta = None
        check(lib().fx_fasta_build_sharded_begin(self._h, comm._c, int(bool(full_name)) | (2 if comp else 0)))

    def fastq_build_sharded(self, comm):
        s = FastqSummary()
        check(lib().fx_fastq_build_sharded(self._h, comm._c, C.byref(s)))
        return s

    def fasta_build_end(self):
        s = FastaSummary()
        check(lib().fx_fasta_build_end(self._h, C.byref(s)))
        self._n_fasta = int(s.n_seq)
        return s

    def fasta_build(self, full_name=False, comp=False):
        self._hdr_cols = True
        self._table_ready = True
        s = FastaSummary()
        check(lib().fx_fasta_build(self._h, int(bool(full_name)) | (2 if comp else 0), C.byref(s)))
        self._n_fasta = int(s.n_seq)
        return s

    def _check_rows(self, n, kind):
        """The C entries fill n_seq / n_reads rows whatever the caller allocated: refuse a wrong n here."""
        have = getattr(self, "_n_fasta" if kind == 0 else "_n_fastq", None)
        if have is None and kind == 0:
            have = int(self.fasta_build_end().n_seq)         # a build was only enqueued: wait for it, learn the count
        if have is not None and int(n) != have:
            raise ValueError("the table holds %d records, the caller asked for %d" % (have, int(n)))

    def fasta_table(self, n):
        self._check_rows(n, 0)
        cols = {k: np.empty(n, dtype=np.int64) for k in ("hoff", "boff", "blen", "slen", "llen")}
        cols.update({k: np.empty(n, dtype=np.int32) for k in ("elen", "norm", "dlen", "name_len")})
        check(lib().fx_fasta_table(self._h, FX_HOST, *[_ptr(cols[k]) for k in (
            "hoff", "boff", "blen", "slen", "llen", "elen", "norm", "dlen", "name_len")]))
        return cols

    def fasta_len_stats(self, count_min=0, half=0.0):
        """Statistics of the record lengths from the table in HBM (fx_fasta_len_stats) -> LenStats."""
        st = LenStats()
        check(lib().fx_fasta_len_stats(self._h, int(count_min), float(half), C.byref(st)))
        return st

    def fasta_line_regular(self, n):
        """int32[n]: 1 where slices of the record may use the line arithmetic (fx_fasta_line_regular)."""
        self._check_rows(n, 0)
        reg = np.zeros(n, dtype=np.int32)
        if n:
            check(lib().fx_fasta_line_regular(self._h, FX_HOST, reg.ctypes.data))
        return reg

    def fasta_comp(self, n):
        self._check_rows(n, 0)
        comp = np.zeros((n, 128), dtype=np.int64)
        check(lib().fx_fasta_comp(self._h, FX_HOST, comp.ctypes.data))
        return comp

    def fasta_comp_sparse(self, guess=0):
        """-> (seqid, abc, num int64 arrays: the non-zero bins in record order, seqid 1-based; total int64[128])."""
        total = np.zeros(128, dtype=np.int64)
        cap = int(guess)
        for _ in range(2):
            arrs = [np.empty(max(cap, 1), dtype=np.int64) for _ in range(3)]
            nout = C.c_int64(0)
            rc = lib().fx_fasta_comp_sparse(self._h, FX_HOST, cap, arrs[0].ctypes.data, arrs[1].ctypes.data, arrs[2].ctypes.data,
                                            C.byref(nout), total.ctypes.data)
            if rc == FX_ERANGE and nout.value > cap:
                cap = int(nout.value)
                continue
            check(rc)
            return arrs[0][:nout.value], arrs[1][:nout.value], arrs[2][:nout.value], total
        raise FxError(FX_ERANGE, "composition did not fit twice")

    def fasta_comp_shard(self, n, lead_from):
        """-> (comp int64[n,128] of the records that start in this shard, lead int64[128]: the bytes before the
        shard's first header line from global offset lead_from on; lead_from < 0: not counted)."""
        self._check_rows(n, 0)
        comp = np.zeros((max(n, 1), 128), dtype=np.int64)
        lead = np.zeros(128, dtype=np.int64)
        check(lib().fx_fasta_comp_shard(self._h, FX_HOST, comp.ctypes.data, int(lead_from), lead.ctypes.data))
        return comp[:n], lead

    # -- FASTQ --------------------------------------------------------------
    def fastq_build(self, comp=False):
        """comp: count the composition on the way (fx_fastq_build_comp: index and base / meta in one read of the stream)."""
        s = FastqSummary()
        check((lib().fx_fastq_build_comp if comp else lib().fx_fastq_build)(self._h, C.byref(s)))
        self._n_fastq = int(s.n_reads)
        return s

    def set_halo(self, halo):
        check(lib().fx_set_halo(self._h, int(halo)))

    def fastq_scan(self):
        """phase 1 of a sharded FASTQ build -> (newlines in the core, offset of the last one or -1)"""
        a, b = C.c_int64(0), C.c_int64(0)
        check(lib().fx_fastq_scan(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fastq_build_ctx(self, line_offset, prev_nl):
        s = FastqSummary()
        check(lib().fx_fastq_build_ctx(self._h, int(line_offset), int(prev_nl), C.byref(s)))
        self._n_fastq = int(s.n_reads)
        return s

    def fastq_table(self, n):
        self._check_rows(n, 1)
        cols = {k: np.empty(n, dtype=np.int64) for k in ("name_off", "rlen", "soff", "qoff")}
        cols.update({k: np.empty(n, dtype=np.int32) for k in ("name_len", "dlen")})
        check(lib().fx_fastq_table(self._h, FX_HOST, _ptr(cols["name_off"]), _ptr(cols["name_len"]),
                                   _ptr(cols["dlen"]), _ptr(cols["rlen"]), _ptr(cols["soff"]), _ptr(cols["qoff"])))
        return cols

    def fastq_comp(self):
        base = np.zeros(5, dtype=np.int64)
        meta = np.zeros(5, dtype=np.int64)
        check(lib().fx_fastq_comp(self._h, base.ctypes.data, meta.ctypes.data))
        return base, meta

    # -- names ----------------------------------------------------------------
    def names_build(self, kind):
        """kind 0: FASTA sequence names, 1: FASTQ read names -> id table in HBM."""
        check(lib().fx_names_build(self._h, int(kind)))

    def names_lookup(self, names):
        """list of str / bytes -- or the names pre-packed as a (bytes, int64 offsets[n + 1]) pair -- -> int64 ids (0-based,
        -1 when absent), one kernel launch."""
        if isinstance(names, tuple) and len(names) == 2 and not isinstance(names[1], (str, int)) and \
                isinstance(names[0], (bytes, bytearray, memoryview, np.ndarray)):
            offs = np.ascontiguousarray(np.frombuffer(names[1], dtype=np.int64) if not isinstance(names[1], np.ndarray) else names[1], dtype=np.int64)
            n = offs.size - 1
            out = np.empty(max(n, 0), dtype=np.int64)
            if n <= 0:
                return out
            raw = np.frombuffer(names[0], dtype=np.uint8) if not isinstance(names[0], np.ndarray) else names[0]
            total = int(offs[n])
            packed = raw if raw.size >= total + 8 else np.concatenate([raw[:total], np.zeros(16, dtype=np.uint8)])
            check(lib().fx_names_lookup(self._h, FX_HOST, n, _ptr(packed), _ptr(offs), _ptr(out)))
            return out
        n = len(names)
        out = np.empty(n, dtype=np.int64)
        if not n:
            return out
        from . import _fxobj
        try:                                                    # one C pass over the list: sizes, then the bytes back to back (+ 16 zero bytes)
            pb, po = _fxobj.pack_names(names)
            packed, offs = np.frombuffer(pb, dtype=np.uint8), np.frombuffer(po, dtype=np.int64)
        except ValueError:                                      # a name with surrogate escapes: encode one by one
            enc = [x if isinstance(x, bytes) else x.encode("utf-8", "surrogateescape") for x in names]
            offs = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(np.fromiter(map(len, enc), dtype=np.int64, count=n), out=offs[1:])
            packed = np.frombuffer(b"".join(enc) + b"\0" * 16, dtype=np.uint8)
        check(lib().fx_names_lookup(self._h, FX_HOST, n, _ptr(packed), _ptr(offs), _ptr(out)))
        return out

    def names_pack(self, kind, n, guess=0):
        """-> (packed uint8, name_off int64[n+1]): the names of the n records back to back, from the table in HBM."""
        offs = np.zeros(int(n) + 1, dtype=np.int64)
        total = C.c_int64(0)
        cap = int(guess)
        for _ in range(2):
            buf = np.empty(max(cap, 1), dtype=np.uint8)
            rc = lib().fx_names_pack(self._h, int(kind), buf.ctypes.data, cap, offs.ctypes.data, C.byref(total))
            if rc == FX_ERANGE and total.value > cap:
                cap = int(total.value)
                continue
            check(rc)
            return buf[:total.value], offs
        raise FxError(FX_ERANGE, "names did not fit twice")

    def fastq_comp_info(self):
        """How the last fastq_build(comp=True) counted -> (runs, runs counted again from the prefixes or -1, one-read result in use)."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int(0)
        check(lib().fx_fastq_comp_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), bool(c.value)

    def fxi_dev_sort(self, kind):
        """The sorted order of the record names, computed and KEPT on the device for fxi_dev_write -> number of adjacent
        equal pairs (0: the names are distinct and the UNIQUE INDEX may be written)."""
        ndup = C.c_int64(0)
        check(lib().fx_fxi_dev_sort(self._h, int(kind), C.byref(ndup)))
        return int(ndup.value)

    FXI_LAPS = ("table_shape", "table_kernels", "table_to_file", "file_grown", "index_shape", "index_kernels", "index_to_file", "host_levels_and_header")

    def fxi_dev_write(self, kind, path, root_table, root_index=0):
        """The big table of a new index file (and, root_index != 0, the UNIQUE INDEX on its name column) as b-tree pages
        formatted on the device (fx_fxi_dev_write) -> dict of the phases in seconds."""
        laps = (C.c_double * 8)()
        check(lib().fx_fxi_dev_write(self._h, int(kind), os.fsencode(path), int(root_table), int(root_index), laps))
        return dict(zip(self.FXI_LAPS, (float(x) for x in laps)))

    # -- one index file from several handles (fx_fxi_part_*: this handle's part) --
    def fxi_part_shape(self, kind, row_base):
        """-> (rows, table leaves, bytes of names) of this handle's part of the table; rowids start at row_base + 1."""
        out = (C.c_int64 * 3)()
        check(lib().fx_fxi_part_shape(self._h, int(kind), int(row_base), out))
        return int(out[0]), int(out[1]), int(out[2])

    def fxi_part_firsts(self, nleaf):
        first = np.empty(int(nleaf), dtype=np.int64)
        check(lib().fx_fxi_part_firsts(self._h, _ptr(first) if nleaf else None))
        return first

    def fxi_part_names(self, kind, d_names, d_lens):
        """Names back to back + their lengths into DEVICE memory (pointers as integers: torch data_ptr())."""
        check(lib().fx_fxi_part_names(self._h, int(kind), C.c_void_p(int(d_names)), C.c_void_p(int(d_lens))))

    def fxi_part_leaves(self, kind, path, first_new_page, leaf_base):
        laps = (C.c_double * 2)()
        check(lib().fx_fxi_part_leaves(self._h, int(kind), os.fsencode(path), int(first_new_page), int(leaf_base), laps))
        return {"table_kernels": float(laps[0]), "table_to_file": float(laps[1])}

    def fxi_dev_build(self, kind, path, root_table, root_index):
        """fxi_dev_sort + fxi_dev_write in one call, the sort and the index shape beside the table's copy-out (fx_fxi_dev_build)
        -> (n_dup, phases in seconds); n_dup > 0: the table alone was written, drop the empty index."""
        laps = (C.c_double * 8)()
        nd = C.c_int64(0)
        check(lib().fx_fxi_dev_build(self._h, int(kind), os.fsencode(path), int(root_table), int(root_index), C.byref(nd), laps))
        d = dict(zip(self.FXI_LAPS, (float(x) for x in laps)))
        d["sort_and_index_shape_not_hidden"] = d.pop("index_shape")
        return int(nd.value), d

    def names_sort(self, kind, n):
        """-> (order int64[n], n_dup): sorted order of the n record names (BINARY collation) computed on the GPU."""
        n = int(n)
        order = np.empty(n, dtype=np.int64)
        ndup = C.c_int64(0)
        check(lib().fx_names_sort(self._h, int(kind), FX_HOST, _ptr(order) if n else None, C.byref(ndup)))
        return order, int(ndup.value)

    # -- fetch (host arrays) ------------------------------------------------
    @staticmethod
    def _i64(a):
        return np.ascontiguousarray(a, dtype=np.int64)

    def fetch_one(self, off, blen, slen, flags=0, skip=0):
        """One range -> bytes (fx_fetch_one: one launch, one wait, no staging copies)."""
        slen = int(slen)
        if slen <= 65536:                                   # the getter path: one buffer per Blob, no allocation per call
            ob = self.__dict__.get("_one")
            if ob is None:
                ob = self.__dict__["_one"] = (C.create_string_buffer(65536), C.c_int64(0))
            buf, got = ob
        else:
            buf, got = C.create_string_buffer(slen), C.c_int64(0)
        rc = lib().fx_fetch_one(self._h, int(off), int(blen), int(skip), slen, int(flags), buf, C.byref(got))
        if rc:
            check(rc)
        return C.string_at(buf, got.value)

    def fetch_ranges(self, off, blen, slen, flags=0, flags_per_query=None, skip=None):
        """-> (uint8 buffer, offsets int64[n+1] (exclusive cumsum of slen), out_len int64[n]).  skip: kept bytes dropped
        in front of each answer (fx_fetch_slices: slice after despacing)."""
        off, blen, slen = self._i64(off), self._i64(blen), self._i64(slen)
        n = off.size
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.maximum(slen, 0), out=offs[1:])
        dst = np.empty(max(int(offs[-1]), 1), dtype=np.uint8)     # the copy back fills all of it (np.zeros would touch every page first)
        out_len = np.zeros(n, dtype=np.int64)
        fpq = None if flags_per_query is None else np.ascontiguousarray(flags_per_query, dtype=np.uint8)
        if n and skip is not None:
            skip = self._i64(skip)
            check(lib().fx_fetch_slices(self._h, FX_HOST, n, _ptr(off), _ptr(blen), _ptr(skip), _ptr(slen), int(flags),
                                        _ptr(fpq), _ptr(dst), _ptr(offs), _ptr(out_len)))
        elif n:
            check(lib().fx_fetch_ranges(self._h, FX_HOST, n, _ptr(off), _ptr(blen), _ptr(slen), int(flags),
                                        _ptr(fpq), _ptr(dst), _ptr(offs), _ptr(out_len)))
        return dst[:int(offs[-1])], offs, out_len

    def fasta_fetch(self, seq_id, start, stop, flags=0, flags_per_query=None):
        seq_id, start, stop = self._i64(seq_id), self._i64(start), self._i64(stop)
        n = seq_id.size
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.maximum(stop - start, 0), out=offs[1:])
        dst = np.empty(max(int(offs[-1]), 1), dtype=np.uint8)     # the copy back fills all of it (np.zeros would touch every page first)
        out_len = np.zeros(n, dtype=np.int64)
        fpq = None if flags_per_query is None else np.ascontiguousarray(flags_per_query, dtype=np.uint8)
        if n:
            check(lib().fx_fasta_fetch(self._h, FX_HOST, n, _ptr(seq_id), _ptr(start), _ptr(stop), int(flags),
                                       _ptr(fpq), _ptr(dst), _ptr(offs), _ptr(out_len)))
        return dst[:int(offs[-1])], offs, out_len

    def fasta_fetch_alloc(self, seq_id, start, stop, flags=0, flags_per_query=None):
        """(record id, start, stop) batches with the layout left to the library (fx_fasta_fetch_alloc): intervals checked on the
        device, answers and offsets in pinned memory -> (uint8 buffer, int64 offsets[n+1]); an invalid query raises
        FxError(FX_ERANGE) whose .first_bad is its index."""
        seq_id, start, stop = self._i64(seq_id), self._i64(start), self._i64(stop)
        n = seq_id.size
        if start.size != n or stop.size != n:
            raise ValueError("ids, starts and stops differ in length")
        fpq = None if flags_per_query is None else np.ascontiguousarray(flags_per_query, dtype=np.uint8)
        dst, offs, bad = C.c_void_p(), C.c_void_p(), C.c_int64(-1)
        rc = lib().fx_fasta_fetch_alloc(self._h, n, _ptr(seq_id), _ptr(start), _ptr(stop), int(flags), _ptr(fpq),
                                        C.byref(dst), C.byref(offs), C.byref(bad))
        if rc:
            _raise(rc, first_bad=int(bad.value))
        o = pinned_array(offs.value, n + 2, np.int64)[:n + 1]
        return pinned_array(dst.value, max(int(o[n]), 1))[:int(o[n])], o

    def fasta_format_alloc(self, n, seq_id=None, start=None, stop=None, flags=0, flags_per_query=None, width=60, hdr=None,
                           hdr_off=None, mask=None, mask_mode=0, mask_byte=78, min_len=0, level=None):
        """FASTA records of n queries (fx_fasta_format_alloc; level 0..2: fx_fasta_format_bgzf_alloc, see below): seq_id None: the records 0..n-1; start = stop = None: whole
        records; hdr / hdr_off: the headers' bytes and their n + 1 offsets, or None for the records' own; mask: None or
        (ids, starts, stops) sorted and disjoint -> (uint8 buffer, int64 offsets[n + 1], records kept, their letters), pinned.
        A bad query raises FxError(FX_ERANGE), a bad mask row FxError(FX_EINVAL), each with .first_bad."""
        def i64(a):
            return None if a is None else np.ascontiguousarray(a, dtype=np.int64)
        seq_id, start, stop, hdr_off = i64(seq_id), i64(start), i64(stop), i64(hdr_off)
        fpq = None if flags_per_query is None else np.ascontiguousarray(flags_per_query, dtype=np.uint8)
        hdr = None if hdr is None else np.ascontiguousarray(hdr, dtype=np.uint8)
        m = (None, None, None) if mask is None else tuple(i64(a) for a in mask)
        n_mask = 0 if mask is None else int(m[0].size)
        if n_mask == 0:
            m = (None, None, None)
        for a in (seq_id, start, stop, fpq):
            if a is not None and a.size != n:
                raise ValueError("a query array does not hold one row per query (%d)" % n)
        if hdr is not None and (hdr_off is None or hdr_off.size != n + 1):
            raise ValueError("hdr_off must hold n + 1 offsets")
        head = (self._h, int(n), _ptr(seq_id), _ptr(start), _ptr(stop), int(flags), _ptr(fpq), int(width), _ptr(hdr), _ptr(hdr_off),
                n_mask, _ptr(m[0]), _ptr(m[1]), _ptr(m[2]), int(mask_mode), int(mask_byte), int(min_len))
        if level is not None:                                  # -> (stream, member offsets, record offsets in the uncompressed stream, kept, letters)
            (zdst, moff, offs), (kept, bases, _, zb, nm) = _call(lib().fx_fasta_format_bgzf_alloc, head + (int(level),), (RAW, RAW, RAW),
                                                                 counters=(0, 0, -1, 0, 0), err=("first_bad", 2))
            return _bgzf_blocks(zdst, moff, zb, nm) + (pinned_array(offs, int(n) + 1, np.int64), kept, bases)
        (dst, offs), (kept, bases, _) = _call(lib().fx_fasta_format_alloc, head, (RAW, RAW), counters=(0, 0, -1), err=("first_bad", 2))
        return _ragged(dst, offs, int(n)) + (kept, bases)

    def fasta_search(self, pattern, rpattern, mode, ids=None, cap=0, counts=False, max_mismatch=None, anchor=0):
        """Every overlapping hit of one pattern on the resident table (fx_fasta_search): pattern / rpattern are the bytes
        searched on + / - (None for a strand that is not in `mode`).  -> (n_hits, (rec, start, strand) pinned arrays or None,
        counts int64[n_sel, 2] or None); more than `cap` hits raise FxError(FX_ERANGE) whose .n_hits is the true count.
        cap = 0 with counts: counts only.  (max_mismatch, anchor: how fasta_search_approx comes through here.)"""
        plen = len(pattern if pattern is not None else rpattern)
        pat = None if pattern is None else np.frombuffer(bytes(pattern), dtype=np.uint8)
        rpat = None if rpattern is None else np.frombuffer(bytes(rpattern), dtype=np.uint8)
        if max_mismatch is None:
            fn, head, cols = lib().fx_fasta_search, (self._h, pat, rpat, plen, int(mode)), (np.int64, np.int64, np.uint8)
        else:
            fn, head = lib().fx_fasta_search_approx, (self._h, pat, rpat, plen, int(mode), int(max_mismatch), int(anchor))
            cols = (np.int64, np.int64, np.uint8, np.uint8)
        return self._hits(fn, head, ids, cap, counts, cols)

    def _hits(self, fn, head, ids, cap, counts, cols):
        """The tail the hit entries share: fn(*head, ids, n_ids, cap, the hit columns, n_hits, counts[n_sel, 2] or NULL) ->
        (n_hits, the columns or None where the entry made none, counts or None)."""
        ids, n_ids = _sel(ids)
        cnt = np.zeros((self._n_selected(ids, n_ids), 2), dtype=np.int64) if counts else None
        hits, (n,) = _call(fn, head + (ids, n_ids, int(cap)), cols, err=("n_hits", 0), tail=(cnt,))
        return n, (None if hits[0] is None else hits), cnt

    def fasta_search_approx(self, pattern, rpattern, mode, max_mismatch, anchor=0, ids=None, cap=0, counts=False):
        """fasta_search with up to max_mismatch mismatching letters per hit, none of them at a position whose bit is set in
        `anchor` (bit j = letter j of `pattern`) (fx_fasta_search_approx) -> (n_hits, (rec, start, strand, mismatch) pinned
        arrays or None, counts or None)."""
        return self.fasta_search(pattern, rpattern, mode, ids, cap, counts, int(max_mismatch), anchor)

    def fasta_search_edit(self, pattern, rpattern, mode, max_edits, report=FX_EDIT_BEST, ids=None, cap=0, counts=False):
        """Every end of the pattern within max_edits edits (Levenshtein) on the resident table, all of them or the best of every
        dip (report: FX_EDIT_ALL / FX_EDIT_BEST) (fx_fasta_search_edit) -> (n_hits, n_ends, (rec, start, stop, strand, edits)
        pinned arrays or None, counts int64[n_sel, 2] or None); more than `cap` ENDS raise FxError(FX_ERANGE) whose .n_ends is
        the true count.  cap = 0 with counts: counts only."""
        plen = len(pattern if pattern is not None else rpattern)
        pat = None if pattern is None else np.frombuffer(bytes(pattern), dtype=np.uint8)
        rpat = None if rpattern is None else np.frombuffer(bytes(rpattern), dtype=np.uint8)
        ids, n_ids = _sel(ids)
        cnt = np.zeros((self._n_selected(ids, n_ids), 2), dtype=np.int64) if counts else None
        rows, (n, n_ends) = _call(lib().fx_fasta_search_edit, (self._h, pat, rpat, plen, int(mode), int(max_edits), int(report), ids, n_ids, int(cap)),
                                  (np.int64, np.int64, np.int64, np.uint8, np.uint8), counters=(0, 0), err=("n_ends", 1), tail=(cnt,))
        return n, n_ends, (None if rows[0] is None else rows), cnt

    def _n_selected(self, ids, n_ids):
        if ids is not None:
            return n_ids
        n_sel = getattr(self, "_n_fasta", None)
        if n_sel is None:
            n_sel = int(self.fasta_build_end().n_seq)         # a build was only enqueued: wait for it, learn the count
        return n_sel

    def fasta_pwm_scan(self, mat, mode, min_score, ids=None, cap=0, counts=False):
        """Every window whose score under the int32 [W, 4] matrix `mat` is >= min_score (fx_fasta_pwm_scan) -> (n_hits,
        (rec, start, strand, score) pinned arrays or None, counts int64[n_sel, 2] or None); more than `cap` hits raise
        FxError(FX_ERANGE) whose .n_hits is the true count.  cap = 0 with counts: counts only."""
        mat = np.ascontiguousarray(mat, dtype=np.int32)
        return self._hits(lib().fx_fasta_pwm_scan, (self._h, mat, mat.shape[0], int(mode), int(min_score)), ids, cap, counts,
                          (np.int64, np.int64, np.uint8, np.int32))

    def fasta_pwm_best(self, mat, mode, ids=None):
        """The best-scoring window of every selected record and strand (fx_fasta_pwm_best) -> (scores int32[n_sel, 2],
        starts int64[n_sel, 2]); (INT32_MIN, -1) where there is none."""
        mat = np.ascontiguousarray(mat, dtype=np.int32)
        ids, n_ids = _sel(ids)
        n_sel = self._n_selected(ids, n_ids)
        scores = np.full((n_sel, 2), np.iinfo(np.int32).min, dtype=np.int32)
        starts = np.full((n_sel, 2), -1, dtype=np.int64)
        _call(lib().fx_fasta_pwm_best, (self._h, mat, mat.shape[0], int(mode), ids, n_ids, scores, starts), counters=())
        return scores, starts

    def fasta_minimizers(self, k, w, flags, ids=None, cap=0, counts=False):
        """The (w, k) minimizers of the selected records (fx_fasta_minimizers; flags: FX_MZ_CANONICAL | FX_MZ_LEX) -> (n_hits,
        (rec, start, strand, code) pinned arrays or None, counts int64[n_sel, 2] or None); more than `cap` rows raise
        FxError(FX_ERANGE) whose .n_hits is the true count.  cap = 0 with counts: counts only."""
        return self._hits(lib().fx_fasta_minimizers, (self._h, int(k), int(w), int(flags)), ids, cap, counts,
                          (np.int64, np.int64, np.uint8, np.uint64))

    def fasta_rank_build(self):
        """The rank index of the resident table (fx_fasta_rank_build); a second call does nothing."""
        check(lib().fx_fasta_rank_build(self._h))

    def fasta_rank_free(self):
        """The rank index's device memory back to the pool (fx_fasta_rank_free); the next region / window / run call rebuilds it."""
        check(lib().fx_fasta_rank_free(self._h))

    def fasta_region_counts(self, seq_id, start, stop):
        """The seven class counts A C G T N other masked of every (record id, start, stop) (fx_fasta_region_counts) ->
        int64[n, 7]; an invalid query raises FxError(FX_ERANGE) whose .first_bad is its index."""
        seq_id, start, stop = self._i64(seq_id), self._i64(start), self._i64(stop)
        n = seq_id.size
        if start.size != n or stop.size != n:
            raise ValueError("ids, starts and stops differ in length")
        counts = pinned_empty(n * 7, np.int64).reshape(n, 7)
        bad = C.c_int64(-1)
        rc = lib().fx_fasta_region_counts(self._h, FX_HOST, n, _ptr(seq_id), _ptr(start), _ptr(stop), _ptr(counts), C.byref(bad))
        if rc:
            _raise(rc, first_bad=int(bad.value))
        return counts

    def fasta_window_counts(self, window, step, partial=True, ids=None, cap=10**8):
        """The windows of the selected records and their class counts (fx_fasta_window_counts) -> (rec, start, stop, counts
        int64[n, 7]) pinned arrays; more than `cap` windows raise FxError(FX_ERANGE) whose .n_rows is the true count."""
        return _call(lib().fx_fasta_window_counts, (self._h, *_sel(ids), int(window), int(step), int(bool(partial)), int(cap)),
                     [np.int64] * 3 + [(np.int64, 7)], err=("n_rows", 0))[0]

    def fasta_class_runs(self, set32, min_len=1, ids=None, cap=10**8):
        """Every maximal interval of letters of the 256-bit set `set32` (32 bytes) of at least min_len letters
        (fx_fasta_class_runs) -> (rec, start, stop) pinned arrays; more than `cap` raise FxError(FX_ERANGE) whose .n_rows is
        the true count."""
        bits = np.frombuffer(bytes(set32), dtype=np.uint8)
        if bits.size != 32:
            raise ValueError("a byte set is 32 bytes")
        return _call(lib().fx_fasta_class_runs, (self._h, bits, int(min_len), *_sel(ids), int(cap)), [np.int64] * 3,
                     counters=(0, 0), err=("n_rows", 1))[0]

    def fasta_low_complexity(self, window=64, threshold=20, min_len=1, ids=None, cap=10**8):
        """The low-complexity intervals of the windowed DUST score (fx_fasta_low_complexity): window 4..64 letters, threshold
        in tenths -> (rec, start, stop) pinned arrays; more than `cap` raise FxError(FX_ERANGE) whose .n_rows is the true
        count."""
        return _call(lib().fx_fasta_low_complexity, (self._h, int(window), int(threshold), int(min_len), *_sel(ids), int(cap)), [np.int64] * 3,
                     counters=(0, 0), err=("n_rows", 1))[0]

    def fastq_complexity(self, ids=None, start=None, end=None):
        """Per query the columns of seq[start:end] (fx_fastq_complexity) -> (length int64, n_triplets int32, dust_sum int64,
        n_diff int32) in pinned memory.  A bad id or interval raises FxError(FX_ERANGE) with .first_bad."""
        return _call(lib().fx_fastq_complexity, (self._h, *self._fastq_queries(ids, start, end)), (np.int64, np.int32, np.int64, np.int32),
                     counters=(0, -1), err=("first_bad", 1))[0]

    def fasta_tandem_repeats(self, min_copies, min_len=0, ids=None, cap=10**8):
        """The perfect tandem repeats of period 1..len(min_copies) <= 8 (fx_fasta_tandem_repeats): min_copies[p - 1] copies at
        least of period p, 0 = not searched -> (rec, start, stop int64, period uint8, motif uint32) pinned arrays ordered by
        record, stop, period; more than `cap` raise FxError(FX_ERANGE) whose .n_rows is the true count."""
        mc = np.ascontiguousarray(min_copies, dtype=np.int32)
        return _call(lib().fx_fasta_tandem_repeats, (self._h, mc, int(mc.size), int(min_len), *_sel(ids), int(cap)),
                     (np.int64, np.int64, np.int64, np.uint8, np.uint32), counters=(0, 0), err=("n_rows", 1))[0]

    def fasta_orfs(self, stop_mask, start_mask, mode=1, strands=3, min_len=0, ids=None, cap=10**8):
        """The open reading frames of the six frames (fx_fasta_orfs): masks by codon index 16 c0 + 4 c1 + c2 in A C G T order,
        mode 0 stop to stop / 1 START to stop, strands 1 + / 2 - / 3 both -> (rec, start, stop int64, frame int8, flags uint8)
        pinned arrays in the order the header states; more than `cap` raise FxError(FX_ERANGE) whose .n_rows is the true
        count."""
        return _call(lib().fx_fasta_orfs, (self._h, int(stop_mask), int(start_mask), int(mode), int(strands), int(min_len), *_sel(ids), int(cap)),
                     (np.int64, np.int64, np.int64, np.int8, np.uint8), counters=(0, 0), err=("n_rows", 1))[0]

    def fasta_translate_alloc(self, seq_id, start, stop, aa64, strand=None, unknown=ord("X")):
        """(record id, start, stop) batches translated by the 64-byte table aa64 (fx_fasta_translate_alloc; strand: None or one
        0 / 1 per query) -> (uint8 amino acids, int64 offsets[n+1]) in pinned memory; an invalid query raises
        FxError(FX_ERANGE) whose .first_bad is its index."""
        seq_id, start, stop = self._i64(seq_id), self._i64(start), self._i64(stop)
        n = seq_id.size
        if start.size != n or stop.size != n or (strand is not None and len(strand) != n):
            raise ValueError("ids, starts, stops and strands differ in length")
        sd = None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)
        tab = np.frombuffer(bytes(aa64), dtype=np.uint8)
        if tab.size != 64:
            raise ValueError("the amino-acid table has %d entries, not 64" % tab.size)
        (dst, offs), _ = _call(lib().fx_fasta_translate_alloc, (self._h, n, seq_id, start, stop, sd, tab, int(unknown)), (RAW, RAW),
                               counters=(-1,), err=("first_bad", 0))
        return _ragged(dst, offs, n)

    def fastq_fetch_alloc(self, read_id, phred=0, seq_flags=0, want=("seq", "qual", "quali")):
        """Reads by id with the layout left to the library (fx_fastq_fetch_alloc) -> (seq, qual, quali, offsets), pinned."""
        read_id = self._i64(read_id)
        n = read_id.size
        w = (1 if "seq" in want else 0) | (2 if "qual" in want else 0) | (4 if "quali" in want else 0)
        ps, pq, pi, po, bad = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64(-1)
        rc = lib().fx_fastq_fetch_alloc(self._h, n, _ptr(read_id), int(phred), int(seq_flags), w, C.byref(ps), C.byref(pq),
                                        C.byref(pi), C.byref(po), C.byref(bad))
        if rc:
            _raise(rc, first_bad=int(bad.value))
        o = pinned_array(po.value, n + 2, np.int64)[:n + 1]
        tot = int(o[n])
        seq = pinned_array(ps.value, max(tot, 1))[:tot] if ps.value else None
        qual = pinned_array(pq.value, max(tot, 1))[:tot] if pq.value else None
        qi = pinned_array(pi.value, max(tot, 1), np.int8)[:tot] if pi.value else None
        return seq, qual, qi, o

    def fastq_read_stats(self, ids=None, phred=0, low_qual=20):
        """Per-read quality statistics (fx_fastq_read_stats) -> dict of pinned columns length, qsum, qmin, qmax, n_low, n_gc,
        n_other in the order of ids (None: every read); an id outside the table raises FxError(FX_ERANGE) with .first_bad."""
        cols, _ = _call(lib().fx_fastq_read_stats, (self._h, *_sel(ids), int(phred), int(low_qual)),
                        [np.int64] * 2 + [np.int16] * 2 + [np.int32] * 3, counters=(0, -1), err=("first_bad", 1))
        return dict(zip(("length", "qsum", "qmin", "qmax", "n_low", "n_gc", "n_other"), cols))

    def fastq_cycle_hist(self, cycles):
        """Per-cycle histograms (fx_fastq_cycle_hist) -> (qual int64[cycles, 256], base int64[cycles, 5], depth int64[cycles]), pinned."""
        cycles = int(cycles)
        pq, pb, pd = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().fx_fastq_cycle_hist(self._h, cycles, C.byref(pq), C.byref(pb), C.byref(pd)))
        return (pinned_array(pq.value, cycles * 256, np.int64).reshape(cycles, 256), pinned_array(pb.value, cycles * 5, np.int64).reshape(cycles, 5),
                pinned_array(pd.value, cycles, np.int64))

    def fastq_select(self, phred=0, low_qual=20, min_len=-1, max_len=-1, mean_qual=(0, 0), low_frac=(0, 0), max_other=-1):
        """Ascending ids of the reads that pass (fx_fastq_select); mean_qual / low_frac are (numerator, denominator) pairs, a
        denominator of 0 and a bound of -1 mean "not asked" -> int64 array in pinned memory."""
        return _call(lib().fx_fastq_select, (self._h, int(phred), int(low_qual), int(min_len), int(max_len), int(mean_qual[0]), int(mean_qual[1]),
                                             int(low_frac[0]), int(low_frac[1]), int(max_other)), [np.int64])[0][0]

    def fastq_trim(self, ids=None, phred=0, clip_front=0, clip_tail=0, adapter=None, min_overlap=1, err=(0, 1), front_qual=None,
                   window=None, tail_qual=None):
        """Per-read surviving interval (fx_fastq_trim) -> (start, end), int64 in pinned memory, in the order of ids (None:
        every read).  adapter: upper-case bytes of A C G T N or None; err = (num, den); window = (length, num, den) or None;
        a threshold None is a step not asked for.  An id outside the table raises FxError(FX_ERANGE) with .first_bad."""
        ad = None if adapter is None else bytes(adapter)
        w = (0, 0, 1) if window is None else window
        head = (self._h, *_sel(ids), int(phred), int(clip_front), int(clip_tail), ad, 0 if ad is None else len(ad), int(min_overlap),
                int(err[0]), int(err[1]), -1 if front_qual is None else int(front_qual), int(w[0]), int(w[1]), int(w[2]),
                -1 if tail_qual is None else int(tail_qual))
        return _call(lib().fx_fastq_trim, head, [np.int64] * 2, counters=(0, -1), err=("first_bad", 1))[0]

    def fastq_format_alloc(self, ids=None, start=None, end=None, min_len=0, level=None):
        """Four-line records of the queries cut to [start, end) (fx_fastq_format_alloc; level 0..2: fx_fastq_format_bgzf_alloc,
        see below; start = end = None: whole reads) ->
        (uint8 buffer, int64 offsets[n + 1], records kept), pinned.  A bad id or interval raises FxError(FX_ERANGE) with
        .first_bad."""
        if level is not None:                                  # -> (stream, member offsets, record offsets in the uncompressed stream, kept)
            (zdst, moff, offs), (n, kept, _, zb, nm) = _call(lib().fx_fastq_format_bgzf_alloc, (self._h, *self._fastq_queries(ids, start, end), int(min_len), int(level)),
                                                             (RAW, RAW, RAW), counters=(0, 0, -1, 0, 0), err=("first_bad", 2))
            return _bgzf_blocks(zdst, moff, zb, nm) + (pinned_array(offs, n + 1, np.int64), kept)
        (dst, offs), (n, kept, _) = _call(lib().fx_fastq_format_alloc, (self._h, *self._fastq_queries(ids, start, end), int(min_len)),
                                          (RAW, RAW), counters=(0, 0, -1), err=("first_bad", 2))
        return _ragged(dst, offs, n) + (kept,)

    def fastq_demux(self, barcodes, src, off, length, mm, margin=1, ids=None, want_order=True):
        """Barcode demultiplexing (fx_fastq_demux) -> dict of pinned columns sample, dist, second (int32, one row per query in
        the order of ids; None: every read), counts (int64[n_samples + 2]) and, with want_order, order (int64[n]) and
        bin_off (int64[n_samples + 3]).  barcodes: uint8[n_samples, sum(length)], upper-case A C G T N; src / off / length /
        mm: one entry per segment (1 or 2).  An id outside the table raises FxError(FX_ERANGE) with .first_bad."""
        bc = np.ascontiguousarray(barcodes, dtype=np.uint8)
        seg = [np.ascontiguousarray(a, dtype=np.int32) for a in (src, off, length, mm)]
        n_seg = int(seg[0].size)
        if bc.ndim != 2 or any(a.ndim != 1 or a.size != n_seg for a in seg) or n_seg not in (1, 2) or bc.shape[1] != int(seg[2].sum()):
            raise ValueError("barcodes must be n_samples rows of sum(length) letters, with one src / off / length / mm per segment")
        n_samples = int(bc.shape[0])
        cols, _ = _call(lib().fx_fastq_demux, (self._h, *_sel(ids), n_seg, *seg, bc, n_samples, int(margin), 1 if want_order else 0),
                        [np.int32] * 3 + [RAW, np.int64, RAW], counters=(0, -1), err=("first_bad", 1))
        out = dict(zip(("sample", "dist", "second"), cols[:3]))
        out["counts"] = pinned_array(cols[3], n_samples + 2, np.int64)
        if want_order:
            out["order"] = cols[4]
            out["bin_off"] = pinned_array(cols[5], n_samples + 3, np.int64)
        return out

    def fastq_pair_overlap(self, mate, ids=None, min_overlap=30, max_diff=5, err=(1, 5)):
        """The overlap of every pair (this blob: read 1, `mate`: read 2; fx_fastq_pair_overlap) -> dict of pinned columns diag,
        overlap, mismatches (int32), end1, end2 (int64) in the order of ids (None: every pair); diag is FX_PAIR_NONE where no
        diagonal is accepted.  err = (num, den).  An id outside the table raises FxError(FX_ERANGE) with .first_bad."""
        cols, _ = _call(lib().fx_fastq_pair_overlap, (self._h, mate._h, *_sel(ids), int(min_overlap), int(max_diff), int(err[0]), int(err[1])),
                        [np.int32] * 3 + [np.int64] * 2, counters=(0, -1), err=("first_bad", 1))
        return dict(zip(("diag", "overlap", "mismatches", "end1", "end2"), cols))

    def fastq_pair_merge_alloc(self, mate, diag, ids=None, min_len=0, level=None):
        """The merged records of the pairs (fx_fastq_pair_merge_alloc; level 0..2: fx_fastq_pair_merge_bgzf_alloc, see below; diag: what fastq_pair_overlap returned for the same
        ids) -> (uint8 buffer, int64 offsets[n + 1], records merged), pinned.  A bad id or diagonal raises
        FxError(FX_ERANGE) with .first_bad."""
        diag = np.ascontiguousarray(diag, dtype=np.int32)
        if level is not None:                                  # -> (stream, member offsets, record offsets in the uncompressed stream, merged)
            (zdst, moff, offs), (n, merged, _, zb, nm) = _call(lib().fx_fastq_pair_merge_bgzf_alloc,
                                                               (self._h, mate._h, *_sel(ids), diag if diag.size else None, int(min_len), int(level)),
                                                               (RAW, RAW, RAW), counters=(0, 0, -1, 0, 0), err=("first_bad", 2))
            return _bgzf_blocks(zdst, moff, zb, nm) + (pinned_array(offs, n + 1, np.int64), merged)
        (dst, offs), (n, merged, _) = _call(lib().fx_fastq_pair_merge_alloc, (self._h, mate._h, *_sel(ids), diag if diag.size else None, int(min_len)),
                                            (RAW, RAW), counters=(0, 0, -1), err=("first_bad", 2))
        return _ragged(dst, offs, n) + (merged,)

    def fasta_kmers(self, k, canonical=False, ids=None, per_record=False):
        """k-mer spectrum of the resident FASTA table (fx_fasta_kmers) -> int64[4**k], or int64[n_sel, 4**k] with per_record
        (k <= 6), in pinned memory.  ids: 0-based record ids, any order, repeats count again; None: every record.  An id
        outside the table raises FxError(FX_ERANGE) with .first_bad."""
        (a,), _ = _call(lib().fx_fasta_kmers, (self._h, int(k), FX_KMER_CANONICAL if canonical else 0, *_sel(ids), 1 if per_record else 0),
                        [(np.int64, 4 ** int(k))], counters=(0, -1), err=("first_bad", 1))
        return a if per_record else a.reshape(-1)

    def fastq_kmers(self, k, canonical=False, ids=None, start=None, end=None):
        """k-mer spectrum of the reads `ids` (None: every read) cut to [start, end) (both None: whole reads) of the resident
        FASTQ table (fx_fastq_kmers) -> int64[4**k] in pinned memory.  A bad id or interval raises FxError(FX_ERANGE) with
        .first_bad."""
        (p,), _ = _call(lib().fx_fastq_kmers, (self._h, int(k), FX_KMER_CANONICAL if canonical else 0, *self._fastq_queries(ids, start, end)),
                        [RAW], counters=(-1,), err=("first_bad", 0))
        return pinned_array(p, 4 ** int(k), np.int64)

    def _kmer_table(self, call, head, min_count, max_bytes):
        cols, (_, nw, parts, _) = _call(call, head + (int(min_count), int(max_bytes)), [np.int64] * 2, counters=(0, 0, 0, -1), err=("first_bad", 3))
        return cols + (nw, parts)

    def fasta_kmer_table(self, k, canonical=False, ids=None, min_count=1, max_bytes=0):
        """Sparse k-mer table of the resident FASTA table (fx_fasta_kmer_table), 1 <= k <= 31 -> (codes int64[n] ascending,
        counts int64[n], n_windows, n_parts), the arrays in pinned memory.  ids as for fasta_kmers; max_bytes = 0: the
        library's default budget of device working memory."""
        head = (self._h, int(k), FX_KMER_CANONICAL if canonical else 0, *_sel(ids))
        return self._kmer_table(lib().fx_fasta_kmer_table, head, min_count, max_bytes)

    def fastq_kmer_table(self, k, canonical=False, ids=None, start=None, end=None, min_count=1, max_bytes=0):
        """Sparse k-mer table of the reads `ids` cut to [start, end) (fx_fastq_kmer_table) -> what fasta_kmer_table returns."""
        head = (self._h, int(k), FX_KMER_CANONICAL if canonical else 0, *self._fastq_queries(ids, start, end))
        return self._kmer_table(lib().fx_fastq_kmer_table, head, min_count, max_bytes)

    def kmer_set(self, k, canonical, codes):
        """A device k-mer set of `codes` on this blob's device (fx_kmer_set_create) -> KmerSet; any blob of the device may use it."""
        return KmerSet(self, k, canonical, codes)

    def fasta_sketch(self, k, flags, ids=None, max_key=1, size=0, oversample=0):
        """Sketches of the selected records (fx_fasta_sketch; flags: FX_SK_CANONICAL | FX_SK_POOLED; ids: distinct ascending
        record ids, None: every record) -> (SketchObj, n_rounds)."""
        ids, n_ids = _sel(ids)
        s, nr = C.c_void_p(), C.c_int(0)
        check(lib().fx_fasta_sketch(self._h, int(k), int(flags), _ptr(ids), n_ids, int(max_key), int(size), int(oversample), C.byref(s), C.byref(nr)))
        return SketchObj(s), int(nr.value)

    def fastq_sketch(self, k, flags, ids=None, start=None, end=None, max_key=1, size=0, oversample=0):
        """The pooled sketch of the reads `ids` cut to [start, end) (fx_fastq_sketch) -> (SketchObj, n_rounds); a bad id or
        interval raises FxError(FX_ERANGE) with .first_bad."""
        ids, n_ids, start, end = self._fastq_queries(ids, start, end)
        s, nr, bad = C.c_void_p(), C.c_int(0), C.c_int64(-1)
        rc = lib().fx_fastq_sketch(self._h, int(k), int(flags), _ptr(ids), n_ids, _ptr(start), _ptr(end), int(max_key), int(size), int(oversample),
                                   C.byref(s), C.byref(nr), C.byref(bad))
        if rc:
            _raise(rc, first_bad=int(bad.value))
        return SketchObj(s), int(nr.value)

    @staticmethod
    def _kmer_hits(call, head, dtype):
        return _call(call, head, [dtype] * 2, counters=(0, -1), err=("first_bad", 1))[0]

    def _fastq_queries(self, ids, start, end):
        """The query batch of the FASTQ interval entries -> (ids, n_ids, start, end) as they go into _call."""
        start = None if start is None else self._i64(start)
        end = None if end is None else self._i64(end)
        if start is not None and start.size == 0:
            start = end = None                                 # no query, no interval
        return (*_sel(ids), start, end)

    def fastq_kmer_hits(self, kset, ids=None, start=None, end=None):
        """Per query the valid windows of seq[start:end] and how many of them are in `kset` (fx_fastq_kmer_hits) ->
        (n_windows, n_hits), int32 in pinned memory.  A bad id or interval raises FxError(FX_ERANGE) with .first_bad."""
        return self._kmer_hits(lib().fx_fastq_kmer_hits, (self._h, kset._s, *self._fastq_queries(ids, start, end)), np.int32)

    def fastq_kmer_screen(self, kset, ids=None, start=None, end=None, min_hits=1, frac=(0, 0), invert=False):
        """The ascending positions of the queries whose hits pass min_hits and the ratio frac = (num, den) (fx_fastq_kmer_screen;
        den 0: not asked) -> int64 in pinned memory."""
        head = (self._h, kset._s, *self._fastq_queries(ids, start, end), int(min_hits), int(frac[0]), int(frac[1]), 1 if invert else 0)
        return _call(lib().fx_fastq_kmer_screen, head, [np.int64], counters=(0, -1), err=("first_bad", 1))[0][0]

    def fasta_kmer_hits(self, kset, ids=None):
        """Per selected record the valid windows and the hits in `kset` (fx_fasta_kmer_hits) -> (n_windows, n_hits), int64."""
        return self._kmer_hits(lib().fx_fasta_kmer_hits, (self._h, kset._s, *_sel(ids)), np.int64)

    def fastq_dup_first(self, ids=None, start=None, end=None, revcomp=False, hash_bits=0):
        """first[q] = the smallest query position whose key seq[start:end] is a duplicate of query q's (fx_fastq_dup_first) ->
        (first int64[n] in pinned memory, n_groups, n_rounds).  hash_bits: the fingerprint bits kept (0: 64); no result but
        n_rounds depends on it.  A bad id or interval raises FxError(FX_ERANGE) with .first_bad."""
        head = (self._h, *self._fastq_queries(ids, start, end), FX_DUP_REVCOMP if revcomp else 0, int(hash_bits))
        cols, (_, groups, rounds, _) = _call(lib().fx_fastq_dup_first, head, [np.int64], counters=(0, 0, 0, -1), err=("first_bad", 3))
        return cols + (groups, rounds)

    def fastq_dedup(self, ids=None, start=None, end=None, revcomp=False, hash_bits=0, min_copies=1, max_copies=-1, want_copies=False):
        """The ascending positions of the first occurrences whose group has min_copies..max_copies members (fx_fastq_dedup;
        max_copies < 0: not asked) -> (pos int64 in pinned memory, copies int64 or None, n_groups, n_rounds)."""
        head = (self._h, *self._fastq_queries(ids, start, end), FX_DUP_REVCOMP if revcomp else 0, int(hash_bits), int(min_copies), int(max_copies))
        cols, (_, groups, rounds, _) = _call(lib().fx_fastq_dedup, head, [np.int64, np.int64 if want_copies else None],
                                             counters=(0, 0, 0, -1), err=("first_bad", 3))
        return cols + (groups, rounds)

    def fastq_fetch(self, read_id, rlen, phred=0, seq_flags=0, want=("seq", "qual", "quali")):
        read_id = self._i64(read_id)
        rlen = self._i64(rlen)
        n = read_id.size
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(rlen, out=offs[1:])
        tot = max(int(offs[-1]), 1)
        seq = np.zeros(tot, dtype=np.uint8) if "seq" in want else None
        qual = np.zeros(tot, dtype=np.uint8) if "qual" in want else None
        qi = np.zeros(tot, dtype=np.int8) if "quali" in want else None
        if n:
            check(lib().fx_fastq_fetch(self._h, FX_HOST, n, _ptr(read_id), int(phred), int(seq_flags),
                                       _ptr(seq), _ptr(qual), _ptr(qi), _ptr(offs)))
        return seq, qual, qi, offs

    def read_fetch(self, soff, qoff, rlen, phred=0, seq_flags=0, want=("seq", "qual", "quali")):
        soff, qoff, rlen = self._i64(soff), self._i64(qoff), self._i64(rlen)
        n = soff.size
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(rlen, out=offs[1:])
        tot = max(int(offs[-1]), 1)
        seq = np.zeros(tot, dtype=np.uint8) if "seq" in want else None
        qual = np.zeros(tot, dtype=np.uint8) if "qual" in want else None
        qi = np.zeros(tot, dtype=np.int8) if "quali" in want else None
        if n:
            check(lib().fx_read_fetch(self._h, FX_HOST, n, _ptr(soff), _ptr(qoff), _ptr(rlen), int(phred),
                                      int(seq_flags), _ptr(seq), _ptr(qual), _ptr(qi), _ptr(offs)))
        return seq, qual, qi, offs


def revcomp_bytes(b, mode=FX_REVERSE | FX_COMPLEMENT, device=0):
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    if a.size:
        check(lib().fx_revcomp(device, FX_HOST, a.ctypes.data, a.size, mode))
    return a.tobytes()
