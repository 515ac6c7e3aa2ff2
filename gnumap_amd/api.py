"""ctypes mirror of include/gnumap_hip.h."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

GM_INDEX_FULL_SA, GM_INDEX_BUILD, GM_INDEX_HOST_ONLY = 1, 2, 4
GM_READ_OK, GM_READ_TOO_MANY, GM_READ_NONE, GM_READ_TOO_SHORT, GM_READ_TOO_POOR = 0, 1, 2, -2, -3
GM_E_CAPACITY = -5
GM_E_BATCH_TOO_LARGE = -9
GM_ROWS_TEXT, GM_ROWS_BAM = 0, 1
GM_ROW_TAG_MD = 1                       # gm_batch_set_row_tags: NM:i and MD:Z
GM_CIGAR_GNUMAP, GM_CIGAR_FORWARD = 0, 1
GM_BGZF_LZ77 = 0x100                    # ORed into a BGZF level of 1: LZ77 matches under the Huffman code

u8p = C.POINTER(C.c_uint8)
u64 = C.c_uint64


class GnumapError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"gnumap_hip error {code}: {msg}")
        self.code = code


class gm_index_info(C.Structure):
    _fields_ = [("l_pac", u64), ("seq_len", u64), ("primary", u64), ("bwt_words", u64), ("n_sa", u64),
                ("sa_intv", C.c_uint32), ("n_seqs", C.c_uint32), ("device_id", C.c_int), ("full_sa", C.c_int), ("hbm_bytes", u64)]


class gm_track_text_stats(C.Structure):
    _fields_ = [("rows", u64), ("bytes", u64), ("slabs", u64), ("host_slabs", u64), ("launches", u64), ("kernel_ms", C.c_double)]


class gm_sam_sort_stats(C.Structure):
    _fields_ = [("rows", u64), ("text_bytes", u64), ("pieces", u64), ("piece_bytes", u64), ("add_s", C.c_double), ("sort_s", C.c_double),
                ("gather_ms", C.c_double), ("gather_bytes", u64), ("download_s", C.c_double), ("bai_ms", C.c_double), ("bai_bytes", u64),
                ("bai_chunks", u64)]


class gm_params(C.Structure):
    _fields_ = [("mer", C.c_int), ("jump", C.c_int), ("min_seed_hits", C.c_int), ("max_kmer_hits", C.c_uint32), ("max_matches", C.c_uint32),
                ("max_gap", C.c_int), ("nw", C.c_int), ("fast", C.c_int), ("unique_only", C.c_int), ("pos_strand", C.c_int), ("neg_strand", C.c_int),
                ("mode", C.c_int), ("align_score", C.c_float), ("align_is_fraction", C.c_int), ("cutoff", C.c_float),
                ("adjust", C.c_float), ("match", C.c_float), ("transition", C.c_float), ("transversion", C.c_float), ("gap", C.c_float),
                ("S", (C.c_float * 4) * 256), ("bin_size", C.c_int), ("print_all_sam", C.c_int), ("illumina", C.c_int), ("finalized", C.c_int)]


class gm_reads(C.Structure):
    _fields_ = [("n", C.c_uint32), ("stride", C.c_uint32), ("bases", C.c_void_p), ("quals", C.c_void_p), ("len", C.c_void_p)]


class gm_pos(C.Structure):
    _fields_ = [("pos", u64), ("strand", C.c_uint8)]


class gm_match(C.Structure):
    _fields_ = [("read", C.c_uint32), ("score", C.c_float), ("first_pos", u64), ("first_strand", C.c_uint8),
                ("pos_begin", C.c_uint32), ("pos_end", C.c_uint32)]


class gm_hits(C.Structure):
    _fields_ = [("n", C.c_uint32), ("status", C.c_void_p), ("self_score", C.c_void_p), ("top_score", C.c_void_p), ("denominator", C.c_void_p),
                ("match_begin", C.c_void_p), ("matches", C.c_void_p), ("matches_cap", u64), ("positions", C.c_void_p), ("positions_cap", u64),
                ("stamp", u64)]


class gm_sam_rec(C.Structure):
    _fields_ = [("read", C.c_uint32), ("pos", u64), ("contig", C.c_uint32), ("chr_pos", u64), ("strand", C.c_uint8), ("mapq", C.c_int32),
                ("a_score", C.c_float), ("post_prob", C.c_float), ("sim_matches", C.c_int32), ("cigar_off", C.c_uint32)]


class gm_sam_out(C.Structure):
    _fields_ = [("recs", C.c_void_p), ("recs_cap", u64), ("n_recs", u64), ("cigar_pool", C.c_void_p), ("cigar_cap", u64), ("cigar_len", u64)]


class gm_read_text(C.Structure):
    _fields_ = [("names", C.c_void_p), ("name_off", C.c_void_p), ("qual_tail", C.c_void_p), ("qual_tail_off", C.c_void_p)]


class gm_sam_text(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_cap", u64), ("text_len", u64), ("n_recs", u64), ("row_off", C.c_void_p), ("row_cap", u64)]


class gm_bam_out(C.Structure):
    _fields_ = [("data", C.c_void_p), ("cap", u64), ("len", u64), ("raw_len", u64), ("n_recs", u64), ("level", C.c_int)]


class gm_text_info(C.Structure):
    _fields_ = [("n", C.c_uint32), ("max_len", C.c_uint32), ("stride", C.c_uint32), ("status", C.c_int32), ("bad_at", u64)]


class gm_text_rec(C.Structure):
    _fields_ = [("name_off", C.c_uint32), ("seq_off", C.c_uint32), ("qual_off", C.c_uint32), ("name_len", C.c_uint32), ("seq_len", C.c_uint32),
                ("qual_len", C.c_uint32)]


GM_TEXT_OK, GM_TEXT_MALFORMED, GM_TEXT_TOO_LONG = 0, 1, 2
TEXT_REC_DTYPE = np.dtype([("name_off", "<u4"), ("seq_off", "<u4"), ("qual_off", "<u4"), ("name_len", "<u4"), ("seq_len", "<u4"), ("qual_len", "<u4")])


class gm_counters(C.Structure):
    _fields_ = [(n, u64) for n in ("reads", "kmers_searched", "occ_calls", "occ_blocks", "seeds_used", "sa_hits", "lf_steps", "candidates",
                                   "nw_cells", "accepted", "vote_retries", "table_lookups")]

GM_K_COUNT = 9


RAW_HIT_DTYPE = np.dtype([("read", "<u4"), ("pos", "<u4"), ("score", "<f4"), ("step", "<u2"), ("strand", "u1"), ("pad", "u1")])
MATCH_DTYPE = np.dtype([("read", "<u4"), ("score", "<f4"), ("first_pos", "<u8"), ("first_strand", "u1"), ("pos_begin", "<u4"), ("pos_end", "<u4")],
                       align=True)
POS_DTYPE = np.dtype([("pos", "<u8"), ("strand", "u1")], align=True)
SAM_DTYPE = np.dtype([("read", "<u4"), ("pos", "<u8"), ("contig", "<u4"), ("chr_pos", "<u8"), ("strand", "u1"), ("mapq", "<i4"),
                      ("a_score", "<f4"), ("post_prob", "<f4"), ("sim_matches", "<i4"), ("cigar_off", "<u4")], align=True)
MATE_ROW_DTYPE = np.dtype([("flag", "<u4"), ("rnext", "<i4"), ("pnext", "<u4"), ("tlen", "<i4")])     # gm_mate_row
MATE_STATS = ("pairs", "both_mapped", "proper", "one_mapped", "none_mapped")                          # gm_mate_stats, in its order
ROW_UNMAPPED = 1 << 63                                                                                # a row source entry that names a read without a record
SNP_DTYPE = np.dtype([("pos", "<u8"), ("contig", "<u4"), ("chr_pos", "<u8"), ("total", "<f4"), ("nuc", "<f4", (5,)), ("p_val", "<f8"), ("ref", "u1"),
                      ("alt1", "u1"), ("alt2", "u1"), ("diploid", "u1")], align=True)

# every symbol include/gnumap_hip.h declares
EXPORTS = ["gm_last_error", "gm_version", "gm_set_option", "gm_selftest_pass_parallel", "gm_index_build", "gm_index_build_on", "gm_index_open", "gm_index_close", "gm_index_prepare", "gm_index_get_info", "gm_index_contig_name",
           "gm_index_contig_offset", "gm_index_window", "gm_params_default", "gm_params_finalize", "gm_params_load_subst", "gm_batch_create", "gm_batch_destroy",
           "gm_batch_upload", "gm_map_batch_device", "gm_batch_counters", "gm_batch_path", "gm_batch_pair_flagged", "gm_batch_set_profiling", "gm_batch_kernel_times", "gm_kernel_name",
           "gm_batch_raw_hits", "gm_stream_create", "gm_stream_destroy", "gm_host_alloc", "gm_host_free", "gm_map_batch", "gm_output_batch",
           "gm_output_batch_text", "gm_map_batch_enqueue", "gm_output_batch_enqueue", "gm_batch_wait", "gm_dev_fmt_g6", "gm_dev_fmt_e2", "gm_dev_scan_u32",
           "gm_dev_mate_resolve", "gm_dev_sa_interval", "gm_dev_locate", "gm_dev_nw_score", "gm_dev_traceback", "gm_dev_prep", "gm_dev_pair_hmm", "gm_coverage_reset", "gm_coverage_bins",
           "gm_coverage_device_ptr", "gm_coverage_add", "gm_coverage_download", "gm_coverage_allreduce", "gm_coverage_write_sgr", "gm_coverage_enable_nuc", "gm_coverage_nuc_device_ptr",
           "gm_coverage_download_nuc", "gm_coverage_write_gmp", "gm_snp_calls", "gm_dev_snp_stat", "gm_coverage_write_gmp_calls",
           "gm_coverage_write_sgr_device", "gm_coverage_write_gmp_device", "gm_coverage_text", "gm_coverage_text_stats",
           "gm_coverage_write_gmp_calls_device", "gm_coverage_calls_text", "gm_coverage_write_vcf",
           "gm_batch_set_adaptor", "gm_batch_trimmed_len", "gm_batch_adaptor_time", "gm_dev_adaptor_trim",
           "gm_batch_set_read_format", "gm_index_set_probe_format", "gm_batch_set_unmapped_rows", "gm_batch_unmapped_rows",
           "gm_batch_set_row_tags", "gm_batch_set_cigar_order", "gm_batch_set_mates", "gm_batch_mate_rows", "gm_batch_mate_stats",
           "gm_batch_upload_text", "gm_map_batch_text", "gm_output_batch_text_resident", "gm_dev_fastq_rows", "gm_dev_fastq_tile_bytes",
           "gm_sam_sorter_create", "gm_sam_sorter_destroy", "gm_output_batch_sorted", "gm_output_batch_sorted_resident", "gm_sam_sorter_finish",
           "gm_sam_sorter_read", "gm_sam_sorter_stats", "gm_sam_sorter_add_rows",
           "gm_bam_header", "gm_bgzf_compress", "gm_bgzf_eof", "gm_output_batch_bam", "gm_output_batch_bam_resident", "gm_sam_sorter_set_rows",
           "gm_sam_sorter_read_bgzf", "gm_batch_bam_times", "gm_sam_sorter_index_begin", "gm_sam_sorter_bai"]


def library_path():
    return os.path.join(HERE, "libgnumap_hip.so")


def load_library():
    """Load the in-tree libgnumap_hip.so.  Fails loudly when it has not been built (no silent fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise GnumapError(-3, f"{path} is missing: build it with `make -C gnumap_amd` (or __graft_entry__.build())")
    L = C.CDLL(path)
    L.gm_last_error.restype = C.c_char_p
    L.gm_version.restype = C.c_char_p
    L.gm_set_option.argtypes = [C.c_char_p, C.c_char_p]
    L.gm_index_build.argtypes = [C.c_char_p]
    L.gm_index_build_on.argtypes = [C.c_char_p, C.c_int, C.c_int]
    L.gm_index_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.gm_index_close.argtypes = [C.c_void_p]; L.gm_index_close.restype = None
    L.gm_index_prepare.argtypes = [C.c_void_p, C.POINTER(gm_params)]
    L.gm_index_get_info.argtypes = [C.c_void_p, C.POINTER(gm_index_info)]
    L.gm_index_contig_name.argtypes = [C.c_void_p, C.c_uint32]; L.gm_index_contig_name.restype = C.c_char_p
    L.gm_index_contig_offset.argtypes = [C.c_void_p, C.c_uint32]; L.gm_index_contig_offset.restype = u64
    L.gm_index_window.argtypes = [C.c_void_p, u64, C.c_uint32, C.c_char_p]
    L.gm_params_default.argtypes = [C.POINTER(gm_params)]; L.gm_params_default.restype = None
    L.gm_params_finalize.argtypes = [C.POINTER(gm_params)]
    L.gm_params_load_subst.argtypes = [C.POINTER(gm_params), C.c_char_p]
    L.gm_batch_create.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.gm_batch_destroy.argtypes = [C.c_void_p]; L.gm_batch_destroy.restype = None
    L.gm_batch_upload.argtypes = [C.c_void_p, C.POINTER(gm_params), C.POINTER(gm_reads), C.c_void_p]
    L.gm_map_batch_device.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.c_void_p]
    L.gm_batch_counters.argtypes = [C.c_void_p, C.POINTER(gm_counters)]
    L.gm_batch_path.argtypes = [C.c_void_p]; L.gm_batch_path.restype = C.c_char_p
    L.gm_batch_pair_flagged.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.gm_map_batch_enqueue.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_reads), C.POINTER(gm_hits), C.c_void_p]
    L.gm_output_batch_enqueue.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_reads), C.POINTER(gm_hits), C.POINTER(gm_sam_out), C.c_void_p]
    L.gm_batch_wait.argtypes = [C.c_void_p]
    L.gm_batch_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.gm_batch_kernel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gm_kernel_name.argtypes = [C.c_int]; L.gm_kernel_name.restype = C.c_char_p
    L.gm_batch_raw_hits.argtypes = [C.c_void_p, C.c_void_p, u64, C.POINTER(u64), C.c_void_p, C.c_void_p, C.c_void_p]
    L.gm_stream_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.gm_stream_destroy.argtypes = [C.c_void_p, C.c_void_p]; L.gm_stream_destroy.restype = None
    L.gm_host_alloc.argtypes = [C.c_size_t]; L.gm_host_alloc.restype = C.c_void_p
    L.gm_host_free.argtypes = [C.c_void_p]; L.gm_host_free.restype = None
    L.gm_map_batch.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_reads), C.POINTER(gm_hits), C.c_void_p]
    L.gm_output_batch.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_reads), C.POINTER(gm_hits), C.POINTER(gm_sam_out), C.c_void_p]
    L.gm_output_batch_text.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_reads), C.POINTER(gm_read_text), C.POINTER(gm_hits),
                                       C.POINTER(gm_sam_text), C.c_void_p]
    L.gm_dev_fmt_g6.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.gm_dev_fmt_e2.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.gm_dev_scan_u32.argtypes = [C.c_void_p, C.c_void_p, u64, C.c_void_p]
    L.gm_dev_mate_resolve.argtypes = [C.c_void_p, C.c_void_p, u64, C.c_void_p, u64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, u64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gm_dev_sa_interval.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.gm_dev_locate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]
    L.gm_dev_nw_score.argtypes = [C.c_void_p, C.POINTER(gm_params), C.POINTER(gm_reads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.gm_dev_traceback.argtypes = [C.c_void_p, C.POINTER(gm_params), C.POINTER(gm_reads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                   C.c_void_p, C.c_uint32, C.c_void_p]
    L.gm_dev_prep.argtypes = [C.c_void_p, C.POINTER(gm_params), C.POINTER(gm_reads), C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.gm_dev_pair_hmm.argtypes = [C.c_void_p, C.POINTER(gm_params), C.POINTER(gm_reads), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.gm_coverage_reset.argtypes = [C.c_void_p, C.c_uint32]
    L.gm_coverage_bins.argtypes = [C.c_void_p]; L.gm_coverage_bins.restype = u64
    L.gm_coverage_device_ptr.argtypes = [C.c_void_p]; L.gm_coverage_device_ptr.restype = C.c_void_p
    L.gm_coverage_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.gm_coverage_download.argtypes = [C.c_void_p, C.c_void_p]
    L.gm_coverage_allreduce.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.gm_coverage_write_sgr.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    L.gm_coverage_enable_nuc.argtypes = [C.c_void_p]
    L.gm_coverage_nuc_device_ptr.argtypes = [C.c_void_p]; L.gm_coverage_nuc_device_ptr.restype = C.c_void_p
    L.gm_coverage_download_nuc.argtypes = [C.c_void_p, C.c_void_p]
    L.gm_coverage_write_gmp.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.c_void_p, C.c_char_p, C.c_int]
    L.gm_snp_calls.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p, u64, C.POINTER(u64), C.c_void_p]
    L.gm_dev_snp_stat.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.gm_coverage_write_gmp_calls.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_char_p, C.c_int]
    L.gm_coverage_write_sgr_device.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.gm_coverage_write_gmp_device.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_char_p, C.c_int]
    L.gm_coverage_text.argtypes = [C.c_void_p, C.POINTER(gm_params), u64, u64, C.c_void_p, u64, C.POINTER(u64)]
    L.gm_coverage_text_stats.argtypes = [C.c_void_p, C.POINTER(gm_track_text_stats)]
    L.gm_coverage_write_gmp_calls_device.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_char_p, C.c_int]
    L.gm_coverage_calls_text.argtypes = [C.c_void_p, C.c_float, C.c_int, u64, u64, C.c_void_p, u64, C.POINTER(u64)]
    L.gm_coverage_write_vcf.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_char_p, C.c_int]
    L.gm_batch_set_adaptor.argtypes = [C.c_void_p, C.c_char_p]
    L.gm_batch_trimmed_len.argtypes = [C.c_void_p, C.c_void_p]
    L.gm_batch_adaptor_time.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(u64)]
    L.gm_dev_adaptor_trim.argtypes = [C.c_void_p, C.POINTER(gm_reads), C.c_char_p, C.c_void_p]
    L.gm_batch_set_read_format.argtypes = [C.c_void_p, C.c_int]
    L.gm_index_set_probe_format.argtypes = [C.c_void_p, C.c_int]
    L.gm_batch_upload_text.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, u64, C.POINTER(gm_text_info), C.c_void_p, u64, C.c_void_p]
    L.gm_map_batch_text.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_hits), C.c_void_p]
    L.gm_output_batch_text_resident.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_hits), C.POINTER(gm_sam_text), C.c_void_p]
    L.gm_dev_fastq_rows.argtypes = [C.c_void_p, C.c_void_p, u64, C.POINTER(gm_text_info), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u64]
    L.gm_dev_fastq_tile_bytes.argtypes = []; L.gm_dev_fastq_tile_bytes.restype = C.c_uint32
    L.gm_sam_sorter_create.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    L.gm_sam_sorter_destroy.argtypes = [C.c_void_p]; L.gm_sam_sorter_destroy.restype = None
    L.gm_output_batch_sorted.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_reads), C.POINTER(gm_read_text), C.POINTER(gm_hits),
                                         C.c_void_p, u64, C.c_void_p]
    L.gm_output_batch_sorted_resident.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_hits), C.c_void_p, u64, C.c_void_p]
    L.gm_sam_sorter_finish.argtypes = [C.c_void_p, C.POINTER(u64), C.POINTER(u64), C.c_void_p]
    L.gm_sam_sorter_read.argtypes = [C.c_void_p, C.c_void_p, u64, C.POINTER(u64), C.c_void_p]
    L.gm_sam_sorter_add_rows.argtypes = [C.c_void_p, u64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u64, C.c_void_p]
    L.gm_sam_sorter_stats.argtypes = [C.c_void_p, C.POINTER(gm_sam_sort_stats)]
    L.gm_bam_header.argtypes = [C.c_void_p, C.c_char_p, u64, C.c_void_p, u64, C.POINTER(u64)]
    L.gm_bgzf_compress.argtypes = [C.c_void_p, C.c_void_p, u64, C.c_int, C.c_void_p, u64, C.POINTER(u64), C.c_void_p]
    L.gm_bgzf_eof.argtypes = [C.c_void_p]
    L.gm_output_batch_bam.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_reads), C.POINTER(gm_read_text), C.POINTER(gm_hits),
                                      C.POINTER(gm_bam_out), C.c_void_p]
    L.gm_output_batch_bam_resident.argtypes = [C.c_void_p, C.POINTER(gm_params), C.c_void_p, C.POINTER(gm_hits), C.POINTER(gm_bam_out), C.c_void_p]
    L.gm_sam_sorter_set_rows.argtypes = [C.c_void_p, C.c_int]
    L.gm_batch_bam_times.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.gm_sam_sorter_read_bgzf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, u64, C.POINTER(u64), C.c_void_p]
    L.gm_sam_sorter_index_begin.argtypes = [C.c_void_p, u64]
    L.gm_sam_sorter_bai.argtypes = [C.c_void_p, C.c_void_p, u64, C.POINTER(u64), C.c_void_p]
    L.gm_batch_set_unmapped_rows.argtypes = [C.c_void_p, C.c_int]
    L.gm_batch_unmapped_rows.argtypes = [C.c_void_p, C.POINTER(u64)]
    L.gm_batch_set_row_tags.argtypes = [C.c_void_p, C.c_uint32]
    L.gm_batch_set_mates.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32]
    L.gm_batch_mate_rows.argtypes = [C.c_void_p, C.c_void_p, u64, C.POINTER(u64)]
    L.gm_batch_mate_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.gm_batch_set_cigar_order.argtypes = [C.c_void_p, C.c_int]
    _LIB = L
    return L


def lib():
    return load_library()


def _chk(rc):
    if rc != 0:
        raise GnumapError(rc, lib().gm_last_error().decode())


def version():
    return lib().gm_version().decode()


def set_option(name, value):
    """gm_set_option: override a GM_* run-time switch for the calls that follow (None: back to the environment)"""
    _chk(lib().gm_set_option(name.encode(), None if value is None else str(value).encode()))


GM_BUILD_AUTO, GM_BUILD_HOST, GM_BUILD_DEVICE = 0, 1, 2


def index_build(fasta, where=GM_BUILD_AUTO, device=0):
    """write <fasta>.gnumap.{pac,ann,amb,bwt,sa}; the suffix-array stage runs on the MI355X when there is one (same bytes)"""
    _chk(lib().gm_index_build_on(os.fsencode(fasta), where, device))


class Params:
    """gm_params with the reference's defaults (inc/const_define.h); keyword overrides, then finalize."""

    def __init__(self, **kw):
        self.c = gm_params()
        lib().gm_params_default(C.byref(self.c))
        for k, v in kw.items():
            if not hasattr(self.c, k):
                raise AttributeError(k)
            setattr(self.c, k, v)
        _chk(lib().gm_params_finalize(C.byref(self.c)))

    def load_subst(self, path):
        """-S / --subst_file: overwrite the lowercase rows of the score table from a 5 x 4 file (readPWM, Driver.cpp:768-859)"""
        _chk(lib().gm_params_load_subst(C.byref(self.c), os.fsencode(path)))
        return self

    def __getattr__(self, k):
        return getattr(self.c, k)


def pack_reads(seqs, quals=None, stride=None):
    """list of bytes -> (bases[n,stride] u8, quals[n,stride] u8, len[n] u16); quals=None (FASTA reads): the second array is None"""
    n = len(seqs)
    mx = max([len(s) for s in seqs] + [1])
    stride = stride or ((mx + 7) // 8) * 8
    B = np.zeros((n, stride), np.uint8); Q = None if quals is None else np.zeros((n, stride), np.uint8); Ln = np.zeros(n, np.uint16)
    for i, s in enumerate(seqs):
        B[i, :len(s)] = np.frombuffer(s, np.uint8); Ln[i] = len(s)
        if quals is not None:
            Q[i, :len(s)] = np.frombuffer(quals[i][:len(s)], np.uint8)
    return B, Q, Ln


def _reads_struct(B, Q, Ln):
    r = gm_reads()
    r.n = B.shape[0]; r.stride = B.shape[1] if B.ndim == 2 else 0
    r.bases = B.ctypes.data; r.quals = None if Q is None else Q.ctypes.data; r.len = Ln.ctypes.data
    return r


GM_READS_FASTQ, GM_READS_FASTA = 0, 1


class Index:
    def __init__(self, fasta, device=0, flags=GM_INDEX_FULL_SA):
        self.h = C.c_void_p()
        _chk(lib().gm_index_open(os.fsencode(fasta), device, flags, C.byref(self.h)))
        self.info = gm_index_info()
        _chk(lib().gm_index_get_info(self.h, C.byref(self.info)))

    def close(self):
        if self.h:
            lib().gm_index_close(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, params):
        """build the k-mer tables / records for these parameters now (gm_index_prepare) instead of inside the first map call"""
        _chk(lib().gm_index_prepare(self.h, C.byref(params.c)))

    def contigs(self):
        return [(lib().gm_index_contig_name(self.h, i).decode(), lib().gm_index_contig_offset(self.h, i)) for i in range(self.info.n_seqs)]

    def window(self, begin, L):
        buf = C.create_string_buffer(L + 1)
        lib().gm_index_window(self.h, begin, L, buf)
        return buf.value

    # ---- unit-level device entry points ----
    def dev_sa_interval(self, kmers):
        m = len(kmers[0]); n = len(kmers)
        flat = b"".join(kmers)
        s = np.zeros(n, np.uint64); e = np.zeros(n, np.uint64)
        _chk(lib().gm_dev_sa_interval(self.h, flat, n, m, s.ctypes.data, e.ctypes.data))
        return s, e

    def dev_locate(self, ranks, use_full_sa):
        ranks = np.ascontiguousarray(ranks, np.uint64); out = np.zeros(len(ranks), np.uint64)
        _chk(lib().gm_dev_locate(self.h, ranks.ctypes.data, len(ranks), int(use_full_sa), out.ctypes.data))
        return out

    def _probe(self, fasta, call):
        """run a unit probe with its gm_reads read as FASTA (Q is then not read) or FASTQ; the index goes back to FASTQ probes"""
        _chk(lib().gm_index_set_probe_format(self.h, GM_READS_FASTA if fasta else GM_READS_FASTQ))
        try:
            _chk(call())
        finally:
            lib().gm_index_set_probe_format(self.h, GM_READS_FASTQ)

    def dev_nw_score(self, params, B, Q, Ln, read_idx, strand, pos, fasta=False):
        r = _reads_struct(B, Q, Ln)
        read_idx = np.ascontiguousarray(read_idx, np.uint32); strand = np.ascontiguousarray(strand, np.uint8); pos = np.ascontiguousarray(pos, np.uint64)
        n = len(read_idx); score = np.zeros(n, np.float32); valid = np.zeros(n, np.uint8)
        self._probe(fasta, lambda: lib().gm_dev_nw_score(self.h, C.byref(params.c), C.byref(r), read_idx.ctypes.data, strand.ctypes.data, pos.ctypes.data, n,
                                                         score.ctypes.data, valid.ctypes.data))
        return score, valid

    def dev_traceback(self, params, B, Q, Ln, read_idx, strand, pos, fasta=False):
        r = _reads_struct(B, Q, Ln)
        read_idx = np.ascontiguousarray(read_idx, np.uint32); strand = np.ascontiguousarray(strand, np.uint8); pos = np.ascontiguousarray(pos, np.uint64)
        n = len(read_idx); stride = 2 * B.shape[1] + 16
        ops = np.zeros((n, stride), np.uint8); ln = np.zeros(n, np.uint16)
        self._probe(fasta, lambda: lib().gm_dev_traceback(self.h, C.byref(params.c), C.byref(r), read_idx.ctypes.data, strand.ctypes.data, pos.ctypes.data, n,
                                                          ops.ctypes.data, stride, ln.ctypes.data))
        return [ops[i, :ln[i]].tobytes() for i in range(n)]

    def dev_prep(self, params, B, Q, Ln, first_row=0, exact=False, fasta=False):
        """gm_dev_prep: the prep kernel alone on rows first_row .. n - 1 (a sub-batch view): dict(status, self_score, min_score,
        pack [n, pack_words], bad_qual, high_qual, qual_lo, qual_hi).  exact: rows in allocations of exactly n x stride bytes"""
        r = _reads_struct(B, Q, Ln)
        n = B.shape[0]
        status = np.zeros(n, np.int8); self_score = np.zeros(n, np.float32); min_score = np.zeros(n, np.float64)
        pw = C.c_uint32(); work = np.zeros(4, np.uint64)
        flat = np.zeros(n * (2 * ((B.shape[1] + 15) // 16) + 16), np.uint32)            # (room for any row layout; cut to pack_words below)
        self._probe(fasta, lambda: lib().gm_dev_prep(self.h, C.byref(params.c), C.byref(r), first_row, int(exact), status.ctypes.data, self_score.ctypes.data,
                                                     min_score.ctypes.data, flat.ctypes.data, C.byref(pw), work.ctypes.data))
        assert n * pw.value <= flat.size
        return dict(status=status, self_score=self_score, min_score=min_score, pack=flat[:n * pw.value].reshape(n, pw.value).copy(),
                    bad_qual=int(work[0]), high_qual=int(work[1]), qual_lo=int(work[2]), qual_hi=int(work[3]))

    def dev_pair_hmm(self, params, B, Q, Ln, read_idx, strand, pos):
        """bin_seq::pairHMM of read read_idx[k] (oriented by strand[k]) against the window at pos[k]: [n][stride][5] floats"""
        r = _reads_struct(B, Q, Ln)
        read_idx = np.ascontiguousarray(read_idx, np.uint32); strand = np.ascontiguousarray(strand, np.uint8); pos = np.ascontiguousarray(pos, np.uint64)
        out = np.zeros((len(read_idx), B.shape[1], 5), np.float32)
        _chk(lib().gm_dev_pair_hmm(self.h, C.byref(params.c), C.byref(r), read_idx.ctypes.data, strand.ctypes.data, pos.ctypes.data, len(read_idx), out.ctypes.data))
        return out

    def adaptor_trim(self, B, Ln, adaptor):
        """gm_dev_adaptor_trim: the length every read of B[n, stride] keeps with -A `adaptor` (SeqReader::FixReads2), uint16[n]"""
        B = np.ascontiguousarray(B, np.uint8); Ln = np.ascontiguousarray(Ln, np.uint16)
        r = _reads_struct(B, B, Ln)
        out = np.zeros(len(Ln), np.uint16)
        _chk(lib().gm_dev_adaptor_trim(self.h, C.byref(r), None if adaptor is None else bytes(adaptor), out.ctypes.data))
        return out

    def dev_fastq_rows(self, text):
        """gm_dev_fastq_rows: FASTQ text cut into rows on the device.  dict(n, max_len, stride, status, bad_at, recs[n] TEXT_REC_DTYPE,
        bases[n, stride], quals[n, stride], len[n]): the block in front of the first record that ends it"""
        text = bytes(text)
        buf = np.frombuffer(text + b"\0", np.uint8)
        info = gm_text_info()
        rc = lib().gm_dev_fastq_rows(self.h, buf.ctypes.data, len(text), C.byref(info), None, None, None, None, 0)      # sizes the buffers
        if rc != GM_E_CAPACITY:
            _chk(rc)
        n, stride = int(info.n), int(info.stride)
        recs = np.zeros(n, TEXT_REC_DTYPE); B = np.zeros((n, stride), np.uint8); Q = np.zeros((n, stride), np.uint8); Ln = np.zeros(n, np.uint16)
        if n:
            _chk(lib().gm_dev_fastq_rows(self.h, buf.ctypes.data, len(text), C.byref(info), recs.ctypes.data, B.ctypes.data, Q.ctypes.data, Ln.ctypes.data, n))
        return dict(n=n, max_len=int(info.max_len), stride=stride, status=int(info.status), bad_at=int(info.bad_at), recs=recs, bases=B, quals=Q, len=Ln)

    def bam_header(self, sam_header=b""):
        """gm_bam_header: the uncompressed bytes that open a BAM file with these header lines and this index's contigs (no device needed)"""
        text = bytes(sam_header); need = u64()
        rc = lib().gm_bam_header(self.h, text, len(text), None, 0, C.byref(need))
        if rc != GM_E_CAPACITY:
            _chk(rc)
        buf = np.zeros(max(int(need.value), 1), np.uint8)
        _chk(lib().gm_bam_header(self.h, text, len(text), buf.ctypes.data, int(need.value), C.byref(need)))
        return buf[:need.value].tobytes()

    def bgzf_compress(self, data, level=1, cap=None, stream=None, lz77=False):
        """gm_bgzf_compress: whole BGZF blocks around `data`, deflated on the device.  lz77: level | GM_BGZF_LZ77, LZ77 matches under the
        Huffman code of level 1.  cap: the output buffer's size (None: the worst case);
        GnumapError with code GM_E_CAPACITY and .needed = the size when the blocks exceed it"""
        src = np.frombuffer(bytes(data) + b"\0", np.uint8)
        n = len(src) - 1
        cap = n + 31 * ((n + 65279) // 65280) if cap is None else int(cap)
        out = np.zeros(cap + 64, np.uint8); got = u64()
        rc = lib().gm_bgzf_compress(self.h, src.ctypes.data, n, _bgzf_level(level, lz77), out.ctypes.data, cap, C.byref(got), stream)
        if rc == GM_E_CAPACITY:
            e = GnumapError(rc, lib().gm_last_error().decode())
            e.needed = int(got.value); e.buffer = out
            raise e
        _chk(rc)
        return out[:got.value].tobytes()

    def dev_fmt_g6(self, values):
        """gm_dev_fmt_g6: printf("%g") of every value as the device prints XA / XP; a list of bytes (b"" = outside the domain)"""
        v = np.ascontiguousarray(values, np.float64); n = len(v)
        out = np.zeros((n, 16), np.uint8); ln = np.zeros(n, np.uint8)
        _chk(lib().gm_dev_fmt_g6(self.h, v.ctypes.data, n, out.ctypes.data, ln.ctypes.data))
        raw = out.tobytes()
        return [raw[16 * i:16 * i + int(ln[i])] for i in range(n)]

    def dev_fmt_e2(self, values):
        """gm_dev_fmt_e2: printf("%.2e") of every value as the device prints the ninth .gmp column's p-value; b"" = outside the domain"""
        v = np.ascontiguousarray(values, np.float64); n = len(v)
        out = np.zeros((n, 16), np.uint8); ln = np.zeros(n, np.uint8)
        _chk(lib().gm_dev_fmt_e2(self.h, v.ctypes.data, n, out.ctypes.data, ln.ctypes.data))
        raw = out.tobytes()
        return [raw[16 * i:16 * i + int(ln[i])] for i in range(n)]

    def dev_scan_u32(self, values):
        """gm_dev_scan_u32: the exclusive 64-bit scan of uint32 values as the map and output steps compute their offsets; n + 1 uint64"""
        v = np.ascontiguousarray(values, np.uint32); n = len(v)
        out = np.zeros(n + 1, np.uint64)
        _chk(lib().gm_dev_scan_u32(self.h, v.ctypes.data, n, out.ctypes.data))
        return out

    def dev_mate_resolve(self, recs, pool, n_reads, min_insert, max_insert, row_src=None):
        """gm_dev_mate_resolve: the mate kernels of set_mates on records of the caller's.  recs: SAM_DTYPE in record order, pool: the
        bytes their cigar_off point into (NUL-terminated strings), row_src: None (one row per record) or uint64 entries, a record
        index or ROW_UNMAPPED | read.  dict(span uint32[n_recs], prim uint64[n_reads] (~0: none), proper uint8[n_reads / 2],
        stats dict, rows MATE_ROW_DTYPE[n_rows])"""
        recs = np.ascontiguousarray(recs, SAM_DTYPE); n = len(recs)
        pool = np.frombuffer(bytes(pool), np.uint8)
        src = None if row_src is None else np.ascontiguousarray(row_src, np.uint64)
        n_rows = n if src is None else len(src)
        span = np.zeros(max(n, 1), np.uint32); prim = np.zeros(max(int(n_reads), 1), np.uint64); proper = np.zeros(max(int(n_reads) // 2, 1), np.uint8)
        st = np.zeros(5, np.uint64); rows = np.zeros(max(n_rows, 1), MATE_ROW_DTYPE)
        _chk(lib().gm_dev_mate_resolve(self.h, recs.ctypes.data, n, pool.ctypes.data if len(pool) else None, len(pool), int(n_reads), int(min_insert), int(max_insert),
                                       None if src is None else src.ctypes.data, n_rows, span.ctypes.data, prim.ctypes.data, proper.ctypes.data,
                                       st.ctypes.data, rows.ctypes.data))
        return dict(span=span[:n], prim=prim[:int(n_reads)], proper=proper[:int(n_reads) // 2], stats={k: int(x) for k, x in zip(MATE_STATS, st)}, rows=rows[:n_rows])

    # ---- coverage ----
    def coverage_reset(self, bin_size):
        _chk(lib().gm_coverage_reset(self.h, bin_size))

    def coverage_bins(self):
        return lib().gm_coverage_bins(self.h)

    def coverage_device_ptr(self):
        return lib().gm_coverage_device_ptr(self.h)

    def coverage_enable_nuc(self):
        """-b / -d: the five per-nucleotide arrays reads[A,C,G,T,N][loc] in HBM (call after coverage_reset)"""
        _chk(lib().gm_coverage_enable_nuc(self.h))

    def coverage_nuc_device_ptr(self):
        return lib().gm_coverage_nuc_device_ptr(self.h)

    def coverage_add(self, pos, span, w, stream=None):
        """gm_coverage_add: amount_genome[(pos+t)/bin] += w for t < span (GenomeBwt::AddScore)"""
        pos = np.ascontiguousarray(pos, np.uint64); span = np.ascontiguousarray(span, np.uint32); w = np.ascontiguousarray(w, np.float32)
        _chk(lib().gm_coverage_add(self.h, pos.ctypes.data, span.ctypes.data, w.ctypes.data, len(pos), stream))

    def coverage_download(self):
        out = np.zeros(self.coverage_bins(), np.float32)
        _chk(lib().gm_coverage_download(self.h, out.ctypes.data))
        return out

    def coverage_download_nuc(self):
        """the five per-nucleotide tracks (a, c, g, t, n), [5 * bins]"""
        out = np.zeros(5 * self.coverage_bins(), np.float32)
        _chk(lib().gm_coverage_download_nuc(self.h, out.ctypes.data))
        return out

    def coverage_write_sgr(self, bins, path):
        bins = np.ascontiguousarray(bins, np.float32)
        _chk(lib().gm_coverage_write_sgr(self.h, bins.ctypes.data, os.fsencode(path), 0))

    # ---- SNP calls (--snp): PrintSNPCall over the tracks in HBM ----
    def snp_calls(self, pval=0.001, monop=False):
        """gm_snp_calls: the rows the reference marks 'Y' (p below --snp_pval), ascending position, as SNP_DTYPE records"""
        cap = 4096
        while True:
            out = np.zeros(cap, SNP_DTYPE); got = u64()
            rc = lib().gm_snp_calls(self.h, pval, int(monop), out.ctypes.data, cap, C.byref(got), None)
            if rc == GM_E_CAPACITY:
                cap = int(got.value)
                continue
            _chk(rc)
            return out[:got.value]

    def dev_snp_stat(self, counts, monop=False):
        """is_snp on [n, 5] float counts: (p-value f8, first maximum i1, second maximum i1 or -1, diploid u1)"""
        counts = np.ascontiguousarray(counts, np.float32).reshape(-1, 5)
        n = len(counts)
        p = np.zeros(n, np.float64); p1 = np.zeros(n, np.int8); p2 = np.zeros(n, np.int8); dip = np.zeros(n, np.uint8)
        _chk(lib().gm_dev_snp_stat(self.h, counts.ctypes.data, n, int(monop), p.ctypes.data, p1.ctypes.data, p2.ctypes.data, dip.ctypes.data))
        return p, p1, p2, dip

    def coverage_write_gmp_calls(self, path, pval=0.001, monop=False):
        """gm_coverage_write_gmp_calls: --snp's .gmp with the likelihood-ratio column, straight from the tracks in HBM"""
        _chk(lib().gm_coverage_write_gmp_calls(self.h, pval, int(monop), os.fsencode(path), 0))

    # ---- track files formatted on the device (k_track_sizes / k_track_rows) ----
    def coverage_text(self, params=None, lo=0, hi=None):
        """gm_coverage_text: the rows of bins [lo, hi) as bytes; params None or normal mode = .sgr rows, else the .gmp rows of its mode"""
        hi = self.coverage_bins() if hi is None else hi
        p = C.byref(getattr(params, "c", params)) if params is not None else None      # a Params or a gm_params
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap); got = u64()
            rc = lib().gm_coverage_text(self.h, p, lo, hi, buf, cap, C.byref(got))
            if rc == GM_E_CAPACITY:
                cap = int(got.value)
                continue
            _chk(rc)
            return buf.raw[:got.value]

    def coverage_write_sgr_device(self, path, append=False):
        """gm_coverage_write_sgr_device: <out>.sgr from the track in HBM, the bytes of coverage_write_sgr"""
        _chk(lib().gm_coverage_write_sgr_device(self.h, os.fsencode(path), int(append)))

    def coverage_write_gmp_device(self, params, path, append=False):
        """gm_coverage_write_gmp_device: the eight-column <out>.gmp of -b / --b2 / -d / --snp from the tracks in HBM"""
        _chk(lib().gm_coverage_write_gmp_device(self.h, C.byref(getattr(params, "c", params)), os.fsencode(path), int(append)))

    def coverage_write_gmp_calls_device(self, path, pval=0.001, monop=False, append=False):
        """gm_coverage_write_gmp_calls_device: the nine-column <out>.gmp of --snp --snp_calls formatted on the device, the bytes of coverage_write_gmp_calls"""
        _chk(lib().gm_coverage_write_gmp_calls_device(self.h, pval, int(monop), os.fsencode(path), int(append)))

    def coverage_calls_text(self, pval=0.001, monop=False, lo=0, hi=None):
        """gm_coverage_calls_text: the nine-column rows of the positions [lo, hi) as bytes"""
        hi = self.coverage_bins() if hi is None else hi
        cap = 1 << 16
        while True:
            buf = C.create_string_buffer(cap); got = u64()
            rc = lib().gm_coverage_calls_text(self.h, pval, int(monop), lo, hi, buf, cap, C.byref(got))
            if rc == GM_E_CAPACITY:
                cap = int(got.value)
                continue
            _chk(rc)
            return buf.raw[:got.value]

    def coverage_write_vcf(self, path, pval=0.001, monop=False, append=False):
        """gm_coverage_write_vcf: <out>.vcf, one row per record of snp_calls (Genome::PrintFinalVCF); the header unless appending"""
        _chk(lib().gm_coverage_write_vcf(self.h, pval, int(monop), os.fsencode(path), int(append)))

    def coverage_text_stats(self):
        """rows, bytes, slabs, host_slabs, launches, kernel_ms of the last device track writer / coverage_text / coverage_calls_text"""
        st = gm_track_text_stats()
        _chk(lib().gm_coverage_text_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in gm_track_text_stats._fields_}


class Batch:
    def __init__(self, index, max_reads, max_len):
        self.index = index
        self.h = C.c_void_p()
        _chk(lib().gm_batch_create(index.h, max_reads, max_len, C.byref(self.h)))
        self._keep = None

    def destroy(self):
        if self.h:
            lib().gm_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def set_adaptor(self, adaptor):
        """-A: trim this adaptor (bytes) from the reads of every block uploaded from now on; None or b"" clears it"""
        _chk(lib().gm_batch_set_adaptor(self.h, None if adaptor is None else bytes(adaptor)))

    def set_unmapped_rows(self, on=True):
        """gm_batch_set_unmapped_rows: from the next call on, output_text / output_text_resident / output_bam / output_bam_resident and
        SamSorter.add_block write one flag-4 row (tag YU:i:<status>) for every read of the block they write no record for; output()
        (the records form) is not affected.  Row counts and row offsets then count rows"""
        _chk(lib().gm_batch_set_unmapped_rows(self.h, int(bool(on))))

    def unmapped_rows(self):
        """gm_batch_unmapped_rows: the rows of reads without a record that the last row-producing output call wrote"""
        n = u64()
        _chk(lib().gm_batch_unmapped_rows(self.h, C.byref(n)))
        return int(n.value)

    def set_row_tags(self, md=True):
        """gm_batch_set_row_tags: from the next call on, every row of the row-producing output calls that prints a record whose CIGAR is
        not "*" carries NM:i and MD:Z behind X0 - of the row as printed, so they agree with the CIGAR order that is set.  GnumapError
        GM_E_UNSUPPORTED with an adaptor set, GM_E_IO when the index has no readable <fa>.gnumap.amb"""
        _chk(lib().gm_batch_set_row_tags(self.h, GM_ROW_TAG_MD if md else 0))

    def set_mates(self, on=True, min_insert=0, max_insert=500):
        """gm_batch_set_mates: from the next call on, reads 2i and 2i + 1 of a block are the mates of pair i in every output call: the
        pair is resolved on the device (include/gnumap_hip.h has the rule) and the rows carry the paired flag, RNEXT, PNEXT and TLEN.
        An odd block, min_insert > max_insert and a pair whose printed names differ make the OUTPUT call raise GM_E_ARG"""
        _chk(lib().gm_batch_set_mates(self.h, int(bool(on)), int(min_insert), int(max_insert)))

    def mate_rows(self, cap=None):
        """gm_batch_mate_rows: the {flag, rnext, pnext, tlen} of every row the last output call produced (MATE_ROW_DTYPE), in row
        order; for output() one per record.  cap: the room to offer (None: ask first); GM_E_CAPACITY raises when it is too small"""
        n = u64()
        if cap is None:
            rc = lib().gm_batch_mate_rows(self.h, None, 0, C.byref(n))
            if rc != GM_E_CAPACITY:
                _chk(rc)
            cap = int(n.value)
        out = np.zeros(max(int(cap), 1), MATE_ROW_DTYPE)
        _chk(lib().gm_batch_mate_rows(self.h, out.ctypes.data, int(cap), C.byref(n)))
        return out[:int(n.value)]

    def mate_stats(self):
        """gm_batch_mate_stats: dict(pairs, both_mapped, proper, one_mapped, none_mapped) of the last output call"""
        v = np.zeros(5, np.uint64)
        _chk(lib().gm_batch_mate_stats(self.h, v.ctypes.data))
        return {k: int(x) for k, x in zip(MATE_STATS, v)}

    def set_cigar_order(self, order="gnumap"):
        """gm_batch_set_cigar_order: "gnumap" - a minus-strand row prints its CIGAR tokens last to first, as the reference does (the
        default); "forward" - in the order the traceback computed them against the forward window, as a plus-strand row does"""
        if order not in ("gnumap", "forward"):
            raise ValueError('set_cigar_order: "gnumap" or "forward"')
        _chk(lib().gm_batch_set_cigar_order(self.h, GM_CIGAR_FORWARD if order == "forward" else GM_CIGAR_GNUMAP))

    def trimmed_len(self):
        """the lengths the kernels used for the block uploaded last (what the adaptor trim kept; the uploaded lengths without one)"""
        out = np.zeros(self.n, np.uint16)
        _chk(lib().gm_batch_trimmed_len(self.h, out.ctypes.data))
        return out

    def adaptor_time(self):
        """(ms, launches) of k_adaptor_trim since the last call, while set_profiling is on"""
        ms = C.c_double(); ln = u64()
        _chk(lib().gm_batch_adaptor_time(self.h, C.byref(ms), C.byref(ln)))
        return float(ms.value), int(ln.value)

    def upload(self, params, B, Q, Ln, stream=None, fasta=False):
        """fasta=True: B holds the letters of FASTA reads (gm_batch_set_read_format), Q is not read (None will do)"""
        self._keep = (B, Q, Ln)
        r = _reads_struct(B, Q, Ln)
        _chk(lib().gm_batch_set_read_format(self.h, GM_READS_FASTA if fasta else GM_READS_FASTQ))
        _chk(lib().gm_batch_upload(self.h, C.byref(params.c), C.byref(r), stream))
        self.n = B.shape[0]

    def upload_text(self, params, text, stream=None, want_recs=True):
        """gm_batch_upload_text: FASTQ text as it stands in the file -> the batch resident as upload() of the rows cut from it would leave
        it.  Returns dict(n, max_len, stride, status, bad_at, recs): recs is the gm_text_rec table (TEXT_REC_DTYPE), None without want_recs"""
        text = bytes(text)
        buf = np.frombuffer(text + b"\0", np.uint8)
        _chk(lib().gm_batch_set_read_format(self.h, GM_READS_FASTQ))
        info = gm_text_info()
        cap = max(len(text) // 64, 64)
        while True:
            recs = np.zeros(cap, TEXT_REC_DTYPE) if want_recs else None
            rc = lib().gm_batch_upload_text(self.h, C.byref(params.c), buf.ctypes.data, len(text), C.byref(info), recs.ctypes.data if want_recs else None, cap, stream)
            if rc == GM_E_CAPACITY:
                cap = int(info.n)
                continue
            _chk(rc)
            break
        self.n = int(info.n); self.stride = int(info.stride); self._keep = None
        return dict(n=self.n, max_len=int(info.max_len), stride=self.stride, status=int(info.status), bad_at=int(info.bad_at),
                    recs=recs[:self.n] if want_recs else None)

    def map_text(self, params, stream=None, mcap=None, pcap=None):
        """gm_map_batch_text: map() for the block upload_text left resident; the same dict.  mcap / pcap: first capacities to try (the call
        is repeated with the sizes GM_E_CAPACITY reports; self.map_calls counts the calls)"""
        n = self.n
        status = np.zeros(n, np.int8); self_score = np.zeros(n, np.float32); top = np.zeros(n, np.float64); den = np.zeros(n, np.float64)
        mbegin = np.zeros(n + 1, np.uint64)
        mcap = 4 * n + 64 if mcap is None else int(mcap); pcap = 8 * n + 64 if pcap is None else int(pcap)
        r = gm_reads(); r.n = n; r.stride = self.stride
        self.map_calls = 0
        while True:
            matches = np.zeros(max(mcap, 1), MATCH_DTYPE); positions = np.zeros(max(pcap, 1), POS_DTYPE)
            h = gm_hits()
            h.n = n; h.status = status.ctypes.data; h.self_score = self_score.ctypes.data; h.top_score = top.ctypes.data
            h.denominator = den.ctypes.data; h.match_begin = mbegin.ctypes.data
            h.matches = matches.ctypes.data; h.matches_cap = mcap; h.positions = positions.ctypes.data; h.positions_cap = pcap
            rc = lib().gm_map_batch_text(self.index.h, C.byref(params.c), self.h, C.byref(h), stream)
            self.map_calls += 1
            if rc == GM_E_CAPACITY:
                mcap, pcap = int(h.matches_cap), int(h.positions_cap)
                continue
            _chk(rc)
            break
        return dict(status=status, self_score=self_score, top_score=top, denominator=den, match_begin=mbegin,
                    matches=matches[:int(mbegin[n])], positions=positions, _struct=h, _reads=r)

    def output_text_resident(self, params, res, stream=None, text_cap=None):
        """gm_output_batch_text_resident on the result of map_text(): (SAM rows as bytes, row offsets [n_recs + 1]); names and quality tails
        are the ones upload_text left on the device.  text_cap as in output_text"""
        tcap = int(text_cap) if text_cap is not None else self.n * (2 * self.stride + 160) + 1024
        rcap = 2 * self.n + 64
        self.text_calls = 0
        while True:
            text = np.zeros(max(tcap, 1), np.uint8); row_off = np.zeros(rcap, np.uint64)
            st = gm_sam_text()
            st.text = text.ctypes.data; st.text_cap = tcap; st.row_off = row_off.ctypes.data; st.row_cap = rcap
            rc = lib().gm_output_batch_text_resident(self.index.h, C.byref(params.c), self.h, C.byref(res["_struct"]), C.byref(st), stream)
            self.text_calls += 1
            if rc == GM_E_CAPACITY:
                tcap, rcap = max(tcap, int(st.text_cap)), max(rcap, int(st.row_cap))
                continue
            _chk(rc)
            break
        return text[:st.text_len].tobytes(), row_off[:st.n_recs + 1].copy()

    def map_device(self, params, stream=None):
        _chk(lib().gm_map_batch_device(self.index.h, C.byref(params.c), self.h, stream))

    def counters(self):
        c = gm_counters()
        _chk(lib().gm_batch_counters(self.h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in gm_counters._fields_}

    def path(self):
        """which kernels the last map_device / map chose"""
        return lib().gm_batch_path(self.h).decode()

    def pair_flagged(self):
        """reads that k_vote_pair left to k_vote_bucket in the last map_device / map (0 when it did not run)"""
        n = C.c_uint32()
        _chk(lib().gm_batch_pair_flagged(self.h, C.byref(n)))
        return int(n.value)

    def set_profiling(self, on=True):
        _chk(lib().gm_batch_set_profiling(self.h, int(on)))

    def kernel_times(self):
        """{kernel name: (total ms, launches)} accumulated since the last call"""
        ms = np.zeros(GM_K_COUNT, np.float64); ln = np.zeros(GM_K_COUNT, np.uint64)
        _chk(lib().gm_batch_kernel_times(self.h, ms.ctypes.data, ln.ctypes.data))
        return {lib().gm_kernel_name(i).decode(): (float(ms[i]), int(ln[i])) for i in range(GM_K_COUNT)}

    def raw_hits(self):
        n = self.n
        status = np.zeros(n, np.int8); self_score = np.zeros(n, np.float32); top = np.zeros(n, np.float32)
        cap = 1024
        while True:
            out = np.zeros(cap, RAW_HIT_DTYPE); got = u64()
            rc = lib().gm_batch_raw_hits(self.h, out.ctypes.data, cap, C.byref(got), status.ctypes.data, self_score.ctypes.data, top.ctypes.data)
            if rc == GM_E_CAPACITY:
                cap = int(got.value) + 16
                continue
            _chk(rc)
            return out[:got.value], status, self_score, top

    def map(self, params, B, Q, Ln, stream=None, fasta=False):
        """gm_map_batch: returns dict(status, self_score, top_score, denominator, match_begin, matches, positions).
        fasta=True: B holds the letters of FASTA reads (gm_batch_set_read_format), Q is not read (None will do)"""
        n = B.shape[0]
        self._keep = (B, Q, Ln); self.n = n
        r = _reads_struct(B, Q, Ln)
        _chk(lib().gm_batch_set_read_format(self.h, GM_READS_FASTA if fasta else GM_READS_FASTQ))
        status = np.zeros(n, np.int8); self_score = np.zeros(n, np.float32); top = np.zeros(n, np.float64); den = np.zeros(n, np.float64)
        mbegin = np.zeros(n + 1, np.uint64)
        mcap, pcap = 4 * n + 64, 8 * n + 64
        while True:
            matches = np.zeros(mcap, MATCH_DTYPE); positions = np.zeros(pcap, POS_DTYPE)
            h = gm_hits()
            h.n = n; h.status = status.ctypes.data; h.self_score = self_score.ctypes.data; h.top_score = top.ctypes.data
            h.denominator = den.ctypes.data; h.match_begin = mbegin.ctypes.data
            h.matches = matches.ctypes.data; h.matches_cap = mcap; h.positions = positions.ctypes.data; h.positions_cap = pcap
            rc = lib().gm_map_batch(self.index.h, C.byref(params.c), self.h, C.byref(r), C.byref(h), stream)
            if rc == GM_E_CAPACITY:
                mcap, pcap = int(h.matches_cap) + 64, int(h.positions_cap) + 64
                continue
            _chk(rc)
            break
        res = dict(status=status, self_score=self_score, top_score=top, denominator=den, match_begin=mbegin,
                   matches=matches[:int(mbegin[n])], positions=positions, _struct=h, _reads=r)
        return res

    def output(self, params, res, stream=None):
        """gm_output_batch on the result of map(): returns (records ndarray, list of CIGAR bytes per record)"""
        rcap, ccap = 2 * self.n + 64, 32 * self.n + 1024
        while True:
            recs = np.zeros(rcap, SAM_DTYPE); pool = np.zeros(ccap, np.uint8)
            so = gm_sam_out()
            so.recs = recs.ctypes.data; so.recs_cap = rcap; so.cigar_pool = pool.ctypes.data; so.cigar_cap = ccap
            rc = lib().gm_output_batch(self.index.h, C.byref(params.c), self.h, C.byref(res["_reads"]), C.byref(res["_struct"]), C.byref(so), stream)
            if rc == GM_E_CAPACITY:
                rcap, ccap = int(so.recs_cap) + 64, int(so.cigar_cap) + 64
                continue
            _chk(rc)
            break
        recs = recs[:so.n_recs]
        raw = pool.tobytes()
        cigars = [raw[o:raw.index(b"\0", o)] for o in recs["cigar_off"]]
        return recs, cigars

    def output_text(self, params, res, names, qual_tails=None, stream=None, text_cap=None):
        """gm_output_batch_text on the result of map(): (SAM rows as bytes, row offsets [n_recs + 1]).  names: one bytes per read (what
        follows '@'); qual_tails: None, or one bytes per read (what a quality line holds beyond the length of its sequence).
        text_cap: first capacity to try (None: a guess; the call is repeated with the size GM_E_CAPACITY reports)."""
        rt, keep = _pack_read_text([bytes(x) for x in names], None if qual_tails is None else [bytes(x) for x in qual_tails], self.n)
        stride = res["_reads"].stride
        tcap = int(text_cap) if text_cap is not None else self.n * (2 * stride + 160) + 1024
        rcap = 2 * self.n + 64
        self.text_calls = 0
        while True:
            text = np.zeros(max(tcap, 1), np.uint8); row_off = np.zeros(rcap, np.uint64)
            st = gm_sam_text()
            st.text = text.ctypes.data; st.text_cap = tcap; st.row_off = row_off.ctypes.data; st.row_cap = rcap
            rc = lib().gm_output_batch_text(self.index.h, C.byref(params.c), self.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), C.byref(st), stream)
            self.text_calls += 1
            if rc == GM_E_CAPACITY:
                tcap, rcap = max(tcap, int(st.text_cap)), max(rcap, int(st.row_cap))
                continue
            _chk(rc)
            break
        del keep
        return text[:st.text_len].tobytes(), row_off[:st.n_recs + 1].copy()


    def _output_bam(self, call, level, bam_cap, stride):
        cap = int(bam_cap) if bam_cap is not None else self.n * (2 * stride + 160) + 1024
        self.bam_calls = 0
        while True:
            buf = np.zeros(max(cap, 1), np.uint8)
            bo = gm_bam_out()
            bo.data = buf.ctypes.data; bo.cap = cap; bo.level = int(level)
            rc = call(bo)
            self.bam_calls += 1
            if rc == GM_E_CAPACITY:
                cap = max(cap + 1, int(bo.cap))
                continue
            _chk(rc)
            break
        self.bam_raw_len, self.bam_n_recs = int(bo.raw_len), int(bo.n_recs)
        return buf[:bo.len].tobytes()

    def bam_times(self):
        """gm_batch_bam_times (set_profiling first): dict(rows_ms, bgzf_ms, raw_bytes, bgzf_in, bgzf_out) since the last call"""
        ms = np.zeros(2, np.float64); by = np.zeros(3, np.uint64)
        _chk(lib().gm_batch_bam_times(self.h, ms.ctypes.data, by.ctypes.data))
        return dict(rows_ms=float(ms[0]), bgzf_ms=float(ms[1]), raw_bytes=int(by[0]), bgzf_in=int(by[1]), bgzf_out=int(by[2]))

    def output_bam(self, params, res, names, qual_tails=None, level=1, stream=None, bam_cap=None, lz77=False):
        """gm_output_batch_bam on the result of map(): the block's BAM records as BGZF blocks (bytes).  names / qual_tails as in output_text;
        lz77 as in Index.bgzf_compress;
        bam_cap: first capacity to try.  self.bam_raw_len / self.bam_n_recs: bytes and number of the records"""
        rt, keep = _pack_read_text([bytes(x) for x in names], None if qual_tails is None else [bytes(x) for x in qual_tails], self.n)
        out = self._output_bam(lambda bo: lib().gm_output_batch_bam(self.index.h, C.byref(params.c), self.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]),
                                                                    C.byref(bo), stream), _bgzf_level(level, lz77), bam_cap, res["_reads"].stride)
        del keep
        return out

    def output_bam_resident(self, params, res, level=1, stream=None, bam_cap=None, lz77=False):
        """gm_output_batch_bam_resident on the result of map_text()"""
        return self._output_bam(lambda bo: lib().gm_output_batch_bam_resident(self.index.h, C.byref(params.c), self.h, C.byref(res["_struct"]), C.byref(bo), stream),
                                _bgzf_level(level, lz77), bam_cap, self.stride)


def _bgzf_level(level, lz77):
    return int(level) | (GM_BGZF_LZ77 if lz77 else 0)


def bgzf_eof():
    """gm_bgzf_eof: the 28 bytes that end a BGZF file"""
    buf = np.zeros(28, np.uint8)
    _chk(lib().gm_bgzf_eof(buf.ctypes.data))
    return buf.tobytes()


class SamSorter:
    """gm_sam_sorter: the SAM rows of a run kept in HBM and read back in coordinate order.  The piece size of its arena is the
    GM_SORT_PIECE switch as it stands when the object is made."""

    def __init__(self, index, rows="text"):
        """rows: "text" (SAM rows) or "bam" (BAM records): what add_block puts into the arena"""
        self.index = index
        self.h = C.c_void_p()
        _chk(lib().gm_sam_sorter_create(index.h, C.byref(self.h)))
        if rows != "text":
            self.set_rows(rows)

    def set_rows(self, rows):
        """gm_sam_sorter_set_rows; before the first block"""
        _chk(lib().gm_sam_sorter_set_rows(self.h, {"text": GM_ROWS_TEXT, "bam": GM_ROWS_BAM}[rows]))

    def destroy(self):
        if self.h:
            lib().gm_sam_sorter_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def add_block(self, batch, params, res, seq, names=None, qual_tails=None, stream=None):
        """the block `batch` was mapped with (res = map() or map_text()) under sequence number seq.  names (one bytes per read, and
        qual_tails as in Batch.output_text): gm_output_batch_sorted; names None: gm_output_batch_sorted_resident, for a block of
        upload_text() / map_text()"""
        if names is None:
            _chk(lib().gm_output_batch_sorted_resident(self.index.h, C.byref(params.c), batch.h, C.byref(res["_struct"]), self.h, int(seq), stream))
            return
        rt, keep = _pack_read_text([bytes(x) for x in names], None if qual_tails is None else [bytes(x) for x in qual_tails], batch.n)
        _chk(lib().gm_output_batch_sorted(self.index.h, C.byref(params.c), batch.h, C.byref(res["_reads"]), C.byref(rt), C.byref(res["_struct"]), self.h,
                                         int(seq), stream))
        del keep

    def add_rows(self, seq, rows, contig, chr_pos, stream=None):
        """gm_sam_sorter_add_rows: rows (list of bytes, or one uint8 array with row_off as second element of a tuple) under the caller's
        keys; contig >= the number of contigs gives the key of a row without a contig"""
        if isinstance(rows, tuple):
            text, off = rows
        else:
            text = np.frombuffer(b"".join(rows) + b"\0", np.uint8)
            off = np.zeros(len(rows) + 1, np.uint64); off[1:] = np.cumsum([len(r) for r in rows], dtype=np.uint64)
        off = np.ascontiguousarray(off, np.uint64)
        c = np.ascontiguousarray(contig, np.uint32); q = np.ascontiguousarray(chr_pos, np.uint64)
        n = len(off) - 1
        assert len(c) == n and len(q) == n
        _chk(lib().gm_sam_sorter_add_rows(self.h, int(seq), text.ctypes.data, off.ctypes.data, c.ctypes.data, q.ctypes.data, n, stream))

    def finish(self, stream=None):
        """sorts; (rows, text bytes)"""
        n = u64(); b = u64()
        _chk(lib().gm_sam_sorter_finish(self.h, C.byref(n), C.byref(b), stream))
        return int(n.value), int(b.value)

    def read(self, cap, stream=None):
        """the next whole rows that fit in cap bytes (b"" = done).  GnumapError with code GM_E_CAPACITY and .needed = the next row's length
        when that row alone is longer than cap"""
        buf = np.zeros(max(int(cap), 1), np.uint8); got = u64()
        rc = lib().gm_sam_sorter_read(self.h, buf.ctypes.data, int(cap), C.byref(got), stream)
        if rc == GM_E_CAPACITY:
            e = GnumapError(rc, lib().gm_last_error().decode())
            e.needed = int(got.value)
            raise e
        _chk(rc)
        return buf[:got.value].tobytes()

    def read_bgzf(self, cap, level=1, stream=None, lz77=False):
        """gm_sam_sorter_read_bgzf: the next whole rows whose BGZF form is sure to fit in cap bytes, as BGZF blocks (b"" = done).  lz77 as in
        Index.bgzf_compress.  GnumapError
        with code GM_E_CAPACITY and .needed = the cap the next row needs when that row alone is too long"""
        buf = np.zeros(max(int(cap), 1), np.uint8); got = u64()
        rc = lib().gm_sam_sorter_read_bgzf(self.h, _bgzf_level(level, lz77), buf.ctypes.data, int(cap), C.byref(got), stream)
        if rc == GM_E_CAPACITY:
            e = GnumapError(rc, lib().gm_last_error().decode())
            e.needed = int(got.value)
            raise e
        _chk(rc)
        return buf[:got.value].tobytes()

    def index_begin(self, file_offset):
        """gm_sam_sorter_index_begin: after finish() and before the first read_bgzf(), on rows="bam".  file_offset: where the first block
        read_bgzf() returns will lie in the file (the bytes of the compressed header)"""
        _chk(lib().gm_sam_sorter_index_begin(self.h, int(file_offset)))

    def bai(self, cap=None, stream=None):
        """gm_sam_sorter_bai: the .bai of the file whose blocks read_bgzf() returned, once all of them have been read.  cap None: asked
        for once and read with the size it needs; a cap that is too small: GnumapError with code GM_E_CAPACITY and .needed = the size"""
        want = 1 << 16 if cap is None else int(cap)
        for _ in range(2):
            buf = np.zeros(max(want, 1), np.uint8); got = u64()
            rc = lib().gm_sam_sorter_bai(self.h, buf.ctypes.data, want, C.byref(got), stream)
            if rc != GM_E_CAPACITY:
                _chk(rc)
                return buf[:got.value].tobytes()
            if cap is not None:
                break
            want = int(got.value)
        e = GnumapError(rc, lib().gm_last_error().decode())
        e.needed = int(got.value); e.buffer = buf
        raise e

    def text(self, cap=1 << 20):
        """every slab that is left, joined"""
        out = []
        while True:
            try:
                t = self.read(cap)
            except GnumapError as e:
                if e.code != GM_E_CAPACITY:
                    raise
                cap = e.needed
                continue
            if not t:
                return b"".join(out)
            out.append(t)

    def stats(self):
        st = gm_sam_sort_stats()
        _chk(lib().gm_sam_sorter_stats(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in gm_sam_sort_stats._fields_}


def _pack_read_text(names, qual_tails, n):
    """(gm_read_text, the arrays it points into) from lists of bytes"""
    if len(names) != n or (qual_tails is not None and len(qual_tails) != n):
        raise ValueError("one name (and one quality tail) per read")
    pool = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
    off = np.zeros(n + 1, np.uint64); off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
    rt = gm_read_text(); rt.names = pool.ctypes.data; rt.name_off = off.ctypes.data
    keep = [pool, off]
    if qual_tails is not None:
        tp = np.frombuffer(b"".join(qual_tails) + b"\0", np.uint8).copy()
        to = np.zeros(n + 1, np.uint64); to[1:] = np.cumsum([len(x) for x in qual_tails], dtype=np.uint64)
        rt.qual_tail = tp.ctypes.data; rt.qual_tail_off = to.ctypes.data
        keep += [tp, to]
    return rt, keep


def pinned_empty(shape, dtype):
    """numpy array over page-locked host memory from gm_host_alloc (freed when the array's owner object is collected)"""
    dt = np.dtype(dtype)
    nbytes = int(np.prod(shape)) * dt.itemsize
    ptr = lib().gm_host_alloc(max(nbytes, 1))
    if not ptr:
        raise GnumapError(-7, lib().gm_last_error().decode())
    buf = (C.c_uint8 * max(nbytes, 1)).from_address(ptr)
    arr = np.frombuffer(buf, dtype=np.uint8, count=nbytes).view(dt).reshape(shape)
    _PINNED[id(buf)] = (buf, ptr)
    return arr


_PINNED = {}


class BlockRunner:
    """The two ABI calls of one block loop iteration (gm_map_batch + gm_output_batch) on caller-owned, page-locked, REUSED buffers:
    what a host driver thread does per block.  One BlockRunner = one gm_batch + one HIP stream + one set of output buffers."""

    def __init__(self, index, params, max_reads, stride, stream=None):
        self.index, self.params, self.max_reads, self.stride, self.stream = index, params, max_reads, stride, stream
        self.batch = Batch(index, max_reads, stride)
        n = max_reads
        self.status = pinned_empty(n, np.int8); self.self_score = pinned_empty(n, np.float32)
        self.top = pinned_empty(n, np.float64); self.den = pinned_empty(n, np.float64); self.mbegin = pinned_empty(n + 1, np.uint64)
        self._alloc_hits(2 * n + 64, 2 * n + 64)
        self._alloc_out(2 * n + 64, 16 * n + 1024)

    def _alloc_hits(self, mcap, pcap):
        self.matches = pinned_empty(mcap, MATCH_DTYPE); self.positions = pinned_empty(pcap, POS_DTYPE)

    def _alloc_out(self, rcap, ccap):
        self.recs = pinned_empty(rcap, SAM_DTYPE); self.pool = pinned_empty(ccap, np.uint8)

    def run(self, B, Q, Ln):
        """B, Q: [n, stride] uint8 (ideally page-locked), Ln: [n] uint16.  Returns (n_matches, n_records)."""
        n = B.shape[0]
        r = _reads_struct(B, Q, Ln)
        L = lib()
        while True:
            h = gm_hits()
            h.n = n; h.status = self.status.ctypes.data; h.self_score = self.self_score.ctypes.data; h.top_score = self.top.ctypes.data
            h.denominator = self.den.ctypes.data; h.match_begin = self.mbegin.ctypes.data
            h.matches = self.matches.ctypes.data; h.matches_cap = len(self.matches)
            h.positions = self.positions.ctypes.data; h.positions_cap = len(self.positions)
            rc = L.gm_map_batch(self.index.h, C.byref(self.params.c), self.batch.h, C.byref(r), C.byref(h), self.stream)
            if rc == GM_E_CAPACITY:
                self._alloc_hits(int(h.matches_cap) + 64, int(h.positions_cap) + 64)
                continue
            _chk(rc)
            break
        while True:
            so = gm_sam_out()
            so.recs = self.recs.ctypes.data; so.recs_cap = len(self.recs); so.cigar_pool = self.pool.ctypes.data; so.cigar_cap = len(self.pool)
            rc = L.gm_output_batch(self.index.h, C.byref(self.params.c), self.batch.h, C.byref(r), C.byref(h), C.byref(so), self.stream)
            if rc == GM_E_CAPACITY:
                self._alloc_out(int(so.recs_cap) + 64, int(so.cigar_cap) + 64)
                continue
            _chk(rc)
            break
        return int(self.mbegin[n]), int(so.n_recs)

    def run_async(self, B, Q, Ln):
        """queue gm_map_batch + gm_output_batch of this block on the batch's service thread (gm_*_enqueue) and return at once; wait()
        gives (n_matches, n_records).  The buffers must have room (a first synchronous run() sizes them)."""
        n = B.shape[0]
        self._n = n
        self._r = _reads_struct(B, Q, Ln); self._keep = (B, Q, Ln)
        h = self._h = gm_hits()
        h.n = n; h.status = self.status.ctypes.data; h.self_score = self.self_score.ctypes.data; h.top_score = self.top.ctypes.data
        h.denominator = self.den.ctypes.data; h.match_begin = self.mbegin.ctypes.data
        h.matches = self.matches.ctypes.data; h.matches_cap = len(self.matches)
        h.positions = self.positions.ctypes.data; h.positions_cap = len(self.positions)
        so = self._so = gm_sam_out()
        so.recs = self.recs.ctypes.data; so.recs_cap = len(self.recs); so.cigar_pool = self.pool.ctypes.data; so.cigar_cap = len(self.pool)
        L = lib()
        _chk(L.gm_map_batch_enqueue(self.index.h, C.byref(self.params.c), self.batch.h, C.byref(self._r), C.byref(h), self.stream))
        _chk(L.gm_output_batch_enqueue(self.index.h, C.byref(self.params.c), self.batch.h, C.byref(self._r), C.byref(h), C.byref(so), self.stream))

    def wait(self):
        rc = lib().gm_batch_wait(self.batch.h)
        if rc == GM_E_CAPACITY:                      # the buffers were too small after all: size them and run the block synchronously
            self._alloc_hits(max(int(self._h.matches_cap), len(self.matches)) + 64, max(int(self._h.positions_cap), len(self.positions)) + 64)
            self._alloc_out(max(int(self._so.recs_cap), len(self.recs)) + 64, max(int(self._so.cigar_cap), len(self.pool)) + 64)
            return self.run(*self._keep)
        _chk(rc)
        return int(self.mbegin[self._n]), int(self._so.n_recs)
