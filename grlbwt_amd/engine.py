"""Host-side mirror of the reference's driver interface over the C-ABI library.

Mirrors include/grl_bwt.hpp:23-79 (grl_bwt_algo = par_phase + ind_phase + write
.rl_bwt) with the same stage names.  Everything runs through
libgrlbwt_hip.so (include/grlbwt_hip.h); there is no CPU path: if the library
is missing or no HIP device is usable this module raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB = os.path.join(_HERE, "csrc", "libgrlbwt_hip.so")

FLAG_KEEP_LEVELS = 1
FLAG_SYNC_DEBUG = 2
FLAG_FORCE_IDX64 = 4
FLAG_CLASSIC_POOL = 8

OK = 0
EILLFORMED = -84
ENOTDNA = -86

# every symbol include/grlbwt_hip.h declares
ABI_SYMBOLS = [
    "grlbwt_abi_version", "grlbwt_backend_name", "grlbwt_strerror", "grlbwt_last_error", "grlbwt_ctx_create", "grlbwt_ctx_destroy",
    "grlbwt_ctx_set_stream", "grlbwt_text_upload", "grlbwt_text_load_file", "grlbwt_text_load_file_range", "grlbwt_rccl_unique_id", "grlbwt_rccl_comm_create",
    "grlbwt_rccl_comm_destroy", "grlbwt_fastx_probe", "grlbwt_text_load_fastx", "grlbwt_fastx_convert_device", "grlbwt_text_attach_device", "grlbwt_get_stats",
    "grlbwt_parse_round", "grlbwt_parse_phase", "grlbwt_round_info_get", "grlbwt_induce_first",
    "grlbwt_induce_level", "grlbwt_induce_phase", "grlbwt_level_info_get", "grlbwt_build", "grlbwt_result_size",
    "grlbwt_result_device_ptr", "grlbwt_result_download", "grlbwt_result_write_file", "grlbwt_result_part", "grlbwt_result_write_part", "grlbwt_level_text_size",
    "grlbwt_level_text_download", "grlbwt_level_bwt_size", "grlbwt_level_bwt_download", "grlbwt_get_counters",
    "grlbwt_selftest", "grlbwt_profile_enable", "grlbwt_profile_dump", "grlbwt_dist_build", "grlbwt_memory_usage", "grlbwt_invert_image", "grlbwt_invert_image_tails",
    "grlbwt_image_plain", "grlbwt_image_rle", "grlbwt_image_stats_get", "grlbwt_image_split_runs",
    "grlbwt_level_grammar_size", "grlbwt_level_grammar_download",
    "grlbwt_alphabet_size", "grlbwt_alphabet_download", "grlbwt_alphabet_compact_device",
    "grlbwt_fm_create", "grlbwt_fm_destroy", "grlbwt_fm_info_get", "grlbwt_fm_count", "grlbwt_fm_locate",
    "grlbwt_invert_image_checkpointed", "grlbwt_fm_walk_info_get",
    "grlbwt_fm_string_lengths", "grlbwt_fm_extract", "grlbwt_fm_extract_info_get",
    "grlbwt_fm_match", "grlbwt_fm_mems", "grlbwt_fm_match_info_get",
    "grlbwt_fm_approx", "grlbwt_fm_approx_info_get",
    "grlbwt_fm_overlaps", "grlbwt_fm_overlaps_of", "grlbwt_fm_overlap_targets", "grlbwt_fm_overlap_info_get",
    "grlbwt_fm_lcp", "grlbwt_fm_lcp_info_get",
    "grlbwt_fm_sa", "grlbwt_fm_sa_info_get",
    "grlbwt_fm_kmers", "grlbwt_fm_kmer_info_get",
    "grlbwt_fm_kmers_canonical", "grlbwt_fm_kmers_canonical_info_get",
    "grlbwt_fm_repeats", "grlbwt_fm_repeat_info_get",
    "grlbwt_docs_create", "grlbwt_docs_destroy", "grlbwt_docs_info_get", "grlbwt_docs_count", "grlbwt_docs_list",
    "grlbwt_debruijn_create", "grlbwt_debruijn_destroy", "grlbwt_debruijn_info_get", "grlbwt_debruijn_nodes", "grlbwt_debruijn_edges",
    "grlbwt_debruijn_unitigs",
    "grlbwt_cdebruijn_create", "grlbwt_cdebruijn_destroy", "grlbwt_cdebruijn_info_get", "grlbwt_cdebruijn_nodes", "grlbwt_cdebruijn_links",
    "grlbwt_cdebruijn_unitigs",
    "grlbwt_merge_create", "grlbwt_merge_info_get", "grlbwt_merge_emit", "grlbwt_merge_interleave", "grlbwt_merge_destroy",
    "grlbwt_merge_files",
    "grlbwt_select_create", "grlbwt_select_info_get", "grlbwt_select_emit", "grlbwt_select_rows", "grlbwt_select_destroy",
    "grlbwt_select_files",
]

FM_LOCATE = 1
FM_CHECKPOINTS = 2
FM_EXTRACT = 4
FM_OVERLAP_PROPER = 1
FM_REPEATS_MAXIMAL = 1
UINT64_MAX = 2 ** 64 - 1
DOCS_OCCURRENCES = 1
SELECT_KEEP = 1
SELECT_CHECKPOINTS = 2


class FmInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_syms", "n_runs", "n_strings", "sigma", "separator", "idx_bytes", "index_bytes",
                                          "top_entries", "flags")]


class MergeInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_syms_a", "n_syms_b", "n_strings_a", "n_strings_b", "sigma", "separator", "rounds",
                                          "rows_changed", "n_runs", "out_bytes", "sb", "fb", "idx_bytes", "tile_rows",
                                          "scratch_bytes", "held_bytes")]


class SelectInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_syms_in", "n_strings_in", "n_runs_in", "n_listed", "rows_marked", "longest_walk",
                                          "n_syms_out", "n_strings_out", "n_runs_out", "out_bytes", "sb", "fb", "separator",
                                          "idx_bytes", "flags", "walk_lanes", "lane_refills", "sample_bits", "n_checkpoints",
                                          "jump_rounds", "scratch_bytes", "held_bytes")]


class WalkInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_strings", "n_checkpoints", "sample_bits", "longest_segment", "longest_chain",
                                          "jump_rounds", "walk_lanes", "lane_refills", "scratch_bytes", "sample_bytes")]


class ExtractInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_ranges", "n_pieces", "n_cells", "walk_steps", "walk_lanes", "lane_refills",
                                          "n_samples", "extract_bytes")]


class MatchInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_patterns", "n_cells", "matched_cells", "longest", "n_capped", "n_mems", "walk_lanes",
                                          "lane_refills")]


class ApproxInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_patterns", "n_cells", "max_mismatches", "max_hits", "n_hits")] + \
               [("hits_by_mismatches", C.c_uint64 * 4)] + \
               [(k, C.c_uint64) for k in ("n_truncated", "steps", "walk_lanes", "lane_refills", "table_bytes")]


class OverlapInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_patterns", "n_cells", "n_hits", "n_targets", "longest", "steps", "walk_lanes",
                                          "lane_refills", "n_ranges", "n_entries", "tile_entries")]


class LcpInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_rows", "n_strings", "lcp_bytes", "cap", "passes", "n_levels", "max_lcp", "n_capped",
                                          "tile_rows", "scratch_bytes")]


class SaInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_rows", "n_strings", "row_begin", "row_end", "string_bytes", "offset_bytes", "n_written",
                                          "form", "walk_steps", "longest_walk", "walk_lanes", "lane_refills", "scratch_bytes")]


class KmerInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("k", "n_rows", "n_strings", "n_distinct", "n_windows", "n_selected", "largest_count", "passes",
                                          "length_passes", "forward_steps", "tile_rows", "tile_kmers", "stage_bytes", "scratch_bytes")]


class CkmerInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("k", "n_rows", "n_strings", "n_distinct", "n_windows", "n_selected", "n_classes", "n_paired",
                                          "n_palindromes", "n_single", "n_no_complement", "largest_total", "passes", "length_passes",
                                          "mate_walks", "backward_steps", "forward_steps", "tile_rows", "tile_kmers", "mate_tile",
                                          "stage_bytes", "scratch_bytes")]


class RepeatInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_rows", "n_strings", "min_len", "max_len", "passes", "n_repeats", "n_maximal", "n_selected",
                                          "longest", "largest_count", "value_bytes", "tile_rows", "tree_fanout", "tree_levels",
                                          "far_searches", "scratch_bytes")]


class DocsInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_rows", "n_strings", "flags", "idx_bytes", "held_bytes", "scratch_bytes", "sort_bits", "form",
                                          "walk_steps", "n_ranges", "n_range_rows", "n_entries", "largest_range", "most_docs",
                                          "tile_entries")]


class DeBruijnInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("k", "n_rows", "n_strings", "n_distinct", "n_nodes", "n_edges", "n_unitigs", "n_circular",
                                          "longest_unitig", "n_cells", "max_in_degree", "max_out_degree", "passes", "length_passes",
                                          "backward_steps", "jump_rounds", "tile_nodes", "tile_cells", "handle_bytes", "scratch_bytes")]


class CDeBruijnInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("k", "n_rows", "n_strings", "n_distinct", "n_nodes", "n_rigid", "n_palindromes", "n_edges", "n_half_edges",
                                          "n_hairpins", "n_unitigs", "n_circular", "longest_unitig", "n_cells", "max_end_degree", "passes",
                                          "length_passes", "mate_backward_steps", "edge_backward_steps", "forward_steps", "cells_forward_steps",
                                          "jump_rounds", "tile_nodes", "tile_cells", "handle_bytes", "scratch_bytes")]


class ImageStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_runs", "sigma", "text_size", "min_run", "max_run", "fit1", "fit2", "fit3")] + \
               [("runs_of", C.c_uint64 * 256), ("freq_of", C.c_uint64 * 256), ("deciles", C.c_uint64 * 9), ("non_maximal", C.c_uint64)]


class SplitInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("runs_before", "runs_after", "overflow_splits", "block_splits", "n_syms", "n_blocks", "out_bytes")]


class Stats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_strings", "n_syms", "min_sym", "max_sym", "max_sym_freq", "sb", "fb")]


class RoundInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_in", "n_phrases", "dict_syms", "n_metasyms", "parse_size", "sigma",
                                          "max_phrase_len", "sort_iters")]


class LevelInfo(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n", "n_runs", "runs_next", "induced_cells", "prebwt_runs", "segments",
                                          "atoms", "chain_steps", "merged_cells")]


class Counters(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("t_stats", "t_classify", "t_hash", "t_dict_sort", "t_dict_groups", "t_emit",
                                          "t_ind_expand", "t_ind_split", "t_ind_assemble", "t_finish")] + \
               [(k, C.c_uint64) for k in ("bytes_classify_hash", "bytes_emit", "bytes_induce_scatter",
                                          "bytes_induce_assemble", "idx_bytes")]


def _as_dict(s):
    return {k: getattr(s, k) for k, _ in s._fields_}


class GrlbwtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("grlbwt error %d: %s" % (code, msg))
        self.code = code


class NotDNA(GrlbwtError):
    """The reference's "The input seems not to be DNA (invalid symbol:X)", exit(1) (fastx_handler.cpp:30-33)."""


FASTX_REVCOMP = 1


def fastx_probe(path, lib=None):
    """(is_fastx, is_gz) as the reference's is_fastx / check_gzip decide them (host only: no device is touched)."""
    L = load_library(lib)
    a, b = C.c_int(0), C.c_int(0)
    rc = L.grlbwt_fastx_probe(os.fsencode(path), C.byref(a), C.byref(b))
    if rc != 0:
        raise GrlbwtError(rc, "cannot probe " + str(path))
    return bool(a.value), bool(b.value)


class IllFormedInput(GrlbwtError):
    """The reference prints "Error: the file is ill formed" and exits 1 (utils.cpp:177-180)."""


_libs = {}
_standin_paths = set()


def _test_allow_standin(path):
    """TESTS ONLY: accept the serial stand-in library at exactly this path (tests/hostsim).  There is deliberately no
    environment switch: nothing outside a test's own code can point the product at a CPU path."""
    _standin_paths.add(os.path.abspath(path))


def load_library(path=None, allow_test_standin=False):
    """dlopen the C-ABI library; fails loudly when it has not been built.  Only the HIP build is accepted:
    the serial stand-in of tests/hostsim identifies itself and is refused unless a test explicitly allows it."""
    path = path or os.environ.get("GRLBWT_HIP_LIB", DEFAULT_LIB)
    allow_test_standin = allow_test_standin or os.path.abspath(path) in _standin_paths
    if path in _libs:
        L = _libs[path]
        if L.grlbwt_backend_name() != b"hip-gfx950" and not allow_test_standin:
            raise RuntimeError("%s is not the HIP library (backend %r); the product has no CPU path" % (path, L.grlbwt_backend_name()))
        return L
    if not os.path.exists(path):
        raise RuntimeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % path)
    if not allow_test_standin:
        # PyTorch ships its own copy of the HIP runtime.  If torch is imported AFTER this library has pulled in
        # /opt/rocm's copy, the process ends up with two runtimes and torch reports "No HIP GPUs are available";
        # importing torch first makes both sides bind to one.  (Processes that never use torch are unaffected.)
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    L = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.grlbwt_abi_version.restype = i32
    L.grlbwt_backend_name.restype = C.c_char_p
    if L.grlbwt_backend_name() != b"hip-gfx950" and not allow_test_standin:
        raise RuntimeError("%s is not the HIP library (backend %r); the product has no CPU path" % (path, L.grlbwt_backend_name()))
    L.grlbwt_strerror.restype = C.c_char_p
    L.grlbwt_strerror.argtypes = [i32]
    L.grlbwt_last_error.restype = C.c_char_p
    L.grlbwt_last_error.argtypes = [vp]
    L.grlbwt_ctx_create.argtypes = [i32, C.c_uint32, C.POINTER(vp)]
    L.grlbwt_ctx_destroy.argtypes = [vp]
    L.grlbwt_ctx_destroy.restype = None
    L.grlbwt_ctx_set_stream.argtypes = [vp, vp]
    L.grlbwt_text_upload.argtypes = [vp, vp, u64, i32]
    L.grlbwt_text_load_file.argtypes = [vp, C.c_char_p, i32]
    L.grlbwt_text_attach_device.argtypes = [vp, vp, u64, i32]
    L.grlbwt_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.grlbwt_parse_round.argtypes = [vp, C.POINTER(RoundInfo), C.POINTER(i32)]
    L.grlbwt_parse_phase.argtypes = [vp, C.POINTER(i32)]
    L.grlbwt_round_info_get.argtypes = [vp, i32, C.POINTER(RoundInfo)]
    L.grlbwt_induce_first.argtypes = [vp]
    L.grlbwt_induce_level.argtypes = [vp, C.POINTER(i32), C.POINTER(LevelInfo)]
    L.grlbwt_induce_phase.argtypes = [vp]
    L.grlbwt_level_info_get.argtypes = [vp, i32, C.POINTER(LevelInfo)]
    L.grlbwt_build.argtypes = [vp]
    L.grlbwt_result_size.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.grlbwt_result_device_ptr.argtypes = [vp, C.POINTER(vp)]
    L.grlbwt_result_download.argtypes = [vp, vp, u64]
    L.grlbwt_result_write_file.argtypes = [vp, C.c_char_p]
    L.grlbwt_result_part.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.grlbwt_result_write_part.argtypes = [vp, C.c_char_p]
    L.grlbwt_level_text_size.argtypes = [vp, i32, C.POINTER(u64)]
    L.grlbwt_level_text_download.argtypes = [vp, i32, vp]
    L.grlbwt_level_bwt_size.argtypes = [vp, i32, C.POINTER(u64)]
    L.grlbwt_level_bwt_download.argtypes = [vp, i32, vp, vp]
    L.grlbwt_level_grammar_size.argtypes = [vp, i32, C.POINTER(u64), C.POINTER(u64)]
    L.grlbwt_level_grammar_download.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    L.grlbwt_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.grlbwt_selftest.argtypes = [vp, u64, u64]
    L.grlbwt_memory_usage.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.grlbwt_invert_image.argtypes = [vp, vp, u64, i32, vp, u64, C.POINTER(u64)]
    L.grlbwt_invert_image_checkpointed.argtypes = [vp, vp, u64, i32, i32, vp, u64, C.POINTER(u64), C.POINTER(WalkInfo)]
    L.grlbwt_fm_walk_info_get.argtypes = [vp, C.POINTER(WalkInfo)]
    L.grlbwt_invert_image_tails.argtypes = [vp, vp, u64, i32, u64, vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.grlbwt_image_plain.argtypes = [vp, vp, u64, vp, u64, i32, C.POINTER(u64)]
    L.grlbwt_image_rle.argtypes = [vp, vp, u64, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_image_stats_get.argtypes = [vp, vp, u64, C.POINTER(ImageStats)]
    L.grlbwt_image_split_runs.argtypes = [vp, vp, u64, i32, u64, vp, u64, C.POINTER(SplitInfo)]
    L.grlbwt_alphabet_size.argtypes = [vp, C.POINTER(u64)]
    L.grlbwt_alphabet_download.argtypes = [vp, vp]
    L.grlbwt_alphabet_compact_device.argtypes = [vp, vp, u64, i32, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_create.argtypes = [vp, vp, u64, C.c_uint32, C.POINTER(vp)]
    L.grlbwt_fm_destroy.argtypes = [vp, vp]
    L.grlbwt_fm_info_get.argtypes = [vp, C.POINTER(FmInfo)]
    L.grlbwt_fm_count.argtypes = [vp, vp, vp, i32, vp, u64, vp, vp]
    L.grlbwt_fm_locate.argtypes = [vp, vp, vp, u64, u64, vp, vp]
    L.grlbwt_fm_string_lengths.argtypes = [vp, vp, vp]
    L.grlbwt_fm_extract.argtypes = [vp, vp, vp, vp, vp, u64, i32, vp, u64, vp, C.POINTER(u64)]
    L.grlbwt_fm_extract_info_get.argtypes = [vp, C.POINTER(ExtractInfo)]
    L.grlbwt_fm_match.argtypes = [vp, vp, vp, i32, vp, u64, u64, vp, vp, vp]
    L.grlbwt_fm_mems.argtypes = [vp, vp, vp, i32, vp, u64, u64, u64, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_match_info_get.argtypes = [vp, C.POINTER(MatchInfo)]
    L.grlbwt_fm_approx.argtypes = [vp, vp, vp, i32, vp, u64, C.c_uint32, u64, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_approx_info_get.argtypes = [vp, C.POINTER(ApproxInfo)]
    L.grlbwt_fm_overlaps.argtypes = [vp, vp, vp, i32, vp, u64, u64, u64, C.c_uint32, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_overlaps_of.argtypes = [vp, vp, vp, u64, u64, u64, C.c_uint32, vp, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_overlap_targets.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_overlap_info_get.argtypes = [vp, C.POINTER(OverlapInfo)]
    L.grlbwt_fm_lcp.argtypes = [vp, vp, u64, i32, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_lcp_info_get.argtypes = [vp, C.POINTER(LcpInfo)]
    L.grlbwt_fm_sa.argtypes = [vp, vp, u64, u64, i32, vp, i32, vp]
    L.grlbwt_fm_sa_info_get.argtypes = [vp, C.POINTER(SaInfo)]
    L.grlbwt_fm_kmers.argtypes = [vp, vp, u64, u64, u64, u64, u64, i32, vp, vp, vp, u64, C.POINTER(u64), vp, u64]
    L.grlbwt_fm_kmer_info_get.argtypes = [vp, C.POINTER(KmerInfo)]
    L.grlbwt_fm_kmers_canonical.argtypes = [vp, vp, u64, u64, u64, u64, u64, vp, u64, i32, vp, vp, vp, vp, vp, u64, C.POINTER(u64), vp, u64]
    L.grlbwt_fm_kmers_canonical_info_get.argtypes = [vp, C.POINTER(CkmerInfo)]
    L.grlbwt_fm_repeats.argtypes = [vp, vp, u64, u64, u64, u64, C.c_uint32, u64, u64, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_fm_repeat_info_get.argtypes = [vp, C.POINTER(RepeatInfo)]
    L.grlbwt_docs_create.argtypes = [vp, vp, C.c_uint32, C.POINTER(vp)]
    L.grlbwt_docs_destroy.argtypes = [vp, vp]
    L.grlbwt_docs_info_get.argtypes = [vp, C.POINTER(DocsInfo)]
    L.grlbwt_docs_count.argtypes = [vp, vp, vp, vp, u64, vp, C.POINTER(u64)]
    L.grlbwt_docs_list.argtypes = [vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
    L.grlbwt_debruijn_create.argtypes = [vp, vp, u64, u64, u64, C.c_uint32, C.POINTER(vp)]
    L.grlbwt_debruijn_destroy.argtypes = [vp, vp]
    L.grlbwt_debruijn_info_get.argtypes = [vp, C.POINTER(DeBruijnInfo)]
    L.grlbwt_debruijn_nodes.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, u64]
    L.grlbwt_debruijn_edges.argtypes = [vp, vp, vp, vp, vp, vp, u64]
    L.grlbwt_debruijn_unitigs.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, u64, u64, u64]
    L.grlbwt_cdebruijn_create.argtypes = [vp, vp, u64, u64, u64, vp, u64, C.c_uint32, C.POINTER(vp)]
    L.grlbwt_cdebruijn_destroy.argtypes = [vp, vp]
    L.grlbwt_cdebruijn_info_get.argtypes = [vp, C.POINTER(CDeBruijnInfo)]
    L.grlbwt_cdebruijn_nodes.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, u64]
    L.grlbwt_cdebruijn_links.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64]
    L.grlbwt_cdebruijn_unitigs.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, u64, u64, u64]
    L.grlbwt_merge_create.argtypes = [vp, vp, u64, vp, u64, i32, u64, C.POINTER(vp)]
    L.grlbwt_merge_info_get.argtypes = [vp, C.POINTER(MergeInfo)]
    L.grlbwt_merge_emit.argtypes = [vp, vp, vp, u64]
    L.grlbwt_merge_interleave.argtypes = [vp, vp, vp]
    L.grlbwt_merge_destroy.argtypes = [vp, vp]
    L.grlbwt_merge_files.argtypes = [vp, C.c_char_p, C.c_char_p, i32, u64, C.c_char_p, C.POINTER(MergeInfo)]
    L.grlbwt_select_create.argtypes = [vp, vp, u64, i32, vp, u64, C.c_uint32, C.POINTER(vp)]
    L.grlbwt_select_info_get.argtypes = [vp, C.POINTER(SelectInfo)]
    L.grlbwt_select_emit.argtypes = [vp, vp, vp, u64]
    L.grlbwt_select_rows.argtypes = [vp, vp, vp]
    L.grlbwt_select_destroy.argtypes = [vp, vp]
    L.grlbwt_select_files.argtypes = [vp, C.c_char_p, vp, u64, i32, C.c_uint32, C.c_char_p, C.POINTER(SelectInfo)]
    L.grlbwt_profile_enable.argtypes = [vp, i32]
    L.grlbwt_profile_dump.argtypes = [vp, C.c_char_p, u64]
    _libs[path] = L
    return L


class Context:
    """One engine context per GPU (grlbwt_ctx)."""

    def __init__(self, device=0, flags=0, lib=None, _test_standin=False):
        self.L = load_library(lib, allow_test_standin=_test_standin)
        h = C.c_void_p()
        rc = self.L.grlbwt_ctx_create(device, flags, C.byref(h))
        if rc != OK:
            raise GrlbwtError(rc, self.L.grlbwt_strerror(rc).decode())
        self._h = h
        self._keep = None

    def _ck(self, rc):
        if rc != OK:
            msg = self.L.grlbwt_last_error(self._h).decode() or self.L.grlbwt_strerror(rc).decode()
            if rc == EILLFORMED:
                raise IllFormedInput(rc, msg)
            if rc == ENOTDNA:
                raise NotDNA(rc, msg)
            raise GrlbwtError(rc, msg)

    def close(self):
        if getattr(self, "_h", None):
            self.L.grlbwt_ctx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- input ----------------------------------------------------------
    def set_stream(self, hip_stream):
        self._ck(self.L.grlbwt_ctx_set_stream(self._h, C.c_void_p(hip_stream)))

    def upload(self, data, cell_bytes=1):
        """collection_stats + first-round input from a host buffer (bytes / numpy)."""
        import numpy as np
        buf = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview))
                                   else np.asarray(data).view(np.uint8).reshape(-1))
        self._keep = buf
        self._ck(self.L.grlbwt_text_upload(self._h, buf.ctypes.data_as(C.c_void_p), len(buf) // cell_bytes, cell_bytes))

    def load_file(self, path, cell_bytes=1):
        """collection_stats + first-round input straight from a file of raw cells (pinned, overlapped upload)."""
        self._keep = None
        self._ck(self.L.grlbwt_text_load_file(self._h, os.fsencode(path), cell_bytes))

    def load_fastx(self, path, rev_comp=False):
        """FASTA/FASTQ (optionally gzip) -> the one-string-per-line text in HBM (fastx2plain_format of the reference);
        returns the number of strings."""
        self._keep = None
        n = C.c_uint64(0)
        self._ck(self.L.grlbwt_text_load_fastx(self._h, os.fsencode(path), FASTX_REVCOMP if rev_comp else 0, C.byref(n)))
        return n.value

    def fastx_convert(self, src_ptr, n_in, rev_comp, dst_ptr, capacity):
        """The conversion alone, device buffer to device buffer: (bytes written, n_strings)."""
        n_out, n_str = C.c_uint64(0), C.c_uint64(0)
        self._ck(self.L.grlbwt_fastx_convert_device(self._h, C.c_void_p(src_ptr), n_in, FASTX_REVCOMP if rev_comp else 0, C.c_void_p(dst_ptr),
                                                    capacity, C.byref(n_out), C.byref(n_str)))
        return n_out.value, n_str.value

    def attach_device(self, dev_ptr, n_cells, cell_bytes=1, keepalive=None):
        """Use cells already resident in HBM (e.g. a torch tensor's data_ptr())."""
        self._keep = keepalive
        self._ck(self.L.grlbwt_text_attach_device(self._h, C.c_void_p(dev_ptr), n_cells, cell_bytes))

    def stats(self):
        s = Stats()
        self._ck(self.L.grlbwt_get_stats(self._h, C.byref(s)))
        return _as_dict(s)

    def alphabet_size(self):
        """Distinct values of a text that was compacted when it was loaded (a symbol of 2^30 - 8 or more); 0: not compacted."""
        n = C.c_uint64()
        self._ck(self.L.grlbwt_alphabet_size(self._h, C.byref(n)))
        return n.value

    def alphabet_download(self):
        """The sorted distinct values of a compacted text: rank r of the stage-wise inspection stands for values[r]."""
        import numpy as np
        out = np.zeros(self.alphabet_size(), dtype=np.uint64)
        self._ck(self.L.grlbwt_alphabet_download(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def alphabet_compact(self, src_ptr, n_cells, cell_bytes, ranks_ptr, values_ptr, capacity_values):
        """The compaction alone, device buffer to device buffer: ranks (uint32 per cell) and sorted distinct values (uint64);
        returns their number."""
        k = C.c_uint64(0)
        self._ck(self.L.grlbwt_alphabet_compact_device(self._h, C.c_void_p(src_ptr), n_cells, cell_bytes, C.c_void_p(ranks_ptr),
                                                       C.c_void_p(values_ptr), capacity_values, C.byref(k)))
        return k.value

    # ---- phases (names follow the reference) -----------------------------
    def parse_round(self):
        info, done = RoundInfo(), C.c_int()
        self._ck(self.L.grlbwt_parse_round(self._h, C.byref(info), C.byref(done)))
        return _as_dict(info), bool(done.value)

    def par_phase(self):
        n = C.c_int()
        self._ck(self.L.grlbwt_parse_phase(self._h, C.byref(n)))
        return n.value

    def round_info(self, r):
        info = RoundInfo()
        self._ck(self.L.grlbwt_round_info_get(self._h, r, C.byref(info)))
        return _as_dict(info)

    def parse2bwt(self):
        self._ck(self.L.grlbwt_induce_first(self._h))

    def infer_lvl_bwt(self):
        lvl, info = C.c_int(), LevelInfo()
        self._ck(self.L.grlbwt_induce_level(self._h, C.byref(lvl), C.byref(info)))
        return lvl.value, _as_dict(info)

    def ind_phase(self):
        self._ck(self.L.grlbwt_induce_phase(self._h))

    def level_info(self, lvl):
        info = LevelInfo()
        self._ck(self.L.grlbwt_level_info_get(self._h, lvl, C.byref(info)))
        return _as_dict(info)

    def build(self):
        """grl_bwt_algo: par_phase + ind_phase on the loaded text."""
        self._ck(self.L.grlbwt_build(self._h))

    # ---- output -----------------------------------------------------------
    def result_size(self):
        nb, nr = C.c_uint64(), C.c_uint64()
        self._ck(self.L.grlbwt_result_size(self._h, C.byref(nb), C.byref(nr)))
        return nb.value, nr.value

    def result_device_ptr(self):
        p = C.c_void_p()
        self._ck(self.L.grlbwt_result_device_ptr(self._h, C.byref(p)))
        return p.value

    def result_part(self):
        """(offset, bytes) of what this context holds of the image: all of it, or this rank's part (collection-level build
        with dist.COMM_KEEP_PARTS)."""
        off, nb = C.c_uint64(), C.c_uint64()
        self._ck(self.L.grlbwt_result_part(self._h, C.byref(off), C.byref(nb)))
        return off.value, nb.value

    def result_bytes(self):
        """The image bytes this context holds (result_part)."""
        _, nb = self.result_part()
        out = (C.c_uint8 * max(nb, 1))()
        self._ck(self.L.grlbwt_result_download(self._h, out, nb))
        return bytes(out)[:nb]

    def write_file(self, path):
        self._ck(self.L.grlbwt_result_write_file(self._h, os.fsencode(path)))

    def write_part(self, path):
        """This context's part at its offset of `path` (created if missing, never truncated)."""
        self._ck(self.L.grlbwt_result_write_part(self._h, os.fsencode(path)))

    # ---- inspection --------------------------------------------------------
    def level_text(self, lvl):
        import numpy as np
        n = C.c_uint64()
        self._ck(self.L.grlbwt_level_text_size(self._h, lvl, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint64)
        self._ck(self.L.grlbwt_level_text_download(self._h, lvl, out.ctypes.data_as(C.c_void_p)))
        return out

    def level_bwt(self, lvl):
        import numpy as np
        n = C.c_uint64()
        self._ck(self.L.grlbwt_level_bwt_size(self._h, lvl, C.byref(n)))
        s = np.zeros(n.value, dtype=np.uint64)
        l = np.zeros(n.value, dtype=np.uint64)
        self._ck(self.L.grlbwt_level_bwt_download(self._h, lvl, s.ctypes.data_as(C.c_void_p), l.ctypes.data_as(C.c_void_p)))
        return s, l

    def level_grammar(self, lvl):
        """(g0, g1, has_hocc, prebwt_sym, prebwt_len) of a level that has been parsed and not yet induced."""
        import numpy as np
        m, p = C.c_uint64(), C.c_uint64()
        self._ck(self.L.grlbwt_level_grammar_size(self._h, lvl, C.byref(m), C.byref(p)))
        g0 = np.zeros(m.value, dtype=np.uint64); g1 = np.zeros(m.value, dtype=np.uint64); hh = np.zeros(m.value, dtype=np.uint8)
        ps = np.zeros(p.value, dtype=np.uint64); pl = np.zeros(p.value, dtype=np.uint64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self._ck(self.L.grlbwt_level_grammar_download(self._h, lvl, ptr(g0), ptr(g1), ptr(hh), ptr(ps), ptr(pl)))
        return g0, g1, hh, ps, pl

    def counters(self):
        c = Counters()
        self._ck(self.L.grlbwt_get_counters(self._h, C.byref(c)))
        return _as_dict(c)

    def invert_image(self, dev_image_ptr, image_bytes, cell_bytes, dev_out_ptr, capacity_cells):
        """reverse_bwt on the device: .rl_bwt image (device) -> the collection's cells (device); returns #cells."""
        n = C.c_uint64()
        self._ck(self.L.grlbwt_invert_image(self._h, C.c_void_p(dev_image_ptr), image_bytes, cell_bytes,
                                            C.c_void_p(dev_out_ptr), capacity_cells, C.byref(n)))
        return n.value

    def invert_image_checkpointed(self, dev_image_ptr, image_bytes, cell_bytes, dev_out_ptr, capacity_cells, sample_bits=0):
        """invert_image for collections of long strings: the LF walks cut at checkpoint rows, one in 2^sample_bits (0: the
        default); returns (#cells, the walk's counters)."""
        n, info = C.c_uint64(), WalkInfo()
        self._ck(self.L.grlbwt_invert_image_checkpointed(self._h, C.c_void_p(dev_image_ptr), image_bytes, cell_bytes, sample_bits,
                                                         C.c_void_p(dev_out_ptr), capacity_cells, C.byref(n), C.byref(info)))
        return n.value, _as_dict(info)

    def invert_image_tails(self, dev_image_ptr, image_bytes, cell_bytes, tail_cells, dev_out_ptr, capacity_cells):
        """The last `tail_cells` cells of every string (slot i of the output: string i's end, right-aligned); returns
        (strings, cells written)."""
        k, n = C.c_uint64(), C.c_uint64()
        self._ck(self.L.grlbwt_invert_image_tails(self._h, C.c_void_p(dev_image_ptr), image_bytes, cell_bytes, tail_cells,
                                                  C.c_void_p(dev_out_ptr), capacity_cells, C.byref(k), C.byref(n)))
        return k.value, n.value

    def image_plain(self, dev_image_ptr, image_bytes, dev_out_ptr, capacity, null_char=-1):
        """grl2plain on the device (scripts/grl2plain.cpp): plain BWT bytes; returns their number."""
        n = C.c_uint64()
        self._ck(self.L.grlbwt_image_plain(self._h, C.c_void_p(dev_image_ptr), image_bytes, C.c_void_p(dev_out_ptr), capacity,
                                           null_char, C.byref(n)))
        return n.value

    def image_rle(self, dev_image_ptr, image_bytes, dev_syms_ptr, dev_lens_ptr, capacity_runs):
        """grlbwt2rle on the device (scripts/grlbwt2rle.cpp): uint8 symbols + uint32 lengths; returns #runs."""
        n = C.c_uint64()
        self._ck(self.L.grlbwt_image_rle(self._h, C.c_void_p(dev_image_ptr), image_bytes, C.c_void_p(dev_syms_ptr),
                                         C.c_void_p(dev_lens_ptr), capacity_runs, C.byref(n)))
        return n.value

    def image_stats(self, dev_image_ptr, image_bytes):
        """bwt_stats on the device (scripts/bwt_stats.cpp)."""
        st = ImageStats()
        self._ck(self.L.grlbwt_image_stats_get(self._h, C.c_void_p(dev_image_ptr), image_bytes, C.byref(st)))
        d = {k: int(getattr(st, k)) for k in ("n_runs", "sigma", "text_size", "min_run", "max_run", "fit1", "fit2", "fit3")}
        d["runs_of"] = list(st.runs_of); d["freq_of"] = list(st.freq_of); d["deciles"] = list(st.deciles)
        d["non_maximal"] = int(st.non_maximal)
        return d

    def image_split_runs(self, dev_image_ptr, image_bytes, bits, block_size, dev_out_ptr, capacity_bytes):
        """split_runs on the device (scripts/split_runs.cpp): the re-encoded image lands in dev_out; returns the counters."""
        si = SplitInfo()
        self._ck(self.L.grlbwt_image_split_runs(self._h, C.c_void_p(dev_image_ptr), image_bytes, bits, block_size,
                                                C.c_void_p(dev_out_ptr), capacity_bytes, C.byref(si)))
        return _as_dict(si)

    def merge_files(self, path_a, path_b, path_out, cell_bytes=1, max_rounds=0):
        """The images in two files merged into the image of "A's strings, then B's", written to path_out; returns the merge's
        counters (ImageMerge.info)."""
        mi = MergeInfo()
        self._ck(self.L.grlbwt_merge_files(self._h, os.fsencode(path_a), os.fsencode(path_b), cell_bytes, max_rounds,
                                           os.fsencode(path_out), C.byref(mi)))
        return _as_dict(mi)

    def select_files(self, path_in, ids, path_out, cell_bytes=1, keep=False, checkpoints=False, sample_bits=0):
        """The image in a file without the strings whose numbers `ids` lists -- or with those alone (keep=True) -- written to
        path_out; returns the selection's counters (ImageSelect.info)."""
        import numpy as np
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.uint64).reshape(-1))
        si = SelectInfo()
        self._ck(self.L.grlbwt_select_files(self._h, os.fsencode(path_in), ids.ctypes.data_as(C.c_void_p), len(ids), cell_bytes,
                                            select_flags(keep, checkpoints, sample_bits), os.fsencode(path_out), C.byref(si)))
        return _as_dict(si)

    def memory_usage(self):
        a, b = C.c_uint64(), C.c_uint64()
        self._ck(self.L.grlbwt_memory_usage(self._h, C.byref(a), C.byref(b)))
        return {"peak_live_bytes": a.value, "reserved_bytes": b.value}

    def profile_enable(self, on=True):
        self._ck(self.L.grlbwt_profile_enable(self._h, 1 if on else 0))

    def profile(self):
        """{kernel name: (launches, total_ms, stated algorithmic bytes)} measured with HIP events on the engine's stream."""
        buf = C.create_string_buffer(1 << 17)
        self._ck(self.L.grlbwt_profile_dump(self._h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, cnt, ms, nbytes = line.rsplit(" ", 3)
            out[name] = (int(cnt), float(ms), int(nbytes))
        return out

    def selftest(self, n=100000, seed=1):
        return self.L.grlbwt_selftest(self._h, n, seed)


class FmIndex:
    """Count and locate patterns in an .rl_bwt image (grlbwt_fm_*): an index made from an image in device memory, which may
    be freed afterwards.  All pointers are device pointers; locate=True also builds what locate() needs, checkpoints=True
    (with locate) the samples that bound a locate walk by 2^sample_bits steps (0: the default) whatever the strings' lengths,
    extract=True (with locate) what extract() and string_lengths() need: the index then stands in for the text."""

    def __init__(self, ctx, dev_image_ptr, image_bytes, locate=False, checkpoints=False, sample_bits=0, extract=False):
        self.ctx = ctx
        h = C.c_void_p()
        if not 0 <= sample_bits <= 255:
            raise GrlbwtError(-22, "sample_bits is 0 or 1 to 20")
        flags = (FM_LOCATE if locate else 0) | (FM_CHECKPOINTS if checkpoints else 0) | (FM_EXTRACT if extract else 0) | (sample_bits << 8)
        ctx._ck(ctx.L.grlbwt_fm_create(ctx._h, C.c_void_p(dev_image_ptr), image_bytes, flags, C.byref(h)))
        self._h = h

    def walk_info(self):
        """The counters of the checkpointed walks that made this index (an index without checkpoints: GrlbwtError)."""
        out = WalkInfo()
        rc = self.ctx.L.grlbwt_fm_walk_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def info(self):
        out = FmInfo()
        rc = self.ctx.L.grlbwt_fm_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def count(self, cells_ptr, cell_bytes, offsets_ptr, n, lo_ptr, hi_ptr):
        """Rows [lo[i], hi[i]) of the BWT whose suffixes start with pattern i = cells [offsets[i], offsets[i + 1])."""
        self.ctx._ck(self.ctx.L.grlbwt_fm_count(self.ctx._h, self._h, C.c_void_p(cells_ptr), cell_bytes, C.c_void_p(offsets_ptr), n,
                                                C.c_void_p(lo_ptr), C.c_void_p(hi_ptr)))

    def locate(self, rows_ptr, n_rows, max_steps, string_ptr, offset_ptr):
        """(string, offset) of every row; UINT64_MAX in both where the offset is above max_steps."""
        self.ctx._ck(self.ctx.L.grlbwt_fm_locate(self.ctx._h, self._h, C.c_void_p(rows_ptr), n_rows, max_steps,
                                                 C.c_void_p(string_ptr), C.c_void_p(offset_ptr)))

    def string_lengths(self, len_ptr):
        """The length of every string, its separator included (n_strings uint64 words)."""
        self.ctx._ck(self.ctx.L.grlbwt_fm_string_lengths(self.ctx._h, self._h, C.c_void_p(len_ptr)))

    def extract(self, string_ptr, begin_ptr, end_ptr, n, cell_bytes, out_ptr, capacity_cells, offsets_ptr):
        """Cells [begin[i], min(end[i], length)) of string[i] for n ranges, back to back in out; offsets[i] = the first cell of
        range i, offsets[n] = the number of cells, which is returned.  UINT64_MAX as an end: to the end of the string."""
        got = C.c_uint64()
        self.ctx._ck(self.ctx.L.grlbwt_fm_extract(self.ctx._h, self._h, C.c_void_p(string_ptr), C.c_void_p(begin_ptr), C.c_void_p(end_ptr),
                                                  n, cell_bytes, C.c_void_p(out_ptr), capacity_cells, C.c_void_p(offsets_ptr), C.byref(got)))
        return got.value

    def extract_info(self):
        """The counters of the last extract() on this index (an index made without extract=True: GrlbwtError)."""
        out = ExtractInfo()
        rc = self.ctx.L.grlbwt_fm_extract_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def match(self, cells_ptr, cell_bytes, offsets_ptr, n, max_len, len_ptr, lo_ptr=None, hi_ptr=None):
        """For every cell of the n patterns (given as to count()) the length of the longest piece ending there that occurs
        inside one string, at most max_len (0: no cap); lo / hi, both or neither, receive the rows of that piece.  A cell that
        is no symbol, or the separator, gets 0."""
        self.ctx._ck(self.ctx.L.grlbwt_fm_match(self.ctx._h, self._h, C.c_void_p(cells_ptr), cell_bytes, C.c_void_p(offsets_ptr), n, max_len,
                                                C.c_void_p(len_ptr), C.c_void_p(lo_ptr), C.c_void_p(hi_ptr)))

    def mems(self, cells_ptr, cell_bytes, offsets_ptr, n, min_len, max_len, pattern_ptr, begin_ptr, mlen_ptr, capacity, lo_ptr=None,
             hi_ptr=None):
        """The maximal exact matches of at least min_len cells (lengths capped by max_len, 0: no cap) as (pattern, begin, length
        [, lo, hi]) in ascending (pattern, end) order; their number is returned.  More than `capacity`: GrlbwtError whose
        n_mems attribute is that number, and nothing is written."""
        got = C.c_uint64()
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_mems(self.ctx._h, self._h, C.c_void_p(cells_ptr), cell_bytes, C.c_void_p(offsets_ptr), n, min_len,
                                                   max_len, C.c_void_p(pattern_ptr), C.c_void_p(begin_ptr), C.c_void_p(mlen_ptr),
                                                   C.c_void_p(lo_ptr), C.c_void_p(hi_ptr), capacity, C.byref(got)))
        except GrlbwtError as e:
            e.n_mems = got.value
            raise
        return got.value

    def match_info(self):
        """The counters of the last match() or mems() on this index."""
        out = MatchInfo()
        rc = self.ctx.L.grlbwt_fm_match_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def approx(self, cells_ptr, cell_bytes, offsets_ptr, n, max_mismatches, max_hits, hit_offsets_ptr, mism_ptr, lo_ptr, hi_ptr,
               capacity, sub_pos_ptr=None, sub_val_ptr=None):
        """Every occurrence of the n patterns (given as to count()) with at most max_mismatches (0 to 3) substituted cells: the
        hits of pattern i are entries [hit_offsets[i], hit_offsets[i + 1]) of (mism, lo, hi), in the order of the search (at a
        cell, from the last one on: the other symbols ascending, then the pattern's own); max_hits cuts each list (0: no cap).
        sub_pos / sub_val, both or neither, receive max_mismatches words per entry: the substituted offsets in descending order
        and the substitutes, UINT64_MAX in unused slots.  The number of hits is returned.  More than `capacity`: GrlbwtError
        whose n_hits attribute is that number, and nothing is written."""
        got = C.c_uint64()
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_approx(self.ctx._h, self._h, C.c_void_p(cells_ptr), cell_bytes, C.c_void_p(offsets_ptr), n,
                                                     max_mismatches, max_hits, C.c_void_p(hit_offsets_ptr), C.c_void_p(mism_ptr),
                                                     C.c_void_p(lo_ptr), C.c_void_p(hi_ptr), C.c_void_p(sub_pos_ptr), C.c_void_p(sub_val_ptr),
                                                     capacity, C.byref(got)))
        except GrlbwtError as e:
            e.n_hits = got.value
            raise
        return got.value

    def approx_info(self):
        """The counters of the last approx() on this index; hits_by_mismatches as a list of four."""
        out = ApproxInfo()
        rc = self.ctx.L.grlbwt_fm_approx_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        d = _as_dict(out)
        d["hits_by_mismatches"] = [int(v) for v in out.hits_by_mismatches]
        return d

    def overlaps(self, cells_ptr, cell_bytes, offsets_ptr, n, min_len, max_len, flags, hit_offsets_ptr, len_ptr, tlo_ptr, thi_ptr, capacity,
                 lo_ptr=None, hi_ptr=None):
        """Which strings of the collection begin with a suffix of the n patterns (given as to count()): the hits of pattern i are
        entries [hit_offsets[i], hit_offsets[i + 1]) of (len = L, [tlo, thi)) in ascending L, max(min_len, 1) <= L <=
        min(the pattern's cells, max_len if not 0); [tlo, thi) are prefix ranks, which overlap_targets() turns into string
        numbers.  flags: FM_OVERLAP_PROPER leaves out L = the whole pattern.  lo / hi, both or neither, receive the rows of the
        suffix.  The number of hits is returned.  More than `capacity`: GrlbwtError whose n_hits attribute is that number, and
        nothing is written."""
        got = C.c_uint64()
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_overlaps(self.ctx._h, self._h, C.c_void_p(cells_ptr), cell_bytes, C.c_void_p(offsets_ptr), n,
                                                       min_len, max_len, flags, C.c_void_p(hit_offsets_ptr), C.c_void_p(len_ptr),
                                                       C.c_void_p(tlo_ptr), C.c_void_p(thi_ptr), C.c_void_p(lo_ptr), C.c_void_p(hi_ptr),
                                                       capacity, C.byref(got)))
        except GrlbwtError as e:
            e.n_hits = got.value
            raise
        return got.value

    def overlaps_of(self, ids_ptr, n, min_len, max_len, flags, hit_offsets_ptr, len_ptr, tlo_ptr, thi_ptr, capacity, lo_ptr=None, hi_ptr=None):
        """overlaps() with strings of the collection as the queries, by number (n uint64 words; an index made with locate=True):
        their cells are read from the index itself."""
        got = C.c_uint64()
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_overlaps_of(self.ctx._h, self._h, C.c_void_p(ids_ptr), n, min_len, max_len, flags,
                                                          C.c_void_p(hit_offsets_ptr), C.c_void_p(len_ptr), C.c_void_p(tlo_ptr),
                                                          C.c_void_p(thi_ptr), C.c_void_p(lo_ptr), C.c_void_p(hi_ptr), capacity, C.byref(got)))
        except GrlbwtError as e:
            e.n_hits = got.value
            raise
        return got.value

    def overlap_targets(self, tlo_ptr, thi_ptr, n, entry_offsets_ptr, string_ptr, capacity, range_ptr=None):
        """The string numbers behind n ranges of prefix ranks (an index made with locate=True): the entries of range r are
        [entry_offsets[r], entry_offsets[r + 1]) of string, in ascending rank; range_ptr (optional) receives r per entry.  The
        number of entries is returned.  More than `capacity`: GrlbwtError whose n_entries attribute is that number, and nothing
        is written."""
        got = C.c_uint64()
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_overlap_targets(self.ctx._h, self._h, C.c_void_p(tlo_ptr), C.c_void_p(thi_ptr), n,
                                                              C.c_void_p(entry_offsets_ptr), C.c_void_p(string_ptr), C.c_void_p(range_ptr),
                                                              capacity, C.byref(got)))
        except GrlbwtError as e:
            e.n_entries = got.value
            raise
        return got.value

    def overlap_info(self):
        """The counters of the last overlaps(), overlaps_of() or overlap_targets() on this index."""
        out = OverlapInfo()
        rc = self.ctx.L.grlbwt_fm_overlap_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    LCP_HIST_FIRST = 1 << 20      # levels the histograms of lcp() are first sized for, where the cap and the rows allow more

    def lcp(self, max_lcp=0, lcp_bytes=4, lcp_ptr=None, want_hist=True):
        """The LCP array of the collection: n_syms values of lcp_bytes bytes (1, 2, 4, 8) into lcp_ptr (None: no array), each
        min(LCP, cap) with cap = min(max_lcp if not 0, 2^(8 * lcp_bytes) - 1).  With want_hist returns (rows_at, suffixes_of),
        numpy uint64 arrays of n_levels entries: rows_at[l] = the rows whose value is exactly l, suffixes_of[l] = the suffixes
        of exactly l cells (distinct_kmers() takes both); without it (None, None).  The histograms are sized for the most levels the
        cap and the number of rows allow, which the call accepts at once; above LCP_HIST_FIRST by the idiom of mems(): that
        capacity first, then the number of levels the refusal reports."""
        import numpy as np
        L, got = self.ctx.L, C.c_uint64()
        if not want_hist:
            self.ctx._ck(L.grlbwt_fm_lcp(self.ctx._h, self._h, max_lcp, lcp_bytes, C.c_void_p(lcp_ptr), None, None, 0, C.byref(got)))
            return None, None
        lim = 2 ** (8 * lcp_bytes) - 1 if lcp_bytes in (1, 2, 4) else UINT64_MAX
        cap = max(1, min(min(max_lcp, lim) if max_lcp else lim, self.info()["n_syms"] + 1, self.LCP_HIST_FIRST))
        while True:
            rows_at, suffixes_of = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
            rc = L.grlbwt_fm_lcp(self.ctx._h, self._h, max_lcp, lcp_bytes, C.c_void_p(lcp_ptr), rows_at.ctypes.data_as(C.c_void_p),
                                 suffixes_of.ctypes.data_as(C.c_void_p), cap, C.byref(got))
            if rc != OK and got.value > cap:
                cap = got.value
                continue
            self.ctx._ck(rc)
            return rows_at[:got.value].copy(), suffixes_of[:got.value].copy()

    def lcp_info(self):
        """The counters of the last lcp() on this index."""
        out = LcpInfo()
        rc = self.ctx.L.grlbwt_fm_lcp_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def suffix_array(self, row_begin=0, row_end=None, string_bytes=4, string_ptr=None, offset_bytes=4, offset_ptr=None):
        """The document array and the generalized suffix array of rows [row_begin, row_end) (None: to the last row): entry
        p - row_begin of string_ptr / offset_ptr receives the string and the offset locate() reports for row p, as values of
        string_bytes / offset_bytes bytes (1, 2, 4, 8).  Either pointer may be None, not both.  An index made with locate=True;
        with checkpoints=True one walk per checkpoint segment, else one per string.  The window bounds the output, not the work."""
        self.ctx._ck(self.ctx.L.grlbwt_fm_sa(self.ctx._h, self._h, row_begin, UINT64_MAX if row_end is None else row_end, string_bytes,
                                             C.c_void_p(string_ptr), offset_bytes, C.c_void_p(offset_ptr)))

    def sa_info(self):
        """The counters of the last suffix_array() that succeeded on this index."""
        out = SaInfo()
        rc = self.ctx.L.grlbwt_fm_sa_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def kmers_raw(self, k, min_count=1, max_count=0, row_begin=0, row_end=None, cell_bytes=1, cells_ptr=None, lo_ptr=None, count_ptr=None,
                  capacity=0, spectrum=None):
        """grlbwt_fm_kmers as it is: device pointers (None: not wanted) for the table's cells (k values of cell_bytes bytes per
        entry), lo and count (uint64 per entry), room for `capacity` entries; spectrum: a numpy uint64 array to fill, or None.
        Returns the number of entries.  More than `capacity` with an array given: GrlbwtError whose n_kmers attribute is that
        number, and nothing is written."""
        got = C.c_uint64()
        sp = spectrum.ctypes.data_as(C.c_void_p) if spectrum is not None else None
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_kmers(self.ctx._h, self._h, k, min_count, max_count, row_begin,
                                                    UINT64_MAX if row_end is None else row_end, cell_bytes, C.c_void_p(cells_ptr),
                                                    C.c_void_p(lo_ptr), C.c_void_p(count_ptr), capacity, C.byref(got), sp,
                                                    0 if spectrum is None else len(spectrum)))
        except GrlbwtError as e:
            e.n_kmers = got.value
            raise
        return got.value

    def kmers(self, k, min_count=1, max_count=0, rows=None, cells=True, cell_bytes=None):
        """The distinct k-mers of the collection with max(min_count, 1) <= count <= max_count (0: no bound) whose first row lo
        lies in rows = (begin, end) (None: all rows), in ascending lo = lexicographic order: (lo, count, cells) as numpy arrays,
        cells of shape (n, k) holding the symbol values (None with cells=False).  [lo, lo + count) is what count() answers for
        the cells.  cell_bytes None: the narrowest width that holds the index's largest symbol, found by trying.  Sized by the idiom
        of mems(): one call that reports the number, one that fills the table."""
        import numpy as np
        on_device = self.ctx.L.grlbwt_backend_name() == b"hip-gfx950"      # (the test stand-in's "device" is host memory)
        if on_device:
            import torch

        def room(nbytes):
            if on_device:
                t = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                return t, t.data_ptr()
            a = np.zeros(max(nbytes, 8), dtype=np.uint8)
            return a, a.ctypes.data

        def back(buf, nbytes):
            if on_device:
                torch.cuda.synchronize()
                return buf.cpu().numpy()[:nbytes].copy()
            return buf[:nbytes].copy()

        rb, re = (0, None) if rows is None else rows
        widths = (1, 2, 4, 8) if cell_bytes is None and cells else (cell_bytes or 1,)
        n = self.kmers_raw(k, min_count, max_count, rb, re)
        (lo, plo), (cnt, pcnt) = room(8 * n), room(8 * n)
        for i, w in enumerate(widths):
            out, pout = room(n * k * w) if cells else (None, None)
            try:
                got = self.kmers_raw(k, min_count, max_count, rb, re, w, pout, plo, pcnt, n)
                break
            except GrlbwtError as e:
                if e.code != -22 or i + 1 == len(widths) or "does not fit" not in str(e):
                    raise
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[w]
        tab = back(out, got * k * w).view(dt).reshape(got, k) if cells else None
        return back(lo, 8 * got).view(np.uint64), back(cnt, 8 * got).view(np.uint64), tab

    def kmer_spectrum(self, k, bins=256):
        """The abundance spectrum: a numpy uint64 array s of `bins` entries (1 to 16384), s[c] = the distinct k-mers of the whole
        collection that occur exactly c times, the last bin holding every count >= bins - 1.  Its sum is the number of distinct
        k-mers."""
        import numpy as np
        s = np.zeros(bins, dtype=np.uint64)
        self.kmers_raw(k, spectrum=s)
        return s

    def kmer_info(self):
        """The counters of the last kmers() / kmer_spectrum() on this index that got as far as counting."""
        out = KmerInfo()
        rc = self.ctx.L.grlbwt_fm_kmer_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    @staticmethod
    def _pairs(pairs):
        """The complement map as grlbwt_fm_kmers_canonical takes it: (array of 2 * n_pairs uint64 or None, n_pairs).  pairs: None
        (the DNA default), a sequence of (a, b) ints, or bytes such as b"ATCG" read pairwise."""
        if pairs is None:
            return None, 0
        if isinstance(pairs, (bytes, bytearray)):
            if len(pairs) % 2:
                raise ValueError("pairs given as bytes are read pairwise: an even number of them")
            flat = list(pairs)
        else:
            flat = [int(v) for ab in pairs for v in ab]
            if len(flat) != 2 * len(pairs):
                raise ValueError("pairs: a sequence of (a, b)")
        return (C.c_uint64 * max(len(flat), 1))(*flat), len(flat) // 2

    def canonical_kmers_raw(self, k, min_count=1, max_count=0, row_begin=0, row_end=None, pairs=None, cell_bytes=1, cells_ptr=None, lo_ptr=None,
                            count_ptr=None, mate_lo_ptr=None, total_ptr=None, capacity=0, spectrum=None):
        """grlbwt_fm_kmers_canonical as it is: device pointers (None: not wanted) for the table's cells (k values of cell_bytes
        bytes per entry), lo, count, mate_lo and total (uint64 per entry), room for `capacity` entries; pairs as _pairs() reads
        them; spectrum: a numpy uint64 array to fill, or None.  Returns the number of entries (classes).  More than `capacity`
        with an array given: GrlbwtError whose n_classes attribute is that number, and nothing is written."""
        got = C.c_uint64()
        sp = spectrum.ctypes.data_as(C.c_void_p) if spectrum is not None else None
        arr, n_pairs = self._pairs(pairs)
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_kmers_canonical(
                self.ctx._h, self._h, k, min_count, max_count, row_begin, UINT64_MAX if row_end is None else row_end,
                None if arr is None else C.cast(arr, C.c_void_p), n_pairs, cell_bytes, C.c_void_p(cells_ptr), C.c_void_p(lo_ptr),
                C.c_void_p(count_ptr), C.c_void_p(mate_lo_ptr), C.c_void_p(total_ptr), capacity, C.byref(got), sp,
                0 if spectrum is None else len(spectrum)))
        except GrlbwtError as e:
            e.n_classes = got.value
            raise
        return got.value

    def canonical_kmers(self, k, min_count=1, max_count=0, rows=None, pairs=None, cells=True, cell_bytes=None):
        """The strand-merged k-mers: one entry per class {x, rc(x)} of the k-mers that occur, under the complement map `pairs`
        (None: DNA, (A,T), (C,G); a sequence of (a, b) values; or bytes read pairwise), with max(min_count, 1) <= total <=
        max_count (0: no bound) whose representative's first row lo lies in rows = (begin, end) (None: all rows), in ascending
        lo: (lo, count, mate_lo, total, cells) as numpy arrays.  lo, count and cells are the representative's own, as kmers()
        gives them; mate_lo is the lo of the other member (the entry's own for a palindrome, UINT64_MAX when there is none) and
        total the sum of both counts.  cells=False: None for the cells.  Sized by the idiom of kmers()."""
        import numpy as np
        on_device = self.ctx.L.grlbwt_backend_name() == b"hip-gfx950"      # (the test stand-in's "device" is host memory)
        if on_device:
            import torch

        def room(nbytes):
            if on_device:
                t = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                return t, t.data_ptr()
            a = np.zeros(max(nbytes, 8), dtype=np.uint8)
            return a, a.ctypes.data

        def back(buf, nbytes):
            if on_device:
                torch.cuda.synchronize()
                return buf.cpu().numpy()[:nbytes].copy()
            return buf[:nbytes].copy()

        rb, re = (0, None) if rows is None else rows
        widths = (1, 2, 4, 8) if cell_bytes is None and cells else (cell_bytes or 1,)
        n = self.canonical_kmers_raw(k, min_count, max_count, rb, re, pairs)
        cols = [room(8 * n) for _ in range(4)]
        for i, w in enumerate(widths):
            out, pout = room(n * k * w) if cells else (None, None)
            try:
                got = self.canonical_kmers_raw(k, min_count, max_count, rb, re, pairs, w, pout, cols[0][1], cols[1][1], cols[2][1], cols[3][1], n)
                break
            except GrlbwtError as e:
                if e.code != -22 or i + 1 == len(widths) or "does not fit" not in str(e):
                    raise
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[w]
        tab = back(out, got * k * w).view(dt).reshape(got, k) if cells else None
        lo, cnt, mate, tot = (back(b, 8 * got).view(np.uint64) for b, _ in cols)
        return lo, cnt, mate, tot, tab

    def canonical_kmer_spectrum(self, k, bins=256, pairs=None):
        """The abundance spectrum of the strand-merged k-mers: s[c] = the classes of the whole collection whose total is exactly
        c, the last bin holding every total >= bins - 1.  Its sum is the number of classes."""
        import numpy as np
        s = np.zeros(bins, dtype=np.uint64)
        self.canonical_kmers_raw(k, pairs=pairs, spectrum=s)
        return s

    def canonical_kmer_info(self):
        """The counters of the last canonical_kmers() / canonical_kmer_spectrum() on this index that got as far as counting."""
        out = CkmerInfo()
        rc = self.ctx.L.grlbwt_fm_kmers_canonical_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def repeats_raw(self, min_len=1, max_len=0, min_count=2, max_count=0, flags=0, row_begin=0, row_end=None, lo_ptr=None, count_ptr=None,
                    len_ptr=None, split_ptr=None, capacity=0):
        """grlbwt_fm_repeats as it is: device pointers (None: not wanted) for lo, count, len and split (uint64 per entry), room for
        `capacity` entries.  Returns the number of entries.  More than `capacity` with an array given: GrlbwtError whose n_repeats
        attribute is that number, and nothing is written."""
        got = C.c_uint64()
        try:
            self.ctx._ck(self.ctx.L.grlbwt_fm_repeats(self.ctx._h, self._h, min_len, max_len, min_count, max_count, flags, row_begin,
                                                      UINT64_MAX if row_end is None else row_end, C.c_void_p(lo_ptr), C.c_void_p(count_ptr),
                                                      C.c_void_p(len_ptr), C.c_void_p(split_ptr), capacity, C.byref(got)))
        except GrlbwtError as e:
            e.n_repeats = got.value
            raise
        return got.value

    def repeats(self, min_len=1, max_len=0, min_count=2, max_count=0, maximal=False, rows=None, split=False):
        """The right-maximal repeats of the collection (maximal=True: those that are left-maximal too) with max(min_len, 1) <= length
        <= max_len (0: no bound) and max(min_count, 2) <= count <= max_count (0: no bound) whose split row lies in rows = (begin, end)
        (None: all rows), in ascending split row: (lo, count, length) as numpy uint64 arrays, with split=True (lo, count, length,
        split).  [lo, lo + count) are the rows count() answers for the repeat's cells.  Sized by the idiom of mems(): one call that
        reports the number, one that fills the table."""
        import numpy as np
        on_device = self.ctx.L.grlbwt_backend_name() == b"hip-gfx950"      # (the test stand-in's "device" is host memory)
        if on_device:
            import torch
        rb, re = (0, None) if rows is None else rows
        flags = FM_REPEATS_MAXIMAL if maximal else 0
        n = self.repeats_raw(min_len, max_len, min_count, max_count, flags, rb, re)
        bufs = []
        for _ in range(4 if split else 3):
            if on_device:
                t = torch.zeros(max(8 * n, 8), dtype=torch.uint8, device="cuda:0")
                bufs.append((t, t.data_ptr()))
            else:
                a = np.zeros(max(8 * n, 8), dtype=np.uint8)
                bufs.append((a, a.ctypes.data))
        if on_device:
            torch.cuda.synchronize()
        got = self.repeats_raw(min_len, max_len, min_count, max_count, flags, rb, re, bufs[0][1], bufs[1][1], bufs[2][1],
                               bufs[3][1] if split else None, n)
        if on_device:
            torch.cuda.synchronize()
        return tuple((b.cpu().numpy() if on_device else b)[:8 * got].copy().view(np.uint64) for b, _ in bufs)

    def repeat_info(self):
        """The counters of the last repeats() on this index that got as far as counting."""
        out = RepeatInfo()
        rc = self.ctx.L.grlbwt_fm_repeat_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def documents(self, occurrences=False):
        """An FmDocs handle: which strings lie behind row ranges, and how many (an index made with locate=True).  occurrences=True
        also keeps what list() needs to count every document's occurrences.  The handle holds no pointer into this index."""
        return FmDocs(self, occurrences)

    def de_bruijn(self, k, min_count=1, max_count=0):
        """A DeBruijn handle: the compacted de Bruijn graph of the k-mers with max(min_count, 1) <= count <= max_count (0: no
        bound) -- the nodes of kmers(k, min_count, max_count), the edges between them, the degrees and the unitigs.  The handle
        holds no pointer into this index; only the cells of the unitigs read it again."""
        return DeBruijn(self, k, min_count, max_count)

    def de_bruijn_canonical(self, k, min_count=1, max_count=0, pairs=None):
        """A CanonicalDeBruijn handle: the strand-merged (bidirected) compacted de Bruijn graph -- the nodes of
        canonical_kmers(k, min_count, max_count, pairs=pairs), the half-edges between their ends and the unitigs as one reading
        each.  pairs is that of canonical_kmers.  The handle holds no pointer into this index; only the cells read it again."""
        return CanonicalDeBruijn(self, k, min_count, max_count, pairs)

    @staticmethod
    def distinct_kmers(rows_at, suffixes_of, k=None):
        """The number of distinct k-mers (windows of k cells that hold no separator) from the histograms of lcp(): the rows with
        an LCP below k less the suffixes of fewer than k cells.  k None: the list c with c[k] for 1 <= k <= n_levels (c[0] is
        0); beyond n_levels the passes did not get that far: ValueError."""
        import numpy as np
        n_levels = len(rows_at)
        if len(suffixes_of) != n_levels:
            raise ValueError("the two histograms differ in length")
        c = np.concatenate([[0], np.cumsum(np.asarray(rows_at, dtype=np.int64)) - np.cumsum(np.asarray(suffixes_of, dtype=np.int64))])
        if k is None:
            return [int(v) for v in c]
        if not 1 <= k <= n_levels:
            raise ValueError("k = %d is outside 1 .. n_levels = %d: the passes did not get that far" % (k, n_levels))
        return int(c[k])

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self.ctx, "_h", None):       # (a closed context has released its indexes)
            self.ctx._ck(self.ctx.L.grlbwt_fm_destroy(self.ctx._h, h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FmDocs:
    """The strings behind row ranges of an FM index (grlbwt_docs_*): the documents of a range [lo, hi) are the distinct strings of
    its rows, reported in ascending first row.  All pointers are device pointers to uint64 words.  Made by FmIndex.documents();
    the index may be closed before the handle."""

    def __init__(self, fm, occurrences=False):
        self.ctx = fm.ctx
        h = C.c_void_p()
        self.ctx._ck(self.ctx.L.grlbwt_docs_create(self.ctx._h, fm._h, DOCS_OCCURRENCES if occurrences else 0, C.byref(h)))
        self._h = h

    def count(self, lo_ptr, hi_ptr, n, ndocs_ptr):
        """ndocs[r] = the number of documents of range r = [lo[r], hi[r]), for n ranges; their sum is returned."""
        got = C.c_uint64()
        self.ctx._ck(self.ctx.L.grlbwt_docs_count(self.ctx._h, self._h, C.c_void_p(lo_ptr), C.c_void_p(hi_ptr), n, C.c_void_p(ndocs_ptr),
                                                  C.byref(got)))
        return got.value

    def list(self, lo_ptr, hi_ptr, n, entry_offsets_ptr, string_ptr, capacity, first_row_ptr=None, occ_ptr=None, range_ptr=None):
        """The documents of range r are entries [entry_offsets[r], entry_offsets[r + 1]) of string (and, optional, first_row, occ,
        range), in ascending first row.  occ needs a handle made with occurrences=True.  The number of entries is returned.
        More than `capacity`: GrlbwtError whose n_entries attribute is that number, and nothing is written."""
        got = C.c_uint64()
        try:
            self.ctx._ck(self.ctx.L.grlbwt_docs_list(self.ctx._h, self._h, C.c_void_p(lo_ptr), C.c_void_p(hi_ptr), n,
                                                     C.c_void_p(entry_offsets_ptr), C.c_void_p(string_ptr), C.c_void_p(first_row_ptr),
                                                     C.c_void_p(occ_ptr), C.c_void_p(range_ptr), capacity, C.byref(got)))
        except GrlbwtError as e:
            e.n_entries = got.value
            raise
        return got.value

    def info(self):
        """The handle, its create, and the counters of the last count() or list() that succeeded on it."""
        out = DocsInfo()
        rc = self.ctx.L.grlbwt_docs_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self.ctx, "_h", None):       # (a closed context has released its handles)
            self.ctx._ck(self.ctx.L.grlbwt_docs_destroy(self.ctx._h, h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeBruijn:
    """The compacted de Bruijn graph of a collection from its FM index (grlbwt_debruijn_*).  Node v is entry v of
    FmIndex.kmers(k, min_count, max_count); the edges are the windows of k + 1 cells between two nodes, in ascending (to, from),
    as the CSR of in-edges; a unitig is a maximal path over edges u -> v with out_degree[u] == in_degree[v] == 1, circular ones
    starting at their smallest node.  The *_raw forms take device pointers (None: not wanted) and capacities; the others size
    themselves from info() and return numpy arrays.  Made by FmIndex.de_bruijn(); the index may be closed before the handle,
    except for unitigs() with cells."""

    def __init__(self, fm, k, min_count=1, max_count=0, flags=0):
        self.ctx, self.fm = fm.ctx, fm
        h = C.c_void_p()
        self.ctx._ck(self.ctx.L.grlbwt_debruijn_create(self.ctx._h, fm._h, k, min_count, max_count, flags, C.byref(h)))
        self._h = h

    def info(self):
        out = DeBruijnInfo()
        rc = self.ctx.L.grlbwt_debruijn_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def nodes_raw(self, lo_ptr=None, count_ptr=None, in_degree_ptr=None, out_degree_ptr=None, unitig_ptr=None, rank_ptr=None, capacity=0):
        """uint64 per node for lo, count, unitig and rank (the node's place inside its unitig), uint32 for the two degrees."""
        self.ctx._ck(self.ctx.L.grlbwt_debruijn_nodes(self.ctx._h, self._h, C.c_void_p(lo_ptr), C.c_void_p(count_ptr), C.c_void_p(in_degree_ptr),
                                                      C.c_void_p(out_degree_ptr), C.c_void_p(unitig_ptr), C.c_void_p(rank_ptr), capacity))

    def edges_raw(self, in_offsets_ptr=None, from_ptr=None, weight_ptr=None, row_ptr=None, capacity=0):
        """in_offsets: n_nodes + 1 uint64; from, weight and row: uint64 per edge, room for `capacity` edges."""
        self.ctx._ck(self.ctx.L.grlbwt_debruijn_edges(self.ctx._h, self._h, C.c_void_p(in_offsets_ptr), C.c_void_p(from_ptr), C.c_void_p(weight_ptr),
                                                      C.c_void_p(row_ptr), capacity))

    def unitigs_raw(self, fm=None, cell_bytes=1, node_offsets_ptr=None, nodes_ptr=None, cells_ptr=None, weight_ptr=None, circular_ptr=None,
                    capacity_unitigs=0, capacity_nodes=0, capacity_cells=0):
        """node_offsets: n_unitigs + 1 uint64; nodes: n_nodes uint64; cells: n_cells values of cell_bytes bytes (needs fm, the
        index the graph was made from); weight: uint64 and circular: a byte per unitig."""
        self.ctx._ck(self.ctx.L.grlbwt_debruijn_unitigs(self.ctx._h, self._h, fm._h if fm is not None else None, cell_bytes,
                                                        C.c_void_p(node_offsets_ptr), C.c_void_p(nodes_ptr), C.c_void_p(cells_ptr),
                                                        C.c_void_p(weight_ptr), C.c_void_p(circular_ptr), capacity_unitigs, capacity_nodes,
                                                        capacity_cells))

    def _rooms(self):
        import numpy as np
        on_device = self.ctx.L.grlbwt_backend_name() == b"hip-gfx950"      # (the test stand-in's "device" is host memory)
        if on_device:
            import torch

        def room(nbytes):
            if on_device:
                t = torch.zeros(max(nbytes, 8), dtype=torch.uint8, device="cuda:0")
                torch.cuda.synchronize()
                return t, t.data_ptr()
            a = np.zeros(max(nbytes, 8), dtype=np.uint8)
            return a, a.ctypes.data

        def back(buf, nbytes, dtype):
            if on_device:
                torch.cuda.synchronize()
                return buf.cpu().numpy()[:nbytes].copy().view(dtype)
            return buf[:nbytes].copy().view(dtype)

        return room, back

    def nodes(self):
        """A dict of numpy arrays: lo, count, unitig, rank (uint64) and in_degree, out_degree (uint32), one entry per node."""
        import numpy as np
        room, back = self._rooms()
        n = self.info()["n_nodes"]
        names = (("lo", 8), ("count", 8), ("in_degree", 4), ("out_degree", 4), ("unitig", 8), ("rank", 8))
        bufs = [room(n * w) for _, w in names]
        self.nodes_raw(*[p for _, p in bufs], capacity=n)
        return {name: back(b, n * w, np.uint64 if w == 8 else np.uint32) for (name, w), (b, _) in zip(names, bufs)}

    def edges(self):
        """(in_offsets, from, weight, row) as numpy uint64 arrays: the in-edges of node v are entries in_offsets[v] .. in_offsets[v + 1]."""
        import numpy as np
        room, back = self._rooms()
        i = self.info()
        n, m = i["n_nodes"], i["n_edges"]
        off, fr, wt, row = room(8 * (n + 1)), room(8 * m), room(8 * m), room(8 * m)
        self.edges_raw(off[1], fr[1], wt[1], row[1], m)
        return back(off[0], 8 * (n + 1), np.uint64), back(fr[0], 8 * m, np.uint64), back(wt[0], 8 * m, np.uint64), back(row[0], 8 * m, np.uint64)

    def unitigs(self, cells=True, cell_bytes=None):
        """A dict of numpy arrays: node_offsets (n_unitigs + 1), nodes (n_nodes), weight and circular per unitig and, with
        cells=True, cells (all unitigs' cells back to back, as symbol values) and cell_offsets (n_unitigs + 1), the closed form
        node_offsets[j] + j * (k - 1).  cell_bytes None: the narrowest width that holds the index's largest symbol, found by trying."""
        import numpy as np
        room, back = self._rooms()
        i = self.info()
        n, u, nc, k = i["n_nodes"], i["n_unitigs"], i["n_cells"], i["k"]
        off, nodes, wt, circ = room(8 * (u + 1)), room(8 * n), room(8 * u), room(u)
        widths = (1, 2, 4, 8) if cell_bytes is None and cells else (cell_bytes or 1,)
        for j, w in enumerate(widths):
            out, pout = room(nc * w) if cells else (None, None)
            try:
                self.unitigs_raw(self.fm if cells else None, w, off[1], nodes[1], pout, wt[1], circ[1], u, n, nc)
                break
            except GrlbwtError as e:
                if e.code != -22 or j + 1 == len(widths) or "does not fit" not in str(e):
                    raise
        res = {"node_offsets": back(off[0], 8 * (u + 1), np.uint64), "nodes": back(nodes[0], 8 * n, np.uint64),
               "weight": back(wt[0], 8 * u, np.uint64), "circular": back(circ[0], u, np.uint8)}
        if cells:
            dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[w]
            res["cells"] = back(out, nc * w, dt)
            res["cell_offsets"] = res["node_offsets"] + np.arange(u + 1, dtype=np.uint64) * np.uint64(max(k, 1) - 1) if nc else np.zeros(u + 1, dtype=np.uint64)
        return res

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self.ctx, "_h", None):       # (a closed context has released its handles)
            self.ctx._ck(self.ctx.L.grlbwt_debruijn_destroy(self.ctx._h, h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

class CanonicalDeBruijn(DeBruijn):
    """The strand-merged compacted de Bruijn graph of a collection from its FM index (grlbwt_cdebruijn_*).  Node v is entry v of
    FmIndex.canonical_kmers(k, min_count, max_count, pairs=pairs); end 2 v is in front of its representative's first cell, end
    2 v + 1 behind its last; the links are the CSR of half-edges over the ends in ascending (source end, other end); a unitig is
    one reading, oriented nodes 2 v + o.  The *_raw forms take device pointers (None: not wanted) and capacities; the others size
    themselves from info() and return numpy arrays.  Made by FmIndex.de_bruijn_canonical(); the index may be closed before the
    handle, except for unitigs() with cells."""

    def __init__(self, fm, k, min_count=1, max_count=0, pairs=None, flags=0):
        self.ctx, self.fm = fm.ctx, fm
        h = C.c_void_p()
        arr, n_pairs = fm._pairs(pairs)
        self.ctx._ck(self.ctx.L.grlbwt_cdebruijn_create(self.ctx._h, fm._h, k, min_count, max_count, None if arr is None else C.cast(arr, C.c_void_p),
                                                        n_pairs, flags, C.byref(h)))
        self._h = h

    def info(self):
        out = CDeBruijnInfo()
        rc = self.ctx.L.grlbwt_cdebruijn_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def nodes_raw(self, lo_ptr=None, count_ptr=None, mate_lo_ptr=None, total_ptr=None, degree0_ptr=None, degree1_ptr=None, unitig_ptr=None,
                  rank_ptr=None, orient_ptr=None, capacity=0):
        """uint64 per node for lo, count, mate_lo, total, unitig and rank, uint32 for the two ends' degrees, a byte for orient."""
        self.ctx._ck(self.ctx.L.grlbwt_cdebruijn_nodes(self.ctx._h, self._h, C.c_void_p(lo_ptr), C.c_void_p(count_ptr), C.c_void_p(mate_lo_ptr),
                                                       C.c_void_p(total_ptr), C.c_void_p(degree0_ptr), C.c_void_p(degree1_ptr),
                                                       C.c_void_p(unitig_ptr), C.c_void_p(rank_ptr), C.c_void_p(orient_ptr), capacity))

    def links_raw(self, end_offsets_ptr=None, other_ptr=None, weight_ptr=None, fwd_row_ptr=None, fwd_count_ptr=None, capacity=0):
        """end_offsets: 2 n_nodes + 1 uint64; other, weight, fwd_row and fwd_count: uint64 per half-edge, room for `capacity`."""
        self.ctx._ck(self.ctx.L.grlbwt_cdebruijn_links(self.ctx._h, self._h, C.c_void_p(end_offsets_ptr), C.c_void_p(other_ptr),
                                                       C.c_void_p(weight_ptr), C.c_void_p(fwd_row_ptr), C.c_void_p(fwd_count_ptr), capacity))

    def edges_raw(self, *a, **kw):
        raise AttributeError("a strand-merged graph has links(), not edges()")

    edges = edges_raw

    def unitigs_raw(self, fm=None, cell_bytes=1, node_offsets_ptr=None, nodes_ptr=None, cells_ptr=None, weight_ptr=None, circular_ptr=None,
                    capacity_unitigs=0, capacity_nodes=0, capacity_cells=0):
        """node_offsets: n_unitigs + 1 uint64; nodes: n_nodes oriented nodes 2 v + o, uint64; cells: n_cells values of cell_bytes
        bytes (needs fm, the index the graph was made from); weight: uint64 and circular: a byte per unitig."""
        self.ctx._ck(self.ctx.L.grlbwt_cdebruijn_unitigs(self.ctx._h, self._h, fm._h if fm is not None else None, cell_bytes,
                                                         C.c_void_p(node_offsets_ptr), C.c_void_p(nodes_ptr), C.c_void_p(cells_ptr),
                                                         C.c_void_p(weight_ptr), C.c_void_p(circular_ptr), capacity_unitigs, capacity_nodes,
                                                         capacity_cells))

    def nodes(self):
        """A dict of numpy arrays, one entry per node: lo, count, mate_lo, total, unitig, rank (uint64), degree0, degree1 (uint32)
        and orient (uint8)."""
        import numpy as np
        room, back = self._rooms()
        n = self.info()["n_nodes"]
        names = (("lo", 8), ("count", 8), ("mate_lo", 8), ("total", 8), ("degree0", 4), ("degree1", 4), ("unitig", 8), ("rank", 8), ("orient", 1))
        bufs = [room(n * w) for _, w in names]
        self.nodes_raw(*[p for _, p in bufs], capacity=n)
        return {name: back(b, n * w, {8: np.uint64, 4: np.uint32, 1: np.uint8}[w]) for (name, w), (b, _) in zip(names, bufs)}

    def links(self):
        """(end_offsets, other, weight, fwd_row, fwd_count) as numpy uint64 arrays: the half-edges of end a = 2 v + e are entries
        end_offsets[a] .. end_offsets[a + 1]."""
        import numpy as np
        room, back = self._rooms()
        i = self.info()
        n, m = i["n_nodes"], i["n_half_edges"]
        off = room(8 * (2 * n + 1))
        cols = [room(8 * m) for _ in range(4)]
        self.links_raw(off[1], *[p for _, p in cols], capacity=m)
        return (back(off[0], 8 * (2 * n + 1), np.uint64),) + tuple(back(b, 8 * m, np.uint64) for b, _ in cols)

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self.ctx, "_h", None):       # (a closed context has released its handles)
            self.ctx._ck(self.ctx.L.grlbwt_cdebruijn_destroy(self.ctx._h, h))



class ImageMerge:
    """The images of collections A and B merged into the image of "A's strings, then B's" (grlbwt_merge_*), without the texts.
    All pointers are device pointers; both images may be freed once the object exists (all rounds have run by then).  Both
    images together may hold at most 256 distinct symbols; the number of rounds is about the longest prefix a suffix of A
    shares with a suffix of B (max_rounds bounds it, 0: no bound of the caller's)."""

    def __init__(self, ctx, a_ptr, a_bytes, b_ptr, b_bytes, cell_bytes, max_rounds=0):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._ck(ctx.L.grlbwt_merge_create(ctx._h, C.c_void_p(a_ptr), a_bytes, C.c_void_p(b_ptr), b_bytes, cell_bytes, max_rounds,
                                          C.byref(h)))
        self._h = h

    def info(self):
        out = MergeInfo()
        rc = self.ctx.L.grlbwt_merge_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def emit(self, out_ptr, capacity_bytes):
        """The merged image into out_ptr (info()["out_bytes"] bytes)."""
        self.ctx._ck(self.ctx.L.grlbwt_merge_emit(self.ctx._h, self._h, C.c_void_p(out_ptr), capacity_bytes))

    def interleave(self, bits_ptr):
        """ceil(n / 64) words: bit p of word p // 64 is set when row p of the merged BWT comes from B."""
        self.ctx._ck(self.ctx.L.grlbwt_merge_interleave(self.ctx._h, self._h, C.c_void_p(bits_ptr)))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self.ctx, "_h", None):       # (a closed context has released its merges)
            self.ctx._ck(self.ctx.L.grlbwt_merge_destroy(self.ctx._h, h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def select_flags(keep=False, checkpoints=False, sample_bits=0):
    if not 0 <= sample_bits <= 255:
        raise GrlbwtError(-22, "sample_bits is 0 or 1 to 20")
    return (SELECT_KEEP if keep else 0) | (SELECT_CHECKPOINTS if checkpoints else 0) | (sample_bits << 8)


class ImageSelect:
    """The image of a collection without the strings `ids` lists -- or, with keep=True, of those strings alone -- from its image,
    without the text (grlbwt_select_*).  All pointers are device pointers; the ids are uint64 string numbers in input order, in any
    order, repeats allowed; the image and the list may be freed once the object exists (the walks have run by then).
    checkpoints=True marks through checkpointed segments, one checkpoint in 2^sample_bits rows (0: the default): the form for
    collections of long strings."""

    def __init__(self, ctx, dev_image_ptr, image_bytes, cell_bytes, dev_ids_ptr, n_ids, keep=False, checkpoints=False, sample_bits=0):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._ck(ctx.L.grlbwt_select_create(ctx._h, C.c_void_p(dev_image_ptr), image_bytes, cell_bytes, C.c_void_p(dev_ids_ptr), n_ids,
                                           select_flags(keep, checkpoints, sample_bits), C.byref(h)))
        self._h = h

    def info(self):
        out = SelectInfo()
        rc = self.ctx.L.grlbwt_select_info_get(self._h, C.byref(out))
        if rc != OK:
            raise GrlbwtError(rc, self.ctx.L.grlbwt_strerror(rc).decode())
        return _as_dict(out)

    def emit(self, out_ptr, capacity_bytes):
        """The image of the remaining strings into out_ptr (info()["out_bytes"] bytes)."""
        self.ctx._ck(self.ctx.L.grlbwt_select_emit(self.ctx._h, self._h, C.c_void_p(out_ptr), capacity_bytes))

    def rows(self, bits_ptr):
        """ceil(n_syms_in / 64) words: bit p of word p // 64 is set when row p of the input BWT lies on a listed string's chain."""
        self.ctx._ck(self.ctx.L.grlbwt_select_rows(self.ctx._h, self._h, C.c_void_p(bits_ptr)))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h and getattr(self.ctx, "_h", None):       # (a closed context has released its selections)
            self.ctx._ck(self.ctx.L.grlbwt_select_destroy(self.ctx._h, h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def grl_bwt_algo(data, cell_bytes=1, device=0, flags=0, lib=None):
    """Bytes of the .rl_bwt the reference would write for `data` (grl_bwt.hpp:23-79)."""
    with Context(device, flags, lib) as ctx:
        ctx.upload(data, cell_bytes)
        ctx.build()
        return ctx.result_bytes()
