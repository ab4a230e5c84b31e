"""hpc_suffix_array_amd -- MI355X-native (gfx950 HIP) Manber-Myers suffix-array
construction behind the C ABI of a-rtemis99/hpc_suffix_array
(src/common/suffix_array.h) plus a 64-bit extended ABI (include/sa_hip.h).
"""
from ._native import SAError, build_library, device_count, lib  # noqa: F401
from .builder import (Collection, DeviceBuilder, FMIndex, LCEIndex, SuffixArray, build_suffix_array, bwt,  # noqa: F401
                      check_suffix_array, compare_substrings,
                      count_patterns, doc_of_positions, document_array, document_frequency, edit_search, find_patterns,
                      hamming_search, inverse_bwt,
                      inverse_suffix_array, lcp_array, lcp_range_min, lf_mapping, list_documents,
                      locate_batch,
                      locate_intervals, locate_patterns, longest_common_extension, longest_previous_factor, lz77_factorize,
                      match_patterns, matching_statistics, maximal_exact_matches, maximal_repeats)

__all__ = ["SAError", "DeviceBuilder", "SuffixArray", "build_suffix_array", "check_suffix_array",
           "lcp_array", "find_patterns", "count_patterns", "locate_patterns", "locate_intervals", "locate_batch",
           "match_patterns", "matching_statistics", "maximal_exact_matches", "longest_previous_factor", "lz77_factorize", "maximal_repeats", "bwt", "inverse_suffix_array",
           "lf_mapping", "inverse_bwt", "FMIndex", "document_array", "doc_of_positions", "document_frequency",
           "list_documents", "Collection", "longest_common_extension", "lcp_range_min", "compare_substrings",
           "LCEIndex", "hamming_search", "edit_search", "build_library", "device_count",
           "lib"]
