"""ctypes binding of libsa_hip.so (include/sa_hip.h, include/suffix_array.h).

The library is built in-tree by ``hpc_suffix_array_amd/csrc/Makefile`` into
``hpc_suffix_array_amd/lib/libsa_hip.so``.  Loading it never touches the GPU;
every compute entry point fails loudly (SAError) when no HIP device is
present -- there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "lib", "libsa_hip.so")
# A/B runs of build variants point SA_LIB_PATH at another in-tree build
LIB_PATH = os.environ.get("SA_LIB_PATH", LIB_PATH)
CSRC = os.path.join(PKG_DIR, "csrc")

SA_MAX_ROUNDS = 64
KERNEL_KINDS = ["init", "hist_first", "hist_keys", "scan", "scatter_first", "scatter_keys",
                "heads", "heads_scan", "rerank", "seg_count", "seg_scan", "seg_write", "alphabet", "pack",
                "sort_u", "windows", "local_sort", "pivot_keys", "pivot_count", "pivot_write"]
SCHEDULE_PACKED = 0
SCHEDULE_REFERENCE = 1
ROUND1_AUTO = 0
ROUND1_LSD = 1
ROUND1_BUCKETED = 2
SA_K_COUNT = len(KERNEL_KINDS)
# sa_find_device flags (include/sa_hip.h SA_FIND_*) and the auto mode's length
# threshold: patterns of up to FIND_LANE_MAX bytes are searched one per lane,
# longer ones one per wavefront
FIND_AUTO = 0
FIND_LANE = 1
FIND_WAVE = 2
FIND_LANE_MAX = 3584
FIND_MODES = {"auto": FIND_AUTO, "lane": FIND_LANE, "wave": FIND_WAVE}
# sa_bwt statistics (include/sa_hip.h SA_BWT_STATS): uint64 words [0] primary,
# [1] runs, [2 + c] count of byte c; BWT_TILE: the ranks one workgroup of the
# BWT kernel handles per iteration (csrc/sa_bwt.h kBwtTile)
BWT_STATS = 258
BWT_TILE = 4096
# sa_locate flags (include/sa_hip.h SA_LOCATE_*) and the tile of the locate
# kernel: output slots per tile = the largest query sorted in LDS (csrc/
# sa_locate.h kLocateTile); LOCATE_SMALL_CHUNKS cuts the large class's radix
# sort into chunks of 2^14 hits (tests)
LOCATE_SA_ORDER = 1
LOCATE_SMALL_CHUNKS = 2
LOCATE_TILE = 2048
LOCATE_ORDERS = {"text": 0, "sa": LOCATE_SA_ORDER}
# sa_mems (include/sa_hip.h SA_MEM_*): the info words ([0] total MEMs, [1]
# candidates, [2] skipped positions), the positive status of a call stopped by
# max_candidates, and the flags that force one right-extension path
MEM_INFO = 3
MEM_TOO_MANY = 1
MEM_LANE = 1
MEM_WAVE = 2
MEM_MODES = {"auto": 0, "lane": MEM_LANE, "wave": MEM_WAVE}
# sa_lpf / sa_lz77 (include/sa_hip.h SA_LPF_NONE): "no earlier occurrence" in a
# uint32 SRC array or phrase source (-1 in the int64 arrays of the Python
# interface); LZ_TILE: the ranks / positions one workgroup handles (csrc/
# sa_lz.h kLzTile)
LPF_NONE = 0xFFFFFFFF
LZ_TILE = 4096
# sa_repeats (include/sa_hip.h SA_REP_*): the kinds, nested (supermaximal within
# maximal within right-maximal), and the info words ([0] repeats listed, [1]
# the sum of hi - lo over them, the pos_cap of sa_locate_device)
REP_RIGHT = 0
REP_MAXIMAL = 1
REP_SUPERMAXIMAL = 2
REP_KINDS = {"right": REP_RIGHT, "maximal": REP_MAXIMAL, "supermaximal": REP_SUPERMAXIMAL}
REP_INFO = 2
# sa_ibwt (include/sa_hip.h SA_IBWT_INFO): the info words ([0] splitters, [1]
# the longest stretch of the chain between two splitters, [2] the steps from
# LF[primary] until the primary row); LF_TILE: the ranks per row of the LF
# count table; IBWT_S: one rank in IBWT_S is a splitter; IBWT_TILE: the ranks
# one workgroup's splitters come from (csrc/sa_ibwt.h kLfTile, kIbwtSplitBits,
# kIbwtTile)
IBWT_INFO = 3
LF_TILE = 32768
IBWT_S = 64
IBWT_TILE = 16384
# sa_fm (include/sa_hip.h SA_FM_INFO, SA_FM_MAX_SAMPLE): the info words of the
# build ([0] sigma, [1] the class, [2] the bytes of the index, [3] the samples);
# FM_ROWS: the BWT bytes per rank block of the three classes (up to 4, up to 16,
# more distinct bytes; csrc/sa_fm.h fm_rows); FM_MAX_SAMPLE: the largest
# sa_sample; FM_HEADER: the bytes of the index's header
FM_INFO = 4
FM_ROWS = (64, 256, 4096)
FM_MAX_SAMPLE = 4096
FM_HEADER = 4096
# collections (include/sa_hip.h SA_DOC_*): "no document" of sa_doc_of (-1 in the
# int64 arrays of the Python interface), the flag that leaves a listing in rank
# order, and the class boundaries of csrc/sa_docs.h: DOC_TILE ranks per chunk of
# a long interval (kDocTile), DOC_GROUP_MAX the longest interval one lane group
# counts (kDocGroupMax), DOC_LDS_DOCS the most documents whose boundaries are
# searched in LDS (kDocLdsDocs)
DOC_NONE = 0xFFFFFFFF
DOC_RANK_ORDER = 1
DOC_TILE = 2048
DOC_GROUP_MAX = 256
DOC_LDS_DOCS = 8192
DOC_ORDERS = {"doc": 0, "rank": DOC_RANK_ORDER}
# longest common extensions (include/sa_hip.h SA_LCE_*): the minimum of no rank
# (-1 in the int64 arrays of the Python interface), the text bytes the position
# forms compare before they ask ISA, LCP and the index (csrc/sa_lce.h
# kLceProbe), the ranks per block and per superblock of the index (kLceBlock,
# kLceSuper) and the bytes of its header
LCE_NONE = 0xFFFFFFFF
LCE_PROBE = 16
LCE_BLOCK = 64
LCE_SUPER = 4096
LCE_HEADER = 4096
# sa_hamming (include/sa_hip.h SA_HAMMING_*): the largest budget k, the info
# words ([0] total occurrences, [1] candidates, [2] pieces searched), the
# positive status of a call stopped by max_candidates, the flags that force one
# verify path, and the longest pattern a lane verifies in auto mode (csrc/
# sa_hamming.h kHamLaneBytes)
HAMMING_MAX_K = 255
HAMMING_INFO = 3
HAMMING_TOO_MANY = 1
HAMMING_LANE = 1
HAMMING_WAVE = 2
HAMMING_MODES = {"auto": 0, "lane": HAMMING_LANE, "wave": HAMMING_WAVE}
HAMMING_LANE_BYTES = 8192
# sa_edit (include/sa_hip.h SA_EDIT_*): the largest budget k (the band of
# 2k + 1 diagonals fits a 64-bit word), the info words ([0] total ends, [1]
# candidates, [2] pieces) and the positive status of a call stopped by
# max_candidates
EDIT_MAX_K = 31
EDIT_INFO = 3
EDIT_TOO_MANY = 1

# every symbol include/*.h declares
DROPIN_SYMBOLS = ["create_suffix_array", "destroy_suffix_array", "build_suffix_array",
                  "build_lcp_array", "find_longest_repeated_substring", "is_valid_suffix_array"]
EXT_SYMBOLS = ["sa_context_create", "sa_context_destroy", "sa_context_set_debug", "sa_workspace_bytes", "sa_build_device",
               "sa_build_ex", "sa_check_device", "sa_check", "sa_lcp_device", "sa_lcp", "sa_generate_text_device",
               "sa_alphabet_device", "sa_pack_keys_device", "sa_sort_pairs_device", "sa_scatter_u64_device",
               "sa_gather_u64_device", "sa_running_max_i64_device", "sa_inclusive_sum_i64_device",
               "sa_count_below_u64_device", "sa_select_u8_device",
               "sa_find_device", "sa_find", "sa_find_ex",
               "sa_match_device", "sa_matching_stats_device", "sa_match", "sa_matching_stats",
               "sa_bwt_device", "sa_bwt", "sa_inverse_device", "sa_inverse",
               "sa_locate_device", "sa_locate",
               "sa_mems_device", "sa_mems",
               "sa_lpf_device", "sa_lpf", "sa_lz77_device", "sa_lz77",
               "sa_repeats_device", "sa_repeats",
               "sa_lf_device", "sa_ibwt_device", "sa_lf", "sa_ibwt", "sa_ibwt_ex",
               "sa_fm_index_bytes", "sa_fm_build_device", "sa_fm_count_device", "sa_fm_locate_device",
               "sa_fm_build", "sa_fm_count", "sa_fm_locate",
               "sa_doc_array_device", "sa_doc_of_device", "sa_doc_frequency_device", "sa_doc_list_device",
               "sa_doc_array", "sa_doc_of", "sa_doc_frequency", "sa_doc_list",
               "sa_lce_index_bytes", "sa_lce_build_device", "sa_lcp_min_device", "sa_lce_device",
               "sa_substr_compare_device", "sa_lcp_min", "sa_lce", "sa_substr_compare",
               "sa_hamming_device", "sa_hamming",
               "sa_edit_device", "sa_edit",
               "sa_dist_begin", "sa_dist_cuts", "sa_dist_plan_cuts", "sa_dist_reserve", "sa_dist_release", "sa_dist_round1", "sa_dist_req_count", "sa_dist_req_fill",
               "sa_dist_answer", "sa_dist_refine",
               "sa_last_error", "sa_host_syncs", "sa_device_count", "sa_version", "sa_struct_size"]


class SAError(RuntimeError):
    """A libsa_hip entry point returned an error code."""


# sa_opts.debug flags (include/sa_hip.h SA_DEBUG_*): alternative paths the
# tests force; every combination gives the same suffix array
DEBUG_FLAGS = {"no_cmp": 0x1, "no_pk8": 0x2, "no_pad": 0x4, "pad_overflow": 0x8, "no_fast32": 0x10,
               "no_pivot": 0x20, "perm_always": 0x40, "no_xq": 0x80, "xq_overflow": 0x100,
               "no_tied": 0x200, "no_key1_round": 0x400, "no_eonly": 0x800,
               "eonly": 0x1000, "fast32_small": 0x2000, "no_round2_fused": 0x4000,
               "ls_one_wg": 0x8000, "no_alpha_sample": 0x10000, "alpha_sample_small": 0x20000,
               "bb17": 0x40000, "bb18": 0x80000}


def debug_bits(names) -> int:
    bits = 0
    for x in names or ():
        if x not in DEBUG_FLAGS:
            raise ValueError(f"unknown debug flag {x!r} (one of {sorted(DEBUG_FLAGS)})")
        bits |= DEBUG_FLAGS[x]
    return bits


class SaOpts(ctypes.Structure):
    _fields_ = [("profile", ctypes.c_int32), ("schedule", ctypes.c_int32), ("init_chars", ctypes.c_int32),
                ("radix", ctypes.c_int32), ("round1", ctypes.c_int32), ("debug", ctypes.c_uint32),
                ("span_extra", ctypes.c_int32), ("tune", ctypes.c_int32)]


class SaStats(ctypes.Structure):
    _fields_ = [
        ("rounds", ctypes.c_int32),
        ("n_kinds", ctypes.c_int32),
        ("total_ms", ctypes.c_double),
        ("h2d_ms", ctypes.c_double),
        ("d2h_ms", ctypes.c_double),
        ("round_ms", ctypes.c_double * SA_MAX_ROUNDS),
        ("distinct", ctypes.c_uint64 * SA_MAX_ROUNDS),
        ("passes", ctypes.c_int32 * SA_MAX_ROUNDS),
        ("sorted_n", ctypes.c_uint64 * SA_MAX_ROUNDS),
        ("prefix_len", ctypes.c_uint64 * SA_MAX_ROUNDS),
        ("schedule", ctypes.c_int32),
        ("init_chars", ctypes.c_int32),
        ("sigma", ctypes.c_int32),
        ("sparse_ranks", ctypes.c_int32),
        ("round1", ctypes.c_int32),
        ("largest_window", ctypes.c_int32),
        ("model_bytes", ctypes.c_uint64),
        ("kern_ms", ctypes.c_double * SA_K_COUNT),
        ("kern_launches", ctypes.c_uint64 * SA_K_COUNT),
        ("kern_bytes", ctypes.c_uint64 * SA_K_COUNT),
        ("round1_segments", ctypes.c_int32),
        ("round1_layout", ctypes.c_int32),
        ("round_bytes", ctypes.c_uint64 * SA_MAX_ROUNDS),
        ("round1_windows", ctypes.c_int32 * 4),
        ("alphabet", ctypes.c_int32),
    ]

    def to_dict(self) -> dict:
        r = self.rounds
        return {
            "rounds": r,
            "total_ms": self.total_ms,
            "h2d_ms": self.h2d_ms,
            "d2h_ms": self.d2h_ms,
            "round_ms": list(self.round_ms[:r]),
            "distinct": [int(x) for x in self.distinct[:r]],
            "passes": list(self.passes[:r]),
            "sorted_n": [int(x) for x in self.sorted_n[:r]],
            "prefix_len": [int(x) for x in self.prefix_len[:r]],
            "schedule": "reference" if self.schedule == SCHEDULE_REFERENCE else "packed",
            "init_chars": self.init_chars,
            "sigma": self.sigma,
            "sparse_ranks": bool(self.sparse_ranks),
            "round1": {ROUND1_LSD: "lsd", ROUND1_BUCKETED: "bucketed", 3: "pivot"}.get(self.round1, "lsd"),
            "largest_window": self.largest_window,
            "round1_segments": {0: "exact", 1: "padded", 2: "padded-overflow", 3: "striped-records",
                                4: "striped-records-overflow"}.get(self.round1_segments, "exact"),
            "round1_layout": {"compact": bool(self.round1_layout & 1), "pk8": bool(self.round1_layout & 2),
                              "xq": bool(self.round1_layout & 4), "eonly": bool(self.round1_layout & 8)},
            # bucketed round 1: digit bits of the second bucket pass (bucket bits - 8 on one GPU)
            "round1_hb": (self.round1_layout >> 4) & 15,
            "reference_model_bytes": int(self.model_bytes),
            "round_bytes": [int(x) for x in self.round_bytes[:r]],
            # bucketed round 1: non-empty windows, one-bucket windows of the fixed-span kernel, windows
            # sorted again with the measured span, skewed windows (first local-sort launch)
            "round1_windows": [int(x) for x in self.round1_windows],
            # where the dense codes came from: a pass over the text, a sample the first bucket pass
            # proved, or a sample it refuted (the build then ran again with the exact alphabet)
            "alphabet": {0: "exact", 1: "sampled", 2: "refuted"}.get(self.alphabet, "exact"),
            "kernels": {k: {"ms": self.kern_ms[i], "launches": int(self.kern_launches[i]),
                            "bytes": int(self.kern_bytes[i])} for i, k in enumerate(KERNEL_KINDS)},
        }


DIST_OK = 0
DIST_UNSUPPORTED = 1
DIST_UNBALANCED = 2


class SaDistInfo(ctypes.Structure):
    """sa_dist_info of include/sa_hip.h (range-partitioned build, per rank)."""
    _fields_ = [("status", ctypes.c_int32), ("sigma", ctypes.c_int32), ("K", ctypes.c_int32),
                ("bucket_bits", ctypes.c_int32), ("m", ctypes.c_uint64), ("sa_off", ctypes.c_uint64),
                ("m_max", ctypes.c_uint64), ("bucket_lo", ctypes.c_uint32), ("bucket_hi", ctypes.c_uint32),
                ("round1_ok", ctypes.c_int32), ("reserved", ctypes.c_int32), ("heads", ctypes.c_uint64),
                ("unsorted", ctypes.c_uint64), ("groups", ctypes.c_uint64)]


class SuffixArrayStruct(ctypes.Structure):
    """SuffixArray of suffix_array.h:16-21 (32 bytes: str@0 n@8 sa@16 lcp@24)."""
    _fields_ = [("str", ctypes.c_void_p), ("n", ctypes.c_int),
                ("sa", ctypes.POINTER(ctypes.c_int)), ("lcp", ctypes.POINTER(ctypes.c_int))]


_lib = None


def source_hash() -> str:
    """SHA-256 (first 16 hex digits) of the sources libsa_hip.so is built
    from: bench.py stamps it on its line and profiles/summarize.py on each
    rocprof summary, so a summary is matched to the code it measured."""
    import glob
    import hashlib
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(CSRC, "sa_*")) + [os.path.join(CSRC, "Makefile")]
                   + glob.glob(os.path.join(PKG_DIR, "..", "include", "*.h")))
    for p in files:
        with open(p, "rb") as f:
            h.update(os.path.basename(p).encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def build_library(force: bool = False) -> str:
    """Compile libsa_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.run(["make", "-s", "-C", CSRC], check=True)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SAError(f"{LIB_PATH} is missing: run `make -C {CSRC}` (or __graft_entry__.build())")
    L = ctypes.CDLL(LIB_PATH)
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    L.sa_context_create.argtypes = [i32, u64, ctypes.POINTER(vp)]
    L.sa_context_create.restype = i32
    L.sa_context_destroy.argtypes = [vp]
    L.sa_context_destroy.restype = None
    L.sa_context_set_debug.argtypes = [vp, ctypes.POINTER(SaOpts)]
    L.sa_context_set_debug.restype = i32
    L.sa_workspace_bytes.argtypes = [u64]
    L.sa_workspace_bytes.restype = u64
    L.sa_build_device.argtypes = [vp, vp, u64, vp, vp, ctypes.POINTER(SaOpts), ctypes.POINTER(SaStats)]
    L.sa_build_device.restype = i32
    L.sa_build_ex.argtypes = [vp, u64, vp, i32, ctypes.POINTER(SaOpts), ctypes.POINTER(SaStats)]
    L.sa_build_ex.restype = i32
    L.sa_check_device.argtypes = [vp, vp, u64, vp, vp]
    L.sa_check_device.restype = i32
    L.sa_check.argtypes = [vp, u64, vp, i32]
    L.sa_check.restype = i32
    L.sa_lcp_device.argtypes = [vp, vp, u64, vp, vp, ctypes.POINTER(u64), ctypes.POINTER(u64), vp]
    L.sa_lcp_device.restype = i32
    L.sa_lcp.argtypes = [vp, u64, vp, i32, vp, ctypes.POINTER(u64), ctypes.POINTER(u64)]
    L.sa_lcp.restype = i32
    L.sa_alphabet_device.argtypes = [vp, u64, ctypes.POINTER(ctypes.c_uint32), vp]
    L.sa_alphabet_device.restype = i32
    L.sa_pack_keys_device.argtypes = [vp, vp, u64, u64, u64, ctypes.POINTER(ctypes.c_uint16), u64,
                                      ctypes.c_uint32, vp, vp]
    L.sa_pack_keys_device.restype = i32
    L.sa_sort_pairs_device.argtypes = [vp, vp, vp, u64, ctypes.c_uint32, vp, vp, vp]
    L.sa_sort_pairs_device.restype = i32
    L.sa_scatter_u64_device.argtypes = [vp, u64, vp, ctypes.c_int64, vp, u64, vp]
    L.sa_scatter_u64_device.restype = i32
    L.sa_gather_u64_device.argtypes = [vp, vp, u64, vp, ctypes.c_int64, u64, vp]
    L.sa_gather_u64_device.restype = i32
    L.sa_running_max_i64_device.argtypes = [vp, u64, vp]
    L.sa_running_max_i64_device.restype = i32
    L.sa_inclusive_sum_i64_device.argtypes = [vp, u64, vp]
    L.sa_inclusive_sum_i64_device.restype = i32
    L.sa_count_below_u64_device.argtypes = [vp, u64, vp, u64, i32, vp, vp]
    L.sa_count_below_u64_device.restype = i32
    L.sa_select_u8_device.argtypes = [vp, u64, vp, ctypes.POINTER(u64), vp]
    L.sa_select_u8_device.restype = i32
    L.sa_find_device.argtypes = [vp, u64, vp, vp, u64, vp, u64, vp, vp, ctypes.c_uint32, vp]
    L.sa_find_device.restype = i32
    L.sa_find.argtypes = [vp, u64, vp, i32, vp, vp, u64, vp, vp]
    L.sa_find.restype = i32
    L.sa_find_ex.argtypes = [vp, u64, vp, i32, vp, vp, u64, vp, vp, ctypes.c_uint32]
    L.sa_find_ex.restype = i32
    L.sa_match_device.argtypes = [vp, u64, vp, vp, u64, vp, u64, vp, vp, vp, ctypes.c_uint32, vp]
    L.sa_match_device.restype = i32
    L.sa_matching_stats_device.argtypes = [vp, u64, vp, vp, u64, u64, vp, vp, vp, ctypes.c_uint32, vp]
    L.sa_matching_stats_device.restype = i32
    L.sa_match.argtypes = [vp, u64, vp, i32, vp, vp, u64, vp, vp, vp, ctypes.c_uint32]
    L.sa_match.restype = i32
    L.sa_matching_stats.argtypes = [vp, u64, vp, i32, vp, u64, u64, vp, vp, vp, ctypes.c_uint32]
    L.sa_matching_stats.restype = i32
    L.sa_bwt_device.argtypes = [vp, u64, vp, vp, vp, vp]
    L.sa_bwt_device.restype = i32
    L.sa_bwt.argtypes = [vp, u64, vp, i32, vp, vp]
    L.sa_bwt.restype = i32
    L.sa_inverse_device.argtypes = [vp, u64, vp, vp, vp]
    L.sa_inverse_device.restype = i32
    L.sa_inverse.argtypes = [vp, u64, i32, vp]
    L.sa_inverse.restype = i32
    L.sa_locate_device.argtypes = [vp, u64, vp, vp, vp, u64, u64, ctypes.c_uint32, vp, vp, u64, ctypes.POINTER(u64), vp]
    L.sa_locate_device.restype = i32
    L.sa_locate.argtypes = [vp, u64, i32, vp, vp, u64, u64, ctypes.c_uint32, vp, vp, u64]
    L.sa_locate.restype = i32
    L.sa_mems_device.argtypes = [vp, vp, u64, vp, vp, u64, u64, u64, u64, ctypes.c_uint32, vp, vp, vp, u64,
                                 ctypes.POINTER(u64), vp]
    L.sa_mems_device.restype = i32
    L.sa_mems.argtypes = [vp, u64, vp, i32, vp, u64, u64, u64, u64, ctypes.c_uint32, vp, vp, vp, u64,
                          ctypes.POINTER(u64)]
    L.sa_mems.restype = i32
    L.sa_hamming_device.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, u64, u64, ctypes.c_uint32, vp, vp, vp, u64,
                                    ctypes.POINTER(u64), vp]
    L.sa_hamming_device.restype = i32
    L.sa_hamming.argtypes = [vp, u64, vp, i32, vp, vp, u64, u64, u64, ctypes.c_uint32, vp, vp, vp, u64,
                             ctypes.POINTER(u64)]
    L.sa_hamming.restype = i32
    L.sa_edit_device.argtypes = [vp, vp, u64, vp, vp, u64, vp, u64, u64, u64, ctypes.c_uint32, vp, vp, vp, vp, u64,
                                 ctypes.POINTER(u64), vp]
    L.sa_edit_device.restype = i32
    L.sa_edit.argtypes = [vp, u64, vp, i32, vp, vp, u64, u64, u64, ctypes.c_uint32, vp, vp, vp, vp, u64,
                          ctypes.POINTER(u64)]
    L.sa_edit.restype = i32
    L.sa_lpf_device.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp]
    L.sa_lpf_device.restype = i32
    L.sa_lz77_device.argtypes = [vp, u64, vp, vp, vp, vp, vp, u64, ctypes.POINTER(u64), vp]
    L.sa_lz77_device.restype = i32
    L.sa_lpf.argtypes = [vp, u64, vp, i32, vp, vp]
    L.sa_lpf.restype = i32
    L.sa_lz77.argtypes = [vp, u64, vp, i32, vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.sa_lz77.restype = i32
    L.sa_repeats_device.argtypes = [vp, vp, u64, vp, vp, u64, u64, ctypes.c_uint32, vp, vp, vp, u64,
                                    ctypes.POINTER(u64), vp]
    L.sa_repeats_device.restype = i32
    L.sa_repeats.argtypes = [vp, u64, vp, i32, u64, u64, ctypes.c_uint32, vp, vp, vp, u64, ctypes.POINTER(u64)]
    L.sa_repeats.restype = i32
    L.sa_lf_device.argtypes = [vp, vp, u64, u64, vp, vp]
    L.sa_lf_device.restype = i32
    L.sa_ibwt_device.argtypes = [vp, vp, u64, u64, vp, vp, ctypes.POINTER(u64), vp]
    L.sa_ibwt_device.restype = i32
    L.sa_lf.argtypes = [vp, u64, u64, vp, i32]
    L.sa_lf.restype = i32
    L.sa_ibwt.argtypes = [vp, u64, u64, vp, vp, i32]
    L.sa_ibwt.restype = i32
    L.sa_ibwt_ex.argtypes = [vp, u64, u64, vp, vp, i32, ctypes.POINTER(u64)]
    L.sa_ibwt_ex.restype = i32
    u32 = ctypes.c_uint32
    L.sa_fm_index_bytes.argtypes = [u64, u32]
    L.sa_fm_index_bytes.restype = u64
    L.sa_fm_build_device.argtypes = [vp, vp, u64, u64, vp, u32, vp, u64, ctypes.POINTER(u64), vp]
    L.sa_fm_build_device.restype = i32
    L.sa_fm_count_device.argtypes = [vp, u64, vp, u64, vp, u64, vp, vp, vp]
    L.sa_fm_count_device.restype = i32
    L.sa_fm_locate_device.argtypes = [vp, vp, u64, vp, vp, u64, u64, u32, vp, vp, u64, ctypes.POINTER(u64), vp]
    L.sa_fm_locate_device.restype = i32
    L.sa_fm_build.argtypes = [vp, u64, u64, vp, i32, u32, vp, u64, ctypes.POINTER(u64)]
    L.sa_fm_build.restype = i32
    L.sa_fm_count.argtypes = [vp, u64, vp, vp, u64, vp, vp]
    L.sa_fm_count.restype = i32
    L.sa_fm_locate.argtypes = [vp, u64, vp, vp, u64, u64, u32, vp, vp, i32, u64]
    L.sa_fm_locate.restype = i32
    L.sa_doc_array_device.argtypes = [vp, u64, vp, vp, u64, vp, vp, vp]
    L.sa_doc_array_device.restype = i32
    L.sa_doc_of_device.argtypes = [vp, u64, u64, vp, u64, vp, vp, vp]
    L.sa_doc_of_device.restype = i32
    L.sa_doc_frequency_device.argtypes = [u64, vp, vp, vp, u64, vp, vp]
    L.sa_doc_frequency_device.restype = i32
    L.sa_doc_list_device.argtypes = [vp, u64, vp, vp, vp, vp, u64, u64, u32, vp, vp, u64, ctypes.POINTER(u64), vp]
    L.sa_doc_list_device.restype = i32
    L.sa_doc_array.argtypes = [vp, u64, i32, vp, u64, vp, vp]
    L.sa_doc_array.restype = i32
    L.sa_doc_of.argtypes = [vp, u64, u64, vp, u64, i32, vp, vp]
    L.sa_doc_of.restype = i32
    L.sa_doc_frequency.argtypes = [vp, u64, i32, vp, vp, u64, vp]
    L.sa_doc_frequency.restype = i32
    L.sa_doc_list.argtypes = [vp, vp, u64, i32, vp, vp, u64, u64, u32, vp, vp, u64]
    L.sa_doc_list.restype = i32
    L.sa_lce_index_bytes.argtypes = [u64]
    L.sa_lce_index_bytes.restype = u64
    L.sa_lce_build_device.argtypes = [u64, vp, vp, u64, vp]
    L.sa_lce_build_device.restype = i32
    L.sa_lcp_min_device.argtypes = [u64, vp, vp, u64, vp, vp, u64, vp, vp]
    L.sa_lcp_min_device.restype = i32
    L.sa_lce_device.argtypes = [u64, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp]
    L.sa_lce_device.restype = i32
    L.sa_substr_compare_device.argtypes = [u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    L.sa_substr_compare_device.restype = i32
    L.sa_lcp_min.argtypes = [vp, u64, i32, vp, vp, u64, vp]
    L.sa_lcp_min.restype = i32
    L.sa_lce.argtypes = [vp, u64, vp, i32, vp, vp, u64, vp]
    L.sa_lce.restype = i32
    L.sa_substr_compare.argtypes = [vp, u64, vp, i32, vp, vp, vp, vp, u64, vp]
    L.sa_substr_compare.restype = i32
    DI =ctypes.POINTER(SaDistInfo)
    L.sa_dist_begin.argtypes = [vp, vp, u64, i32, i32, ctypes.POINTER(ctypes.c_uint32), vp, vp, DI]
    L.sa_dist_cuts.argtypes = [vp, ctypes.POINTER(u64), DI]
    L.sa_dist_plan_cuts.argtypes = [i32, u64, i32, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_uint32),
                                    ctypes.POINTER(u64)]
    L.sa_dist_release.argtypes = [vp]
    L.sa_dist_reserve.argtypes = [vp, u64, i32]
    L.sa_dist_round1.argtypes = [vp, vp, vp, DI, ctypes.POINTER(SaStats)]
    L.sa_dist_req_count.argtypes = [vp, u64, ctypes.POINTER(u64), vp, DI]
    L.sa_dist_req_fill.argtypes = [vp, u64, vp, vp]
    L.sa_dist_answer.argtypes = [vp, vp, u64, vp, vp]
    L.sa_dist_refine.argtypes = [vp, u64, vp, vp, vp, DI]
    for f in (L.sa_dist_begin, L.sa_dist_cuts, L.sa_dist_plan_cuts, L.sa_dist_reserve, L.sa_dist_release,
              L.sa_dist_round1, L.sa_dist_req_count, L.sa_dist_req_fill,
              L.sa_dist_answer, L.sa_dist_refine):
        f.restype = i32
    L.sa_generate_text_device.argtypes = [vp, u64, u64, ctypes.c_char_p, ctypes.c_uint32, vp]
    L.sa_generate_text_device.restype = i32
    L.sa_last_error.argtypes = []
    L.sa_last_error.restype = ctypes.c_char_p
    L.sa_host_syncs.argtypes = []
    L.sa_host_syncs.restype = ctypes.c_uint64
    L.sa_device_count.argtypes = []
    L.sa_device_count.restype = i32
    L.sa_version.argtypes = []
    L.sa_version.restype = ctypes.c_char_p
    P = ctypes.POINTER(SuffixArrayStruct)
    L.create_suffix_array.argtypes = [ctypes.c_char_p, i32]
    L.create_suffix_array.restype = P
    L.destroy_suffix_array.argtypes = [P]
    L.destroy_suffix_array.restype = None
    L.build_suffix_array.argtypes = [P]
    L.build_suffix_array.restype = None
    L.build_lcp_array.argtypes = [P]
    L.build_lcp_array.restype = None
    L.find_longest_repeated_substring.argtypes = [P]
    L.find_longest_repeated_substring.restype = vp
    L.is_valid_suffix_array.argtypes = [P]
    L.is_valid_suffix_array.restype = i32
    _lib = L
    return L


def check(rc: int, what: str) -> int:
    if rc < 0:
        raise SAError(f"{what}: {lib().sa_last_error().decode(errors='replace')} (code {rc})")
    return rc


def device_count() -> int:
    return lib().sa_device_count()


def require_device() -> None:
    """Fail loudly when the HIP path cannot run (no silent fallback)."""
    if device_count() <= 0:
        raise SAError("no HIP device visible: libsa_hip builds suffix arrays on an MI355X only")
