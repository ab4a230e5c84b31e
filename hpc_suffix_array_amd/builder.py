"""Host-side mirror of the reference's suffix-array interface over libsa_hip.

Reference interface (src/common/suffix_array.h:24-29, manber_myers.c):
    create_suffix_array / build_suffix_array / build_lcp_array /
    find_longest_repeated_substring / is_valid_suffix_array / destroy
``SuffixArray`` below drives exactly those six C symbols of libsa_hip.so
through ctypes (the drop-in boundary), with the same argument meaning and
the same results.  ``build_suffix_array`` / ``check_suffix_array`` use the
64-bit extended ABI (sa_build_ex / sa_check) and ``DeviceBuilder`` the
device-resident one (sa_build_device) that bench.py times.

Nothing here computes a suffix array on the CPU: every path runs the HIP
kernels, and raises SAError when no GPU is visible.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N


def _as_bytes_array(text) -> np.ndarray:
    if isinstance(text, (bytes, bytearray, memoryview)):
        return np.frombuffer(bytes(text), dtype=np.uint8)
    if isinstance(text, str):
        return np.frombuffer(text.encode("latin-1"), dtype=np.uint8)
    return np.ascontiguousarray(text, dtype=np.uint8)


def _sa_array(sa) -> np.ndarray:
    """Contiguous; uint32 / int32 (width 4) as they are, any other dtype as int64 (width 8)."""
    s = np.ascontiguousarray(sa)
    return s if s.dtype in (np.uint32, np.int32, np.int64) else s.astype(np.int64)


def _stream(stream):
    """A HIP stream handle (an int) as the void* of the C side; None: the null stream."""
    return None if stream is None else ctypes.c_void_p(int(stream))


def _find_mode(mode: str) -> int:
    """The SA_FIND_* flags of ``mode``."""
    if mode not in N.FIND_MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(N.FIND_MODES)}")
    return N.FIND_MODES[mode]


SCHEDULES = {"packed": N.SCHEDULE_PACKED, "reference": N.SCHEDULE_REFERENCE}
RADIX = {"onesweep": 0, "reduce_scan": 1}
ROUND1 = {"auto": N.ROUND1_AUTO, "lsd": N.ROUND1_LSD, "bucketed": N.ROUND1_BUCKETED}


def _opts(profile: bool = False, schedule: str = "packed", init_chars: int = 0,
          radix: str = "onesweep", round1: str = "auto", debug=(), span_extra: int = 0,
          tune: int = 0) -> N.SaOpts:
    """sa_opts; ``debug``: names of N.DEBUG_FLAGS (alternative paths the
    tests force), ``span_extra`` / ``tune``: the debug / A/B fields of
    include/sa_hip.h."""
    o = N.SaOpts()
    o.profile = 1 if profile else 0
    o.schedule = SCHEDULES[schedule]
    o.init_chars = int(init_chars)
    o.radix = RADIX[radix]
    o.round1 = ROUND1[round1]
    o.debug = N.debug_bits(debug)
    o.span_extra = int(span_extra)
    o.tune = int(tune)
    return o


def build_suffix_array(text, width: int = 4, profile: bool = False, return_stats: bool = False,
                       schedule: str = "packed", init_chars: int = 0, radix: str = "onesweep",
                       round1: str = "auto", debug=(), span_extra: int = 0, tune: int = 0):
    """Suffix array of ``text`` (bytes / uint8 array), built on the GPU.

    Unsigned-byte order, end of string smallest (== the reference's order on
    its valid domain, manber_myers.c:81-133).  Returns uint32 (width 4) or
    int64 (width 8); with ``return_stats`` also the per-round statistics.
    ``schedule``: "packed" (default; packed K-symbol first round, later rounds
    re-sort unsorted groups only) or "reference" (h = 1, 2, 4, ... over all
    n suffixes, round for round as manber_myers.c:94-125).  ``round1``
    (packed): "auto", "lsd" (full radix sort of the packed first key) or
    "bucketed" (two bucket passes + per-window LDS sort).  ``debug`` /
    ``span_extra`` / ``tune``: forced alternative paths (tests, A/B runs).

    From 2^26 bytes the packed schedule takes the alphabet from a sample of
    the text, and the first bucket pass proves it on every byte
    (``stats["alphabet"]``: "exact", "sampled" or "refuted").  A text with a
    symbol in none of the sampled blocks pays one wasted first and second
    pass before the build runs again with the exact alphabet;
    ``debug=("no_alpha_sample",)`` always scans the whole text instead."""
    t = _as_bytes_array(text)
    n = int(t.size)
    N.require_device()
    out = np.empty(max(n, 1), dtype=np.uint32 if width == 4 else np.int64)
    st = N.SaStats()
    L = N.lib()
    N.check(L.sa_build_ex(t.ctypes.data if n else None, n, out.ctypes.data, width,
                          ctypes.byref(_opts(profile, schedule, init_chars, radix, round1, debug, span_extra, tune)),
                          ctypes.byref(st)),
            "sa_build_ex")
    out = out[:n]
    return (out, st.to_dict()) if return_stats else out


def check_suffix_array(text, sa) -> bool:
    """O(n) GPU validity check (replaces is_valid_suffix_array, :184-202)."""
    t = _as_bytes_array(text)
    s = _sa_array(sa)
    if s.size != t.size:
        return False
    N.require_device()
    width = 8 if s.dtype == np.int64 else 4
    r = N.check(N.lib().sa_check(t.ctypes.data if t.size else None, t.size,
                                 s.ctypes.data if s.size else None, width), "sa_check")
    return bool(r)


def lcp_array(text, sa, width: int = 4):
    """LCP array of a valid suffix array on the GPU plus the longest repeated
    substring (replaces build_lcp_array, manber_myers.c:135-157, and
    find_longest_repeated_substring, :159-182).

    Returns (lcp, lrs) with lcp[0] = 0, lcp[r] = lcp(SA[r-1], SA[r]) as uint32
    (width 4) or int64 (width 8), and lrs = (length, SA position) of the first
    r with the strictly largest lcp ((0, 0) when nothing repeats)."""
    t = _as_bytes_array(text)
    s = _sa_array(sa)
    n = int(t.size)
    if s.size != n:
        raise ValueError(f"SA has {s.size} entries for a text of {n} bytes")
    N.require_device()
    out = np.empty(max(n, 1), dtype=np.uint32 if width == 4 else np.int64)
    ln, pos = ctypes.c_uint64(), ctypes.c_uint64()
    N.check(N.lib().sa_lcp(t.ctypes.data if n else None, n, s.ctypes.data if n else None,
                           8 if s.dtype == np.int64 else 4, out.ctypes.data, ctypes.byref(ln), ctypes.byref(pos)),
            "sa_lcp")
    return out[:n], (int(ln.value), int(pos.value))


def _pack_patterns(patterns):
    """(buffer uint8, offsets uint64 of nq + 1) of a batch of patterns: a
    sequence of bytes / str / uint8 arrays is concatenated; a
    ``(buffer, offsets)`` pair (offsets: an integer numpy array that is not
    uint8, or a list of ints) is taken as it is."""
    if isinstance(patterns, tuple) and len(patterns) == 2:
        o = patterns[1]
        is_off = (isinstance(o, np.ndarray) and o.dtype.kind in "iu" and o.dtype != np.uint8) or (
            isinstance(o, (list, tuple)) and all(isinstance(x, (int, np.integer)) for x in o))
        if is_off:
            off = np.asarray(o)
            if off.ndim != 1 or off.size < 1:
                raise ValueError("pattern offsets: one-dimensional, nq + 1 entries")
            if off.dtype.kind == "i" and (off < 0).any():
                raise ValueError("pattern offsets are negative")
            buf = _as_bytes_array(patterns[0]).reshape(-1)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            if int(off[-1]) > buf.size:
                raise ValueError(f"pattern offsets end at {int(off[-1])}, the buffer holds {buf.size} bytes")
            return buf, off
    if isinstance(patterns, (bytes, bytearray, memoryview, str)):
        raise TypeError("patterns: a sequence of patterns or a (buffer, offsets) pair, not one pattern")
    parts = [_as_bytes_array(p).reshape(-1) for p in patterns]
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
        buf = np.concatenate(parts) if int(off[-1]) else np.zeros(0, np.uint8)
    else:
        buf = np.zeros(0, np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8), off


def _find_host(t_ptr, n: int, sa_ptr, width: int, patterns, mode: str):
    """sa_find_ex over host pointers: (lo, hi) as int64 arrays."""
    flags = _find_mode(mode)
    buf, off = _pack_patterns(patterns)
    nq = int(off.size) - 1
    lo = np.zeros(nq, dtype=np.uint64)
    hi = np.zeros(nq, dtype=np.uint64)
    if nq:
        N.check(N.lib().sa_find_ex(t_ptr if n else None, n, sa_ptr if n else None, width,
                                   buf.ctypes.data if buf.size else None, off.ctypes.data, nq,
                                   lo.ctypes.data, hi.ctypes.data, flags), "sa_find")
    return lo.astype(np.int64), hi.astype(np.int64)


def _text_and_sa(text, sa):
    t = _as_bytes_array(text)
    s = _sa_array(sa)
    if s.size != t.size:
        raise ValueError(f"SA has {s.size} entries for a text of {t.size} bytes")
    return t, s


def find_patterns(text, sa, patterns, mode: str = "auto"):
    """SA intervals of a batch of patterns, searched on the GPU (sa_find).

    ``sa`` is the suffix array of ``text``; ``patterns`` is a sequence of
    bytes / str / uint8 arrays or a ``(buffer, offsets)`` pair with nq + 1
    non-decreasing offsets.  Returns ``(lo, hi)``, two int64 arrays: pattern
    q of m bytes occurs at the text positions ``sa[lo[q]:hi[q]]`` (SA order),
    and ``lo[q] == hi[q]`` is its insertion point when it does not occur.
    Unsigned-byte order, end of string smallest; binary-safe; the empty
    pattern gives ``(0, n)``.  ``mode``: "auto", or "lane" / "wave" to force
    one kernel for every pattern (tests, A/B runs)."""
    t, s = _text_and_sa(text, sa)
    N.require_device()
    return _find_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4, patterns, mode)


def count_patterns(text, sa, patterns, mode: str = "auto") -> np.ndarray:
    """Occurrences of each pattern in ``text`` (int64): hi - lo of find_patterns."""
    lo, hi = find_patterns(text, sa, patterns, mode)
    return hi - lo


def locate_patterns(text, sa, patterns, mode: str = "auto") -> list:
    """Text positions of each pattern, ascending: the host slices
    ``sa[lo:hi]`` of find_patterns, sorted."""
    lo, hi = find_patterns(text, sa, patterns, mode)
    s = np.asarray(sa)
    return [np.sort(s[a:b].astype(np.int64)) for a, b in zip(lo.tolist(), hi.tolist())]


def _locate_flags(order: str, chunks: bool = False) -> int:
    if order not in N.LOCATE_ORDERS:
        raise ValueError(f"order {order!r}: one of {sorted(N.LOCATE_ORDERS)}")
    return N.LOCATE_ORDERS[order] | (N.LOCATE_SMALL_CHUNKS if chunks else 0)


def locate_intervals(sa, lo, hi, max_hits: int = 0, order: str = "text", _chunks: bool = False):
    """Text positions of a batch of SA intervals, expanded and sorted on the
    GPU (sa_locate), in CSR form.

    ``lo`` / ``hi``: what find_patterns or match_patterns return.  Returns
    ``(offsets, positions)``, both int64: query q has the
    ``min(hi[q] - lo[q], max_hits)`` positions
    ``positions[offsets[q]:offsets[q + 1]]`` (``max_hits=0``: no cap), the
    entries ``sa[lo[q]:lo[q] + count]`` sorted ascending, or as they lie in
    the SA with ``order="sa"``.  A capped query keeps its first ``max_hits``
    hits in SA order (then sorted): not the smallest positions."""
    flags = _locate_flags(order, _chunks)
    if max_hits < 0:
        raise ValueError("max_hits is negative")
    s = _sa_array(sa)
    lo = np.ascontiguousarray(lo, dtype=np.uint64).reshape(-1)
    hi = np.ascontiguousarray(hi, dtype=np.uint64).reshape(-1)
    if lo.size != hi.size:
        raise ValueError(f"{lo.size} lower and {hi.size} upper bounds")
    N.require_device()
    n, nq, width = int(s.size), int(lo.size), 8 if s.dtype == np.int64 else 4
    cnt = np.where(hi >= lo, hi - lo, 0)          # the C side rejects lo > hi
    if max_hits:
        cnt = np.minimum(cnt, np.uint64(max_hits))
    total = int(cnt.sum(dtype=np.uint64))
    off = np.zeros(nq + 1, dtype=np.uint64)
    pos = np.empty(max(total, 1), dtype=np.int64 if width == 8 else np.uint32)
    N.check(N.lib().sa_locate(s.ctypes.data if n else None, n, width, lo.ctypes.data if nq else None,
                              hi.ctypes.data if nq else None, nq, int(max_hits), flags, off.ctypes.data,
                              pos.ctypes.data, total), "sa_locate")
    return off.astype(np.int64), pos[:total].astype(np.int64)


def locate_batch(text, sa, patterns, max_hits: int = 0, order: str = "text", mode: str = "auto"):
    """find_patterns followed by locate_intervals: ``(offsets, positions)``,
    the occurrences of pattern q are ``positions[offsets[q]:offsets[q + 1]]``
    (ascending; ``order="sa"``: SA order; at most ``max_hits`` of them)."""
    lo, hi = find_patterns(text, sa, patterns, mode)
    return locate_intervals(sa, lo, hi, max_hits, order)


def _match_host(t_ptr, n: int, sa_ptr, width: int, patterns, mode: str, bounds: bool):
    """sa_match over host pointers: (length, lo, hi) as int64 arrays, or the
    lengths alone."""
    flags = _find_mode(mode)
    buf, off = _pack_patterns(patterns)
    nq = int(off.size) - 1
    out = np.zeros((3 if bounds else 1, nq), dtype=np.uint64)
    if nq:
        N.check(N.lib().sa_match(t_ptr if n else None, n, sa_ptr if n else None, width,
                                 buf.ctypes.data if buf.size else None, off.ctypes.data, nq, out[0].ctypes.data,
                                 out[1].ctypes.data if bounds else None, out[2].ctypes.data if bounds else None,
                                 flags), "sa_match")
    out = out.astype(np.int64)
    return (out[0], out[1], out[2]) if bounds else out[0]


def match_patterns(text, sa, patterns, mode: str = "auto", bounds: bool = True):
    """Longest match of each pattern of a batch, searched on the GPU (sa_match).

    ``text``, ``sa``, ``patterns`` and ``mode`` are those of find_patterns.
    Returns ``(length, lo, hi)``, three int64 arrays: ``length[q]`` is the
    largest l for which the first l bytes of pattern q occur in ``text``, and
    that prefix occurs at the text positions ``sa[lo[q]:hi[q]]``.  A pattern
    that occurs whole gets its find_patterns interval; ``length == 0`` (the
    empty pattern, a first byte the text does not hold) gives ``(0, n)``.
    ``bounds=False`` returns the lengths alone and skips the two bound
    searches."""
    t, s = _text_and_sa(text, sa)
    N.require_device()
    return _match_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4, patterns, mode,
                       bounds)


def matching_statistics(text, sa, query, max_len: int = 0, mode: str = "auto", bounds: bool = True):
    """Matching statistics of ``query`` against ``text`` on the GPU
    (sa_matching_stats): one longest-match query per position of ``query``.

    Entry i answers ``query[i:]`` (``query[i:i + max_len]`` when ``max_len``
    is not 0) as match_patterns would: ``(length, lo, hi)``, int64 arrays of
    ``len(query)`` entries, or the lengths alone with ``bounds=False``.
    ``mode``: "auto" takes the one-query-per-lane kernel when no query can be
    longer than FIND_LANE_MAX bytes and the one-query-per-wavefront kernel
    otherwise; "lane" / "wave" force one."""
    flags = _find_mode(mode)
    if max_len < 0:
        raise ValueError("max_len is negative")
    t, s = _text_and_sa(text, sa)
    N.require_device()
    q = _as_bytes_array(query).reshape(-1)
    n, m = int(t.size), int(q.size)
    out = np.zeros((3 if bounds else 1, m), dtype=np.uint64)
    if m:
        N.check(N.lib().sa_matching_stats(t.ctypes.data if n else None, n, s.ctypes.data if n else None,
                                          8 if s.dtype == np.int64 else 4, q.ctypes.data, m, int(max_len),
                                          out[0].ctypes.data, out[1].ctypes.data if bounds else None,
                                          out[2].ctypes.data if bounds else None, flags),
                "sa_matching_stats")
    out = out.astype(np.int64)
    return (out[0], out[1], out[2]) if bounds else out[0]


def _mem_mode(mode: str) -> int:
    """The SA_MEM_* flags of ``mode``."""
    if mode not in N.MEM_MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(N.MEM_MODES)}")
    return N.MEM_MODES[mode]


def _mems_host(t_ptr, n: int, sa_ptr, width: int, query, min_len: int, max_occ: int, max_candidates: int, mode: str,
               return_info: bool):
    """sa_mems over host pointers: a sizing call, then the call that fills
    the arrays; (qpos, tpos, length) as int64, with the info dict on request."""
    flags = _mem_mode(mode)
    if min_len < 1:
        raise ValueError("min_len must be at least 1")
    if max_occ < 0 or max_candidates < 0:
        raise ValueError("max_occ and max_candidates: 0 (none) or a positive bound")
    q = _as_bytes_array(query).reshape(-1)
    m = int(q.size)
    off = np.zeros(m + 1, dtype=np.uint64)
    info = (ctypes.c_uint64 * N.MEM_INFO)()
    L = N.lib()

    def call(tpos, length, cap):
        rc = N.check(L.sa_mems(t_ptr if n else None, n, sa_ptr if n else None, width, q.ctypes.data if m else None, m,
                               int(min_len), int(max_occ), int(max_candidates), flags, off.ctypes.data,
                               None if tpos is None else tpos.ctypes.data,
                               None if length is None else length.ctypes.data, cap, info), "sa_mems")
        if rc == N.MEM_TOO_MANY:
            raise N.SAError(f"sa_mems: {int(info[1])} candidates are more than max_candidates = {max_candidates} "
                            f"(raise it, raise min_len, or set max_occ)")

    call(None, None, 0)
    total = int(info[0])
    dt = np.int64 if width == 8 else np.uint32
    tpos, length = np.empty(max(total, 1), dtype=dt), np.empty(max(total, 1), dtype=dt)
    if total:
        call(tpos, length, total)
        if int(info[0]) != total:
            raise N.SAError(f"sa_mems: {int(info[0])} MEMs after a sizing call that counted {total}")
    o = off.astype(np.int64)
    qpos = np.repeat(np.arange(m, dtype=np.int64), np.diff(o))
    out = (qpos, tpos[:total].astype(np.int64), length[:total].astype(np.int64))
    if return_info:
        return out + ({"total": total, "candidates": int(info[1]), "skipped": int(info[2]), "offsets": o},)
    return out


def maximal_exact_matches(text, sa, query, min_len: int, max_occ: int = 0, max_candidates: int = 0,
                          mode: str = "auto", return_info: bool = False):
    """Maximal exact matches of ``query`` against ``text`` on the GPU (sa_mems).

    ``sa`` is the suffix array of ``text``.  Returns ``(qpos, tpos, length)``,
    three int64 arrays sorted by (qpos, tpos): ``query[qpos:qpos + length] ==
    text[tpos:tpos + length]``, ``length >= min_len``, and the match can be
    extended neither to the left nor to the right.  Every such triple is
    listed once.  ``max_occ`` (0: none) drops the matches whose first
    ``min_len`` bytes occur more than ``max_occ`` times in the text: the
    repeat filter of seeders, and the bound on the work, which is proportional
    to the candidates (the seed occurrences of the positions that stay).
    ``max_candidates`` (0: none) raises SAError, with the candidate count in
    the message, instead of enumerating more candidates than that.
    ``mode``: "auto", or "lane" / "wave" to force one right-extension path
    (tests, A/B runs).  ``return_info=True`` appends a dict: ``total``,
    ``candidates``, ``skipped`` (positions dropped by ``max_occ``) and
    ``offsets`` (the CSR offsets over the query positions, len(query) + 1)."""
    t, s = _text_and_sa(text, sa)
    _mem_mode(mode)
    N.require_device()
    return _mems_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4, query, min_len,
                      max_occ, max_candidates, mode, return_info)


def _hamming_mode(mode: str) -> int:
    """The SA_HAMMING_* flags of ``mode``."""
    if mode not in N.HAMMING_MODES:
        raise ValueError(f"mode {mode!r}: one of {sorted(N.HAMMING_MODES)}")
    return N.HAMMING_MODES[mode]


def _hamming_k(k, max_candidates) -> None:
    if not 0 <= int(k) <= N.HAMMING_MAX_K:
        raise ValueError(f"k = {k}: 0 .. {N.HAMMING_MAX_K}")
    if max_candidates < 0:
        raise ValueError("max_candidates: 0 (none) or a positive bound")


def _hamming_host(t_ptr, n: int, sa_ptr, width: int, patterns, k: int, max_candidates: int, mode: str,
                  return_info: bool):
    """sa_hamming over host pointers: a sizing call, then the call that fills
    the arrays; (offsets int64, positions int64, distances uint8), with the
    info dict on request."""
    flags = _hamming_mode(mode)
    _hamming_k(k, max_candidates)
    buf, poff = _pack_patterns(patterns)
    nq = int(poff.size) - 1
    off = np.zeros(nq + 1, dtype=np.uint64)
    info = (ctypes.c_uint64 * N.HAMMING_INFO)()
    L = N.lib()

    def call(pos, dist, cap):
        rc = N.check(L.sa_hamming(t_ptr if n else None, n, sa_ptr if n else None, width,
                                  buf.ctypes.data if buf.size else None, poff.ctypes.data, nq, int(k),
                                  int(max_candidates), flags, off.ctypes.data,
                                  None if pos is None else pos.ctypes.data,
                                  None if dist is None else dist.ctypes.data, cap, info), "sa_hamming")
        if rc == N.HAMMING_TOO_MANY:
            raise N.SAError(f"sa_hamming: {int(info[1])} candidates are more than max_candidates = "
                            f"{max_candidates} (raise it, or lower k)")

    call(None, None, 0)
    total = int(info[0])
    pos = np.empty(max(total, 1), dtype=np.int64 if width == 8 else np.uint32)
    dist = np.empty(max(total, 1), dtype=np.uint8)
    if total:
        call(pos, dist, total)
        if int(info[0]) != total:
            raise N.SAError(f"sa_hamming: {int(info[0])} occurrences after a sizing call that counted {total}")
    out = (off.astype(np.int64), pos[:total].astype(np.int64), dist[:total].copy())
    if return_info:
        return out + ({"total": total, "candidates": int(info[1]), "pieces": int(info[2])},)
    return out


def hamming_search(text, sa, patterns, k: int, max_candidates: int = 0, mode: str = "auto",
                   return_info: bool = False):
    """Occurrences of each pattern with at most ``k`` substitutions, searched
    on the GPU (sa_hamming).

    ``text``, ``sa`` and ``patterns`` are those of find_patterns; ``k`` (0 ..
    HAMMING_MAX_K) is the budget of every pattern of the call.  Returns
    ``(offsets, positions, distances)``: pattern q of m bytes occurs at the
    text positions ``positions[offsets[q]:offsets[q + 1]]`` (int64, ascending,
    each once), ``p + m <= n``, with ``distances`` (uint8) of them the number
    of bytes at which ``text[p:p + m]`` and the pattern differ, at most ``k``.
    The empty pattern occurs at every position of [0, n) with distance 0; a
    pattern of up to ``k`` bytes occurs at every ``p <= n - m``.  The work is
    proportional to the candidates, the exact occurrences of the k + 1 pieces
    of every pattern: ``max_candidates`` (0: none) raises SAError, with the
    count in the message, instead of enumerating more than that.  ``mode``:
    "auto", or "lane" / "wave" to force one verify path (tests, A/B runs).
    ``return_info=True`` appends a dict: ``total``, ``candidates`` and
    ``pieces`` (nq (k + 1))."""
    t, s = _text_and_sa(text, sa)
    _hamming_mode(mode)
    _hamming_k(k, max_candidates)
    packed = _pack_patterns(patterns)
    N.require_device()
    return _hamming_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4, packed, k,
                         max_candidates, mode, return_info)


def _edit_k(k, max_candidates) -> None:
    if not 0 <= int(k) <= N.EDIT_MAX_K:
        raise ValueError(f"k = {k}: 0 .. {N.EDIT_MAX_K}")
    if max_candidates < 0:
        raise ValueError("max_candidates: 0 (none) or a positive bound")


def _edit_host(t_ptr, n: int, sa_ptr, width: int, patterns, k: int, max_candidates: int, return_starts: bool,
               return_info: bool):
    """sa_edit over host pointers: a sizing call, then the call that fills the
    arrays; (offsets int64, ends int64, starts int64, distances uint8), with
    the info dict on request.  Without ``return_starts`` the backward DP is
    skipped and starts / distances are None."""
    _edit_k(k, max_candidates)
    buf, poff = _pack_patterns(patterns)
    nq = int(poff.size) - 1
    off = np.zeros(nq + 1, dtype=np.uint64)
    info = (ctypes.c_uint64 * N.EDIT_INFO)()
    L = N.lib()

    def call(end, start, dist, cap):
        rc = N.check(L.sa_edit(t_ptr if n else None, n, sa_ptr if n else None, width,
                               buf.ctypes.data if buf.size else None, poff.ctypes.data, nq, int(k),
                               int(max_candidates), 0, off.ctypes.data,
                               None if end is None else end.ctypes.data,
                               None if start is None else start.ctypes.data,
                               None if dist is None else dist.ctypes.data, cap, info), "sa_edit")
        if rc == N.EDIT_TOO_MANY:
            raise N.SAError(f"sa_edit: {int(info[1])} candidates are more than max_candidates = "
                            f"{max_candidates} (raise it, or lower k)")

    call(None, None, None, 0)
    total = int(info[0])
    wide = np.int64 if width == 8 else np.uint32
    end = np.empty(max(total, 1), dtype=wide)
    start = np.empty(max(total, 1), dtype=wide) if return_starts else None
    dist = np.empty(max(total, 1), dtype=np.uint8) if return_starts else None
    if total:
        call(end, start, dist, total)
        if int(info[0]) != total:
            raise N.SAError(f"sa_edit: {int(info[0])} ends after a sizing call that counted {total}")
    out = (off.astype(np.int64), end[:total].astype(np.int64),
           start[:total].astype(np.int64) if return_starts else None, dist[:total].copy() if return_starts else None)
    if return_info:
        return out + ({"total": total, "candidates": int(info[1]), "pieces": int(info[2])},)
    return out


def edit_search(text, sa, patterns, k: int, max_candidates: int = 0, return_starts: bool = True,
                return_info: bool = False):
    """Occurrences of each pattern with at most ``k`` substitutions, insertions
    and deletions, searched on the GPU (sa_edit).

    ``text``, ``sa`` and ``patterns`` are those of find_patterns; ``k`` (0 ..
    EDIT_MAX_K = 31) is the budget of every pattern of the call.  Returns
    ``(offsets, ends, starts, distances)``: pattern q matches with at most k
    edits at the ends ``ends[offsets[q]:offsets[q + 1]]`` (int64, ascending,
    each once): ``e`` is listed when some ``text[s:e]`` is within edit distance
    k of the pattern.  ``distances`` (uint8) is the least such distance D(e)
    and ``starts`` (int64) the largest s that reaches it, the shortest best
    match.  A pattern of up to ``k`` bytes would match at every end: it is not
    searched and its list is empty.  A pattern longer than the text is
    searched.  ``return_starts=False`` skips the pass that computes starts and
    distances and returns None for both.  The work is proportional to the
    candidates, the exact occurrences of the k + 1 pieces of every pattern:
    ``max_candidates`` (0: none) raises SAError, with the count in the message,
    instead of enumerating more than that.  ``return_info=True`` appends a
    dict: ``total``, ``candidates`` and ``pieces`` (nq (k + 1))."""
    t, s = _text_and_sa(text, sa)
    _edit_k(k, max_candidates)
    packed = _pack_patterns(patterns)
    N.require_device()
    return _edit_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4, packed, k,
                      max_candidates, return_starts, return_info)


def _none_to_minus_one(a: np.ndarray) -> np.ndarray:
    """uint32 / int64 results as int64, "none" (all ones at either width) as -1."""
    out = a.astype(np.int64)
    out[out == N.LPF_NONE] = -1
    return out


def _lpf_host(t_ptr, n: int, sa_ptr, width: int):
    """sa_lpf over host pointers: (lpf, src) as int64, src -1 where none."""
    dt = np.int64 if width == 8 else np.uint32
    lpf, src = np.empty(max(n, 1), dtype=dt), np.empty(max(n, 1), dtype=dt)
    N.check(N.lib().sa_lpf(t_ptr if n else None, n, sa_ptr if n else None, width, lpf.ctypes.data, src.ctypes.data),
            "sa_lpf")
    return lpf[:n].astype(np.int64), _none_to_minus_one(src[:n])


def _lz77_host(t_ptr, n: int, sa_ptr, width: int):
    """sa_lz77 over host pointers, one call (z <= n, so n entries always fit):
    LPF on the device once, the sizing parse and the writing parse, only z in
    between.  (pos, length, src) as int64."""
    dt = np.int64 if width == 8 else np.uint32
    pos, length, src = (np.empty(max(n, 1), dtype=dt) for _ in range(3))
    z = ctypes.c_uint64()
    N.check(N.lib().sa_lz77(t_ptr if n else None, n, sa_ptr if n else None, width, pos.ctypes.data, length.ctypes.data,
                            src.ctypes.data, n, ctypes.byref(z)), "sa_lz77")
    k = int(z.value)
    return pos[:k].astype(np.int64), length[:k].astype(np.int64), _none_to_minus_one(src[:k])


def _lz_with_lcp(t: np.ndarray, s: np.ndarray, lcp, parse: bool):
    """The device forms over torch tensors, for a caller who has the LCP array
    already: the text is not uploaded and the LCP is not computed again."""
    import torch
    n = int(t.size)
    l = np.ascontiguousarray(lcp)
    if l.size != n:
        raise ValueError(f"LCP has {l.size} entries for a text of {n} bytes")
    if n and (int(s.min()) < 0 or int(s.max()) >= n):
        raise N.SAError("SA entry out of range")
    if n and (int(l.min()) < 0 or int(l.max()) > n):
        raise N.SAError("LCP entry out of range")
    if n == 0:
        e = np.zeros(0, dtype=np.int64)
        return (e, e.copy(), e.copy()) if parse else (e, e.copy())
    dev = torch.device("cuda", 0)

    def up(a):
        return torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(dev)

    def down(x, k):
        return x[:k].cpu().numpy().view(np.uint32)

    d_sa, d_lcp = up(s), up(l)
    d_lpf, d_src = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    db = DeviceBuilder(n)
    try:
        torch.cuda.synchronize()
        db.lpf(None, n, d_sa, d_lcp, d_lpf, d_src)
        if not parse:
            torch.cuda.synchronize()
            return down(d_lpf, n).astype(np.int64), _none_to_minus_one(down(d_src, n))
        z = db.lz77(n, d_lpf, d_src, None, None, None, 0)
        d_out = [torch.empty(max(z, 1), dtype=torch.int32, device=dev) for _ in range(3)]
        if db.lz77(n, d_lpf, d_src, d_out[0], d_out[1], d_out[2], z) != z:
            raise N.SAError(f"sa_lz77_device: the phrase count changed after a sizing call that counted {z}")
        return (down(d_out[0], z).astype(np.int64), down(d_out[1], z).astype(np.int64),
                _none_to_minus_one(down(d_out[2], z)))
    finally:
        db.close()


def longest_previous_factor(text, sa, lcp=None):
    """Longest previous factor array of ``text`` on the GPU (sa_lpf).

    ``sa`` is the suffix array of ``text``.  Returns ``(lpf, src)``, two int64
    arrays in text order: ``lpf[i]`` is the length of the longest prefix of
    ``text[i:]`` that also starts at some ``j < i`` (the two occurrences may
    overlap), and ``src[i]`` is the canonical such ``j`` of include/sa_hip.h,
    -1 where ``lpf[i] == 0``.  No text is compared: the lengths are LCP range
    minima, so a highly repetitive text costs what its length costs.  ``lcp``:
    the LCP array of ``sa`` as lcp_array gives it, when the caller has it; the
    device forms then run on it and the LCP is not computed again."""
    t, s = _text_and_sa(text, sa)
    N.require_device()
    if lcp is not None:
        return _lz_with_lcp(t, s, lcp, False)
    return _lpf_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4)


def lz77_factorize(text, sa, lcp=None):
    """Greedy, self-referential LZ77 factorisation of ``text`` on the GPU
    (sa_lz77).

    Returns ``(pos, length, src)``, three int64 arrays with one entry per
    phrase in text order: the phrases tile the text (``pos[0] == 0``,
    ``pos[k + 1] == pos[k] + length[k]``), ``text[pos:pos + length]`` is the
    longest prefix of ``text[pos:]`` that occurs earlier, copied from ``src``
    (the copy may run into the phrase itself), and a literal has ``length == 1``
    and ``src == -1``.  ``len(pos)`` is z, the number of phrases.  LPF is
    computed on the device once and parsed there; only z comes back in
    between.  ``lcp`` as for longest_previous_factor."""
    t, s = _text_and_sa(text, sa)
    N.require_device()
    if lcp is not None:
        return _lz_with_lcp(t, s, lcp, True)
    return _lz77_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4)


def _rep_kind(kind: str) -> int:
    if kind not in N.REP_KINDS:
        raise ValueError(f"unknown kind {kind!r} (one of {sorted(N.REP_KINDS)})")
    return N.REP_KINDS[kind]


def _rep_filters(min_len: int, min_occ: int):
    if int(min_len) < 0 or int(min_occ) < 0:
        raise ValueError("min_len and min_occ must not be negative")
    return int(min_len), int(min_occ)


def _repeats_host(t_ptr, n: int, sa_ptr, width: int, min_len: int, min_occ: int, kind: int):
    """sa_repeats over host pointers, one call (a text has fewer than n
    repeats, so n entries always fit): (length, lo, hi) as int64."""
    min_len, min_occ = _rep_filters(min_len, min_occ)
    dt = np.int64 if width == 8 else np.uint32
    length, lo, hi = (np.empty(max(n, 1), dtype=dt) for _ in range(3))
    info = (ctypes.c_uint64 * N.REP_INFO)()
    N.check(N.lib().sa_repeats(t_ptr if n else None, n, sa_ptr if n else None, width, min_len, min_occ, kind,
                               length.ctypes.data, lo.ctypes.data, hi.ctypes.data, n, info), "sa_repeats")
    k = int(info[0])
    return length[:k].astype(np.int64), lo[:k].astype(np.int64), hi[:k].astype(np.int64)


def _repeats_with_lcp(t: np.ndarray, s: np.ndarray, lcp, min_len: int, min_occ: int, kind: str):
    """The device form over torch tensors, for a caller who has the LCP array
    already: the sizing call, then the writing call into outputs of that size."""
    import torch
    min_len, min_occ = _rep_filters(min_len, min_occ)
    n = int(t.size)
    l = np.ascontiguousarray(lcp)
    if l.size != n:
        raise ValueError(f"LCP has {l.size} entries for a text of {n} bytes")
    if n and (int(s.min()) < 0 or int(s.max()) >= n):
        raise N.SAError("SA entry out of range")
    if n and (int(l.min()) < 0 or int(l.max()) > n):
        raise N.SAError("LCP entry out of range")
    if n <= 1:
        e = np.zeros(0, dtype=np.int64)
        return e, e.copy(), e.copy()
    dev = torch.device("cuda", 0)

    def up(a):
        return torch.from_numpy(a.astype(np.uint32).view(np.int32)).to(dev)

    def down(x, k):
        return x[:k].cpu().numpy().view(np.uint32).astype(np.int64)

    d_text, d_sa, d_lcp = torch.from_numpy(t.copy()).to(dev), up(s), up(l)
    db = DeviceBuilder(n)
    try:
        torch.cuda.synchronize()
        count, _ = db.repeats(d_text, n, d_sa, d_lcp, min_len, min_occ, kind, None, None, None, 0)
        d_out = [torch.empty(max(count, 1), dtype=torch.int32, device=dev) for _ in range(3)]
        if db.repeats(d_text, n, d_sa, d_lcp, min_len, min_occ, kind, d_out[0], d_out[1], d_out[2], count)[0] != count:
            raise N.SAError(f"sa_repeats_device: the count changed after a sizing call that counted {count}")
        return down(d_out[0], count), down(d_out[1], count), down(d_out[2], count)
    finally:
        db.close()


def maximal_repeats(text, sa, min_len: int = 1, min_occ: int = 2, kind: str = "maximal", lcp=None):
    """The repeats of ``text`` on the GPU (sa_repeats), as SA intervals.

    ``sa`` is the suffix array of ``text``.  Returns ``(length, lo, hi)``,
    three int64 arrays with one entry per repeat: the string
    ``text[sa[lo]:sa[lo] + length]`` occurs exactly at ``sa[lo:hi]``, at least
    twice, and its occurrences are not all followed by the same byte
    (right-maximal).  ``kind``: ``"right"`` lists every such repeat (the LCP
    intervals: the internal nodes of the suffix tree), ``"maximal"`` those
    whose occurrences are not all preceded by the same byte either,
    ``"supermaximal"`` the maximal repeats that are no proper substring of
    another maximal repeat.  ``min_len`` and ``min_occ`` filter by length and
    by ``hi - lo``.  The order is that of the repeats' heads (include/
    sa_hip.h), so two calls agree exactly; ``locate_intervals(sa, lo, hi)``
    gives every occurrence.  ``lcp``: the LCP array of ``sa`` as lcp_array
    gives it, when the caller has it; the device form then runs on it and the
    LCP is not computed again."""
    t, s = _text_and_sa(text, sa)
    k = _rep_kind(kind)
    _rep_filters(min_len, min_occ)
    N.require_device()
    if lcp is not None:
        return _repeats_with_lcp(t, s, lcp, min_len, min_occ, kind)
    return _repeats_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4, min_len, min_occ, k)


def _bwt_host(t_ptr, n: int, sa_ptr, width: int, stats: bool):
    """sa_bwt over host pointers: (bwt uint8[n], the SA_BWT_STATS words or None)."""
    out = np.empty(max(n, 1), dtype=np.uint8)
    st = np.zeros(N.BWT_STATS, dtype=np.uint64) if stats else None
    N.check(N.lib().sa_bwt(t_ptr if n else None, n, sa_ptr if n else None, width, out.ctypes.data,
                           st.ctypes.data if stats else None), "sa_bwt")
    return out[:n], st


def bwt(text, sa, stats: bool = False):
    """Burrows-Wheeler transform of ``text`` from its suffix array ``sa``, on
    the GPU (sa_bwt).

    ``bwt[r] = text[sa[r] - 1]``, and ``text[n - 1]`` at the primary index,
    the one rank with ``sa[r] == 0``: n bytes, a permutation of the text's.
    Returns ``(bwt, primary)``, a uint8 array and an int; with ``stats=True``
    ``(bwt, primary, runs, counts)``: the number of maximal runs of equal
    bytes in ``bwt`` and the int64[256] byte histogram, both counted by the
    same kernel.  Without ``stats`` the kernel does neither and the primary
    index is looked up in the host ``sa``."""
    t, s = _text_and_sa(text, sa)
    N.require_device()
    n = int(t.size)
    out, st = _bwt_host(t.ctypes.data, n, s.ctypes.data, 8 if s.dtype == np.int64 else 4, stats)
    if stats:
        return out, int(st[0]), int(st[1]), st[2:].astype(np.int64)
    zero = np.flatnonzero(s == 0)
    if n and zero.size != 1:
        raise N.SAError(f"sa_bwt: the SA holds {zero.size} entries equal to 0, not one")
    return out, int(zero[0]) if n else 0


def inverse_suffix_array(sa, width: int = 4):
    """Inverse of the suffix array ``sa`` on the GPU (sa_inverse):
    ``isa[sa[r]] = r``, uint32 (width 4) or int64 (width 8).  An ``sa`` that
    is not a permutation of 0 .. n-1 raises SAError."""
    if width not in (4, 8):
        raise ValueError("width must be 4 or 8")
    s = _sa_array(sa)
    n = int(s.size)
    if s.itemsize != width:   # the C entry point takes input and output at one width
        if width == 4 and n and (int(s.min()) < 0 or int(s.max()) >= n):
            raise N.SAError("sa_inverse: SA entry out of range")
        s = s.astype(np.int64 if width == 8 else np.uint32)
    N.require_device()
    out = np.empty(max(n, 1), dtype=np.uint32 if width == 4 else np.int64)
    N.check(N.lib().sa_inverse(s.ctypes.data if n else None, n, width, out.ctypes.data), "sa_inverse")
    return out[:n]


def _bwt_and_primary(bwt, primary):
    b = _as_bytes_array(bwt)
    n = int(b.size)
    p = int(primary)
    if p < 0:
        raise ValueError(f"primary index {p} is negative")
    return b, n, p   # p >= n is the library's to reject, before any device work


def _ibwt_info(words) -> dict:
    return {"splitters": int(words[0]), "longest_sublist": int(words[1]), "steps": int(words[2])}


def lf_mapping(bwt, primary: int, width: int = 4):
    """LF-mapping of ``(bwt, primary)`` on the GPU (sa_lf), in the convention
    of :func:`bwt`: order the rows ``primary, 0, 1, ..`` (the primary row
    first, the rest in rank order) and sort them stably by their byte;
    ``lf[r]`` is where row r lands.  For the BWT of a text it is the rank of
    the suffix one position to the left: ``lf[isa[i]] == isa[i - 1]`` and
    ``lf[primary] == isa[n - 1]``.  uint32 (width 4) or int64 (width 8); a
    permutation of 0 .. n-1 whatever the bytes are."""
    if width not in (4, 8):
        raise ValueError("width must be 4 or 8")
    b, n, p = _bwt_and_primary(bwt, primary)
    out = np.empty(max(n, 1), dtype=np.uint32 if width == 4 else np.int64)
    N.check(N.lib().sa_lf(b.ctypes.data if n else None, n, p, out.ctypes.data, width), "sa_lf")
    return out[:n]


def inverse_bwt(bwt, primary: int, return_sa: bool = False, width: int = 4, return_info: bool = False):
    """The text whose Burrows-Wheeler transform is ``(bwt, primary)``, on the
    GPU (sa_ibwt): the inverse of :func:`bwt`.  Returns the text as a uint8
    array; with ``return_sa`` ``(text, sa)``, the suffix array (uint32 or
    int64 by ``width``) coming out of the same walk; with ``return_info`` a
    dict is appended: ``splitters`` and ``longest_sublist`` of the list
    ranking and ``steps``, n - 1 for a BWT.

    A pair that is the BWT of no text raises SAError, "not a BWT"."""
    if width not in (4, 8):
        raise ValueError("width must be 4 or 8")
    b, n, p = _bwt_and_primary(bwt, primary)
    text = np.empty(max(n, 1), dtype=np.uint8)
    sa = np.empty(max(n, 1), dtype=np.uint32 if width == 4 else np.int64) if return_sa else None
    info = (ctypes.c_uint64 * N.IBWT_INFO)()
    N.check(N.lib().sa_ibwt_ex(b.ctypes.data if n else None, n, p, text.ctypes.data,
                               sa.ctypes.data if return_sa else None, width, info), "sa_ibwt")
    out = (text[:n],) + ((sa[:n],) if return_sa else ()) + ((_ibwt_info(info),) if return_info else ())
    return out[0] if len(out) == 1 else out


def _doc_offsets(doc_off) -> np.ndarray:
    """The D + 1 offsets of a collection as uint64 (the C side checks their values)."""
    off = np.asarray(doc_off)
    if off.ndim != 1 or off.size < 2 or off.dtype.kind not in "iu":
        raise ValueError("doc_off: a one-dimensional integer array of D + 1 entries, D >= 1")
    if off.dtype.kind == "i" and (off < 0).any():
        raise ValueError("doc_off has a negative entry")
    return np.ascontiguousarray(off, dtype=np.uint64)


def _doc_intervals(lo, hi):
    lo = np.ascontiguousarray(lo, dtype=np.uint64).reshape(-1)
    hi = np.ascontiguousarray(hi, dtype=np.uint64).reshape(-1)
    if lo.size != hi.size:
        raise ValueError(f"{lo.size} lower and {hi.size} upper bounds")
    return lo, hi


def _doc_order(order: str) -> int:
    if order not in N.DOC_ORDERS:
        raise ValueError(f"order {order!r}: one of {sorted(N.DOC_ORDERS)}")
    return N.DOC_ORDERS[order]


def document_array(sa, doc_off, prev: bool = True):
    """The document array of a collection on the GPU (sa_doc_array).

    ``sa`` is the suffix array of the concatenated documents and ``doc_off``
    their D + 1 non-decreasing offsets (``doc_off[0] == 0``, ``doc_off[D] ==
    len(sa)``; document d is ``text[doc_off[d]:doc_off[d + 1]]``, empty
    documents allowed).  Returns ``(da, prv)``, or ``da`` alone with
    ``prev=False``: ``da[r]`` is the document in which ``sa[r]`` lies and
    ``prv[r]`` is 1 + the nearest smaller rank of the same document (0: none),
    what document_frequency and list_documents take.  uint32 for a 32-bit
    ``sa``, int64 for an int64 one."""
    s = _sa_array(sa)
    off = _doc_offsets(doc_off)
    n, width = int(s.size), 8 if s.dtype == np.int64 else 4
    dt = np.int64 if width == 8 else np.uint32
    da = np.empty(max(n, 1), dtype=dt)
    pv = np.empty(max(n, 1), dtype=dt) if prev else None
    if n:
        N.require_device()
    N.check(N.lib().sa_doc_array(s.ctypes.data if n else None, n, width, off.ctypes.data, int(off.size) - 1,
                                 da.ctypes.data, pv.ctypes.data if prev else None), "sa_doc_array")
    return (da[:n], pv[:n]) if prev else da[:n]


def doc_of_positions(doc_off, n: int, positions):
    """(document, offset inside it) of text positions on the GPU (sa_doc_of):
    two int64 arrays, both -1 for a position that is not below ``n``.
    ``positions``: what locate_intervals returns."""
    off = _doc_offsets(doc_off)
    pos = np.ascontiguousarray(positions, dtype=np.int64).reshape(-1)
    if (pos < 0).any():
        raise ValueError("a position is negative")
    pos = np.minimum(pos, N.DOC_NONE)          # anything at or above n is "none"
    count = int(pos.size)
    doc = np.empty(max(count, 1), dtype=np.int64)
    rel = np.empty(max(count, 1), dtype=np.int64)
    if count:
        N.require_device()
    N.check(N.lib().sa_doc_of(off.ctypes.data, int(off.size) - 1, int(n), pos.ctypes.data if count else None, count, 8,
                              doc.ctypes.data, rel.ctypes.data), "sa_doc_of")
    doc, rel = doc[:count], rel[:count]
    none = doc == N.DOC_NONE
    doc[none] = -1
    rel[none] = -1
    return doc, rel


def document_frequency(prev, lo, hi) -> np.ndarray:
    """In how many documents each SA interval occurs, counted on the GPU
    (sa_doc_frequency): int64, one entry per interval.  ``prev``: the second
    array of document_array; ``lo`` / ``hi``: what find_patterns,
    match_patterns or maximal_repeats return."""
    p = _sa_array(prev)
    lo, hi = _doc_intervals(lo, hi)
    n, nq = int(p.size), int(lo.size)
    df = np.zeros(max(nq, 1), dtype=np.uint64)
    if n and nq:
        N.require_device()
    N.check(N.lib().sa_doc_frequency(p.ctypes.data if n else None, n, 8 if p.dtype == np.int64 else 4,
                                     lo.ctypes.data if nq else None, hi.ctypes.data if nq else None, nq,
                                     df.ctypes.data), "sa_doc_frequency")
    return df[:nq].astype(np.int64)


def list_documents(da, prev, lo, hi, max_docs: int = 0, order: str = "doc"):
    """The distinct documents of a batch of SA intervals, listed on the GPU
    (sa_doc_list), in CSR form.

    ``da`` / ``prev``: what document_array returns.  Returns ``(offsets,
    docs)``, both int64: interval q occurs in the documents
    ``docs[offsets[q]:offsets[q + 1]]``, ascending, or in the order of their
    first ranks with ``order="rank"``.  ``max_docs`` (0: no cap) keeps the
    first ``max_docs`` documents in rank order (then sorted): not the smallest
    ids."""
    flags = _doc_order(order)
    if max_docs < 0:
        raise ValueError("max_docs is negative")
    d, p = _sa_array(da), _sa_array(prev)
    if d.size != p.size or d.dtype.itemsize != p.dtype.itemsize:
        raise ValueError("da and prev: the same length and width")
    lo, hi = _doc_intervals(lo, hi)
    n, nq, width = int(d.size), int(lo.size), 8 if d.dtype == np.int64 else 4
    off = np.zeros(nq + 1, dtype=np.uint64)
    L = N.lib()

    def call(out, cap):
        N.check(L.sa_doc_list(d.ctypes.data if n else None, p.ctypes.data if n else None, n, width,
                              lo.ctypes.data if nq else None, hi.ctypes.data if nq else None, nq, int(max_docs), flags,
                              off.ctypes.data, out, cap), "sa_doc_list")

    call(None, 0)                               # the host sizes the output from prev
    total = int(off[nq])
    docs = np.empty(max(total, 1), dtype=np.int64 if width == 8 else np.uint32)
    if total:
        N.require_device()
        call(docs.ctypes.data, total)
    return off.astype(np.int64), docs[:total].astype(np.int64)


def _lce_queries(*arrays):
    """Query arrays of one length as uint64 (negative entries rejected)."""
    out = []
    for a in arrays:
        a = np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
        if (a < 0).any():
            raise ValueError("a position, bound or length is negative")
        out.append(a.astype(np.uint64))
    if any(a.size != out[0].size for a in out):
        raise ValueError("query arrays of different lengths: " + ", ".join(str(a.size) for a in out))
    return out


def _lce_none_to_minus_one(a: np.ndarray) -> np.ndarray:
    a = a.astype(np.int64)
    a[a == N.LCE_NONE] = -1
    return a


def lcp_range_min(lcp, lo, hi) -> np.ndarray:
    """``min lcp[lo + 1 : hi]`` of a batch of SA intervals ``[lo, hi)`` on the
    GPU (sa_lcp_min): the length of the longest common prefix of all suffixes
    of the interval, its string depth.  ``lcp``: what lcp_array returns;
    ``lo`` / ``hi``: what find_patterns, match_patterns, maximal_repeats or
    FMIndex.find return.  int64, -1 where there is no minimum: an interval of
    fewer than two ranks, or one that breaks ``lo < hi <= n``.  The index over
    ``lcp`` is built for the call; LCEIndex keeps one."""
    p = _sa_array(lcp)
    lo, hi = _lce_queries(lo, hi)
    n, nq = int(p.size), int(lo.size)
    out = np.full(max(nq, 1), N.LCE_NONE, dtype=np.uint64)
    if nq and ((hi <= n) & (lo < hi) & (hi - np.minimum(lo, hi) >= 2)).any():
        N.require_device()
    N.check(N.lib().sa_lcp_min(p.ctypes.data if n else None, n, 8 if p.dtype == np.int64 else 4,
                               lo.ctypes.data if nq else None, hi.ctypes.data if nq else None, nq, out.ctypes.data),
            "sa_lcp_min")
    return _lce_none_to_minus_one(out[:nq])


def _lce_host(t_ptr, n: int, sa_ptr, width: int, i, j) -> np.ndarray:
    """sa_lce over host pointers: int64 lengths."""
    i, j = _lce_queries(i, j)
    nq = int(i.size)
    out = np.zeros(max(nq, 1), dtype=np.uint64)
    if n and nq:
        N.require_device()
    N.check(N.lib().sa_lce(t_ptr if n else None, n, sa_ptr if n else None, width, i.ctypes.data if nq else None,
                           j.ctypes.data if nq else None, nq, out.ctypes.data), "sa_lce")
    return out[:nq].astype(np.int64)


def longest_common_extension(text, sa, i, j) -> np.ndarray:
    """``lce(i, j)``, the length of the longest common prefix of the suffixes
    at text positions ``i[q]`` and ``j[q]``, for a batch of pairs on the GPU
    (sa_lce): int64.  A position at or past the end is the empty suffix (0);
    ``lce(i, i) = n - i``.  LCP, the inverse suffix array and the index are
    computed for the call from ``(text, sa)``; LCEIndex keeps them in HBM."""
    t, s = _text_and_sa(text, sa)
    return _lce_host(t.ctypes.data, int(t.size), s.ctypes.data, 8 if s.dtype == np.int64 else 4, i, j)


def compare_substrings(text, sa, i, li, j, lj) -> np.ndarray:
    """Order of the substrings ``text[i:i + li]`` and ``text[j:j + lj]``
    (lengths clipped to the text's end) for a batch of pairs on the GPU
    (sa_substr_compare): int8, -1, 0 or +1, what comparing the two bytes
    objects gives."""
    t, s = _text_and_sa(text, sa)
    i, li, j, lj = _lce_queries(i, li, j, lj)
    n, nq = int(t.size), int(i.size)
    out = np.zeros(max(nq, 1), dtype=np.int8)
    if n and nq:
        N.require_device()
    p = lambda a: a.ctypes.data if nq else None  # noqa: E731
    N.check(N.lib().sa_substr_compare(t.ctypes.data if n else None, n, s.ctypes.data if n else None,
                                      8 if s.dtype == np.int64 else 4, p(i), p(li), p(j), p(lj), nq, out.ctypes.data),
            "sa_substr_compare")
    return out[:nq]


def _to_torch(a: np.ndarray):
    """A numpy array as a host tensor (copied first when it is read-only: torch wants a writable one)."""
    import torch
    return torch.from_numpy(a if a.flags.writeable else a.copy())


def _dev_ptr(x):
    """The device address of a tensor (None for an empty one) or an int as it is."""
    if x is None:
        return None
    if isinstance(x, int):
        return x
    return int(x.data_ptr()) if x.numel() else None


def _dev_words(x, name: str):
    """A contiguous device tensor of 32-bit entries."""
    if not hasattr(x, "data_ptr") or x.element_size() != 4 or not x.is_contiguous():
        raise ValueError(f"{name}: a contiguous device tensor of 32-bit entries")
    return x


def _lce_build_dev(L, lcp, stream=None):
    import torch
    lcp = _dev_words(lcp, "lcp")
    n = int(lcp.numel())
    nbytes = int(L.sa_lce_index_bytes(n))
    index = torch.empty(nbytes, dtype=torch.uint8, device=lcp.device)
    N.check(L.sa_lce_build_device(n, _dev_ptr(lcp), _dev_ptr(index), nbytes, _stream(stream)), "sa_lce_build_device")
    return index


def _lce_same_length(*qs):
    if any(int(a.numel()) != int(qs[0].numel()) for a in qs):
        raise ValueError("query tensors of different lengths: " + ", ".join(str(int(a.numel())) for a in qs))
    return int(qs[0].numel())


def _lce_out(out, nq: int, dtype, device):
    """The output tensor of a query: the caller's (nq entries of dtype) or a new one."""
    import torch
    if out is None:
        return torch.empty(nq, dtype=dtype, device=device)
    if int(out.numel()) != nq or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"out: a contiguous {dtype} tensor of {nq} entries")
    return out


def _lcp_min_dev(L, lcp, index, lo, hi, index_bytes=None, stream=None, out=None):
    import torch
    lcp, lo, hi = _dev_words(lcp, "lcp"), _dev_words(lo, "lo"), _dev_words(hi, "hi")
    nq = _lce_same_length(lo, hi)
    out = _lce_out(out, nq, torch.int32, lo.device)
    N.check(L.sa_lcp_min_device(int(lcp.numel()), _dev_ptr(lcp), _dev_ptr(index),
                                int(index.numel()) if index_bytes is None else int(index_bytes), _dev_ptr(lo),
                                _dev_ptr(hi), nq, _dev_ptr(out), _stream(stream)), "sa_lcp_min_device")
    return out


def _lce_dev(L, isa, lcp, index, i, j, text=None, lengths=None, index_bytes=None, stream=None, out=None):
    """sa_lce_device, or sa_substr_compare_device with ``lengths = (li, lj)``."""
    import torch
    isa, lcp, i, j = _dev_words(isa, "isa"), _dev_words(lcp, "lcp"), _dev_words(i, "i"), _dev_words(j, "j")
    n = int(lcp.numel())
    if int(isa.numel()) != n or (text is not None and int(text.numel()) != n):
        raise ValueError("text, isa and lcp: the same length")
    if text is not None and (text.element_size() != 1 or not text.is_contiguous()):
        raise ValueError("text: a contiguous device tensor of bytes")
    ib = int(index.numel()) if index_bytes is None else int(index_bytes)
    if lengths is None:
        nq = _lce_same_length(i, j)
        out = _lce_out(out, nq, torch.int32, i.device)
        N.check(L.sa_lce_device(n, _dev_ptr(text), _dev_ptr(isa), _dev_ptr(lcp), _dev_ptr(index), ib, _dev_ptr(i),
                                _dev_ptr(j), nq, _dev_ptr(out), _stream(stream)), "sa_lce_device")
        return out
    li, lj = _dev_words(lengths[0], "li"), _dev_words(lengths[1], "lj")
    nq = _lce_same_length(i, li, j, lj)
    out = _lce_out(out, nq, torch.int8, i.device)
    N.check(L.sa_substr_compare_device(n, _dev_ptr(text), _dev_ptr(isa), _dev_ptr(lcp), _dev_ptr(index), ib, _dev_ptr(i),
                                       _dev_ptr(li), _dev_ptr(j), _dev_ptr(lj), nq, _dev_ptr(out), _stream(stream)),
            "sa_substr_compare_device")
    return out


class SuffixArray:
    """The reference's SuffixArray object (suffix_array.h:16-21) driven
    through the drop-in C symbols of libsa_hip.so.

    >>> s = SuffixArray(b"banana"); s.build(); s.sa   -> [5, 3, 1, 0, 4, 2]
    """

    def __init__(self, text, n: Optional[int] = None):
        raw = bytes(_as_bytes_array(text))
        self.L = N.lib()
        self.n = len(raw) if n is None else int(n)
        self._buf = ctypes.create_string_buffer(raw, max(len(raw), self.n) + 1)
        self.p = self.L.create_suffix_array(self._buf, self.n)     # manber_myers.c:51-69
        if not self.p:
            raise MemoryError("create_suffix_array returned NULL")

    def build(self) -> None:
        if self.n > 0:
            N.require_device()
        self.L.build_suffix_array(self.p)                           # :81-133

    def build_lcp(self) -> None:
        self.L.build_lcp_array(self.p)                              # :135-157

    def longest_repeated_substring(self) -> Optional[bytes]:
        r = self.L.find_longest_repeated_substring(self.p)          # :159-182
        if not r:
            return None
        s = ctypes.string_at(r)
        ctypes.CDLL(None).free(ctypes.c_void_p(r))
        return s

    def is_valid(self) -> bool:
        if self.n > 0:
            N.require_device()
        return bool(self.L.is_valid_suffix_array(self.p))           # :184-202

    def find(self, pattern, mode: str = "auto") -> tuple:
        """(lo, hi): ``pattern`` occurs at ``sa[lo:hi]`` (sa_find at width 4
        over the object's own str / sa; build() first)."""
        N.require_device()
        c = self.p.contents
        lo, hi = _find_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4, [pattern], mode)
        return int(lo[0]), int(hi[0])

    def longest_match(self, pattern, mode: str = "auto") -> tuple:
        """(length, lo, hi): the first ``length`` bytes of ``pattern`` are its
        longest prefix that occurs in the text, at ``sa[lo:hi]`` (sa_match at
        width 4 over the object's own str / sa; build() first)."""
        N.require_device()
        c = self.p.contents
        ln, lo, hi = _match_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4, [pattern], mode, True)
        return int(ln[0]), int(lo[0]), int(hi[0])

    def bwt(self) -> tuple:
        """(bytes, primary): the Burrows-Wheeler transform of the text and its
        primary index (sa_bwt at width 4 over the object's own str / sa;
        build() first)."""
        N.require_device()
        c = self.p.contents
        out, st = _bwt_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4, True)
        return out.tobytes(), int(st[0])

    def mems(self, query, min_len: int, max_occ: int = 0, max_candidates: int = 0, mode: str = "auto",
             return_info: bool = False):
        """(qpos, tpos, length): the maximal exact matches of ``query`` against
        the text, as maximal_exact_matches gives them (sa_mems at width 4 over
        the object's own str / sa; build() first)."""
        N.require_device()
        c = self.p.contents
        return _mems_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4, query, min_len, max_occ,
                          max_candidates, mode, return_info)

    def hamming(self, pattern_or_patterns, k: int, max_candidates: int = 0, mode: str = "auto",
                return_info: bool = False):
        """Occurrences with at most ``k`` substitutions, as hamming_search gives
        them (sa_hamming at width 4 over the object's own str / sa; build()
        first).  One pattern (bytes, str, bytearray, memoryview or a uint8
        array) returns ``(positions, distances)``; a sequence of patterns or a
        ``(buffer, offsets)`` pair returns ``(offsets, positions,
        distances)``."""
        N.require_device()
        c = self.p.contents
        one = isinstance(pattern_or_patterns, (bytes, bytearray, memoryview, str)) or (
            isinstance(pattern_or_patterns, np.ndarray) and pattern_or_patterns.dtype == np.uint8
            and pattern_or_patterns.ndim == 1)
        out = _hamming_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4,
                            [pattern_or_patterns] if one else pattern_or_patterns, k, max_candidates, mode, return_info)
        return out[1:] if one else out

    def edit(self, pattern_or_patterns, k: int, max_candidates: int = 0, return_starts: bool = True,
             return_info: bool = False):
        """Occurrences with at most ``k`` substitutions, insertions and
        deletions, as edit_search gives them (sa_edit at width 4 over the
        object's own str / sa; build() first).  One pattern (bytes, str,
        bytearray, memoryview or a uint8 array) returns ``(ends, starts,
        distances)``; a sequence of patterns or a ``(buffer, offsets)`` pair
        returns ``(offsets, ends, starts, distances)``."""
        N.require_device()
        c = self.p.contents
        one = isinstance(pattern_or_patterns, (bytes, bytearray, memoryview, str)) or (
            isinstance(pattern_or_patterns, np.ndarray) and pattern_or_patterns.dtype == np.uint8
            and pattern_or_patterns.ndim == 1)
        out = _edit_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4,
                         [pattern_or_patterns] if one else pattern_or_patterns, k, max_candidates, return_starts,
                         return_info)
        return out[1:] if one else out

    def lpf(self) -> tuple:
        """(lpf, src): the longest previous factor array of the text and its
        canonical sources, as longest_previous_factor gives them (sa_lpf at
        width 4 over the object's own str / sa; build() first)."""
        N.require_device()
        c = self.p.contents
        return _lpf_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4)

    def lz77(self) -> tuple:
        """(pos, length, src): the LZ77 factorisation of the text, as
        lz77_factorize gives it (sa_lz77 at width 4 over the object's own str
        / sa; build() first)."""
        N.require_device()
        c = self.p.contents
        return _lz77_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4)

    def repeats(self, min_len: int = 1, min_occ: int = 2, kind: str = "maximal") -> tuple:
        """(length, lo, hi): the repeats of the text as SA intervals, as
        maximal_repeats gives them (sa_repeats at width 4 over the object's
        own str / sa; build() first)."""
        k = _rep_kind(kind)
        N.require_device()
        c = self.p.contents
        return _repeats_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4, min_len, min_occ, k)

    def lce(self, i: int, j: int) -> int:
        """Length of the longest common prefix of the suffixes at ``i`` and
        ``j`` (sa_lce at width 4 over the object's own str / sa; build()
        first).  The one-shot form: LCEIndex answers batches."""
        c = self.p.contents
        return int(_lce_host(c.str, self.n, ctypes.cast(c.sa, ctypes.c_void_p).value, 4, [i], [j])[0])

    def count(self, pattern) -> int:
        lo, hi = self.find(pattern)
        return hi - lo

    def locate(self, pattern) -> np.ndarray:
        """Text positions of ``pattern``, ascending."""
        lo, hi = self.find(pattern)
        return np.sort(self.sa[lo:hi].astype(np.int64))

    @property
    def text(self) -> bytes:
        return ctypes.string_at(self.p.contents.str, self.n)

    @property
    def sa(self) -> np.ndarray:
        if self.n == 0:
            return np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(self.p.contents.sa, shape=(self.n,)).copy()

    @property
    def lcp(self) -> np.ndarray:
        if self.n == 0:
            return np.zeros(0, dtype=np.int32)
        return np.ctypeslib.as_array(self.p.contents.lcp, shape=(self.n,)).copy()

    def close(self) -> None:
        if getattr(self, "p", None):
            self.L.destroy_suffix_array(self.p)                     # :71-78
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class FMIndex:
    """An FM-index of a text, built on the GPU (sa_fm_build): counts and
    locates patterns with neither the text nor the suffix array, in about
    1.25 n bytes plus 8 n / sa_sample for the samples (1.5625 n at the default
    32; ``sa_sample=0``: count only).  The index is one flat byte buffer
    (``to_bytes`` / ``from_bytes``) held in host memory; every query stages it
    to the GPU as the other host forms stage the text and the SA
    (``DeviceBuilder.fm_*`` keeps it in HBM).

    >>> fm = FMIndex.from_text(b"banana"); fm.count([b"ana"])   -> [2]
    >>> fm.locate([b"ana"])                                      -> ([0, 2], [1, 3])
    """

    def __init__(self, buf: np.ndarray):
        buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
        if buf.size < N.FM_HEADER or bytes(buf[:8]) != b"SAMFIDX1":
            raise N.SAError("not an FM-index: no header")
        w = buf[:64].view(np.uint64)                  # FmHeader of csrc/sa_fm.h: n at 16, last .. rec at 32, bytes at 56
        u = buf[:56].view(np.uint32)
        self.n = int(w[2])
        self.sigma = int(u[9])
        self.sa_sample = int(u[10])
        if int(w[7]) > buf.size:
            raise N.SAError(f"not an FM-index: the header states {int(w[7])} bytes, the buffer holds {buf.size}")
        self._buf = buf[:int(w[7])]

    @property
    def nbytes(self) -> int:
        return int(self._buf.size)

    @classmethod
    def from_bwt(cls, bwt, primary: int, sa=None, sa_sample: int = 32) -> "FMIndex":
        """From ``(bwt, primary)`` as :func:`bwt` returns them.  ``sa``: the
        suffix array, sampled every ``sa_sample`` text positions; without it
        (and ``sa_sample > 0``) it is rebuilt by ``inverse_bwt``."""
        b, n, p = _bwt_and_primary(bwt, primary)
        sa_sample = int(sa_sample)
        if sa_sample < 0:
            raise ValueError("sa_sample is negative")
        if sa_sample and n and sa is None:
            sa = inverse_bwt(b, p, return_sa=True)[1]
        s = None
        if sa_sample and n:
            s = _sa_array(sa)
            if s.size != n:
                raise ValueError(f"SA has {s.size} entries for a BWT of {n} bytes")
        L = N.lib()
        cap = int(L.sa_fm_index_bytes(n, min(sa_sample, 0xFFFFFFFF)))
        buf = np.zeros(cap, dtype=np.uint8)
        info = (ctypes.c_uint64 * N.FM_INFO)()
        N.check(L.sa_fm_build(b.ctypes.data if n else None, n, p, None if s is None else s.ctypes.data,
                              8 if s is not None and s.dtype == np.int64 else 4, min(sa_sample, 0xFFFFFFFF),
                              buf.ctypes.data, cap, info), "sa_fm_build")
        return cls(buf[:int(info[2])].copy())

    @classmethod
    def from_sa(cls, text, sa, sa_sample: int = 32) -> "FMIndex":
        """From a text and its suffix array (the BWT is taken on the GPU)."""
        t, s = _text_and_sa(text, sa)
        if t.size == 0:
            return cls.from_bwt(b"", 0, None, sa_sample)
        b, p = bwt(t, s)
        return cls.from_bwt(b, p, s, sa_sample)

    @classmethod
    def from_text(cls, text, sa_sample: int = 32) -> "FMIndex":
        """Suffix array, BWT and index in one go, all on the GPU."""
        t = _as_bytes_array(text)
        if t.size == 0:
            return cls.from_bwt(b"", 0, None, sa_sample)
        return cls.from_sa(t, build_suffix_array(t), sa_sample)

    def to_bytes(self) -> bytes:
        return self._buf.tobytes()

    @classmethod
    def from_bytes(cls, data) -> "FMIndex":
        return cls(np.frombuffer(bytes(data), dtype=np.uint8))

    def find(self, patterns):
        """``(lo, hi)``, int64: where pattern q occurs, exactly the interval
        of find_patterns; where it does not, ``(0, 0)`` (not the insertion
        point).  The empty pattern gives ``(0, n)``."""
        buf, off = _pack_patterns(patterns)
        nq = int(off.size) - 1
        lo = np.zeros(nq, dtype=np.uint64)
        hi = np.zeros(nq, dtype=np.uint64)
        N.check(N.lib().sa_fm_count(self._buf.ctypes.data, self.nbytes, buf.ctypes.data if buf.size else None,
                                    off.ctypes.data, nq, lo.ctypes.data, hi.ctypes.data), "sa_fm_count")
        return lo.astype(np.int64), hi.astype(np.int64)

    def count(self, patterns) -> np.ndarray:
        """Occurrences of each pattern (int64)."""
        lo, hi = self.find(patterns)
        return hi - lo

    def locate(self, patterns, max_hits: int = 0, order: str = "text"):
        """``(offsets, positions)`` as locate_batch returns them: the
        occurrences of pattern q are ``positions[offsets[q]:offsets[q + 1]]``,
        ascending (``order="sa"``: SA order; at most ``max_hits`` of them, the
        first in SA order)."""
        lo, hi = self.find(patterns)
        return self.locate_intervals(lo, hi, max_hits, order)

    def locate_intervals(self, lo, hi, max_hits: int = 0, order: str = "text", _chunks: bool = False):
        """locate_intervals with the index in place of the suffix array."""
        flags = _locate_flags(order, _chunks)
        if max_hits < 0:
            raise ValueError("max_hits is negative")
        lo = np.ascontiguousarray(lo, dtype=np.uint64).reshape(-1)
        hi = np.ascontiguousarray(hi, dtype=np.uint64).reshape(-1)
        if lo.size != hi.size:
            raise ValueError(f"{lo.size} lower and {hi.size} upper bounds")
        nq = int(lo.size)
        cnt = np.where(hi >= lo, hi - lo, 0)
        if max_hits:
            cnt = np.minimum(cnt, np.uint64(max_hits))
        total = int(cnt.sum(dtype=np.uint64))
        off = np.zeros(nq + 1, dtype=np.uint64)
        pos = np.empty(max(total, 1), dtype=np.uint32)
        N.check(N.lib().sa_fm_locate(self._buf.ctypes.data, self.nbytes, lo.ctypes.data if nq else None,
                                     hi.ctypes.data if nq else None, nq, int(max_hits), flags, off.ctypes.data,
                                     pos.ctypes.data, 4, total), "sa_fm_locate")
        return off.astype(np.int64), pos[:total].astype(np.int64)


class Collection:
    """A collection of documents behind one suffix array built on the GPU.

    The documents are concatenated, each followed by the one-byte
    ``separator`` when one is given (it lies inside its document's range, so
    a pattern without that byte never matches across two documents).  Without
    a separator nothing is inserted and an occurrence belongs to the document
    in which it starts.  The suffix array is built at once; the document
    array and PRV on the first query that needs them.

    >>> with Collection([b"abab", b"", b"ba"], separator=b"\\x00") as c:
    ...     c.document_frequency([b"ab", b"ba"])     -> [1, 2]
    """

    def __init__(self, documents, separator=None):
        parts = [_as_bytes_array(d).reshape(-1) for d in documents]
        if not parts:
            raise ValueError("a collection has at least one document")
        if separator is not None:
            sep = _as_bytes_array(separator).reshape(-1)
            if sep.size != 1:
                raise ValueError("separator: one byte")
            parts = [np.concatenate([p, sep]) for p in parts]
        self._off = np.zeros(len(parts) + 1, dtype=np.uint64)
        self._off[1:] = np.cumsum([p.size for p in parts], dtype=np.uint64)
        self._text = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint8)
        self.n = int(self._text.size)
        self.D = len(parts)
        self._sa = build_suffix_array(self._text) if self.n else np.zeros(0, dtype=np.uint32)
        self._da = self._prev = None

    def _docs(self):
        if self._da is None:
            self._da, self._prev = document_array(self._sa, self._off)
        return self._da, self._prev

    @property
    def doc_offsets(self) -> np.ndarray:
        """The D + 1 offsets of the documents in the concatenated text (int64)."""
        return self._off.astype(np.int64)

    @property
    def text(self) -> bytes:
        return self._text.tobytes()

    @property
    def sa(self) -> np.ndarray:
        return self._sa.copy()

    def find(self, patterns):
        """(lo, hi) of each pattern in the collection's suffix array, as find_patterns gives them."""
        return find_patterns(self._text, self._sa, patterns)

    def count(self, patterns) -> np.ndarray:
        """Occurrences of each pattern over all documents (int64)."""
        lo, hi = self.find(patterns)
        return hi - lo

    def document_frequency(self, patterns) -> np.ndarray:
        """In how many documents each pattern occurs (int64)."""
        lo, hi = self.find(patterns)
        return document_frequency(self._docs()[1], lo, hi)

    def list_documents(self, patterns, max_docs: int = 0):
        """``(offsets, docs)`` in CSR form: pattern q occurs in the documents
        ``docs[offsets[q]:offsets[q + 1]]``, ascending (list_documents)."""
        lo, hi = self.find(patterns)
        da, prev = self._docs()
        return list_documents(da, prev, lo, hi, max_docs)

    def locate(self, patterns) -> list:
        """Per pattern ``(doc, offset)``, two int64 arrays: its occurrences in
        text order as (document, position inside the document)."""
        lo, hi = self.find(patterns)
        off, pos = locate_intervals(self._sa, lo, hi)
        doc, rel = doc_of_positions(self._off, self.n, pos)
        return [(doc[a:b], rel[a:b]) for a, b in zip(off[:-1].tolist(), off[1:].tolist())]

    def close(self) -> None:
        self._sa = np.zeros(0, dtype=np.uint32)
        self._text = np.zeros(0, dtype=np.uint8)
        self._da = self._prev = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class LCEIndex:
    """Longest common extensions of a text, answered on the GPU: the text, its
    inverse suffix array, its LCP array, its suffix array and the range-minimum
    index over LCP (sa_lce_build_device; about 0.4 n bytes) stay in HBM, and a
    batch of queries is one kernel.

    >>> with LCEIndex.from_text(b"abababc") as x:
    ...     x.lce([0, 1], [2, 3])                   -> [4, 3]
    ...     x.compare([0], [2], [2], [2])           -> [0]      (b"ab" == b"ab")
    ...     x.interval_depth([0], [3])              -> [2]      (ranks 0 .. 2 share b"ab")
    """

    _MAGIC = b"SALCEBL1"

    def __init__(self, text, isa, lcp, index, sa=None):
        self.L = N.lib()
        self.n = int(lcp.numel())
        self._text, self._isa, self._lcp, self._index, self._sa = text, isa, lcp, index, sa

    @staticmethod
    def _padded(torch, nbytes: int, dtype, count: int):
        """``count`` entries at the front of an allocation of at least nbytes bytes, zeroed."""
        item = torch.empty(0, dtype=dtype).element_size()
        return torch.zeros((nbytes + item - 1) // item + 64, dtype=dtype, device="cuda")[:count]

    @classmethod
    def _from_device_sa(cls, b, torch, d_text, n: int, d_sa) -> "LCEIndex":
        d_lcp = cls._padded(torch, 4 * n, torch.int32, n)
        d_isa = cls._padded(torch, 4 * n, torch.int32, n)
        if n:
            b.lcp(d_text, n, d_sa, d_lcp)
            b.inverse(n, d_sa, d_isa)
        return cls(d_text, d_isa, d_lcp, _lce_build_dev(b.L, d_lcp), d_sa)

    @classmethod
    def from_sa(cls, text, sa) -> "LCEIndex":
        """From a text and its suffix array (checked on the GPU: SAError when it is not)."""
        import torch
        t, s = _text_and_sa(text, sa)
        n = int(t.size)
        N.require_device()
        if n and s.dtype == np.int64:
            if int(s.min()) < 0 or int(s.max()) >= n:
                raise N.SAError("LCEIndex: SA entry out of range")
        b = DeviceBuilder(max(n, 1))
        try:
            d_text = cls._padded(torch, n + 256, torch.uint8, n)
            d_sa = cls._padded(torch, 4 * n, torch.int32, n)
            if n:
                d_text.copy_(_to_torch(t))
                d_sa.copy_(_to_torch(s.astype(np.uint32).view(np.int32)))
                if not b.check(d_text, n, d_sa):
                    raise N.SAError("LCEIndex: not a valid suffix array of the text")
            return cls._from_device_sa(b, torch, d_text, n, d_sa)
        finally:
            b.close()

    @classmethod
    def from_text(cls, text) -> "LCEIndex":
        """Suffix array, LCP, inverse and index in one go, all on the GPU."""
        import torch
        t = _as_bytes_array(text).reshape(-1)
        n = int(t.size)
        N.require_device()
        b = DeviceBuilder(max(n, 1))
        try:
            d_text = cls._padded(torch, n + 256, torch.uint8, n)
            d_sa = cls._padded(torch, 4 * n, torch.int32, n)
            if n:
                d_text.copy_(_to_torch(t))
                b.build(d_text, n, d_sa)
            return cls._from_device_sa(b, torch, d_text, n, d_sa)
        finally:
            b.close()

    @property
    def nbytes(self) -> int:
        """Bytes of the range-minimum index alone."""
        return int(self._index.numel())

    def _queries(self, *arrays):
        import torch
        qs = [np.minimum(a, np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32) for a in _lce_queries(*arrays)]
        return [torch.from_numpy(a).to(self._lcp.device) for a in qs]

    def _open(self):
        if self._lcp is None:
            raise N.SAError("the LCEIndex is closed")

    def lce(self, i, j, probe: bool = True) -> np.ndarray:
        """``lce(i[q], j[q])`` for a batch of position pairs: int64.  ``probe=False``
        skips the comparison of the first bytes of the text; the answers are the same."""
        self._open()
        i, j = self._queries(i, j)
        out = _lce_dev(self.L, self._isa, self._lcp, self._index, i, j, self._text if probe else None)
        return out.cpu().numpy().view(np.uint32).astype(np.int64)

    def compare(self, i, li, j, lj, probe: bool = True) -> np.ndarray:
        """Order of ``text[i:i + li]`` and ``text[j:j + lj]`` for a batch: int8, -1, 0 or +1."""
        self._open()
        i, li, j, lj = self._queries(i, li, j, lj)
        out = _lce_dev(self.L, self._isa, self._lcp, self._index, i, j, self._text if probe else None, (li, lj))
        return out.cpu().numpy()

    def interval_depth(self, lo, hi) -> np.ndarray:
        """String depth of the SA intervals ``[lo, hi)``: the length of the
        longest common prefix of their suffixes, ``n - sa[lo]`` for an
        interval of one suffix; int64, -1 for an empty or broken interval."""
        self._open()
        lo64, hi64 = _lce_queries(lo, hi)
        lo, hi = self._queries(lo64, hi64)
        out = _lcp_min_dev(self.L, self._lcp, self._index, lo, hi)
        depth = _lce_none_to_minus_one(out.cpu().numpy().view(np.uint32))
        one = np.flatnonzero((lo64 < hi64) & (hi64 <= self.n) & (hi64 - np.minimum(lo64, hi64) == 1))
        if one.size:
            if self._sa is None:
                raise N.SAError("the depth of a one-suffix interval needs the suffix array: build with from_sa or from_text")
            import torch
            at = torch.from_numpy(lo64[one].astype(np.int64)).to(self._sa.device)
            depth[one] = self.n - self._sa[at].cpu().numpy().view(np.uint32).astype(np.int64)
        return depth

    def to_bytes(self) -> bytes:
        """Everything the queries need as one byte string: text, ISA, LCP, SA and the index."""
        self._open()
        parts = [self._text, self._isa, self._lcp, self._index] + ([self._sa] if self._sa is not None else [])
        head = self._MAGIC + np.array([self.n, self.nbytes, 0 if self._sa is None else 1], np.uint64).tobytes()
        return head + b"".join(p.cpu().numpy().tobytes() for p in parts)

    @classmethod
    def from_bytes(cls, data) -> "LCEIndex":
        import torch
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        if buf.size < 32 or bytes(buf[:8]) != cls._MAGIC:
            raise N.SAError("not an LCE index: no header")
        n, ib, has_sa = (int(x) for x in buf[8:32].view(np.uint64))
        sizes = [n, 4 * n, 4 * n, ib] + ([4 * n] if has_sa else [])
        if has_sa > 1 or ib != int(N.lib().sa_lce_index_bytes(n)) or buf.size != 32 + sum(sizes):
            raise N.SAError(f"not an LCE index: {buf.size} bytes do not hold n = {n}")
        N.require_device()
        parts, at = [], 32
        for k, size in enumerate(sizes):
            dtype = torch.uint8 if k in (0, 3) else torch.int32
            d = cls._padded(torch, size + 256, dtype, size // (1 if k in (0, 3) else 4))
            if size:
                d.copy_(torch.from_numpy(buf[at:at + size].copy().view(np.uint8 if k in (0, 3) else np.int32)))
            parts.append(d)
            at += size
        return cls(*parts)

    def close(self) -> None:
        self._text = self._isa = self._lcp = self._index = self._sa = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class DeviceBuilder:
    """Device-resident builder: text and SA live in HBM (torch tensors or raw
    device pointers).  Holds one sa_context (workspace sized for max_n)."""

    def __init__(self, max_n: int, device: int = 0):
        N.require_device()
        self.L = N.lib()
        self.ctx = ctypes.c_void_p()
        N.check(self.L.sa_context_create(device, max_n, ctypes.byref(self.ctx)), "sa_context_create")
        self.device = device

    @staticmethod
    def _ptr(x) -> int:
        return x if isinstance(x, int) else int(x.data_ptr())

    @classmethod
    def _opt(cls, x):
        """A pointer that may be absent (None: NULL)."""
        return None if x is None else cls._ptr(x)

    def build(self, d_text, n: int, d_sa, stream=None, profile: bool = False, schedule: str = "packed",
              init_chars: int = 0, radix: str = "onesweep", round1: str = "auto", debug=(), span_extra: int = 0,
              tune: int = 0) -> dict:
        """Build the SA of the n bytes at d_text into the n uint32 at d_sa."""
        st = N.SaStats()
        s = _stream(stream)
        N.check(self.L.sa_build_device(self.ctx, self._ptr(d_text), n, self._ptr(d_sa), s,
                                       ctypes.byref(_opts(profile, schedule, init_chars, radix, round1, debug,
                                                          span_extra, tune)),
                                       ctypes.byref(st)),
                "sa_build_device")
        return st.to_dict()

    def set_debug(self, debug=(), span_extra: int = 0, tune: int = 0) -> None:
        """Debug / tune fields for the context's sa_dist_* phases (they take
        no sa_opts; sa_build_device applies its own)."""
        N.check(self.L.sa_context_set_debug(self.ctx, ctypes.byref(_opts(debug=debug, span_extra=span_extra,
                                                                          tune=tune))), "sa_context_set_debug")

    def generate_text(self, d_out, n: int, alphabet: bytes, seed: int = 1, stream=None) -> None:
        """Fill n device bytes with the seeded splitmix64 text."""
        s = _stream(stream)
        N.check(self.L.sa_generate_text_device(self._ptr(d_out), n, seed, alphabet, len(alphabet), s),
                "sa_generate_text_device")

    def check(self, d_text, n: int, d_sa, stream=None) -> bool:
        s = _stream(stream)
        return bool(N.check(self.L.sa_check_device(self.ctx, self._ptr(d_text), n, self._ptr(d_sa), s),
                            "sa_check_device"))

    def lcp(self, d_text, n: int, d_sa, d_lcp, stream=None) -> tuple:
        """LCP of the SA at d_sa into the n uint32 at d_lcp (16-byte aligned,
        not d_sa: the placement stores 16 bytes at a time; a misaligned d_lcp
        raises SAError before any launch); returns the longest repeated
        substring as (length, SA position).  d_sa must be a valid suffix array
        of the text (check).  Waits for ``stream``."""
        s = _stream(stream)
        ln, pos = ctypes.c_uint64(), ctypes.c_uint64()
        N.check(self.L.sa_lcp_device(self.ctx, self._ptr(d_text), n, self._ptr(d_sa), self._ptr(d_lcp),
                                     ctypes.byref(ln), ctypes.byref(pos), s), "sa_lcp_device")
        return int(ln.value), int(pos.value)

    def find(self, d_text, n: int, d_sa, d_pat, pat_bytes: int, d_off, nq: int, d_lo, d_hi, stream=None,
             mode: str = "auto") -> None:
        """SA intervals of nq patterns, everything in HBM (sa_find_device):
        pattern q is bytes d_off[q] .. d_off[q + 1] (uint64, nq + 1 entries) of
        the pat_bytes at d_pat; [d_lo[q], d_hi[q]) (uint32) is its interval in
        the SA at d_sa.  Enqueued on ``stream``; does not wait for it."""
        flags = _find_mode(mode)
        s = _stream(stream)
        N.check(self.L.sa_find_device(self._ptr(d_text), n, self._ptr(d_sa), self._ptr(d_pat), pat_bytes,
                                      self._ptr(d_off), nq, self._ptr(d_lo), self._ptr(d_hi), flags, s),
                "sa_find_device")

    def match(self, d_text, n: int, d_sa, d_pat, pat_bytes: int, d_off, nq: int, d_len, d_lo=None, d_hi=None,
              stream=None, mode: str = "auto") -> None:
        """Longest match of nq patterns, everything in HBM (sa_match_device):
        the patterns are given as for find; d_len[q] (uint32) is the length of
        pattern q's longest prefix that occurs in the text and
        [d_lo[q], d_hi[q]) that prefix's interval in the SA at d_sa.
        ``d_lo=None, d_hi=None`` asks for the lengths only.  Enqueued on
        ``stream``; does not wait for it."""
        flags = _find_mode(mode)
        s = _stream(stream)
        N.check(self.L.sa_match_device(self._ptr(d_text), n, self._ptr(d_sa), self._ptr(d_pat), pat_bytes,
                                       self._ptr(d_off), nq, self._ptr(d_len),
                                       None if d_lo is None else self._ptr(d_lo),
                                       None if d_hi is None else self._ptr(d_hi), flags, s),
                "sa_match_device")

    def matching_statistics(self, d_text, n: int, d_sa, d_query, m: int, d_len, d_lo=None, d_hi=None,
                            max_len: int = 0, stream=None, mode: str = "auto") -> None:
        """Matching statistics of the m bytes at d_query against the text,
        everything in HBM (sa_matching_stats_device): entry i of d_len, d_lo
        and d_hi (uint32, m entries each) answers d_query[i : i + max_len]
        (to the end when max_len is 0) as match does.  ``d_lo=None,
        d_hi=None`` asks for the lengths only.  Enqueued on ``stream``; does
        not wait for it."""
        flags = _find_mode(mode)
        s = _stream(stream)
        N.check(self.L.sa_matching_stats_device(self._ptr(d_text), n, self._ptr(d_sa), self._ptr(d_query), m, max_len,
                                                self._ptr(d_len), None if d_lo is None else self._ptr(d_lo),
                                                None if d_hi is None else self._ptr(d_hi), flags, s),
                "sa_matching_stats_device")

    def bwt(self, d_text, n: int, d_sa, d_bwt, d_stats=None, stream=None) -> None:
        """Burrows-Wheeler transform of the text from the SA at d_sa into the
        n bytes at d_bwt (any byte alignment), everything in HBM
        (sa_bwt_device).  ``d_stats``: N.BWT_STATS uint64 words in device
        memory ([0] primary index, [1] runs, [2 + c] count of byte c), zeroed
        and filled by the call; None skips the statistics.  Enqueued on
        ``stream``; does not wait for it."""
        s = _stream(stream)
        N.check(self.L.sa_bwt_device(self._ptr(d_text), n, self._ptr(d_sa), self._ptr(d_bwt),
                                     None if d_stats is None else self._ptr(d_stats), s), "sa_bwt_device")

    def inverse(self, n: int, d_sa, d_isa, stream=None) -> None:
        """Inverse suffix array of the SA at d_sa into the n uint32 at d_isa
        (16-byte aligned, not d_sa): d_isa[d_sa[r]] = r (sa_inverse_device).
        Waits for ``stream``; raises SAError when d_sa is not a permutation."""
        s = _stream(stream)
        N.check(self.L.sa_inverse_device(self.ctx, n, self._ptr(d_sa), self._ptr(d_isa), s), "sa_inverse_device")

    def lf(self, d_bwt, n: int, primary: int, d_lf, stream=None) -> None:
        """LF-mapping of the n BWT bytes at d_bwt (any byte alignment) with
        primary index ``primary`` into the n uint32 at d_lf (sa_lf_device;
        see lf_mapping).  Enqueued on ``stream``; does not wait for it."""
        s = _stream(stream)
        N.check(self.L.sa_lf_device(self.ctx, self._ptr(d_bwt), n, primary, self._ptr(d_lf), s), "sa_lf_device")

    def ibwt(self, d_bwt, n: int, primary: int, d_text, d_sa=None, stream=None) -> dict:
        """Inverse BWT in HBM (sa_ibwt_device): the text of (d_bwt, primary)
        into the n bytes at d_text (any byte alignment, not d_bwt) and, when
        ``d_sa`` is given, its suffix array into the n uint32 there.  One host
        wait.  Returns the info dict of inverse_bwt.  A pair that is no BWT
        raises SAError, "not a BWT", and leaves d_text and d_sa untouched."""
        s = _stream(stream)
        info = (ctypes.c_uint64 * N.IBWT_INFO)()
        N.check(self.L.sa_ibwt_device(self.ctx, self._ptr(d_bwt), n, primary, self._ptr(d_text), self._opt(d_sa),
                                      info, s), "sa_ibwt_device")
        return _ibwt_info(info)

    def fm_index_bytes(self, n: int, sa_sample: int = 32) -> int:
        """Bytes to allocate for the index of n BWT bytes before its alphabet
        is known (sa_fm_index_bytes)."""
        return int(self.L.sa_fm_index_bytes(n, sa_sample))

    def fm_build(self, d_bwt, n: int, primary: int, d_index, index_bytes: int, d_sa=None, sa_sample: int = 32,
                 stream=None) -> dict:
        """FM-index of the n BWT bytes at d_bwt into the index_bytes >=
        fm_index_bytes(n, sa_sample) bytes at d_index (16-byte aligned), in
        HBM (sa_fm_build_device).  ``d_sa``: the suffix array, None iff
        ``sa_sample`` is 0; it and the text may be freed afterwards.  One
        host wait.  Returns ``{"sigma", "class", "bytes", "samples"}``."""
        info = (ctypes.c_uint64 * N.FM_INFO)()
        N.check(self.L.sa_fm_build_device(self.ctx, self._ptr(d_bwt), n, primary, self._opt(d_sa), int(sa_sample),
                                          self._ptr(d_index), int(index_bytes), info, _stream(stream)),
                "sa_fm_build_device")
        return {"sigma": int(info[0]), "class": int(info[1]), "bytes": int(info[2]), "samples": int(info[3])}

    def fm_count(self, d_index, index_bytes: int, d_pat, pat_bytes: int, d_off, nq: int, d_lo, d_hi,
                 stream=None) -> None:
        """Backward search of nq patterns (given as for find) in the index at
        d_index (sa_fm_count_device): [d_lo[q], d_hi[q]) is find's interval
        where the pattern occurs and (0, 0) where it does not.  Enqueued on
        ``stream``; does not wait for it."""
        N.check(self.L.sa_fm_count_device(self._ptr(d_index), int(index_bytes), self._ptr(d_pat), pat_bytes,
                                          self._ptr(d_off), nq, self._ptr(d_lo), self._ptr(d_hi), _stream(stream)),
                "sa_fm_count_device")

    def fm_locate(self, d_index, index_bytes: int, d_lo, d_hi, nq: int, d_off, d_pos, pos_cap: int,
                  max_hits: int = 0, order: str = "text", stream=None, _chunks: bool = False) -> int:
        """locate with the index at d_index in place of (n, d_sa)
        (sa_fm_locate_device): the same outputs, the same sizing call with
        ``d_pos=None``.  Returns the total number of hits.  Waits for
        ``stream``."""
        total = ctypes.c_uint64()
        N.check(self.L.sa_fm_locate_device(self.ctx, self._ptr(d_index), int(index_bytes), self._ptr(d_lo),
                                           self._ptr(d_hi), nq, int(max_hits), _locate_flags(order, _chunks),
                                           self._ptr(d_off), None if d_pos is None else self._ptr(d_pos), int(pos_cap),
                                           ctypes.byref(total), _stream(stream)), "sa_fm_locate_device")
        return int(total.value)

    def locate(self, n: int, d_sa, d_lo, d_hi, nq: int, d_off, d_pos, pos_cap: int, max_hits: int = 0,
               order: str = "text", stream=None, _chunks: bool = False) -> int:
        """Sorted hit lists of nq SA intervals in CSR form, everything in HBM
        (sa_locate_device): d_lo / d_hi (uint32) as find writes them, d_off
        nq + 1 uint64, d_pos pos_cap uint32 at any 4-byte alignment.  Returns
        the total number of hits.  Positions are written only when the total
        fits pos_cap and d_pos is not None: call once with ``d_pos=None`` to
        size the output, allocate, and call again.  Waits for ``stream``."""
        s = _stream(stream)
        total = ctypes.c_uint64()
        N.check(self.L.sa_locate_device(self.ctx, n, self._ptr(d_sa), self._ptr(d_lo), self._ptr(d_hi), nq,
                                        int(max_hits), _locate_flags(order, _chunks), self._ptr(d_off),
                                        None if d_pos is None else self._ptr(d_pos), int(pos_cap),
                                        ctypes.byref(total), s), "sa_locate_device")
        return int(total.value)

    def doc_array(self, n: int, d_sa, d_doc_off, D: int, d_da, d_prev=None, stream=None) -> None:
        """Document array and PRV of a collection, everything in HBM
        (sa_doc_array_device): d_sa n uint32, d_doc_off D + 1 uint64, d_da /
        d_prev n uint32 each (either may be None, not both).  d_da alone is
        only enqueued on ``stream``; with d_prev the call waits for it once
        (the radix sort by document)."""
        o = self._opt
        N.check(self.L.sa_doc_array_device(self.ctx, n, o(d_sa), self._ptr(d_doc_off), int(D), o(d_da), o(d_prev),
                                           _stream(stream)), "sa_doc_array_device")

    def doc_of(self, d_doc_off, D: int, n: int, d_pos, count: int, d_doc, d_rel=None, stream=None) -> None:
        """(document, offset inside it) of count uint32 positions, everything
        in HBM (sa_doc_of_device): d_doc / d_rel count uint32 each (either may
        be None, not both), N.DOC_NONE for a position that is not below n.
        Enqueued on ``stream``; does not wait for it."""
        o = self._opt
        N.check(self.L.sa_doc_of_device(self._ptr(d_doc_off), int(D), n, o(d_pos), count, o(d_doc), o(d_rel),
                                        _stream(stream)), "sa_doc_of_device")

    def doc_frequency(self, n: int, d_prev, d_lo, d_hi, nq: int, d_df, stream=None) -> None:
        """Document frequency of nq SA intervals, everything in HBM
        (sa_doc_frequency_device): d_lo / d_hi (uint32) as find, match,
        fm_count or repeats write them, d_df nq uint32.  Enqueued on
        ``stream``; does not wait for it."""
        o = self._opt
        N.check(self.L.sa_doc_frequency_device(n, o(d_prev), o(d_lo), o(d_hi), nq, o(d_df), _stream(stream)),
                "sa_doc_frequency_device")

    def doc_list(self, n: int, d_da, d_prev, d_lo, d_hi, nq: int, d_off, d_docs, docs_cap: int, max_docs: int = 0,
                 order: str = "doc", stream=None) -> int:
        """The distinct documents of nq SA intervals in CSR form, everything in
        HBM (sa_doc_list_device): d_off nq + 1 uint64, d_docs docs_cap uint32
        at any 4-byte alignment.  Returns the total number of ids.  They are
        written only when the total fits docs_cap and d_docs is not None: call
        once with ``d_docs=None`` to size the output, allocate, and call
        again.  Waits for ``stream``."""
        o = self._opt
        total = ctypes.c_uint64()
        N.check(self.L.sa_doc_list_device(self.ctx, n, o(d_da), o(d_prev), o(d_lo), o(d_hi), nq, int(max_docs),
                                          _doc_order(order), o(d_off), o(d_docs), int(docs_cap), ctypes.byref(total),
                                          _stream(stream)), "sa_doc_list_device")
        return int(total.value)

    def lce_index_bytes(self, n: int) -> int:
        """Bytes of the LCE index of n ranks (sa_lce_index_bytes): exact."""
        return int(self.L.sa_lce_index_bytes(n))

    def lce_build(self, lcp, stream=None):
        """The range-minimum index over the LCP array in the device tensor
        ``lcp`` (n 32-bit entries, 16-byte aligned, as ``lcp`` writes them), in
        HBM (sa_lce_build_device): a new uint8 tensor of lce_index_bytes(n)
        bytes.  Enqueued on ``stream``; does not wait for it."""
        return _lce_build_dev(self.L, lcp, stream)

    def lcp_min(self, lcp, index, lo, hi, stream=None, index_bytes=None, out=None):
        """``min lcp[lo + 1 : hi]`` of the SA intervals in the device tensors
        ``lo`` / ``hi`` (32-bit entries, as find, match, fm_count or repeats
        write them), everything in HBM (sa_lcp_min_device): an int32 tensor
        whose bits are uint32, N.LCE_NONE where there is no minimum (``out``,
        or a new one).  Enqueued on ``stream``; does not wait for it."""
        return _lcp_min_dev(self.L, lcp, index, lo, hi, index_bytes, stream, out)

    def lce(self, isa, lcp, index, i, j, text=None, stream=None, index_bytes=None, out=None):
        """``lce(i[q], j[q])`` of the text positions in the device tensors
        ``i`` / ``j`` (32-bit entries), everything in HBM (sa_lce_device):
        ``isa`` as ``inverse`` writes it, ``lcp`` as ``lcp`` does, ``index`` from
        ``lce_build``; with ``text`` (the n bytes) the first N.LCE_PROBE bytes
        are compared before the arrays are asked.  An int32 tensor whose bits
        are uint32 (``out``, or a new one).  Enqueued on ``stream``; does not
        wait for it."""
        return _lce_dev(self.L, isa, lcp, index, i, j, text, None, index_bytes, stream, out)

    def substr_compare(self, isa, lcp, index, i, li, j, lj, text=None, stream=None, index_bytes=None, out=None):
        """Order of the substrings ``[i, i + li)`` and ``[j, j + lj)`` of the
        text, everything in HBM (sa_substr_compare_device): an int8 tensor of
        -1, 0, +1 (``out``, or a new one).  The arguments of ``lce`` plus the
        two length tensors.  Enqueued on ``stream``; does not wait for it."""
        return _lce_dev(self.L, isa, lcp, index, i, j, text, (li, lj), index_bytes, stream, out)

    def mems(self, d_text, n: int, d_sa, d_query, m: int, min_len: int, d_off, d_tpos, d_len, out_cap: int,
             max_occ: int = 0, max_candidates: int = 0, mode: str = "auto", stream=None) -> tuple:
        """Maximal exact matches of the m bytes at d_query against the text,
        everything in HBM (sa_mems_device): d_off m + 1 uint64, d_tpos / d_len
        out_cap uint32 each at any 4-byte alignment.  Returns ``(total,
        candidates, skipped)``.  The triples are written only when the total
        fits out_cap and d_tpos / d_len are not None: call once with
        ``d_tpos=None, d_len=None`` to size the outputs (d_off is filled),
        allocate, and call again.  Raises SAError when the candidates exceed
        ``max_candidates``.  Waits for ``stream``."""
        flags = _mem_mode(mode)
        s = _stream(stream)
        info = (ctypes.c_uint64 * N.MEM_INFO)()
        rc = N.check(self.L.sa_mems_device(self.ctx, self._ptr(d_text), n, self._ptr(d_sa), self._ptr(d_query), m,
                                           int(min_len), int(max_occ), int(max_candidates), flags, self._ptr(d_off),
                                           None if d_tpos is None else self._ptr(d_tpos),
                                           None if d_len is None else self._ptr(d_len), int(out_cap), info, s),
                     "sa_mems_device")
        if rc == N.MEM_TOO_MANY:
            raise N.SAError(f"sa_mems_device: {int(info[1])} candidates are more than max_candidates = "
                            f"{max_candidates}")
        return int(info[0]), int(info[1]), int(info[2])

    def hamming(self, d_text, n: int, d_sa, d_pat, pat_bytes: int, d_pat_off, nq: int, k: int, d_off, d_pos, d_dist,
                out_cap: int, max_candidates: int = 0, mode: str = "auto", stream=None) -> tuple:
        """Occurrences with at most ``k`` substitutions of the nq patterns at
        d_pat (pat_bytes bytes, nq + 1 uint64 offsets at d_pat_off), everything
        in HBM (sa_hamming_device): d_off nq + 1 uint64, d_pos out_cap uint32
        at any 4-byte alignment, d_dist out_cap bytes or None.  Returns
        ``(total, candidates, pieces)``.  Positions and distances are written
        only when the total fits out_cap and d_pos is not None: call once with
        ``d_pos=None, d_dist=None`` to size the outputs (d_off is filled),
        allocate, and call again.  Raises SAError when the candidates exceed
        ``max_candidates``.  Waits for ``stream``."""
        flags = _hamming_mode(mode)
        _hamming_k(k, max_candidates)
        s = _stream(stream)
        o = self._opt
        info = (ctypes.c_uint64 * N.HAMMING_INFO)()
        rc = N.check(self.L.sa_hamming_device(self.ctx, o(d_text), n, o(d_sa), o(d_pat), pat_bytes, o(d_pat_off), nq,
                                              int(k), int(max_candidates), flags, o(d_off), o(d_pos), o(d_dist),
                                              int(out_cap), info, s), "sa_hamming_device")
        if rc == N.HAMMING_TOO_MANY:
            raise N.SAError(f"sa_hamming_device: {int(info[1])} candidates are more than max_candidates = "
                            f"{max_candidates}")
        return int(info[0]), int(info[1]), int(info[2])

    def edit(self, d_text, n: int, d_sa, d_pat, pat_bytes: int, d_pat_off, nq: int, k: int, d_off, d_end, d_start,
             d_dist, out_cap: int, max_candidates: int = 0, stream=None) -> tuple:
        """Occurrences with at most ``k`` edits of the nq patterns at d_pat
        (pat_bytes bytes, nq + 1 uint64 offsets at d_pat_off), everything in
        HBM (sa_edit_device): d_off nq + 1 uint64, d_end out_cap uint32 at any
        4-byte alignment, d_start likewise or None, d_dist out_cap bytes or
        None.  Returns ``(total, candidates, pieces)``.  Ends, starts and
        distances are written only when the total fits out_cap and d_end is
        not None: call once with ``d_end=None, d_start=None, d_dist=None`` to
        size the outputs (d_off is filled), allocate, and call again.  Raises
        SAError when the candidates exceed ``max_candidates``.  Waits for
        ``stream``."""
        _edit_k(k, max_candidates)
        s = _stream(stream)
        o = self._opt
        info = (ctypes.c_uint64 * N.EDIT_INFO)()
        rc = N.check(self.L.sa_edit_device(self.ctx, o(d_text), n, o(d_sa), o(d_pat), pat_bytes, o(d_pat_off), nq,
                                           int(k), int(max_candidates), 0, o(d_off), o(d_end), o(d_start), o(d_dist),
                                           int(out_cap), info, s), "sa_edit_device")
        if rc == N.EDIT_TOO_MANY:
            raise N.SAError(f"sa_edit_device: {int(info[1])} candidates are more than max_candidates = "
                            f"{max_candidates}")
        return int(info[0]), int(info[1]), int(info[2])

    def lpf(self, d_text, n: int, d_sa, d_lcp, d_lpf, d_src, stream=None) -> None:
        """Longest previous factor array and its canonical sources into the n
        uint32 at d_lpf and d_src (text order, any 4-byte alignment; "none" is
        N.LPF_NONE), everything in HBM (sa_lpf_device).  With ``d_lcp`` (the
        LCP array of d_sa, n uint32) the text is not read and ``d_text`` may be
        None: the call is then only enqueued on ``stream``.  ``d_lcp=None``
        computes the LCP array first, as lcp does."""
        s = _stream(stream)
        o = self._opt
        N.check(self.L.sa_lpf_device(self.ctx, o(d_text), n, o(d_sa), o(d_lcp), o(d_lpf), o(d_src), s),
                "sa_lpf_device")

    def lz77(self, n: int, d_lpf, d_src, d_pos, d_len, d_fsrc, out_cap: int, stream=None) -> int:
        """Greedy LZ77 parse of the LPF / SRC arrays lpf wrote, everything in
        HBM (sa_lz77_device): phrase k is (d_pos[k], d_len[k], d_fsrc[k]),
        out_cap uint32 each at any 4-byte alignment, a literal with length 1
        and source N.LPF_NONE.  Returns z, the number of phrases.  The phrases
        are written only when z fits out_cap and the three outputs are not
        None: call once with ``None, None, None, 0`` to size them, allocate,
        and call again.  Waits for ``stream``."""
        s = _stream(stream)
        z = ctypes.c_uint64()
        o = self._opt
        N.check(self.L.sa_lz77_device(self.ctx, n, o(d_lpf), o(d_src), o(d_pos), o(d_len), o(d_fsrc), int(out_cap),
                                      ctypes.byref(z), s), "sa_lz77_device")
        return int(z.value)

    def repeats(self, d_text, n: int, d_sa, d_lcp, min_len: int, min_occ: int, kind: str, d_len, d_lo, d_hi,
                out_cap: int, stream=None) -> tuple:
        """The repeats of the text as SA intervals, everything in HBM
        (sa_repeats_device): repeat k has length d_len[k] and occurs exactly at
        d_sa[d_lo[k] .. d_hi[k]), out_cap uint32 each at any 4-byte alignment,
        in the order of their heads.  ``kind``: "right" (every right-maximal
        repeat; with ``d_lcp`` neither the text nor the SA is read and both may
        be None), "maximal" or "supermaximal".  ``d_lcp=None`` computes the LCP
        array first, as lcp does.  Returns ``(count, total_occ)``: the repeats
        and the sum of hi - lo over them, which is locate's pos_cap for
        ``locate(n, d_sa, d_lo, d_hi, count, ...)``.  They are written only
        when count fits out_cap and the three outputs are not None: call once
        with ``None, None, None, 0`` to size them, allocate, and call again.
        Waits for ``stream``."""
        s = _stream(stream)
        info = (ctypes.c_uint64 * N.REP_INFO)()
        o = self._opt
        N.check(self.L.sa_repeats_device(self.ctx, o(d_text), n, o(d_sa), o(d_lcp), int(min_len), int(min_occ),
                                         _rep_kind(kind), o(d_len), o(d_lo), o(d_hi), int(out_cap), info, s),
                "sa_repeats_device")
        return int(info[0]), int(info[1])

    def close(self) -> None:
        if self.ctx:
            self.L.sa_context_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
