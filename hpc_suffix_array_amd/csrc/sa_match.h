// sa_match.h -- longest-match queries and matching statistics over a built
// suffix array (sa_match / sa_matching_stats and their _device forms of
// include/sa_hip.h).  sa_find answers "where does P occur"; for a P that does
// not occur whole it has only an insertion point.  This answers the next
// question: which is the longest prefix of P that occurs, and where.  Asked
// at every position of a query string, that is its matching statistics.
//
// For a query P of m bytes: len is the largest l <= m for which P[0 .. l)
// occurs in the text, and [lo, hi) is the sa_find interval of P[0 .. len).
// len == m gives what sa_find gives for P; len == 0 gives [0, n) (m == 0, or
// a first byte the text does not hold); n == 0 gives len 0 and [0, 0).
//
// match_interval is find_interval (sa_find.h) with what that search throws
// away kept: its descent carries l and r, the bytes P shares with the
// suffixes just outside the two ends of the range.  When the range closes
// with no full match the two ends are the neighbours of the insertion point
// and both have been probed (an end at 0 or at n has no neighbour and stays
// 0), so len = max(l, r).  The bounds of P[0 .. len) are then the lower bound
// left of the neighbour that reached len and the upper bound right of it:
// the same two bound searches, with len in the place of m.  No suffix shares
// more than len bytes with P, so a probe of all of P matches P[0 .. len)
// exactly when it shares len bytes: the probe (cmp(rank, start, k) of
// sa_find.h) is the same one.  For the ranges of those two searches the
// descent keeps where each end stood before its shared length last grew:
// everything further out shares less than len.
// The first part of this header compiles with g++ (tests/cpp/match_check.cpp).
// The HIP part needs sa_host.h before it (the host form's staging, buffers
// and checks), and with it sa_build.hip's set_err / SA_HIP / SA_TRY.
#pragma once
#include <stdint.h>

#include "sa_find.h"

namespace sa {

// len, and with Bounds [lo, hi), of a pattern of m bytes among n suffixes;
// cmp(rank, start, k) is one probe as in find_interval.  Phase 0 descends to
// a full match M (then len = m and phases 1 and 2 are find_interval's) or
// until the range closes; phase 1 is the lower bound in [a0, M), phase 2 the
// upper bound in (M, b0); one loop, so that the probe is expanded once.
// Without Bounds it returns when len is known (lo, hi: [0, n)).  All
// positions are 64-bit.  Every probe is of a rank below n and the range
// shrinks with each, whatever cmp answers: an invalid SA ends with some
// result.
template <bool Bounds, class Cmp>
SA_HD void match_interval(uint64_t n, uint64_t m, const Cmp& cmp, uint64_t& len, uint64_t& lo, uint64_t& hi) {
    len = 0;
    lo = 0;
    hi = n;
    if (m == 0 || n == 0) return;
    // (a0, l0) / (b0, r0): the left / right end before l / r last grew.  Phase 0 ends where M and the match
    // length L begin: they take over a0 and l0, so that the search holds one position more than find_interval's
    uint64_t a = 0, b = n, l = 0, r = 0, a0 = 0, l0 = 0, b0 = n, r0 = 0, k = 0;
    uint64_t &M = a0, &L = l0;
    int phase = 0;
    bool edge = m > kFindEdge;
    for (;;) {
        if (a >= b) {
            if (phase == 0) {   // closed at the insertion point a: its neighbours are a - 1 (l) and a (r)
                const uint64_t at = a, best = l > r ? l : r;
                if (!Bounds || best == 0) {
                    len = best;
                    return;
                }
                if (l == best) {   // l > 0: a probe answered "below", so at > 0
                    b = at - 1;
                    a = a0;
                    l = l0;
                } else {           // the left neighbour falls short: lo = at, by an empty phase 1
                    b = at;
                }
                if (r == best) {   // r > 0: a probe answered "above", so at < n
                    M = at;
                } else {           // the right neighbour falls short: hi = at, by an empty phase 2
                    M = at - 1;
                    b0 = at;
                }
                L = r = best;
                phase = 1;
                continue;
            }
            if (phase == 1) {   // lower bound done: the upper bound in (M, b0), left end matched
                lo = a;
                a = M + 1;
                b = b0;
                l = L;
                r = r0;
                phase = 2;
                continue;
            }
            hi = a;
            len = L;
            return;
        }
        const uint64_t mid = edge ? b - 1 : a + ((b - a) >> 1);
        edge = false;
        const int c = cmp(mid, l < r ? l : r, k);
        if (phase == 0) {
            if (c < 0) {
                if (Bounds && k > l) {
                    a0 = a;
                    l0 = l;
                }
                a = mid + 1;
                l = k;
            } else if (c > 0) {
                if (Bounds && k > r) {
                    b0 = b;
                    r0 = r;
                }
                b = mid;
                r = k;
            } else {   // all of P: from here on as find_interval
                if (!Bounds) {
                    len = m;
                    return;
                }
                M = mid;
                L = m;
                b0 = b;
                r0 = r;
                b = mid;
                r = m;
                phase = 1;
            }
        } else if (k >= L) {   // starts with P[0 .. L)
            if (phase == 1) b = mid;
            else a = mid + 1;
        } else if (c < 0) {
            a = mid + 1;
            l = k;
        } else {
            b = mid;
            r = k;
        }
    }
}

// the scalar search: one probe = compare_words over sa_at / text_word / pat_word
template <bool Bounds, class SaAt, class TextWord, class PatWord>
SA_HD void match_scalar(uint64_t n, uint64_t m, const SaAt& sa_at, const TextWord& text_word, const PatWord& pat_word,
                        uint64_t& len, uint64_t& lo, uint64_t& hi) {
    match_interval<Bounds>(n, m, [&](uint64_t rank, uint64_t start, uint64_t& k) {
        return compare_words((uint64_t)sa_at(rank), n, m, start, text_word, pat_word, k);
    }, len, lo, hi);
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

namespace sa {

// Where the queries of a launch lie in the one byte buffer the kernels read:
// operator()(q, a, m) gives query q as bytes [a, a + m) of it.
// Batch form: query q is pattern q of an offset array (find_pattern's clamps).
struct BatchQueries {
    const uint64_t* __restrict__ off;
    uint64_t pat_bytes;
    __device__ __forceinline__ void operator()(uint64_t q, uint64_t& a, uint64_t& m) const {
        find_pattern(off, q, pat_bytes, a, m);
    }
};

// Sliding form: query i is what follows position i of a string of m bytes,
// cut at cap bytes (1 <= cap <= m; i < m).
struct SlidingQueries {
    uint64_t m, cap;
    __device__ __forceinline__ void operator()(uint64_t q, uint64_t& a, uint64_t& len) const {
        a = q;
        len = cap < m - q ? cap : m - q;
    }
};

// k_find_lane's shape: one query per lane, grid-stride over the queries of
// m in [min_m, max_m], the first two words of the query in registers.
template <bool Bounds, class Queries>
__global__ __launch_bounds__(kBlock) void k_match_lane(const uint8_t* __restrict__ text, uint64_t n,
                                                       const uint32_t* __restrict__ sa,
                                                       const uint8_t* __restrict__ pat, uint64_t pat_bytes,
                                                       const Queries queries, uint64_t nq, uint64_t min_m,
                                                       uint64_t max_m, uint32_t* __restrict__ len_out,
                                                       uint32_t* __restrict__ lo_out, uint32_t* __restrict__ hi_out) {
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock) {
        uint64_t pa, m;
        queries(q, pa, m);
        if (m < min_m || m > max_m) continue;
        const uint64_t w0 = load8(pat, pa, pat_bytes), w1 = load8(pat, pa + 8, pat_bytes);
        uint64_t len, lo, hi;
        match_scalar<Bounds>(n, m, [&](uint64_t rank) { return sa[rank]; },
                             [&](uint64_t p) { return load8(text, p, n); },
                             [&](uint64_t o) { return o == 0 ? w0 : o == 8 ? w1 : load8(pat, pa + o, pat_bytes); },
                             len, lo, hi);
        len_out[q] = (uint32_t)len;
        if (Bounds) {
            lo_out[q] = (uint32_t)lo;
            hi_out[q] = (uint32_t)hi;
        }
    }
}

// x, which is the same in every lane, in a form the compiler knows to be so
__device__ __forceinline__ uint64_t wave_uniform(uint64_t x) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32;
}

// k_find_wave's shape: one query per wavefront over WaveCompare, the
// descriptors of kFindGroup queries read together.  What reaches the search
// comes from shuffles of one lane's values, from ballots and from kernel
// arguments: it is wave-uniform, and the search runs in lockstep.  The
// shuffled values and each probe's answer pass through wave_uniform, so that
// the search's state (ten positions and lengths) lives in scalar registers
// and the kernel keeps k_find_wave's 8 waves per SIMD.
template <bool Bounds, class Queries>
__global__ __launch_bounds__(kBlock) void k_match_wave(const uint8_t* __restrict__ text, uint64_t n,
                                                       const uint32_t* __restrict__ sa,
                                                       const uint8_t* __restrict__ pat, uint64_t pat_bytes,
                                                       const Queries queries, uint64_t nq, uint64_t min_m,
                                                       uint64_t max_m, uint32_t* __restrict__ len_out,
                                                       uint32_t* __restrict__ lo_out, uint32_t* __restrict__ hi_out) {
    const uint32_t lane = lane_id();
    const uint64_t groups = (nq + kFindGroup - 1) / kFindGroup;
    for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave_id(); g < groups; g += (uint64_t)gridDim.x * kWaves) {
        const uint64_t q = g * kFindGroup + lane;
        uint64_t pa = 0, m = 0;
        bool mine = false;
        if (lane < kFindGroup && q < nq) {
            queries(q, pa, m);
            mine = m >= min_m && m <= max_m;
        }
        uint64_t todo = __ballot(mine);
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const WaveCompare cmp{text, n, sa, pat, pat_bytes,
                                  wave_uniform((uint64_t)__shfl((unsigned long long)pa, j, kWave)),
                                  wave_uniform((uint64_t)__shfl((unsigned long long)m, j, kWave))};
            uint64_t len, lo, hi;
            match_interval<Bounds>(n, cmp.m, [&](uint64_t rank, uint64_t start, uint64_t& k) {
                uint64_t shared;
                const int c = cmp(rank, start, shared);
                k = wave_uniform(shared);
                return __builtin_amdgcn_readfirstlane(c);
            }, len, lo, hi);
            if (lane == 0) {
                len_out[g * kFindGroup + j] = (uint32_t)len;
                if (Bounds) {
                    lo_out[g * kFindGroup + j] = (uint32_t)lo;
                    hi_out[g * kFindGroup + j] = (uint32_t)hi;
                }
            }
        }
    }
}

// find_device's launch shape.  lane_max: the lane kernel takes the queries of
// up to lane_max bytes and the wave kernel the rest; a kernel with nothing to
// take is not launched when that is known here (the sliding form).
template <bool Bounds, class Queries>
static void match_launch(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_buf,
                         uint64_t buf_bytes, const Queries& queries, uint64_t nq, bool lane, bool wave,
                         uint64_t lane_max, uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi, hipStream_t s) {
    // 8 workgroups of 256 threads fill a CU at 8 waves per SIMD
    const uint64_t kMaxGrid = 256 * 8;
    const uint64_t all = ~0ull;
    if (lane) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nq + kBlock - 1) / kBlock, kMaxGrid);
        hipLaunchKernelGGL((k_match_lane<Bounds, Queries>), dim3(grid), dim3(kBlock), 0, s, d_text, n, d_sa, d_buf,
                           buf_bytes, queries, nq, (uint64_t)0, wave ? lane_max : all, d_len, d_lo, d_hi);
    }
    if (wave) {
        const uint64_t groups = (nq + kFindGroup - 1) / kFindGroup;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((groups + kWaves - 1) / kWaves, kMaxGrid);
        hipLaunchKernelGGL((k_match_wave<Bounds, Queries>), dim3(grid), dim3(kBlock), 0, s, d_text, n, d_sa, d_buf,
                           buf_bytes, queries, nq, lane ? lane_max + 1 : (uint64_t)0, all, d_len, d_lo, d_hi);
    }
}

static int match_device_args(const void* d_text, const void* d_sa, const void* d_buf, const void* d_len,
                             const void* d_lo, const void* d_hi, uint64_t n) {
    if (!d_text || !d_sa || !d_buf || !d_len) return set_err(SA_E_INVALID, "NULL device pointer");
    if (!d_lo != !d_hi) return set_err(SA_E_INVALID, "d_lo and d_hi: both or neither");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    return SA_OK;
}

// batch form (sa_match_device): auto splits by pattern length at kFindLaneMax
static int match_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                        uint64_t pat_bytes, const uint64_t* d_off, uint64_t nq, uint32_t* d_len, uint32_t* d_lo,
                        uint32_t* d_hi, uint32_t flags, hipStream_t s) {
    if (flags > SA_FIND_WAVE) return set_err(SA_E_INVALID, "flags must be 0, SA_FIND_LANE or SA_FIND_WAVE");
    if (nq == 0) return SA_OK;
    if (!d_off) return set_err(SA_E_INVALID, "NULL device pointer");
    if (int rc = match_device_args(d_text, d_sa, d_pat, d_len, d_lo, d_hi, n)) return rc;
    const BatchQueries queries{d_off, pat_bytes};
    const bool lane = flags != SA_FIND_WAVE, wave = flags != SA_FIND_LANE;
    if (d_lo) match_launch<true>(d_text, n, d_sa, d_pat, pat_bytes, queries, nq, lane, wave, kFindLaneMax, d_len, d_lo, d_hi, s);
    else match_launch<false>(d_text, n, d_sa, d_pat, pat_bytes, queries, nq, lane, wave, kFindLaneMax, d_len, d_lo, d_hi, s);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// sliding form (sa_matching_stats_device): one query per position of the m
// bytes at d_query, each cut at max_len bytes (0: none).  Every position has
// the same cap, so auto cannot split by length: it takes the lane kernel when
// no query can be longer than kFindLaneMax bytes (a cap, or a short query
// string) and the wave kernel otherwise.
static int match_stats_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query,
                              uint64_t m, uint64_t max_len, uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi,
                              uint32_t flags, hipStream_t s) {
    if (flags > SA_FIND_WAVE) return set_err(SA_E_INVALID, "flags must be 0, SA_FIND_LANE or SA_FIND_WAVE");
    if (m == 0) return SA_OK;
    if (int rc = match_device_args(d_text, d_sa, d_query, d_len, d_lo, d_hi, n)) return rc;
    const uint64_t cap = max_len && max_len < m ? max_len : m;
    const SlidingQueries queries{m, cap};
    const bool lane = flags == SA_FIND_LANE || (flags == 0 && cap <= kFindLaneMax);
    if (d_lo) match_launch<true>(d_text, n, d_sa, d_query, m, queries, m, lane, !lane, 0, d_len, d_lo, d_hi, s);
    else match_launch<false>(d_text, n, d_sa, d_query, m, queries, m, lane, !lane, 0, d_len, d_lo, d_hi, s);
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// host in, host out (sa_match: off != NULL, nq patterns in buf; sa_matching_stats:
// off == NULL, nq = the length of the string at buf), over the steps of sa_host.h
static int match_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* buf,
                      const uint64_t* off, uint64_t nq, uint64_t max_len, bool sliding, uint64_t* len_out,
                      uint64_t* lo_out, uint64_t* hi_out, uint32_t flags) {
    SA_TRY(check_width(sa_width));
    if (flags > SA_FIND_WAVE) return set_err(SA_E_INVALID, "flags must be 0, SA_FIND_LANE or SA_FIND_WAVE");
    if (nq == 0) return SA_OK;
    if ((!sliding && !off) || !len_out || (n && (!text || !sa))) return set_err(SA_E_INVALID, "NULL host pointer");
    if (!lo_out != !hi_out) return set_err(SA_E_INVALID, "lo_out and hi_out: both or neither");
    SA_TRY(check_n32(n));
    uint64_t buf_bytes = nq;
    if (!sliding) {
        for (uint64_t q = 0; q < nq; ++q)
            if (off[q] > off[q + 1]) return set_err(SA_E_INVALID, "pattern offsets decrease at %llu", (unsigned long long)q);
        buf_bytes = off[nq];
    }
    if (buf_bytes && !buf) return set_err(SA_E_INVALID, "NULL host pointer");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    SA_TRY(need_device());
    const bool bounds = lo_out != nullptr;
    DevBuf d_text, d_sa, d_buf, d_off, d_res;   // d_res: len | lo | hi
    SA_TRY(d_text.alloc(align_up(n + 1, 256)));
    SA_TRY(d_sa.alloc(align_up(n + 1, 64) * 4));
    SA_TRY(d_buf.alloc(align_up(buf_bytes + 1, 256)));
    SA_TRY(d_off.alloc((sliding ? 1 : nq + 1) * 8));   // the sliding form has no offsets: nothing is uploaded
    SA_TRY(d_res.alloc(nq * 4 * (bounds ? 3 : 1)));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}, {d_buf.p, buf, buf_bytes},
                   {d_off.p, off, sliding ? 0 : (nq + 1) * 8}}));
    uint32_t* d_len = d_res.as<uint32_t>();
    uint32_t* d_lo = bounds ? d_len + nq : nullptr;
    uint32_t* d_hi = bounds ? d_len + 2 * nq : nullptr;
    SA_TRY(sliding ? match_stats_device(d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_buf.as<uint8_t>(), nq, max_len,
                                        d_len, d_lo, d_hi, flags, nullptr)
                   : match_device(d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_buf.as<uint8_t>(), buf_bytes,
                                  d_off.as<uint64_t>(), nq, d_len, d_lo, d_hi, flags, nullptr));
    return download_u64({{len_out, d_len}, {lo_out, d_lo}, {hi_out, d_hi}}, nq);
}

}  // namespace sa

extern "C" {

int sa_match_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat, uint64_t pat_bytes,
                    const uint64_t* d_pat_off, uint64_t nq, uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi,
                    uint32_t flags, void* stream) {
    return sa::match_device(d_text, n, d_sa, d_pat, pat_bytes, d_pat_off, nq, d_len, d_lo, d_hi, flags,
                            (hipStream_t)stream);
}

int sa_matching_stats_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_query,
                             uint64_t m, uint64_t max_len, uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi,
                             uint32_t flags, void* stream) {
    return sa::match_stats_device(d_text, n, d_sa, d_query, m, max_len, d_len, d_lo, d_hi, flags, (hipStream_t)stream);
}

int sa_match(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat, const uint64_t* pat_off,
             uint64_t nq, uint64_t* len_out, uint64_t* lo_out, uint64_t* hi_out, uint32_t flags) {
    return sa::match_host(text, n, sa, sa_width, pat, pat_off, nq, 0, false, len_out, lo_out, hi_out, flags);
}

int sa_matching_stats(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* query, uint64_t m,
                      uint64_t max_len, uint64_t* len_out, uint64_t* lo_out, uint64_t* hi_out, uint32_t flags) {
    return sa::match_host(text, n, sa, sa_width, query, nullptr, m, max_len, true, len_out, lo_out, hi_out, flags);
}

}  // extern "C"

#endif   // __HIPCC__
