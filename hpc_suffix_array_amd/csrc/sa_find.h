// sa_find.h -- batched exact-match pattern search over a built suffix array
// (sa_find / sa_find_device of include/sa_hip.h).  The reference stops at the
// SA, its LCP and the longest repeat; this is the query a suffix array exists
// for, answered where the SA already lies: text, SA, patterns and results all
// stay in HBM.
//
// Order: the builder's (unsigned bytes, end of string smallest).  Pattern P
// of m bytes has the interval [lo, hi) of SA positions r with
// SA[r] + m <= n and text[SA[r] .. SA[r] + m) == P; a suffix shorter than m
// that is a proper prefix of P sorts below P; lo == hi is the insertion point
// when nothing matches.
//
// One search (find_interval) serves the host check, the lane kernel and the
// wave kernel; they differ in how one probe compares P with a suffix:
//   * it descends [a, b) until a probe matches all of P, then takes the lower
//     bound left of that probe and the upper bound right of it: about
//     log2 n + 2 log2(count) probes, not 2 log2 n;
//   * it carries l and r, the bytes P shares with the suffixes just outside
//     the two ends of the range (Manber & Myers 1993, section 4, without the
//     Llcp / Rlcp tables): every suffix inside the range shares min(l, r)
//     bytes with P, so a probe starts there.  A matched end counts as m;
//   * a pattern of more than kFindEdge bytes probes the last rank first, which
//     makes the right end a real suffix: without it r stays 0 while the
//     descent only moves right (a pattern near the top of the order, a text of
//     one symbol) and every probe starts again at byte 0.
// The first part of this header compiles with g++ (tests/cpp/find_check.cpp).
// The HIP part needs sa_host.h before it (the host form's staging, buffers
// and checks), and with it sa_build.hip's set_err / SA_HIP / SA_TRY.
#pragma once
#include <stdint.h>

#include "sa_search.h"   // SA_HD

namespace sa {

// patterns of up to kFindLaneMax bytes go to k_find_lane in auto mode, longer
// ones to k_find_wave (= SA_FIND_LANE_MAX of include/sa_hip.h)
constexpr uint64_t kFindLaneMax = 3584;
constexpr uint64_t kFindEdge = 16;    // longer patterns probe rank n - 1 first
constexpr uint32_t kFindGroup = 8;    // queries one wavefront looks at together (k_find_wave)

// One probe by 8-byte words: P against the suffix at s from byte `start`
// (rounded down to a word of P, so that the lane kernel's register words
// line up) on.  k = the bytes they share; < 0: the suffix sorts below P
// (a mismatch, or the suffix ends inside P), 0: P is a prefix of it, > 0: above.
// text_word(p): little-endian 8 bytes at text position p, zero at or past n;
// pat_word(q): the same at byte q of P (what lies past m is cut at lim).
// The words are byte-swapped so that the integer compare is the
// lexicographic one.  s >= n (an invalid SA) reads as the empty suffix.
template <class TextWord, class PatWord>
SA_HD int compare_words(uint64_t s, uint64_t n, uint64_t m, uint64_t start, const TextWord& text_word,
                        const PatWord& pat_word, uint64_t& k) {
    const uint64_t slen = s < n ? n - s : 0;
    const uint64_t lim = m < slen ? m : slen;
    for (uint64_t off = start & ~7ull; off < lim; off += 8) {
        const uint64_t a = __builtin_bswap64(text_word(s + off)), b = __builtin_bswap64(pat_word(off));
        if (a != b) {
            const uint64_t j = off + (uint64_t)(__builtin_clzll(a ^ b) >> 3);
            if (j < lim) {
                k = j;
                return a > b ? 1 : -1;
            }
            break;
        }
    }
    k = lim;
    return lim == m ? 0 : -1;
}

// [lo, hi) of a pattern of m bytes among n suffixes; cmp(rank, start, k) is
// one probe as above.  Phase 0 descends to a match M, phase 1 is the lower
// bound in [a, M), phase 2 the upper bound in (M, b); one loop, so that the
// probe is expanded once.  All positions are 64-bit (a + b passes 2^32 above
// n = 2^31).  Every probe is of a rank below n and the range shrinks with
// each, whatever cmp answers: an invalid SA ends with some interval.
template <class Cmp>
SA_HD void find_interval(uint64_t n, uint64_t m, const Cmp& cmp, uint64_t& lo, uint64_t& hi) {
    lo = 0;
    hi = n;
    if (m == 0 || n == 0) return;
    uint64_t a = 0, b = n, l = 0, r = 0, M = 0, b0 = 0, r0 = 0, k = 0;
    int phase = 0;
    bool edge = m > kFindEdge;
    for (;;) {
        if (a >= b) {
            if (phase == 0) {
                lo = hi = a;
                return;
            }
            if (phase == 1) {   // lower bound done: the upper bound in (M, b0), left end matched
                lo = a;
                a = M + 1;
                b = b0;
                l = m;
                r = r0;
                phase = 2;
                continue;
            }
            hi = a;
            return;
        }
        const uint64_t mid = edge ? b - 1 : a + ((b - a) >> 1);
        edge = false;
        const int c = cmp(mid, l < r ? l : r, k);
        if (c < 0) {
            a = mid + 1;
            l = k;
        } else if (c > 0) {
            b = mid;
            r = k;
        } else if (phase == 0) {   // first match: the lower bound in [a, M), right end matched
            M = mid;
            b0 = b;
            r0 = r;
            b = mid;
            r = m;
            phase = 1;
        } else if (phase == 1) {
            b = mid;
        } else {
            a = mid + 1;
        }
    }
}

// the scalar search: one probe = compare_words over sa_at / text_word / pat_word
template <class SaAt, class TextWord, class PatWord>
SA_HD void find_scalar(uint64_t n, uint64_t m, const SaAt& sa_at, const TextWord& text_word, const PatWord& pat_word,
                       uint64_t& lo, uint64_t& hi) {
    find_interval(n, m, [&](uint64_t rank, uint64_t start, uint64_t& k) {
        return compare_words((uint64_t)sa_at(rank), n, m, start, text_word, pat_word, k);
    }, lo, hi);
}

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

#include "sa_lcp.h"   // load8

namespace sa {

static_assert(kFindLaneMax == SA_FIND_LANE_MAX, "sa_hip.h states the auto mode's length threshold");

// pattern q of the batch: bytes [a, a + m) of the pattern buffer.  The offsets
// are clamped to pat_bytes and a decreasing pair is the empty pattern, so no
// offset array can send a load outside the buffer.
__device__ __forceinline__ void find_pattern(const uint64_t* __restrict__ off, uint64_t q, uint64_t pat_bytes,
                                             uint64_t& a, uint64_t& m) {
    const uint64_t o0 = off[q], o1 = off[q + 1];
    a = o0 < pat_bytes ? o0 : pat_bytes;
    const uint64_t e = o1 < pat_bytes ? o1 : pat_bytes;
    m = e > a ? e - a : 0;
}

// One query per lane, grid-stride over the queries of m in [min_m, max_m].
// The probes are dependent random loads (SA[mid], then the text at it): the
// kernel lives on occupancy, not on bandwidth; the top levels of the descent
// are the same few SA entries and text words for every query and stay in L2.
// The first two words of P are kept in registers: with 4 symbols and
// n = 2^28 a probe is decided within 16 bytes unless it (nearly) matches.
__global__ __launch_bounds__(kBlock) void k_find_lane(const uint8_t* __restrict__ text, uint64_t n,
                                                      const uint32_t* __restrict__ sa,
                                                      const uint8_t* __restrict__ pat, uint64_t pat_bytes,
                                                      const uint64_t* __restrict__ off, uint64_t nq, uint64_t min_m,
                                                      uint64_t max_m, uint32_t* __restrict__ lo_out,
                                                      uint32_t* __restrict__ hi_out) {
    for (uint64_t q = (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < nq; q += (uint64_t)gridDim.x * kBlock) {
        uint64_t pa, m;
        find_pattern(off, q, pat_bytes, pa, m);
        if (m < min_m || m > max_m) continue;
        const uint64_t w0 = load8(pat, pa, pat_bytes), w1 = load8(pat, pa + 8, pat_bytes);
        uint64_t lo, hi;
        find_scalar(n, m, [&](uint64_t rank) { return sa[rank]; },
                    [&](uint64_t p) { return load8(text, p, n); },
                    [&](uint64_t o) { return o == 0 ? w0 : o == 8 ? w1 : load8(pat, pa + o, pat_bytes); }, lo, hi);
        lo_out[q] = (uint32_t)lo;
        hi_out[q] = (uint32_t)hi;
    }
}

// One probe by a whole wavefront: each step covers 64 x 8 = 512 bytes, the
// first mismatch is the lowest set bit of a ballot.  Every argument is
// wave-uniform, so the search around it runs in lockstep.
struct WaveCompare {
    const uint8_t* __restrict__ text;
    uint64_t n;
    const uint32_t* __restrict__ sa;
    const uint8_t* __restrict__ pat;
    uint64_t pat_bytes, pa, m;
    __device__ __forceinline__ int operator()(uint64_t rank, uint64_t start, uint64_t& k) const {
        const uint64_t s = sa[rank];
        const uint64_t slen = s < n ? n - s : 0;
        const uint64_t lim = m < slen ? m : slen;
        const uint32_t lane = lane_id();
        for (uint64_t off = start & ~7ull; off < lim; off += (uint64_t)kWave * 8) {
            const uint64_t o = off + (uint64_t)lane * 8;
            bool mis = false, above = false;
            uint32_t j = 0;
            if (o < lim) {
                const uint64_t a = __builtin_bswap64(load8(text, s + o, n));
                const uint64_t b = __builtin_bswap64(load8(pat, pa + o, pat_bytes));
                if (a != b) {
                    j = (uint32_t)(__builtin_clzll(a ^ b) >> 3);
                    mis = o + j < lim;
                    above = a > b;
                }
            }
            const uint64_t bm = __ballot(mis);
            if (bm) {
                const int f = __builtin_ctzll(bm);
                const uint64_t am = __ballot(mis && above);
                k = off + (uint64_t)f * 8 + (uint32_t)__shfl((int)j, f, kWave);
                return ((am >> f) & 1ull) ? 1 : -1;
            }
        }
        k = lim;
        return lim == m ? 0 : -1;
    }
};

// One query per wavefront, for long patterns: a 100 KB pattern against a
// repetitive text is 200 steps per probe here, not one lane's 12,800.  A
// wavefront reads the offsets of kFindGroup queries with one load (in auto
// mode most of them belong to the lane kernel and are skipped together) and
// searches those of its length class one after the other.
__global__ __launch_bounds__(kBlock) void k_find_wave(const uint8_t* __restrict__ text, uint64_t n,
                                                      const uint32_t* __restrict__ sa,
                                                      const uint8_t* __restrict__ pat, uint64_t pat_bytes,
                                                      const uint64_t* __restrict__ off, uint64_t nq, uint64_t min_m,
                                                      uint64_t max_m, uint32_t* __restrict__ lo_out,
                                                      uint32_t* __restrict__ hi_out) {
    const uint32_t lane = lane_id();
    const uint64_t groups = (nq + kFindGroup - 1) / kFindGroup;
    for (uint64_t g = (uint64_t)blockIdx.x * kWaves + wave_id(); g < groups; g += (uint64_t)gridDim.x * kWaves) {
        const uint64_t q = g * kFindGroup + lane;
        uint64_t pa = 0, m = 0;
        bool mine = false;
        if (lane < kFindGroup && q < nq) {
            find_pattern(off, q, pat_bytes, pa, m);
            mine = m >= min_m && m <= max_m;
        }
        uint64_t todo = __ballot(mine);
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            WaveCompare cmp{text, n, sa, pat, pat_bytes, (uint64_t)__shfl((unsigned long long)pa, j, kWave),
                            (uint64_t)__shfl((unsigned long long)m, j, kWave)};
            uint64_t lo, hi;
            find_interval(n, cmp.m, cmp, lo, hi);
            if (lane == 0) {
                lo_out[g * kFindGroup + j] = (uint32_t)lo;
                hi_out[g * kFindGroup + j] = (uint32_t)hi;
            }
        }
    }
}

static int find_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat,
                       uint64_t pat_bytes, const uint64_t* d_off, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi,
                       uint32_t flags, hipStream_t s) {
    if (flags > SA_FIND_WAVE) return set_err(SA_E_INVALID, "flags must be 0, SA_FIND_LANE or SA_FIND_WAVE");
    if (nq == 0) return SA_OK;
    if (!d_text || !d_sa || !d_pat || !d_off || !d_lo || !d_hi) return set_err(SA_E_INVALID, "NULL device pointer");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    // 8 workgroups of 256 threads fill a CU at 8 waves per SIMD
    const uint64_t kMaxGrid = 256 * 8;
    const uint64_t all = ~0ull;
    if (flags != SA_FIND_WAVE) {
        const uint32_t grid = (uint32_t)std::min<uint64_t>((nq + kBlock - 1) / kBlock, kMaxGrid);
        hipLaunchKernelGGL(k_find_lane, dim3(grid), dim3(kBlock), 0, s, d_text, n, d_sa, d_pat, pat_bytes, d_off, nq,
                           (uint64_t)0, flags == SA_FIND_LANE ? all : kFindLaneMax, d_lo, d_hi);
    }
    if (flags != SA_FIND_LANE) {
        const uint64_t groups = (nq + kFindGroup - 1) / kFindGroup;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((groups + kWaves - 1) / kWaves, kMaxGrid);
        hipLaunchKernelGGL(k_find_wave, dim3(grid), dim3(kBlock), 0, s, d_text, n, d_sa, d_pat, pat_bytes, d_off, nq,
                           flags == SA_FIND_WAVE ? (uint64_t)0 : kFindLaneMax + 1, all, d_lo, d_hi);
    }
    SA_HIP(hipGetLastError());
    return SA_OK;
}

// host in, host out (sa_find / sa_find_ex), over the steps of sa_host.h
static int find_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat,
                     const uint64_t* pat_off, uint64_t nq, uint64_t* lo_out, uint64_t* hi_out, uint32_t flags) {
    SA_TRY(check_width(sa_width));
    if (flags > SA_FIND_WAVE) return set_err(SA_E_INVALID, "flags must be 0, SA_FIND_LANE or SA_FIND_WAVE");
    if (nq == 0) return SA_OK;
    if (!pat_off || !lo_out || !hi_out || (n && (!text || !sa))) return set_err(SA_E_INVALID, "NULL host pointer");
    SA_TRY(check_n32(n));
    for (uint64_t q = 0; q < nq; ++q)
        if (pat_off[q] > pat_off[q + 1]) return set_err(SA_E_INVALID, "pattern offsets decrease at %llu", (unsigned long long)q);
    const uint64_t pat_bytes = pat_off[nq];
    if (pat_bytes && !pat) return set_err(SA_E_INVALID, "NULL host pointer");
    std::vector<uint32_t> narrow;
    const void* src = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src));
    SA_TRY(need_device());
    DevBuf d_text, d_sa, d_pat, d_off, d_lo, d_hi;
    SA_TRY(d_text.alloc(align_up(n + 1, 256)));
    SA_TRY(d_sa.alloc(align_up(n + 1, 64) * 4));
    SA_TRY(d_pat.alloc(align_up(pat_bytes + 1, 256)));
    SA_TRY(d_off.alloc((nq + 1) * 8));
    SA_TRY(d_lo.alloc(nq * 4));
    SA_TRY(d_hi.alloc(nq * 4));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src, n * 4}, {d_pat.p, pat, pat_bytes}, {d_off.p, pat_off, (nq + 1) * 8}}));
    SA_TRY(find_device(d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), d_pat.as<uint8_t>(), pat_bytes,
                       d_off.as<uint64_t>(), nq, d_lo.as<uint32_t>(), d_hi.as<uint32_t>(), flags, nullptr));
    return download_u64({{lo_out, d_lo.as<uint32_t>()}, {hi_out, d_hi.as<uint32_t>()}}, nq);
}

}  // namespace sa

extern "C" {

int sa_find_device(const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint8_t* d_pat, uint64_t pat_bytes,
                   const uint64_t* d_pat_off, uint64_t nq, uint32_t* d_lo, uint32_t* d_hi, uint32_t flags,
                   void* stream) {
    return sa::find_device(d_text, n, d_sa, d_pat, pat_bytes, d_pat_off, nq, d_lo, d_hi, flags, (hipStream_t)stream);
}

int sa_find(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat, const uint64_t* pat_off,
            uint64_t nq, uint64_t* lo_out, uint64_t* hi_out) {
    return sa::find_host(text, n, sa, sa_width, pat, pat_off, nq, lo_out, hi_out, 0);
}

int sa_find_ex(const uint8_t* text, uint64_t n, const void* sa, int sa_width, const uint8_t* pat,
               const uint64_t* pat_off, uint64_t nq, uint64_t* lo_out, uint64_t* hi_out, uint32_t flags) {
    return sa::find_host(text, n, sa, sa_width, pat, pat_off, nq, lo_out, hi_out, flags);
}

}  // extern "C"

#endif   // __HIPCC__
