// sa_repeats.h -- the repeats of the text as LCP intervals: right-maximal,
// maximal and supermaximal (sa_repeats / sa_repeats_device of
// include/sa_hip.h).
//
// A repeat is (len, lo, hi): lcp[lo] < len, lcp[k] >= len for lo < k < hi with
// equality somewhere, lcp[hi] < len (lcp[0] and lcp[n] read as 0); the string
// T[SA[lo] .. SA[lo] + len) occurs exactly at SA[lo .. hi).  Its head is the
// smallest k in (lo, hi) with lcp[k] == len; a rank is the head of at most one
// repeat, so one lane per rank decides and the output is in head order.
// Rank k >= 1 with l = lcp[k] >= 1 is a head iff the nearest j < k with
// lcp[j] <= l has lcp[j] < l; then lo = j and hi = the nearest rank above k
// with lcp < l, or n.  Both are nearest-smaller-value searches on the LCP
// array: sa_lz.h's walk over a hierarchy of minima, here over LCP minima alone
// and with the comparison as a parameter (<= to the left, < to the right).
//
//   k_rep_minima   one workgroup per tile of kLzTile ranks: LCP into LDS, the
//                  tile's 64 level-1 minima by wavefront reductions, its
//                  level-2 minimum from those; both written to the global
//                  hierarchy (fan-out kLzFan).  For SA_REP_MAXIMAL also the
//                  break bits D[k] = (prev(k) != prev(k - 1)), prev(k) =
//                  T[SA[k] - 1] gathered as the BWT gathers it (START, a 257th
//                  symbol, for SA[k] == 0): one ballot word per 64 ranks, the
//                  breaks before each word inside its tile, the tile's breaks.
//   k_rep_reduce   levels 3 and up, one lane per node, one launch per level.
//   scan_i64       over the tiles' break counts (SA_REP_MAXIMAL).
//   k_rep_count    one workgroup per tile, the tile and its two levels in LDS
//                  again.  lcp[k] < min_len: nothing.  lcp[k - 1] == lcp[k]:
//                  no head.  lcp[k - 1] < lcp[k]: a head with lo = k - 1, no
//                  walk.  Only a descent walks left, only a head walks right;
//                  a walk runs in the tile first and goes on in the global
//                  hierarchy from the tile's edge, kLpfChunk nodes a step with
//                  their loads issued together (sa_lz.h says why the chunk is
//                  no array).  A walk passes at most kLzFan - 1 nodes per
//                  level up and as many down, whatever the LCP values are.
//                  Left-maximal: "some break in (lo, hi)" is a difference of
//                  two break ranks (word, count before the word, tile sum).
//                  Supermaximal: only a head with lo = k - 1 can be one; it
//                  scans forward while lcp == len, at most 257 ranks, with a
//                  256-bit seen mask in four registers picked by compares and
//                  START apart, and needs neither walk nor break bits.  The
//                  plateaus are disjoint, so the scans read O(n) ranks.
//                  Accepted heads: one bit per rank; per tile their number
//                  and the sum of hi - lo.
//   scan_i64       over the tiles' counts and over the tiles' sums.
//   k_rep_emit     (len, lo, hi) at tile base + rank among the tile's accepted
//                  heads: a stable compaction in head order.  It reads the
//                  count on the device, so it is launched before the host
//                  knows it, and writes nothing when the count exceeds
//                  out_cap.  It walks again for the accepted heads instead of
//                  reading stored intervals: storing (lo, hi) for every rank
//                  would cost 8 n bytes of temporary and 8 n bytes of traffic
//                  each way, the bits cost n / 8 bytes, and the second walk is
//                  paid by accepted heads only.
//
// Host waits per call.  sa_repeats_device with d_lcp: one (the count and the
// sum of hi - lo, after everything is enqueued); without: sa_lcp_device's own
// and that one.  Temporaries, stream-ordered: about 0.38 n bytes for
// SA_REP_MAXIMAL (n / 15.75 hierarchy, n / 8 break words, n / 16 break counts,
// n / 8 accept bits, 24 bytes per tile), about 0.19 n for the other kinds, plus
// 4 n when the LCP array is computed here.
//
// The walks, the break rank and the supermaximal scan compile on the host:
// tests/cpp/repeats_check.cpp checks them against the substring dictionary.
// Measurements and the resource report: DESIGN.md section 16.  The HIP part
// needs sa_host.h, sa_locate.h (LocBuf), sa_query.h (mem_block_excl), sa_lz.h
// and sa_build.hip's scan_i64 and lcp_device before it.
#pragma once
#include <stdint.h>

#include "sa_lz.h"   // SA_HD, SA_LZ_UNROLL, kLzFan, kLzTile, kLpfChunk, lpf_level_counts

namespace sa {

constexpr uint32_t kRepRight = 0;          // = SA_REP_RIGHT
constexpr uint32_t kRepMaximal = 1;        // = SA_REP_MAXIMAL
constexpr uint32_t kRepSupermaximal = 2;   // = SA_REP_SUPERMAXIMAL
constexpr int kRepInfo = 2;                // = SA_REP_INFO
constexpr uint32_t kRepStart = 256;        // prev() of the suffix at position 0: no byte
constexpr int kRepSuperMax = 257;          // occurrences of a supermaximal repeat: 256 bytes and START
constexpr uint32_t kRepWordRanks = 64;     // ranks per word of break bits

// nodes of level lv over n >= 1 entries with fan-out 64: ceil(n / 64^lv), what
// lpf_level_counts<64> gives for every level it has
SA_HD uint64_t rep_level_count(uint64_t n, int lv) { return ((n - 1) >> (6 * lv)) + 1; }

// LE: the nearest entry <= v; else the nearest entry < v
template <bool LE>
SA_HD bool rep_hit(uint32_t x, uint32_t v) {
    return LE ? x <= v : x < v;
}

// Nodes hi, hi - 1, .. lo of level lv (lo <= hi): at = the first whose minimum hits.
template <bool LE, int CHUNK, class H>
SA_HD bool rep_scan_down(const H& h, int lv, uint64_t hi, uint64_t lo, uint32_t v, uint64_t& at) {
    for (uint64_t c = hi;; c -= CHUNK) {
        const uint64_t left = c - lo + 1;
        int hit = -1;
        // no exit inside: the CHUNK loads are issued together
        SA_LZ_UNROLL
        for (int j = 0; j < CHUNK; ++j) {
            const uint32_t x = h(lv, (uint64_t)j < left ? c - j : c);   // past the run: node c again
            if ((uint64_t)j < left && hit < 0 && rep_hit<LE>(x, v)) hit = j;
        }
        if (hit >= 0) {
            at = c - (uint64_t)hit;
            return true;
        }
        if (left <= (uint64_t)CHUNK) return false;
    }
}

// nodes lo, lo + 1, .. hi - 1 of level lv (lo < hi), in that order
template <bool LE, int CHUNK, class H>
SA_HD bool rep_scan_up(const H& h, int lv, uint64_t lo, uint64_t hi, uint32_t v, uint64_t& at) {
    for (uint64_t c = lo;; c += CHUNK) {
        const uint64_t left = hi - c;
        int hit = -1;
        SA_LZ_UNROLL
        for (int j = 0; j < CHUNK; ++j) {
            const uint32_t x = h(lv, (uint64_t)j < left ? c + j : c);
            if ((uint64_t)j < left && hit < 0 && rep_hit<LE>(x, v)) hit = j;
        }
        if (hit >= 0) {
            at = c + (uint64_t)hit;
            return true;
        }
        if (left <= (uint64_t)CHUNK) return false;
    }
}

// The nearest index below r whose entry hits v, over the hierarchy `h` of
// minima (h(level, idx): the minimum; h.count(level); h.levels(); level 0: the
// entries).  False when there is none; a caller whose hierarchy is a window
// goes on from the window's first rank.
template <bool LE, uint32_t F, int CHUNK, class H>
SA_HD bool rep_walk_left(const H& h, uint64_t r, uint32_t v, uint64_t& at) {
    if (r == 0) return false;
    const int levels = h.levels();
    uint64_t idx = r - 1;
    int lv = 0;
    for (;;) {
        // the last child of its parent: the parent ends where it ends
        while (lv + 1 < levels && idx % F == F - 1) {
            idx /= F;
            ++lv;
        }
        // down to the first child of the same parent (to node 0 at the top)
        const uint64_t lo = lv + 1 < levels ? idx - idx % F : 0;
        if (rep_scan_down<LE, CHUNK>(h, lv, idx, lo, v, idx)) break;
        if (lo == 0) return false;
        idx = lo - 1;
    }
    while (lv > 0) {   // the answer is inside node idx: its last child that hits
        --lv;
        const uint64_t first = idx * F;
        uint64_t c = first + F - 1;
        if (c >= h.count(lv)) c = h.count(lv) - 1;
        if (c < first || !rep_scan_down<LE, CHUNK>(h, lv, c, first, v, idx)) return false;   // a node that does not hold its own minimum
    }
    at = idx;
    return true;
}

// the nearest index above r whose entry hits v
template <bool LE, uint32_t F, int CHUNK, class H>
SA_HD bool rep_walk_right(const H& h, uint64_t r, uint32_t v, uint64_t& at) {
    const int levels = h.levels();
    uint64_t idx = r + 1;
    int lv = 0;
    if (idx >= h.count(0)) return false;
    for (;;) {
        // the first child of its parent: the parent starts where it starts
        while (lv + 1 < levels && idx % F == 0) {
            idx /= F;
            ++lv;
        }
        // up to the last child of the same parent (to the last node at the top)
        uint64_t hi = lv + 1 < levels ? idx - idx % F + F : h.count(lv);
        if (hi > h.count(lv)) hi = h.count(lv);
        if (rep_scan_up<LE, CHUNK>(h, lv, idx, hi, v, idx)) break;
        if (hi >= h.count(lv)) return false;
        idx = hi;
    }
    while (lv > 0) {
        --lv;
        const uint64_t first = idx * F;
        uint64_t end = first + F;
        if (end > h.count(lv)) end = h.count(lv);
        if (first >= end || !rep_scan_up<LE, CHUNK>(h, lv, first, end, v, idx)) return false;
    }
    at = idx;
    return true;
}

// Is rank base + i >= 1 (l = its LCP entry >= 1, before = the entry of the rank
// below it) the head of a repeat, and if so, where does the repeat start?
// `win` is the window of ranks [base, base + win.count(0)), `g` the whole
// hierarchy, whose entry 0 reads as 0.
template <uint32_t F, class W, class G>
SA_HD bool rep_head_lo(const W& win, const G& g, uint64_t base, uint64_t i, uint32_t l, uint32_t before, uint64_t& lo) {
    if (before == l) return false;   // the plateau's head is further left
    if (before < l) {                // an ascent: the interval opens here
        lo = base + i - 1;
        return true;
    }
    uint64_t j;
    if (rep_walk_left<true, F, 1>(win, i, l, j)) {
        lo = base + j;
        return win(0, j) < l;
    }
    if (rep_walk_left<true, F, kLpfChunk>(g, base, l, j)) {   // from the window's first rank
        lo = j;
        return g(0, j) < l;
    }
    lo = 0;   // (an entry 0 that is not below l >= 1: it reads as 0)
    return true;
}

// where the repeat of length l whose head is rank base + i ends
template <uint32_t F, class W, class G>
SA_HD uint64_t rep_head_hi(const W& win, const G& g, uint64_t base, uint64_t i, uint32_t l, uint64_t n) {
    uint64_t j;
    if (rep_walk_right<false, F, 1>(win, i, l, j)) return base + j;
    if (rep_walk_right<false, F, kLpfChunk>(g, base + win.count(0) - 1, l, j)) return j;   // from its last
    return n;
}

// Breaks at ranks <= x (x < n).  b.word(w): bit k = D[64 w + k]; b.count(w):
// the breaks of w's tile in front of word w; b.tile(t): the breaks of the
// tiles in front of tile t.  WPT: words per tile.
template <uint32_t WPT, class B>
SA_HD uint64_t rep_break_rank(const B& b, uint64_t x) {
    const uint64_t w = x / kRepWordRanks;
    const uint64_t m = b.word(w) & (~0ull >> (63u - (uint32_t)(x % kRepWordRanks)));
    return b.tile(w / WPT) + b.count(w) + (uint64_t)__builtin_popcountll(m);
}

// prev(lo), .., prev(hi - 1) are not all equal: some D[k] with lo < k < hi
template <uint32_t WPT, class B>
SA_HD bool rep_left_maximal(const B& b, uint64_t lo, uint64_t hi) {
    return rep_break_rank<WPT>(b, hi - 1) != rep_break_rank<WPT>(b, lo);
}

// A head k with lo = k - 1 and len = lcp(k): is the repeat supermaximal, that
// is lcp == len on all of (lo, hi) and the prev symbols of [lo, hi) pairwise
// distinct?  hi = its end then.  lcp(r) for k < r < n, prev(r): a byte or
// kRepStart.  At most kRepSuperMax ranks are read.
template <class Lcp, class Prev>
SA_HD bool rep_supermaximal(const Lcp& lcp, const Prev& prev, uint64_t n, uint64_t k, uint32_t len, uint64_t& hi) {
    uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    bool start = false;
    uint64_t r = k - 1;
    for (int members = 0;; ++members) {
        if (members == kRepSuperMax) return false;   // a 258th occurrence: two share a symbol
        const uint32_t c = prev(r);
        if (c >= kRepStart) {
            if (start) return false;
            start = true;
        } else {
            const uint64_t bit = 1ull << (c & 63u);
            const uint32_t w = c >> 6;
            const uint64_t cur = w == 0 ? m0 : w == 1 ? m1 : w == 2 ? m2 : m3;
            if (cur & bit) return false;
            m0 |= w == 0 ? bit : 0;
            m1 |= w == 1 ? bit : 0;
            m2 |= w == 2 ? bit : 0;
            m3 |= w == 3 ? bit : 0;
        }
        ++r;
        if (r >= n) break;
        if (r > k) {
            const uint32_t x = lcp(r);
            if (x < len) break;
            if (x > len) return false;   // a longer repeat inside
        }
    }
    hi = r;
    return true;
}

// the filters as the kernels compare them: 0 reads as 1, and 0 and 1 as 2
SA_HD uint64_t rep_min_len(uint64_t min_len) { return min_len < 1 ? 1 : min_len; }
SA_HD uint64_t rep_min_occ(uint64_t min_occ) { return min_occ < 2 ? 2 : min_occ; }

}  // namespace sa

#if defined(__HIPCC__) || defined(__HIP__)

namespace sa {

static_assert(SA_REP_RIGHT == kRepRight && SA_REP_MAXIMAL == kRepMaximal && SA_REP_SUPERMAXIMAL == kRepSupermaximal &&
                  SA_REP_INFO == kRepInfo,
              "sa_hip.h states these");
constexpr uint32_t kRepTileWords = kLzTile / kRepWordRanks;   // 64 words of break bits per tile
static_assert(kRepWordRanks == (uint32_t)kWave && kRepTileWords == (uint32_t)kWave,
              "a ballot is a word; one wavefront scans a tile's words");

// The global hierarchy: level 0 is the LCP array (entry 0 reads as 0), levels
// 1 and up lie one after the other in `nodes`, level k from off(k).  No member
// is an array: a lane indexes the levels by a value of its own, and an array
// in a kernel argument that is indexed so is copied to scratch (136 bytes per
// lane in a first form).  The counts are arithmetic, the offsets a chain of
// selects.
struct RepLevels {
    const uint32_t* __restrict__ lcp;
    const uint32_t* __restrict__ nodes;
    uint64_t n;                      // >= 1
    uint32_t o2, o3, o4, o5, o6;     // where levels 2 .. 6 start (level 1 starts at 0)
    int n_levels;
    __device__ __forceinline__ int levels() const { return n_levels; }
    __device__ __forceinline__ uint64_t count(int lv) const { return rep_level_count(n, lv); }
    __device__ __forceinline__ uint32_t off(int lv) const {
        return lv == 1 ? 0u : lv == 2 ? o2 : lv == 3 ? o3 : lv == 4 ? o4 : lv == 5 ? o5 : o6;
    }
    __device__ __forceinline__ uint32_t operator()(int lv, uint64_t i) const {
        if (lv == 0) return i ? lcp[i] : 0u;
        return nodes[(uint64_t)off(lv) + i];
    }
};
static_assert(kLzFan == 64 && kLpfMaxLevels == 7, "count() shifts by 6 a level; off() knows levels 1 .. 6");

// a tile in LDS: c0 entries, c1 level-1 minima, one level-2 minimum
struct RepLocal {
    const uint32_t* s_l0;
    const uint32_t* s_l1;
    const uint32_t* s_l2;
    uint32_t c0, c1;
    __device__ __forceinline__ int levels() const { return 3; }
    __device__ __forceinline__ uint64_t count(int lv) const { return lv == 0 ? c0 : lv == 1 ? c1 : 1u; }
    __device__ __forceinline__ uint32_t operator()(int lv, uint64_t i) const {
        return lv == 0 ? s_l0[i] : lv == 1 ? s_l1[i] : s_l2[0];
    }
};

// the break bits: tinc = the inclusive sums of the tiles' breaks
struct RepBreaks {
    const uint64_t* __restrict__ words;
    const uint32_t* __restrict__ wcnt;
    const int64_t* __restrict__ tinc;
    __device__ __forceinline__ uint64_t word(uint64_t w) const { return words[w]; }
    __device__ __forceinline__ uint64_t count(uint64_t w) const { return wcnt[w]; }
    __device__ __forceinline__ uint64_t tile(uint64_t t) const { return t ? (uint64_t)tinc[t - 1] : 0; }
};

// prev() of a suffix: an SA entry >= n is clamped
__device__ __forceinline__ uint32_t rep_prev(const uint8_t* __restrict__ text, uint32_t sa_entry, uint64_t n) {
    if (sa_entry == 0) return kRepStart;
    return text[std::min<uint64_t>(sa_entry, n) - 1];
}

// Tile `tile` of the LCP array into LDS (rank 0 reads as 0, what lies past n
// as all ones, the minimum's identity), its level-1 minima into s_l1 and its
// level-2 minimum into s_l2[0].  Ends with a barrier.
__device__ __forceinline__ void rep_load_tile(const uint32_t* __restrict__ lcp, uint64_t n, uint64_t tile, uint32_t* s_l0,
                                              uint32_t* s_l1, uint32_t* s_l2) {
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    const uint64_t base = tile * kLzTile;
#pragma unroll
    for (int j = 0; j < kLzPer; ++j) {
        const uint32_t i = j * kBlock + tid;
        s_l0[i] = base + i >= n ? ~0u : base + i == 0 ? 0u : lcp[base + i];
    }
    __syncthreads();
    constexpr uint32_t per_wave = kLzFan / kWaves;   // 16 nodes per wavefront
    for (uint32_t k = 0; k < per_wave; ++k) {
        const uint32_t node = wave * per_wave + k;
        uint32_t x = s_l0[node * kLzFan + lane];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) x = lz_min32(x, (uint32_t)__shfl_xor((int)x, o, kWave));
        if (lane == 0) s_l1[node] = x;
    }
    __syncthreads();
    if (wave == 0) {
        uint32_t x = s_l1[lane];
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) x = lz_min32(x, (uint32_t)__shfl_xor((int)x, o, kWave));
        if (lane == 0) s_l2[0] = x;
    }
    __syncthreads();
}

// c1 = the nodes of level 1 (ceil(n / 64)); l2 is NULL when level 1 is the
// top.  BREAKS: words and wcnt have kRepTileWords entries per tile, tbrk one.
template <bool BREAKS>
__global__ __launch_bounds__(kBlock) void k_rep_minima(const uint8_t* __restrict__ text, const uint32_t* __restrict__ sa,
                                                       const uint32_t* __restrict__ lcp, uint64_t n, uint64_t c1,
                                                       uint32_t* __restrict__ l1, uint32_t* __restrict__ l2,
                                                       uint64_t* __restrict__ words, uint32_t* __restrict__ wcnt,
                                                       int64_t* __restrict__ tbrk) {
    __shared__ uint32_t s_l0[kLzTile], s_l1[kLzFan], s_l2[1];
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x, base = tile * kLzTile;
    rep_load_tile(lcp, n, tile, s_l0, s_l1, s_l2);
    const uint64_t g = tile * kLzFan + tid;
    if (tid < kLzFan && g < c1) l1[g] = s_l1[tid];
    if (tid == 0 && l2) l2[tile] = s_l2[0];
    if (BREAKS) {
        __shared__ uint16_t s_p[kLzTile + 1];   // s_p[i + 1] = prev(base + i); s_p[0]: the rank in front of the tile
        __shared__ uint32_t s_c[kRepTileWords];
        const uint32_t lane = lane_id(), wave = tid / kWave;
#pragma unroll
        for (int j = 0; j < kLzPer; ++j) {
            const uint32_t i = j * kBlock + tid;
            s_p[i + 1] = base + i < n ? (uint16_t)rep_prev(text, sa[base + i], n) : (uint16_t)0;
        }
        if (tid == 0) s_p[0] = base ? (uint16_t)rep_prev(text, sa[base - 1], n) : (uint16_t)0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kLzPer; ++j) {
            const uint32_t i = j * kBlock + tid;
            const bool d = base + i < n && base + i > 0 && s_p[i + 1] != s_p[i];
            const uint64_t m = __ballot(d);   // ranks base + 64 (4 j + wave) ..: one word
            if (lane == 0) {
                const uint32_t w = (uint32_t)j * kWaves + wave;
                words[tile * kRepTileWords + w] = m;
                s_c[w] = (uint32_t)__popcll(m);
            }
        }
        __syncthreads();
        if (wave == 0) {
            const uint32_t c = s_c[lane];
            uint32_t incl = c;
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)incl, o, kWave);
                if ((int)lane >= o) incl += y;
            }
            wcnt[tile * kRepTileWords + lane] = incl - c;
            if (lane == kWave - 1) tbrk[tile] = (int64_t)incl;
        }
    }
}

// out[p] = the minimum of in[p * 64 .. p * 64 + 64) (cut at cin)
__global__ __launch_bounds__(kBlock) void k_rep_reduce(const uint32_t* __restrict__ in, uint64_t cin,
                                                       uint32_t* __restrict__ out, uint64_t cout) {
    const uint64_t p = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= cout) return;
    uint32_t x = ~0u;
    const uint64_t e = std::min<uint64_t>(p * kLzFan + kLzFan, cin);
    for (uint64_t i = p * kLzFan; i < e; ++i) x = lz_min32(x, in[i]);
    out[p] = x;
}

// bits[t * kBlock + lane of the workgroup]: bit j = rank t * kLzTile + 16 *
// lane + j is an accepted head; tcnt[t] = the tile's accepted heads, tocc[t] =
// the sum of their hi - lo.  min_len >= 1 and min_occ >= 2.
template <uint32_t KIND>
__global__ __launch_bounds__(kBlock) void k_rep_count(RepLevels g, uint64_t n, const uint8_t* __restrict__ text,
                                                      const uint32_t* __restrict__ sa, uint64_t min_len,
                                                      uint64_t min_occ, RepBreaks brk, uint16_t* __restrict__ bits,
                                                      int64_t* __restrict__ tcnt, int64_t* __restrict__ tocc) {
    __shared__ uint32_t s_l0[kLzTile], s_l1[kLzFan], s_l2[1];
    __shared__ uint8_t s_f[kLzTile];
    __shared__ uint32_t s_w[kWaves];
    __shared__ unsigned long long s_occ;
    const uint32_t tid = threadIdx.x;
    const uint64_t tile = blockIdx.x, base = tile * kLzTile;
    if (tid == 0) s_occ = 0;
    rep_load_tile(g.lcp, n, tile, s_l0, s_l1, s_l2);
    RepLocal loc;
    loc.s_l0 = s_l0;
    loc.s_l1 = s_l1;
    loc.s_l2 = s_l2;
    loc.c0 = (uint32_t)std::min<uint64_t>(kLzTile, n - base);
    loc.c1 = (loc.c0 + kLzFan - 1) / kLzFan;
    unsigned long long occ = 0;
    for (int j = 0; j < kLzPer; ++j) {
        const uint32_t i = j * kBlock + tid;
        const uint64_t r = base + i;
        bool accept = false;
        if (i < loc.c0 && r >= 1) {
            const uint32_t l = s_l0[i];
            if (l >= 1 && (uint64_t)l >= min_len) {
                const uint32_t before = i ? s_l0[i - 1] : g(0, base - 1);
                uint64_t lo = 0, hi = 0;
                if (KIND == kRepSupermaximal) {
                    const auto lcp_at = [&](uint64_t x) { return x - base < (uint64_t)loc.c0 ? s_l0[x - base] : g.lcp[x]; };
                    const auto prev_at = [&](uint64_t x) { return rep_prev(text, sa[x], n); };
                    if (before < l && rep_supermaximal(lcp_at, prev_at, n, r, l, hi)) {
                        lo = r - 1;
                        accept = hi - lo >= min_occ;
                    }
                } else if (rep_head_lo<kLzFan>(loc, g, base, i, l, before, lo)) {
                    hi = rep_head_hi<kLzFan>(loc, g, base, i, l, n);
                    accept = hi - lo >= min_occ && (KIND == kRepRight || rep_left_maximal<kRepTileWords>(brk, lo, hi));
                }
                if (accept) occ += hi - lo;
            }
        }
        s_f[i] = accept ? 1 : 0;
    }
    if (occ) atomicAdd(&s_occ, occ);
    __syncthreads();
    uint32_t b = 0;
#pragma unroll
    for (int j = 0; j < kLzPer; ++j) b |= s_f[kLzPer * tid + j] ? 1u << j : 0u;
    uint32_t sum;
    (void)mem_block_excl((uint32_t)__popc(b), s_w, sum);
    bits[tile * kBlock + tid] = (uint16_t)b;
    if (tid == 0) {
        tcnt[tile] = (int64_t)sum;
        tocc[tile] = (int64_t)s_occ;
    }
}

// tbase: the inclusive sums of the tile counts; nothing is written when the
// count exceeds out_cap
__global__ __launch_bounds__(kBlock) void k_rep_emit(RepLevels g, uint64_t n, const uint16_t* __restrict__ bits,
                                                     const int64_t* __restrict__ tbase, uint64_t out_cap,
                                                     uint32_t* __restrict__ len, uint32_t* __restrict__ lo_out,
                                                     uint32_t* __restrict__ hi_out) {
    __shared__ uint32_t s_l0[kLzTile], s_l1[kLzFan], s_l2[1];
    __shared__ uint32_t s_w[kWaves];
    const uint32_t tid = threadIdx.x;
    const uint64_t t = blockIdx.x, base = t * kLzTile;
    const uint64_t count = (uint64_t)tbase[gridDim.x - 1];
    const uint64_t first = t ? (uint64_t)tbase[t - 1] : 0;
    if (count > out_cap || (uint64_t)tbase[t] == first) return;   // uniform
    rep_load_tile(g.lcp, n, t, s_l0, s_l1, s_l2);
    RepLocal loc;
    loc.s_l0 = s_l0;
    loc.s_l1 = s_l1;
    loc.s_l2 = s_l2;
    loc.c0 = (uint32_t)std::min<uint64_t>(kLzTile, n - base);
    loc.c1 = (loc.c0 + kLzFan - 1) / kLzFan;
    uint32_t b = bits[t * kBlock + tid];
    uint32_t sum;
    uint64_t o = first + mem_block_excl((uint32_t)__popc(b), s_w, sum);
    while (b) {
        const int j = __builtin_ctz(b);
        b &= b - 1u;
        const uint32_t i = (uint32_t)kLzPer * tid + (uint32_t)j;
        if (i >= loc.c0 || base + i == 0 || o >= count) break;
        const uint32_t l = s_l0[i];
        const uint32_t before = i ? s_l0[i - 1] : g(0, base - 1);
        uint64_t lo = 0;
        (void)rep_head_lo<kLzFan>(loc, g, base, i, l, before, lo);
        const uint64_t hi = rep_head_hi<kLzFan>(loc, g, base, i, l, n);
        len[o] = l;
        lo_out[o] = (uint32_t)lo;
        hi_out[o] = (uint32_t)hi;
        ++o;
    }
}

// the checks of sa_repeats_device, all before any HIP call
static int repeats_check_args(const sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa,
                              const uint32_t* d_lcp, uint32_t kind, const uint32_t* d_len, const uint32_t* d_lo,
                              const uint32_t* d_hi, const uint64_t* info) {
    if (!c) return set_err(SA_E_INVALID, "context is NULL");
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (n > 0xFFFFFFFFull) return set_err(SA_E_INVALID, "n too large");
    if (kind > kRepSupermaximal) return set_err(SA_E_INVALID, "unknown kind %u", kind);
    const int given = (d_len ? 1 : 0) + (d_lo ? 1 : 0) + (d_hi ? 1 : 0);
    if (given != 0 && given != 3) return set_err(SA_E_INVALID, "d_len, d_lo and d_hi: all or none");
    if (n <= 1) return SA_OK;
    if (!d_lcp || kind != kRepRight) {
        if (!d_text) return set_err(SA_E_INVALID, "d_text is NULL (only SA_REP_RIGHT with d_lcp does without)");
        if (!d_sa) return set_err(SA_E_INVALID, "d_sa is NULL (only SA_REP_RIGHT with d_lcp does without)");
    }
    if (given) {
        if (((uintptr_t)d_len | (uintptr_t)d_lo | (uintptr_t)d_hi) & 3u)
            return set_err(SA_E_INVALID, "an output is not 4-byte aligned");
        SA_TRY(check_no_alias({d_len, d_lo, d_hi}, {d_text, d_sa, d_lcp}));
        SA_TRY(check_distinct({d_len, d_lo, d_hi}));
    }
    return SA_OK;
}

// Host waits: one, for the count and the sum (after sa_lcp_device's own when
// d_lcp is NULL).
static int repeats_device(sa_context* c, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lcp,
                          uint64_t min_len, uint64_t min_occ, uint32_t kind, uint32_t* d_len, uint32_t* d_lo,
                          uint32_t* d_hi, uint64_t out_cap, uint64_t* info, hipStream_t s) {
    SA_TRY(repeats_check_args(c, d_text, n, d_sa, d_lcp, kind, d_len, d_lo, d_hi, info));
    info[0] = info[1] = 0;
    if (n <= 1) return SA_OK;
    SA_HIP(hipSetDevice(c->device));
    LocBuf own_lcp;
    if (!d_lcp) {
        SA_TRY(own_lcp.alloc(align_up(n, 64) * 4, s));
        SA_TRY(lcp_device(c, d_text, n, d_sa, (uint32_t*)own_lcp.p, nullptr, s));
        d_lcp = (const uint32_t*)own_lcp.p;
    }
    const bool breaks = kind == kRepMaximal;
    uint64_t cnt[kLpfMaxLevels], off[kLpfMaxLevels] = {0, 0, 0, 0, 0, 0, 0};
    const int n_levels = lpf_level_counts<kLzFan>(n, cnt);
    uint64_t nodes = 0;
    for (int lv = 1; lv < n_levels; ++lv) {
        off[lv] = nodes;
        nodes += cnt[lv];   // < 2^27 in all
    }
    const uint64_t tiles = (n + kLzTile - 1) / kLzTile;   // <= 2^20
    const uint64_t words = breaks ? tiles * kRepTileWords : 0;
    // break words (8) | tile breaks, counts, sums (8 each) | hierarchy (4) | breaks before a word (4) | accept bits (2)
    const uint64_t b_words = words * 8, b_tile = tiles * 8, b_nodes = align_up(nodes, 64) * 4, b_wcnt = words * 4,
                   b_bits = tiles * kBlock * 2;
    LocBuf tmp;
    SA_TRY(tmp.alloc(b_words + 3 * b_tile + b_nodes + b_wcnt + b_bits, s));
    uint64_t* d_words = (uint64_t*)tmp.p;
    int64_t* d_tbrk = (int64_t*)((uint8_t*)tmp.p + b_words);
    int64_t* d_tcnt = d_tbrk + tiles;
    int64_t* d_tocc = d_tcnt + tiles;
    uint32_t* d_nodes = (uint32_t*)(d_tocc + tiles);
    uint32_t* d_wcnt = (uint32_t*)((uint8_t*)d_nodes + b_nodes);
    uint16_t* d_bits = (uint16_t*)((uint8_t*)d_wcnt + b_wcnt);
    RepLevels g;
    g.lcp = d_lcp;
    g.nodes = d_nodes;
    g.n = n;
    g.o2 = (uint32_t)off[2];
    g.o3 = (uint32_t)off[3];
    g.o4 = (uint32_t)off[4];
    g.o5 = (uint32_t)off[5];
    g.o6 = (uint32_t)off[6];
    g.n_levels = n_levels;
    uint32_t* l1 = d_nodes;
    uint32_t* l2 = n_levels > 2 ? d_nodes + off[2] : nullptr;
    if (breaks)
        hipLaunchKernelGGL(k_rep_minima<true>, dim3((uint32_t)tiles), dim3(kBlock), 0, s, d_text, d_sa, d_lcp, n, cnt[1],
                           l1, l2, d_words, d_wcnt, d_tbrk);
    else
        hipLaunchKernelGGL(k_rep_minima<false>, dim3((uint32_t)tiles), dim3(kBlock), 0, s, d_text, d_sa, d_lcp, n,
                           cnt[1], l1, l2, d_words, d_wcnt, d_tbrk);
    for (int lv = 3; lv < n_levels; ++lv)
        hipLaunchKernelGGL(k_rep_reduce, dim3((uint32_t)((cnt[lv] + kBlock - 1) / kBlock)), dim3(kBlock), 0, s,
                           (const uint32_t*)(d_nodes + off[lv - 1]), cnt[lv - 1], d_nodes + off[lv], cnt[lv]);
    SA_HIP(hipGetLastError());
    if (breaks) SA_TRY(scan_i64<ScanSum>(d_tbrk, tiles, s));
    const RepBreaks brk{d_words, d_wcnt, d_tbrk};
    const uint64_t ml = rep_min_len(min_len), mo = rep_min_occ(min_occ);
    if (kind == kRepRight)
        hipLaunchKernelGGL(k_rep_count<kRepRight>, dim3((uint32_t)tiles), dim3(kBlock), 0, s, g, n, d_text, d_sa, ml, mo,
                           brk, d_bits, d_tcnt, d_tocc);
    else if (kind == kRepMaximal)
        hipLaunchKernelGGL(k_rep_count<kRepMaximal>, dim3((uint32_t)tiles), dim3(kBlock), 0, s, g, n, d_text, d_sa, ml,
                           mo, brk, d_bits, d_tcnt, d_tocc);
    else
        hipLaunchKernelGGL(k_rep_count<kRepSupermaximal>, dim3((uint32_t)tiles), dim3(kBlock), 0, s, g, n, d_text, d_sa,
                           ml, mo, brk, d_bits, d_tcnt, d_tocc);
    SA_HIP(hipGetLastError());
    SA_TRY(scan_i64<ScanSum>(d_tcnt, tiles, s));
    SA_TRY(scan_i64<ScanSum>(d_tocc, tiles, s));
    if (d_len) {
        hipLaunchKernelGGL(k_rep_emit, dim3((uint32_t)tiles), dim3(kBlock), 0, s, g, n, (const uint16_t*)d_bits,
                           (const int64_t*)d_tcnt, out_cap, d_len, d_lo, d_hi);
        SA_HIP(hipGetLastError());
    }
    uint64_t* h = host_u64<kHwRepeats, 2>(c);
    SA_HIP(hipMemcpyAsync(h, d_tcnt + (tiles - 1), 8, hipMemcpyDeviceToHost, s));
    SA_HIP(hipMemcpyAsync(h + 1, d_tocc + (tiles - 1), 8, hipMemcpyDeviceToHost, s));
    SA_HIP(host_sync(s));
    info[0] = h[0];
    info[1] = h[1];
    return SA_OK;
}

// Host in, host out: the SA is checked against the text, then one call of the
// device form writes into device outputs of min(out_cap, n) entries.
static int repeats_host(const uint8_t* text, uint64_t n, const void* sa, int sa_width, uint64_t min_len, uint64_t min_occ,
                        uint32_t kind, void* len_out, void* lo_out, void* hi_out, uint64_t out_cap, uint64_t* info) {
    SA_TRY(check_width(sa_width));
    SA_TRY(check_n32(n));
    if (!info) return set_err(SA_E_INVALID, "info is NULL");
    if (kind > kRepSupermaximal) return set_err(SA_E_INVALID, "unknown kind %u", kind);
    if (n && !text) return set_err(SA_E_INVALID, "text is NULL");
    if (n && !sa) return set_err(SA_E_INVALID, "sa is NULL");
    const int given = (len_out ? 1 : 0) + (lo_out ? 1 : 0) + (hi_out ? 1 : 0);
    if (given != 0 && given != 3) return set_err(SA_E_INVALID, "len_out, lo_out and hi_out: all or none");
    SA_TRY(check_distinct({len_out, lo_out, hi_out}));
    if (n) SA_TRY(check_no_alias({len_out, lo_out, hi_out}, {text, sa}));
    std::vector<uint32_t> narrow;
    const void* src32 = nullptr;
    SA_TRY(narrow_sa(sa, n, sa_width, narrow, &src32));
    info[0] = info[1] = 0;
    if (n <= 1) return SA_OK;
    SA_TRY(need_device());
    std::lock_guard<std::mutex> lk(g_mu);
    sa_context* c = nullptr;
    SA_TRY(global_ctx(n, &c));
    DevBuf d_text, d_sa, d_len, d_lo, d_hi;
    SA_TRY(d_text.alloc(align_up(n, 256)));
    SA_TRY(d_sa.alloc(align_up(n, 64) * 4));
    SA_TRY(upload({{d_text.p, text, n}, {d_sa.p, src32, n * 4}}));
    const int valid = check_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), nullptr);
    if (valid == 0) return set_err(SA_E_INVALID, "not a valid suffix array of the text");
    if (valid != 1) return valid;
    const uint64_t cap = given ? std::min<uint64_t>(out_cap, n) : 0;   // a text has fewer than n repeats
    if (given) {
        SA_TRY(d_len.alloc(align_up(cap + 1, 64) * 4));
        SA_TRY(d_lo.alloc(align_up(cap + 1, 64) * 4));
        SA_TRY(d_hi.alloc(align_up(cap + 1, 64) * 4));
    }
    uint64_t got[kRepInfo] = {0, 0};
    SA_TRY(repeats_device(c, d_text.as<uint8_t>(), n, d_sa.as<uint32_t>(), nullptr, min_len, min_occ, kind,
                          d_len.as<uint32_t>(), d_lo.as<uint32_t>(), d_hi.as<uint32_t>(), cap, got, nullptr));
    info[0] = got[0];
    info[1] = got[1];
    if (!given || got[0] > out_cap) return SA_OK;
    SA_TRY(copy_d2h(len_out, d_len.as<uint32_t>(), got[0], sa_width, nullptr));
    SA_TRY(copy_d2h(lo_out, d_lo.as<uint32_t>(), got[0], sa_width, nullptr));
    SA_TRY(copy_d2h(hi_out, d_hi.as<uint32_t>(), got[0], sa_width, nullptr));
    return SA_OK;
}

}  // namespace sa

extern "C" {

int sa_repeats_device(sa_context* ctx, const uint8_t* d_text, uint64_t n, const uint32_t* d_sa, const uint32_t* d_lcp,
                      uint64_t min_len, uint64_t min_occ, uint32_t kind, uint32_t* d_len, uint32_t* d_lo, uint32_t* d_hi,
                      uint64_t out_cap, uint64_t info[SA_REP_INFO], void* stream) {
    return sa::repeats_device(ctx, d_text, n, d_sa, d_lcp, min_len, min_occ, kind, d_len, d_lo, d_hi, out_cap, info,
                              (hipStream_t)stream);
}

int sa_repeats(const uint8_t* text, uint64_t n, const void* sa, int sa_width, uint64_t min_len, uint64_t min_occ,
               uint32_t kind, void* len_out, void* lo_out, void* hi_out, uint64_t out_cap, uint64_t info[SA_REP_INFO]) {
    return sa::repeats_host(text, n, sa, sa_width, min_len, min_occ, kind, len_out, lo_out, hi_out, out_cap, info);
}

}  // extern "C"

#endif   // __HIPCC__
